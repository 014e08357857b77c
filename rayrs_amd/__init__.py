"""rayrs_amd -- MI355X (gfx950) build of rayrs-lib's per-pixel radiance integrator.

The product is librayrs_hip.so (hand-written HIP kernels behind the C ABI of
include/rayrs_hip.h); this package is the thin host-side mirror of the
rayrs-lib Scene / Camera / Object / Material interface on top of it.  Nothing
here computes radiance on the CPU and nothing falls back to a CPU path.
"""
from .api import (SKY, Axis, Bake, BvhHeuristic, Camera, Emission, Film, Fresnel, History, Lightmap, Material, MeshLights, Object, Scene, denoise, denoise_guided, emitters, frame_sample_chunk,
                  make_params, mesh_emitters, render, render_ao, render_features, render_finish, render_launch, render_lit, render_multi, render_sequence,
                  render_until, bake_until, orbit, probe_directions, probe_grid, sh_basis, sh_irradiance, sh_radiance, unwrap_triangles)

__all__ = ["SKY", "Axis", "Bake", "BvhHeuristic", "Camera", "Emission", "Film", "Fresnel", "History", "Lightmap", "Material", "MeshLights", "Object", "Scene",
           "denoise", "denoise_guided", "emitters", "frame_sample_chunk", "make_params", "mesh_emitters", "render", "render_ao", "render_features", "render_finish", "render_launch", "render_lit", "render_multi",
           "render_sequence", "render_until", "bake_until", "orbit", "probe_directions", "probe_grid", "sh_basis", "sh_irradiance", "sh_radiance", "unwrap_triangles"]
