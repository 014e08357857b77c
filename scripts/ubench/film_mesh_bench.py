"""Measurements for the mesh-lit films and bakes (profiles/film_mesh.txt).  Run on a GPU box:

  python scripts/ubench/film_mesh_bench.py [OUT [RES [TAU]]]

The scene is config 3's with its lamp built as the 320-triangle emissive icosphere of scripts/ubench/mesh_lights_bench.py's case
(b), under make_hdri(64, 32); the group is all of its triangles, the list beside it is empty, and "sky" adds SKY to it.  One JSON
line per measurement, printed and appended to OUT (default profiles/film_mesh.txt):

  (a) a 16-sample pass of a plain film and of a mesh film at RES x RES (default 1024), on both walks, the mesh film without and
      with SKY, beside the one-shot frame of the same 16 samples in the same run -- render() for the plain film,
      render_lit(direct=True, mesh=group) for the mesh film: legs in the order A B B A, A the film's pass and B the one-shot
      frame; a leg is REPEATS calls in a row, each pass on a fresh film made before the clock starts; wall time around them,
      given per call, and the pass's own HIP-event time.  The one-shot frame also downloads an f64 image (and, lit, a query
      plane), which the pass does not: the film's figure is therefore also given with an image() read.  The one-shot call is
      the code there was before the films took a group.
  (b) render_until(TAU, adaptive=True, passes of 16, cap 128) on the plain film and on the two mesh films, default walk: wall
      time, pixel-samples, the pixels left unconverged and the non-finite ones.  TAU defaults to 0.2.
  (c) the bake, at the first hits of 2^18 rays aimed at the root box (the point set of profiles/lit_rates.txt and
      scripts/ubench/bake_bench.py): a 16-sample pass of the mesh bake beside the one-shot scene.irradiance(mesh=group) on
      device tensors, A B B A as in (a), on both walks, without and with SKY; and bake_until(TAU, passes of 16, cap 256),
      adaptive against uniform, as bake_bench.py has it.

The waves' thresholds are the radiance queries' defaults (radiance_kernels.h); they were not swept for these item orders.  Only
comparisons within one run count; no figure is asserted."""
import json
import os
import sys
import tempfile
import time

import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one

torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import rayrs_amd  # noqa: E402
from rayrs_amd import SKY, procedural, scenes  # noqa: E402
from rayrs_amd.api import Emission, Object  # noqa: E402

PASS, CHUNK, BOUNCES = 16, 4, 50
FILM_CAP, BAKE_CAP = 128, 256
REPEATS = 5
N_RAYS = 1 << 18


def emit(out, row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def unit_vectors(n, gen):
    v = torch.randn((n, 3), dtype=torch.float64, device="cuda:0", generator=gen)
    return v / v.norm(dim=1, keepdim=True)


def icosphere_scene():
    """config 3 with a small emissive icosphere of 320 triangles where its rectangle lamp was, the same power spread over its area
    (mesh_lights_bench.py's case (b)): (camera args, objects, heuristic)."""
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_3_{os.getuid()}.ply")
    cam_args, objs, heur, _, _ = scenes.config(3, ply_path=ply)
    rect = objs[-1]
    assert rect.kind == "plane" and len(rayrs_amd.emitters(objs)) == 1
    v, f = procedural.icosphere(2)
    area = 4.0 * np.pi * 0.35 ** 2
    ball = Object.from_triangles((v * 0.35 + (0.0, rect.pos - 0.5, 0.0)).astype(np.float32), f.astype(np.uint32), rect.mat,
                                 Emission.new(rect.emission.strength * (rect.umax - rect.umin) ** 2 / area, rect.emission.color))
    return cam_args, list(objs[:-1]) + ball, heur


def abba(make_a, run_a, run_b):
    """A B B A: A = run_a on REPEATS fresh objects of make_a, B = REPEATS calls of run_b.  (legs ms a call, A's results)"""
    legs, kept = [], None
    for leg in "ABBA":
        if leg == "A":
            fresh = [make_a() for _ in range(REPEATS)]
            ms, kept = timed(lambda: [run_a(x) for x in fresh])
            for x in fresh:
                x.close()
        else:
            ms, _ = timed(lambda: [run_b() for _ in range(REPEATS)])
        legs.append(round(ms / REPEATS, 3))
    return legs, kept


def main(out=os.path.join(ROOT, "profiles", "film_mesh.txt"), res=1024, tau=0.2):
    res, tau = int(res), float(tau)
    cam_args, objs, heur = icosphere_scene()
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, res, res))
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(64, 32), device=0)
    group = scene.mesh_lights(rayrs_amd.mesh_emitters(objs))
    info = scene.info()
    emit(out, {"config": 3, "lamp": "icosphere", "group": len(group), "group_area": group.total, "res": res, "pass_samples": PASS,
               "repeats_per_leg": REPEATS, "sample_chunk": CHUNK, "max_bounces": BOUNCES, "tau": tau, "film_cap": FILM_CAP, "bake_cap": BAKE_CAP,
               "n_prims": info["n_prims"], "command": "python scripts/ubench/film_mesh_bench.py " + " ".join(sys.argv[1:])})
    kinds = {"plain": None, "mesh": [], "mesh+sky": [SKY]}

    def film_of(kind, fast=False):
        kw = {} if kinds[kind] is None else dict(lights=kinds[kind], direct=True, mesh=group)
        return rayrs_amd.Film(scene, cam, sample_chunk=CHUNK, max_bounces=BOUNCES, fast_traversal=fast, **kw)

    def frame_of(kind, fast):
        if kinds[kind] is None:
            return lambda: rayrs_amd.render(scene, cam, PASS, BOUNCES, sample_chunk=CHUNK, out_f64=True, fast_traversal=fast)
        return lambda: rayrs_amd.render_lit(scene, cam, PASS, kinds[kind], max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast,
                                            queries=True, direct=True, mesh=group)

    # ---- (a) a film pass against the one-shot frame
    for fast in (False, True):
        for kind in kinds:   # warm: the group's and the sky's tables, the scratch, the kernels' code objects
            film_of(kind, fast).render(CHUNK), frame_of(kind, fast)()
        for kind in kinds:
            legs, sts = abba(lambda: film_of(kind, fast), lambda film: film.render(PASS), frame_of(kind, fast))
            film = film_of(kind, fast)
            film.render(PASS)
            read_ms, _ = timed(lambda: film.image(out_f64=True))
            film.close()
            a, b = (legs[0] + legs[3]) / 2, (legs[1] + legs[2]) / 2
            emit(out, {"a": "16-sample pass", "walk": "fast" if fast else "default", "film": kind,
                       "one_shot": "render" if kinds[kind] is None else "render_lit(direct=True, mesh=group)", "legs_ms_ABBA": legs,
                       "film_pass_ms": round(a, 3), "film_pass_event_ms": round(sum(st["total_ms"] for st in sts) / REPEATS, 3),
                       "image_read_ms": round(read_ms, 3), "one_shot_ms": round(b, 3), "film_over_one_shot": round(a / b, 3),
                       "film_and_read_over_one_shot": round((a + read_ms) / b, 3), "rays": sts[0]["rays"]})

    # ---- (b) adaptive films to a noise level
    for kind in kinds:
        film = film_of(kind)
        ms, (st, why) = timed(lambda: rayrs_amd.render_until(film, tau, 0.0, pass_samples=PASS, max_samples=FILM_CAP, adaptive=True))
        emit(out, {"b": "render_until adaptive", "walk": "default", "film": kind, "tau": tau, "cap": FILM_CAP, "wall_ms": round(ms, 1),
                   "stopped": why, "samples_max": st["samples"], "pixel_samples": st.get("pixel_samples"), "pixels": st["pixels"],
                   "unconverged": st["unconverged"], "nonfinite": st["nonfinite"], "rays": st["rays"]})
        film.close()

    # ---- (c) the bake
    box = torch.tensor(info["root_box"], dtype=torch.float64, device="cuda:0")
    lo, hi = box[0::2], box[1::2]
    centre, diag = (lo + hi) * 0.5, float((hi - lo).norm())
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0x5EED)
    o = (centre + unit_vectors(N_RAYS, gen) * (0.75 * diag)).contiguous()
    d = (lo + torch.rand((N_RAYS, 3), dtype=torch.float64, device="cuda:0", generator=gen) * (hi - lo) - o).contiguous()
    t, obj, nrm = scene.intersect(o, d, normals=True)
    hit = obj.view(torch.int32) != -1
    p = (o + d * t[:, None])[hit].contiguous()
    n = torch.where((nrm * d).sum(dim=1, keepdim=True) > 0.0, -nrm, nrm)[hit].contiguous()
    p_host, n_host = p.cpu().numpy(), n.cpu().numpy()
    bias = 1e-4 * diag
    emit(out, {"c": "points", "aimed_rays": N_RAYS, "points": len(p_host), "bias": bias})
    strategies = {"unlit": None, "mesh": [], "mesh+sky": [SKY]}

    def bake_of(strategy, fast=False):
        kw = {} if strategies[strategy] is None else dict(lights=strategies[strategy], direct=True, mesh=group)
        return rayrs_amd.Bake(scene, p_host, n_host, sample_chunk=CHUNK, max_bounces=BOUNCES, seed=0x5EED, bias=bias, fast_traversal=fast, **kw)

    def query_of(strategy, fast):
        kw = {} if strategies[strategy] is None else dict(lights=strategies[strategy], direct=True, mesh=group)
        return lambda: scene.irradiance(p, n, samples=PASS, bias=bias, max_bounces=BOUNCES, seed=0x5EED, sample_chunk=CHUNK, fast_traversal=fast,
                                        queries=True, **kw)

    for fast in (False, True):
        for strategy in strategies:
            bake_of(strategy, fast).render(CHUNK), query_of(strategy, fast)()
        for strategy in strategies:
            legs, sts = abba(lambda: bake_of(strategy, fast), lambda bake: bake.render(PASS), query_of(strategy, fast))
            a, b = (legs[0] + legs[3]) / 2, (legs[1] + legs[2]) / 2
            emit(out, {"c": "16-sample pass", "walk": "fast" if fast else "default", "bake": strategy, "legs_ms_ABBA": legs,
                       "bake_pass_ms": round(a, 3), "bake_pass_event_ms": round(sum(st["kernel_ms"] for st in sts) / REPEATS, 3),
                       "one_shot_ms": round(b, 3), "bake_over_one_shot": round(a / b, 3), "rays": sts[0]["rays"],
                       "mray_s_bake": round(sts[0]["rays"] / a / 1e3, 1)})
    for strategy in strategies:
        row = {"c": "bake_until", "walk": "default", "bake": strategy, "tau": tau, "cap": BAKE_CAP}
        for adaptive in (True, False):
            bake = bake_of(strategy)
            ms, (st, why) = timed(lambda: rayrs_amd.bake_until(bake, tau, pass_samples=PASS, max_samples=BAKE_CAP, adaptive=adaptive))
            row["adaptive" if adaptive else "uniform"] = {"wall_ms": round(ms, 1), "stopped": why, "samples_max": st["samples"],
                                                          "point_samples": st["point_samples"], "unconverged": st["unconverged"],
                                                          "nonfinite": st["nonfinite"], "rays": st["rays"]}
            bake.close()
        row["adaptive_over_uniform_wall"] = round(row["adaptive"]["wall_ms"] / row["uniform"]["wall_ms"], 3)
        row["adaptive_over_uniform_point_samples"] = round(row["adaptive"]["point_samples"] / row["uniform"]["point_samples"], 3)
        emit(out, row)
    group.close()


if __name__ == "__main__":
    main(*sys.argv[1:4])
