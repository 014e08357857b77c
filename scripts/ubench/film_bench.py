"""The progressive film against the plain render on a BASELINE.json config at full size (on the GPU box): wall and
HIP-event times and the frames' sha256 of rayrs_render, of a one-pass film, and of the same samples in 2, 4 and 16 passes.
usage: python scripts/ubench/film_bench.py CONFIG [profile]   (profile: one render and one one-pass film, for a kernel trace)"""
import hashlib, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import rayrs_amd
from rayrs_amd import procedural, scenes

config = int(sys.argv[1])
mode = sys.argv[2] if len(sys.argv) > 2 else "all"
RES = {1: 256, 2: 1024, 3: 1024, 4: 2048, 5: 2048}
ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_{config}_{os.getuid()}.ply") if config in (3, 5) else None
cam_args, objs, heur, spp, bounces = scenes.config(config, ply_path=ply) if ply else scenes.config(config)
cam_args = scenes.camera_for_resolution(cam_args, RES[config], RES[config])
scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(1024, 512), device=0)
cam = rayrs_amd.Camera(*cam_args)
chunk = rayrs_amd.frame_sample_chunk(cam.x_pixels(), cam.y_pixels(), spp, 4) or spp
print(json.dumps({"config": config, "res": RES[config], "spp": spp, "chunk": chunk, "local_pool": scene.info()["local_pool"]}), flush=True)
sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()[:16]

def plain():
    t = time.perf_counter()
    img, st = rayrs_amd.render(scene, cam, spp, bounces, seed=0x5EED, sample_chunk=chunk)
    return {"what": "render", "wall_ms": (time.perf_counter() - t) * 1e3, "total_ms": st["total_ms"], "trace_ms": st["trace_ms"],
            "resolve_ms": st["total_ms"] - st["trace_ms"], "rays": st["rays"], "sha": sha(img)}

def film(passes):
    t = time.perf_counter()
    f = rayrs_amd.Film(scene, cam, sample_chunk=chunk, max_bounces=bounces, seed=0x5EED)
    tot = tr = 0.0; rays = 0
    for _ in range(passes):
        st = f.render(spp // passes)
        tot += st["total_ms"]; tr += st["trace_ms"]; rays += st["rays"]
    img = f.image()
    wall = (time.perf_counter() - t) * 1e3
    f.close()
    return {"what": f"film x{passes}", "wall_ms": wall, "total_ms": tot, "trace_ms": tr, "accumulate_ms": tot - tr, "rays": rays, "sha": sha(img)}

if mode == "profile":   # one render and one one-pass film, for a kernel trace
    print(json.dumps(plain()), flush=True); print(json.dumps(film(1)), flush=True); sys.exit(0)
plain()  # warm-up: allocations
for job in (plain, lambda: film(1), lambda: film(1), plain, lambda: film(2), lambda: film(4), lambda: film(16), lambda: film(1), plain):
    print(json.dumps(job()), flush=True)
