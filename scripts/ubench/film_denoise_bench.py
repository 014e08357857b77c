"""First-hit features and the five-level a-trous filter on a BASELINE.json config at full size (on the GPU box), beside that
box's frame time: wall times of render_features(samples=16) and of Film.denoised(levels=5) (both include the copy of
their planes to the host; the film's second call finds its features on the device), and the frame's own time.
usage: python scripts/ubench/film_denoise_bench.py CONFIG [profile]
       rocprofv3 --kernel-trace --stats -d DIR -- python scripts/ubench/film_denoise_bench.py CONFIG profile
(profile: one features pass and one denoise after a 16-sample film pass, for the kernels' own times)"""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
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


def timed(what, fn):
    t = time.perf_counter()
    fn()
    print(json.dumps({"what": what, "wall_ms": round((time.perf_counter() - t) * 1e3, 3)}), flush=True)


film = rayrs_amd.Film(scene, cam, sample_chunk=chunk, max_bounces=bounces, seed=0x5EED)
st = film.render(16)
print(json.dumps({"what": "film pass of 16 samples", "total_ms": st["total_ms"], "rays": st["rays"]}), flush=True)
repeats = 1 if mode == "profile" else 3
for _ in range(repeats):
    timed("render_features(samples=16)", lambda: rayrs_amd.render_features(scene, cam, samples=16))
for k in range(repeats):
    timed("Film.denoised(levels=5)" + (", features made" if k == 0 else ", features kept"), lambda: film.denoised(levels=5))
timed("Film.image()", lambda: film.image())
if mode != "profile":
    img, st = rayrs_amd.render(scene, cam, spp, bounces, seed=0x5EED, sample_chunk=chunk)
    print(json.dumps({"what": f"frame of {spp} samples", "total_ms": st["total_ms"], "rays": st["rays"]}), flush=True)
