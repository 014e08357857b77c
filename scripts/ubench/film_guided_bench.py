"""The variance-guided filter beside the feature-guided one on a BASELINE.json config at full size (on the GPU box), with
film_denoise_bench.py's setup: wall times of Film.noise(), Film.denoised(levels=5) and Film.denoised_guided(levels=5) after
a 16-sample film pass (all include the copy of their planes to the host; the features are made once and kept), or, with
`quality`, the RMSE of the raw frame, denoised() and denoised_guided() against a long reference of the same film settings.
usage: python scripts/ubench/film_guided_bench.py CONFIG [profile]
       rocprofv3 --kernel-trace --stats -d DIR -- python scripts/ubench/film_guided_bench.py CONFIG profile
       python scripts/ubench/film_guided_bench.py quality SCENE RES REF_SPP
(profile: one call of each after the pass, for the kernels' own times.  Per pixel and level atrous_kernel reads 25 taps of
24 B colour + 56 B features = 2000 B and writes 24 B; guided_atrous_kernel 25 taps of a 32 B record + 56 B features and 9
records of the prefilter = 2488 B and writes 32 B.  quality: SCENE is a scenes.* function of the docs/renders scenes, the
reference REF_SPP samples of the same seed and chunk; uniform films of 16 and 64 samples, and adaptive ones from 16 samples
on, capped at 64 and at 256, at tau 0.2.)"""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import rayrs_amd
from rayrs_amd import procedural, scenes


def timed(what, fn):
    t = time.perf_counter()
    fn()
    print(json.dumps({"what": what, "wall_ms": round((time.perf_counter() - t) * 1e3, 3)}), flush=True)


def bench(config, mode):
    RES = {1: 256, 2: 1024, 3: 1024, 4: 2048, 5: 2048}
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_{config}_{os.getuid()}.ply") if config in (3, 5) else None
    cam_args, objs, heur, spp, bounces = scenes.config(config, ply_path=ply) if ply else scenes.config(config)
    cam_args = scenes.camera_for_resolution(cam_args, RES[config], RES[config])
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(1024, 512), device=0)
    cam = rayrs_amd.Camera(*cam_args)
    chunk = rayrs_amd.frame_sample_chunk(cam.x_pixels(), cam.y_pixels(), spp, 4) or spp
    print(json.dumps({"config": config, "res": RES[config], "spp": spp, "chunk": chunk}), flush=True)
    film = rayrs_amd.Film(scene, cam, sample_chunk=chunk, max_bounces=bounces, seed=0x5EED)
    st = film.render(16)
    print(json.dumps({"what": "film pass of 16 samples", "total_ms": st["total_ms"], "rays": st["rays"]}), flush=True)
    film.features(16)
    repeats = 1 if mode == "profile" else 3
    for _ in range(repeats):
        timed("Film.noise()", lambda: film.noise())
    for _ in range(repeats):
        timed("Film.denoised(levels=5), features kept", lambda: film.denoised(levels=5))
    for _ in range(repeats):
        timed("Film.denoised_guided(levels=5), features kept", lambda: film.denoised_guided(levels=5))
    timed("Film.image()", lambda: film.image())


def quality(scene_name, res, ref_spp):
    cam_args, objs, heur = getattr(scenes, scene_name)()
    cam_args = scenes.camera_for_resolution(cam_args, res, res * 5 // 24 if "spheres" in scene_name else res)
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(1024, 512), device=0)
    cam = rayrs_amd.Camera(*cam_args)
    new = lambda: rayrs_amd.Film(scene, cam, sample_chunk=4, max_bounces=50, seed=0x5EED)  # noqa: E731
    ref_film = new()
    ref_film.render(ref_spp)
    ref = ref_film.image(out_f64=True)
    ref_film.close()
    print(json.dumps({"scene": scene_name, "pixels": [cam.x_pixels(), cam.y_pixels()], "reference_spp": ref_spp}), flush=True)

    def rmse(img):
        d = np.asarray(img, dtype=np.float64) - ref
        ok = np.isfinite(d).all(axis=2)
        return round(float(np.sqrt((d[ok] ** 2).mean())), 6)

    def report(what, film):
        per = film.sample_map()
        print(json.dumps({"film": what, "mean_spp": round(float(per.mean()), 2), "min_spp": int(per.min()), "max_spp": int(per.max()),
                          "rmse_raw": rmse(film.image(out_f64=True)), "rmse_denoised": rmse(film.denoised(out_f64=True)),
                          "rmse_denoised_guided": rmse(film.denoised_guided(out_f64=True))}), flush=True)

    for n in (16, 64):
        film = new()
        film.render(n)
        report(f"uniform {n}", film)
        film.close()
    for cap in (64, 256):
        film = new()
        film.render(16)
        rayrs_amd.render_until(film, 0.2, pass_samples=16, max_samples=cap, adaptive=True)
        report(f"adaptive 16 .. {cap}, tau 0.2", film)
        film.close()


if sys.argv[1] == "quality":
    quality(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
else:
    bench(int(sys.argv[1]), sys.argv[2] if len(sys.argv) > 2 else "all")
