"""Temporal accumulation on a BASELINE.json config at full size (on the GPU box), with film_guided_bench.py's setup: an orbit
of four frames at 16 samples each, every frame's film pushed into one history.  Per frame, measured in the same run: the
frame's render time (the pass's own total_ms), the push by its HIP events (features, frame, noise plane, copies of the
features, reprojection: History.push_times()), and one level of Film.denoised_guided on the same film -- the yardstick: a
guided level makes 34 taps per pixel where the reprojection makes 4, so a reprojection slower than one level means the
history's plane layout is losing.  With `quality`, per frame of the same orbit, the RMSE of the raw frame, of
Film.denoised_guided, of the history and of History.denoised_guided against a long reference from the frame's own camera.
usage: python scripts/ubench/film_temporal_bench.py CONFIG [DEGREES]
       python scripts/ubench/film_temporal_bench.py quality SCENE RES REF_SPP [DEGREES]
(DEGREES: the whole orbit's, default 8: two degrees a frame.  One guided level is (levels=3 - levels=1) / 2 of the best of
three host-clock times of calls that end in a blocking copy: the difference drops the pack, the features and the copy.  Per
pixel temporal_kernel reads 76 B of A's frame and features, up to 4 taps of 60 B of B's features, variance and weight and 24 B
of colour for the valid ones, and writes 40 B; a guided level reads 2488 B.)"""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import rayrs_amd
from rayrs_amd import procedural, scenes

FRAMES, SPP = 4, 16


def best_ms(fn, repeats=3):
    best = None
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None or ms < best else best
    return best


def bench(config, degrees):
    RES = {1: 256, 2: 1024, 3: 1024, 4: 2048, 5: 2048}
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_{config}_{os.getuid()}.ply") if config in (3, 5) else None
    cam_args, objs, heur, spp, bounces = scenes.config(config, ply_path=ply) if ply else scenes.config(config)
    cam_args = scenes.camera_for_resolution(cam_args, RES[config], RES[config])
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(1024, 512), device=0)
    cam = rayrs_amd.Camera(*cam_args)
    print(json.dumps({"config": config, "res": RES[config], "frames": FRAMES, "spp": SPP, "orbit_degrees": degrees}), flush=True)
    history = rayrs_amd.History(device=0)
    worst = None
    for i in range(FRAMES + 1):      # frame 0 twice: the first time warms every kernel up and is not reported
        frame = max(i - 1, 0)
        if i == 1:
            history.reset()
        film = rayrs_amd.Film(scene, rayrs_amd.orbit(cam, frame * degrees / FRAMES), sample_chunk=4, max_bounces=bounces, seed=0x5EED)
        st = film.render(SPP)
        history.push(film)
        times = history.push_times()
        t1 = best_ms(lambda: film.denoised_guided(levels=1))
        t3 = best_ms(lambda: film.denoised_guided(levels=3))
        level_ms = (t3 - t1) / 2.0
        weight = history.weight()
        film.close()
        if i == 0:
            continue
        row = {"frame": frame, "render_ms": round(st["total_ms"], 3), "push_ms": {k: round(v, 3) for k, v in times.items()},
               "guided_level_ms": round(level_ms, 3), "guided_levels_1_and_3_ms": [round(t1, 3), round(t3, 3)],
               "history_mean_weight": round(float(weight.mean()), 2), "pixels_with_history": round(float((weight > SPP).mean()), 4)}
        print(json.dumps(row), flush=True)
        if frame > 0:
            ratio = times["reproject_ms"] / level_ms
            worst = ratio if worst is None or ratio > worst else worst
    print(json.dumps({"reprojection_over_one_guided_level_worst_frame": round(worst, 3),
                      "verdict": "the planes hold: no packed records" if worst < 1.0 else "the planes lose: pack the taps"}), flush=True)


def quality(scene_name, res, ref_spp, degrees):
    cam_args, objs, heur = getattr(scenes, scene_name)()
    cam_args = scenes.camera_for_resolution(cam_args, res, res * 5 // 24 if "spheres" in scene_name else res)
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(1024, 512), device=0)
    cam = rayrs_amd.Camera(*cam_args)
    print(json.dumps({"scene": scene_name, "pixels": [cam.x_pixels(), cam.y_pixels()], "reference_spp": ref_spp, "frames": FRAMES,
                      "spp": SPP, "orbit_degrees": degrees}), flush=True)
    cams = [rayrs_amd.orbit(cam, i * degrees / FRAMES) for i in range(FRAMES)]
    for i, (film, history) in enumerate(rayrs_amd.render_sequence(scene, cams, SPP, sample_chunk=4, max_bounces=50, seed=0x5EED)):
        ref_film = rayrs_amd.Film(scene, cams[i], sample_chunk=4, max_bounces=50, seed=0xBEEF)   # another seed than the frames'
        ref_film.render(ref_spp)
        ref = ref_film.image(out_f64=True)
        ref_film.close()

        def rmse(img):
            d = np.asarray(img, dtype=np.float64) - ref
            ok = np.isfinite(d).all(axis=2)
            return round(float(np.sqrt((d[ok] ** 2).mean())), 6)

        print(json.dumps({"frame": i, "rmse_raw": rmse(film.image(out_f64=True)), "rmse_guided": rmse(film.denoised_guided(out_f64=True)),
                          "rmse_temporal": rmse(history.image(out_f64=True)),
                          "rmse_temporal_guided": rmse(history.denoised_guided(out_f64=True)),
                          "history_mean_weight": round(float(history.weight().mean()), 2)}), flush=True)
        film.close()


if sys.argv[1] == "quality":
    quality(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]) if len(sys.argv) > 5 else 8.0)
else:
    bench(int(sys.argv[1]), float(sys.argv[2]) if len(sys.argv) > 2 else 8.0)
