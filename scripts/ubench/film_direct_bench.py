"""Measurements for the direct-lit films (profiles/film_direct.txt).  Run on a GPU box:

  python scripts/ubench/film_direct_bench.py [OUT [RES [TAU [CAP]]]]

On the config-3 scene (the mesh under its lamp) at RES x RES (default 1024), under the procedural sky (make_hdri) and under the
studio map (make_studio_hdri), one JSON line per measurement, printed and appended to OUT (default profiles/film_direct.txt):

  (a) a 16-sample pass of a plain film, of a _direct film (the scene's lamp) and of a _sky film (the lamp and the sky), each on a
      fresh film, beside render_lit(direct=True) of 16 samples with the same list in the same run (the plain film beside
      render()): legs in the order A B B A, A the film's pass and B the one-shot frame, wall time around the call that returns
      when the work is done, and the pass's own HIP-event time where it has one.  The one-shot frame also downloads an f64 image
      and a query plane, which the pass does not: the film's figure to compare is therefore also given with an image() read.
  (b) render_until(tau, adaptive=True) to the same TAU (default 0.2) and cap (default 128 samples) in passes of 16 on the three
      films: the samples taken, the wall time and the unconverged pixels left.

The waves' thresholds are the radiance queries' defaults (radiance_kernels.h); they were not swept for the film's item order."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import rayrs_amd  # noqa: E402
from rayrs_amd import SKY, procedural, scenes  # noqa: E402

PASS = 16


def emit(out, row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def timed(fn):
    t0 = time.perf_counter()
    result = fn()
    return (time.perf_counter() - t0) * 1e3, result


def main(out="profiles/film_direct.txt", res=1024, tau=0.2, cap=128):
    res, tau, cap = int(res), float(tau), int(cap)
    cam_args, objs, heur, _, mb = scenes.config(3)
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, res, res))
    lamps = rayrs_amd.emitters(objs)
    emit(out, {"config": 3, "res": res, "pass_samples": PASS, "sample_chunk": 4, "max_bounces": mb, "lights": lamps, "tau": tau, "cap": cap,
               "command": "python scripts/ubench/film_direct_bench.py " + " ".join(sys.argv[1:])})
    for map_name, hdri in (("procedural", procedural.make_hdri(1024, 512)), ("studio", procedural.make_studio_hdri(1024, 512))):
        scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, hdri, device=0)
        kinds = {"plain": {}, "direct": dict(lights=lamps, direct=True), "sky": dict(lights=lamps + [SKY], direct=True)}

        def film_of(kind):
            return rayrs_amd.Film(scene, cam, sample_chunk=4, max_bounces=mb, **kinds[kind])

        def one_shot(kind):
            if kind == "plain":
                return lambda: rayrs_amd.render(scene, cam, PASS, mb, sample_chunk=4, out_f64=True)
            return lambda: rayrs_amd.render_lit(scene, cam, PASS, kinds[kind]["lights"], max_bounces=mb, sample_chunk=4, queries=True, direct=True)

        for kind in kinds:   # warm: the sky's table, the scratch, the kernels' code objects
            film_of(kind).render(4), one_shot(kind)()
        for kind in kinds:
            legs, event_ms, with_read, rays = [], [], [], None
            for leg in "ABBA":
                if leg == "A":
                    film = film_of(kind)
                    ms, st = timed(lambda: film.render(PASS))
                    read_ms, _ = timed(lambda: film.image(out_f64=True))
                    legs.append(round(ms, 3)), event_ms.append(round(st["total_ms"], 3)), with_read.append(round(ms + read_ms, 3))
                    rays = st["rays"]
                    film.close()
                else:
                    ms, _ = timed(one_shot(kind))
                    legs.append(round(ms, 3))
            a, b = (legs[0] + legs[3]) / 2, (legs[1] + legs[2]) / 2
            emit(out, {"map": map_name, "a": "16-sample pass", "film": kind, "one_shot": "render" if kind == "plain" else "render_lit(direct=True)",
                       "legs_ms_ABBA": legs, "film_pass_ms": round(a, 3), "film_pass_and_read_ms": round(sum(with_read) / 2, 3),
                       "film_pass_event_ms": event_ms, "one_shot_ms": round(b, 3), "film_over_one_shot": round(a / b, 3),
                       "film_and_read_over_one_shot": round(sum(with_read) / 2 / b, 3), "rays": rays})
        for kind in kinds:
            film = film_of(kind)
            ms, (st, why) = timed(lambda: rayrs_amd.render_until(film, tau, 0.0, pass_samples=PASS, max_samples=cap, adaptive=True))
            emit(out, {"map": map_name, "b": "render_until adaptive", "film": kind, "tau": tau, "cap": cap, "wall_ms": round(ms, 1), "stopped": why,
                       "samples_max": st["samples"], "pixel_samples": st.get("pixel_samples"), "unconverged": st["unconverged"],
                       "nonfinite": st["nonfinite"], "rays": st["rays"]})
            film.close()


if __name__ == "__main__":
    main(*sys.argv[1:5])
