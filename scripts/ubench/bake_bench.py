"""Measurements for the bake (profiles/bake_rates.txt).  Run on a GPU box:

  python scripts/ubench/bake_bench.py [OUT [TAU [CAP]]]

On the config-3 scene (the mesh under its lamp, make_hdri(64, 32)), at the first hits of 2^18 rays aimed at the root box -- the
point set of scripts/ubench/lit_bench.py and profiles/lit_rates.txt, the normal turned to face the ray that found it, bias 1e-4
diagonals -- for the unlit, the direct-lit and the sky bake on both walks, sample_chunk 4, max_bounces 50.  One JSON line per
measurement, printed and appended to OUT (default profiles/bake_rates.txt):

  (a) a uniform pass of 16 samples on a fresh bake beside the one-shot scene.irradiance(...) of the same 16 samples with
      sample_chunk=4 and the same list, in the same run: legs in the order A B B A, A the bake's pass and B the one-shot query on
      device tensors (its _launch form, no copy either way); a leg is REPEATS calls in a row, each pass on a fresh bake made before
      the clock starts, wall time around them and a wait for the device, given per call.  The ratio is the price of the bake's
      records and item order.  The pass's own HIP-event time and the host form of the query (which uploads the
      points and downloads the answers) are given beside them.
  (b) bake_until(tau, passes of 16, cap CAP) adaptive against uniform passes to the same TAU (default 0.2) and CAP (default 256):
      wall time, point-samples spent, points left unconverged.

The waves' thresholds are the radiance queries' defaults (radiance_kernels.h); they were not swept for the bake's item order.
Only comparisons within one run count."""
import json
import os
import sys
import tempfile
import time

import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one

torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import rayrs_amd  # noqa: E402
from rayrs_amd import SKY, procedural, scenes  # noqa: E402

N_RAYS = 1 << 18
PASS, CHUNK, BOUNCES = 16, 4, 50
REPEATS = 20


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


def main(out=os.path.join(ROOT, "profiles", "bake_rates.txt"), tau=0.2, cap=256):
    tau, cap = float(tau), int(cap)
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_3_{os.getuid()}.ply")
    cam_args, objs, heur, spp, _ = scenes.config(3, ply_path=ply)
    lamps = rayrs_amd.emitters(objs)
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(64, 32), device=0)
    info = scene.info()
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
    emit(out, {"config": 3, "aimed_rays": N_RAYS, "points": len(p_host), "pass_samples": PASS, "repeats_per_leg": REPEATS, "sample_chunk": CHUNK, "max_bounces": BOUNCES,
               "lights": lamps, "tau": tau, "cap": cap, "n_prims": info["n_prims"],
               "command": "python scripts/ubench/bake_bench.py " + " ".join(sys.argv[1:])})
    strategies = {"unlit": {}, "direct": dict(lights=lamps, direct=True), "sky": dict(lights=lamps + [SKY], direct=True)}
    for fast in (False, True):
        walk = "fast" if fast else "default"

        def bake_of(strategy):
            return rayrs_amd.Bake(scene, p_host, n_host, sample_chunk=CHUNK, max_bounces=BOUNCES, seed=0x5EED, bias=bias, fast_traversal=fast,
                                  **strategies[strategy])

        def one_shot(strategy, a, b):
            return lambda: scene.irradiance(a, b, samples=PASS, bias=bias, max_bounces=BOUNCES, seed=0x5EED, sample_chunk=CHUNK,
                                            fast_traversal=fast, queries=True, **strategies[strategy])

        for strategy in strategies:   # warm: the sky's table, the scratch, the kernels' code objects
            bake_of(strategy).render(CHUNK), one_shot(strategy, p, n)()
        for strategy in strategies:
            legs, event_ms, rays = [], [], None
            query, query_host = one_shot(strategy, p, n), one_shot(strategy, p_host, n_host)
            for leg in "ABBA":
                if leg == "A":
                    bakes = [bake_of(strategy) for _ in range(REPEATS)]
                    ms, sts = timed(lambda: [bake.render(PASS) for bake in bakes])
                    legs.append(round(ms / REPEATS, 3)), event_ms.append(round(sum(st["kernel_ms"] for st in sts) / REPEATS, 3))
                    rays = sts[0]["rays"]
                    for bake in bakes:
                        bake.close()
                else:
                    ms, _ = timed(lambda: [query() for _ in range(REPEATS)])
                    legs.append(round(ms / REPEATS, 3))
            query_host()
            host_ms, _ = timed(lambda: [query_host() for _ in range(REPEATS)])
            host_ms /= REPEATS
            a, b = (legs[0] + legs[3]) / 2, (legs[1] + legs[2]) / 2
            emit(out, {"walk": walk, "a": "16-sample pass", "bake": strategy, "legs_ms_ABBA": legs, "bake_pass_ms": round(a, 3),
                       "bake_pass_event_ms": event_ms, "one_shot_ms": round(b, 3), "bake_over_one_shot": round(a / b, 3),
                       "one_shot_host_form_ms": round(host_ms, 3), "rays": rays, "mray_s_bake": round(rays / a / 1e3, 1)})
        for strategy in strategies:
            row = {"walk": walk, "b": "bake_until", "bake": strategy, "tau": tau, "cap": cap}
            for adaptive in (True, False):
                bake = bake_of(strategy)
                ms, (st, why) = timed(lambda: rayrs_amd.bake_until(bake, tau, pass_samples=PASS, max_samples=cap, adaptive=adaptive))
                row["adaptive" if adaptive else "uniform"] = {"wall_ms": round(ms, 1), "stopped": why, "samples_max": st["samples"],
                                                              "point_samples": st["point_samples"], "unconverged": st["unconverged"],
                                                              "nonfinite": st["nonfinite"], "rays": st["rays"]}
                bake.close()
            row["adaptive_over_uniform_wall"] = round(row["adaptive"]["wall_ms"] / row["uniform"]["wall_ms"], 3)
            row["adaptive_over_uniform_point_samples"] = round(row["adaptive"]["point_samples"] / row["uniform"]["point_samples"], 3)
            emit(out, row)


if __name__ == "__main__":
    main(*sys.argv[1:4])
