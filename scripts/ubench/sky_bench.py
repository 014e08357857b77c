"""The sky as a light of direct lighting against direct lighting with the lamps only and the unlit radiance queries, on a
BASELINE.json config's scene under two environment maps (on the GPU box): Scene.irradiance and Scene.radiance without lights, with
lights=emitters(objs), direct=True, and with lights=emitters(objs) + [SKY], direct=True, on the same device tensors in the same run,
timed with HIP events on torch's current stream.
usage: python scripts/ubench/sky_bench.py [CONFIG [OUT]]   (CONFIG: default 3, the mesh under an area light; OUT: default profiles/sky_rates.txt)

The maps: "procedural", procedural.make_hdri(64, 32), the bright sky of profiles/direct_rates.txt; "studio",
procedural.make_studio_hdri(64, 32), black but for a window above the clip value 3 and a dimmer softbox.  The library clips a map to
[0, 3] as the reference does, so no texel is brighter than 3: the gain of sampling the sky is bounded by how uneven a clipped map
can be.

Rays, as scripts/ubench/lit_bench.py makes them (the two sets of profiles/lit_rates.txt): 2^18 rays from a sphere around the
scene's root box (radius 1.5 half-diagonals), each aimed at a random point of the box.  Two sets, each on both walks, max_bounces
50, sample_chunk 4:
  "irradiance": at the rays' first hits (the normal turned to face the ray that found it), S_IRR samples a point, bias 1e-4 diagonals;
  "radiance":   on the rays themselves, S_RAD samples a ray.
Per map, set and walk:

  (a) the rate.  Mray/s = the sum of the call's `queries` (every Bvh::intersect call of its paths, the shadow queries among them)
      over the time of a call.  Direct and sky (A) are each timed against unlit (B) in A B B A order (each leg REPEATS calls between
      two events, after a warm-up call of each).  The three make different paths, so queries per path are given beside the rates,
      and ms per call is the figure that (b) multiplies.
  (b) the noise at equal samples.  The call is repeated with SEEDS seeds; a ray's variance is the variance of its answer over
      the seeds, summed over the three channels, and the figure is the mean over the rays whose answers are finite under all
      three strategies (the rest are counted per strategy).  variance x time = that mean times (a)'s ms per call, as a ratio to
      unlit's: below 1, the strategy reaches a given noise sooner than the cosine lobe alone.  The means are printed: the three
      estimate the same light.

Only comparisons within one run count; boxes differ by a few percent.  No figure is asserted.  Writes OUT (every line it prints, with
the hash of the library's sources)."""
import glob, hashlib, json, os, sys, tempfile
import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one
torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import rayrs_amd
from rayrs_amd import SKY, procedural, scenes

REPEATS = 10
SEEDS = 16
N_RAYS = 1 << 18
S_IRR, S_RAD, CHUNK, BOUNCES = 16, 4, 4, 50
STRATEGIES = ("unlit", "direct", "sky")
PREAMBLE = """Sky sampling (DESIGN.md 19): Scene.irradiance and Scene.radiance with lights=emitters(objs) + [SKY], direct=True against the same
calls with the lamps only and without lights, under the procedural sky and under the studio map -- the rate, and at equal samples the
per-ray variance and variance x time.
Every block below is one call of scripts/ubench/sky_bench.py CONFIG on one MI355X box; the lines are the script's own output (its
docstring says how the rays are made, what A B B A means here and how the variance is taken).

"""
LINES = []


def say(obj):
    line = json.dumps(obj)
    LINES.append(line)
    print(line, flush=True)


def source_hash():
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "rayrs_amd", "csrc", "*.[ch]*")) + glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if f.endswith((".o", ".s")):
            continue
        h.update(os.path.relpath(f, ROOT).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def unit_vectors(n, gen):
    v = torch.randn((n, 3), dtype=torch.float64, device="cuda:0", generator=gen)
    return v / v.norm(dim=1, keepdim=True)


def leg_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPEATS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / REPEATS


def abba(a, b):
    """ms per call of a and of b: A B B A, the two legs of each averaged."""
    a(), b()
    torch.cuda.synchronize()
    a1, b1, b2, a2 = leg_ms(a), leg_ms(b), leg_ms(b), leg_ms(a)
    return (a1 + a2) / 2.0, (b1 + b2) / 2.0, [round(x, 3) for x in (a1, b1, b2, a2)]


def run_set(scene, sky_map, name, a, b, samples, bias, fast, lights):
    def call(how, seed=0x5EED, queries=False):
        kw = dict(samples=samples, max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast, queries=queries, seed=seed,
                  lights=None if how == "unlit" else lights + [SKY] if how == "sky" else lights, direct=how != "unlit")
        return scene.irradiance(a, b, bias=bias, **kw) if name == "irradiance" else scene.radiance(a, b, **kw)

    case = {"map": sky_map, "set": name, "walk": "fast" if fast else "default", "items": len(a), "samples": samples, "lights": len(lights)}
    rays = {how: int(call(how, queries=True)[1].to(torch.int64).sum()) for how in STRATEGIES}
    ms, legs, unlit_legs = {}, {}, []
    for how in ("direct", "sky"):
        ms[how], unlit_ms, legs[how] = abba(lambda: call(how), lambda: call("unlit"))
        unlit_legs.append(unlit_ms)
    ms["unlit"] = sum(unlit_legs) / len(unlit_legs)
    say({**case, "a": "rate", "mray_s": {how: round(rays[how] / ms[how] / 1e3, 1) for how in STRATEGIES},
         "ms": {how: round(ms[how], 3) for how in STRATEGIES},
         "ms_over_unlit": {how: round(ms[how] / ms["unlit"], 3) for how in ("direct", "sky")},
         "queries_per_path": {how: round(rays[how] / (len(a) * samples), 3) for how in STRATEGIES}, "legs_ms_ABBA": legs})
    var, finite, mean = {}, {}, {}
    for how in STRATEGIES:
        runs = torch.stack([call(how, seed=0xB0B + k) for k in range(SEEDS)])   # (SEEDS, n, 3)
        finite[how] = torch.isfinite(runs).all(dim=2).all(dim=0)
        var[how], mean[how] = runs.var(dim=0, unbiased=True).sum(dim=1), runs.mean(dim=0)
        del runs
    ok = finite["unlit"] & finite["direct"] & finite["sky"]
    v = {how: float(var[how][ok].mean()) for how in STRATEGIES}
    say({**case, "b": "variance at equal samples", "seeds": SEEDS,
         "rays_with_a_non_finite_answer": {how: int((~finite[how]).sum()) for how in STRATEGIES}, "rays_compared": int(ok.sum()),
         "mean_per_ray_variance": v, "variance_over_unlit": {how: round(v[how] / v["unlit"], 4) for how in ("direct", "sky")},
         "mean_radiance": {how: [round(float(x), 5) for x in mean[how][ok].mean(dim=0)] for how in STRATEGIES},
         "variance_x_ms": {how: v[how] * ms[how] for how in STRATEGIES},
         "variance_x_time_over_unlit": {how: round(v[how] * ms[how] / (v["unlit"] * ms["unlit"]), 4) for how in ("direct", "sky")}})


def bench(config, out):
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_{config}_{os.getuid()}.ply") if config in (3, 5) else None
    cam_args, objs, heur, spp, bounces = scenes.config(config, ply_path=ply) if ply else scenes.config(config)
    lights = rayrs_amd.emitters(objs)
    if not lights:
        raise SystemExit(f"config {config} has no emissive sphere or plane")
    maps = {"procedural": procedural.make_hdri(64, 32), "studio": procedural.make_studio_hdri(64, 32)}
    scenes_by_map = {m: rayrs_amd.Scene(objs, 1e-6, 1e6, heur, hdri, device=0) for m, hdri in maps.items()}
    scene = scenes_by_map["procedural"]
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
    say({"config": config, "aimed_rays": N_RAYS, "points": len(p), "repeats_per_leg": REPEATS, "n_prims": info["n_prims"], "lights": lights,
         "hot_count": info["hot_count"], "root_box_diagonal": round(diag, 4), "max_bounces": BOUNCES, "sample_chunk": CHUNK,
         "command": f"python scripts/ubench/sky_bench.py {config}", "source_hash": source_hash()})
    for sky_map, sc in scenes_by_map.items():
        cells, total = sc.sky_table()
        say({"map": sky_map, "size": [64, 32], "table_total": total, "cells_not_black": int((cells > 0.0).sum()), "cells": int(cells.size),
             "largest_cell_over_mean": round(float(cells.max() / cells.mean()), 2)})
        for fast in (False, True):
            run_set(sc, sky_map, "irradiance", p, n, S_IRR, 1e-4 * diag, fast, lights)
            run_set(sc, sky_map, "radiance", o, d, S_RAD, 0.0, fast, lights)
    fresh = not os.path.exists(out)
    with open(out, "a") as f:
        if fresh:
            f.write(PREAMBLE)
        f.write("\n".join(LINES) + "\n\n")


bench(int(sys.argv[1]) if len(sys.argv) > 1 else 3, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sky_rates.txt"))
