"""Light sampling against the unlit radiance queries on a BASELINE.json config's scene (on the GPU box): Scene.irradiance and
Scene.radiance with lights=emitters(objs) and without, on the same device tensors in the same run, timed with HIP events on
torch's current stream.
usage: python scripts/ubench/lit_bench.py [CONFIG [OUT]]   (CONFIG: default 3, the mesh under an area light; OUT: default profiles/lit_rates.txt)

Rays, as scripts/ubench/radiance_bench.py makes them: 2^18 rays from a sphere around the scene's root box (radius 1.5
half-diagonals), each aimed at a random point of the box.  Two sets, each on both walks, max_bounces 50, sample_chunk 4:
  "irradiance": at the rays' first hits (the normal turned to face the ray that found it), S_IRR samples a point, bias 1e-4 diagonals;
  "radiance":   on the rays themselves, S_RAD samples a ray.
Per set and walk:

  (a) the rate.  Mray/s = the sum of the call's `queries` (every Bvh::intersect call of its paths) over the time of a call, lit
      (A) against unlit (B) in A B B A order (each leg REPEATS calls between two events, after a warm-up call of each): what the
      four-draw arm and the K density tests cost.  The two make different paths, so queries per path are given beside the rates,
      and ms per call is the figure that (b) multiplies.
  (b) the noise at equal samples.  The call is repeated with SEEDS seeds; a ray's variance is the variance of its answer over
      the seeds, summed over the three channels, and the figure is the mean over the rays whose answers are all finite (the rest
      are counted: a Lambertian rectangle of the list that a path scatters on can draw itself, and the operation then divides 0
      by 0 -- include/rayrs_hip.h LIGHT SAMPLING).  variance x time = that mean times (a)'s ms per call: below 1 as a ratio of
      lit to unlit, light sampling reaches a given noise sooner.

Only comparisons within one run count; boxes differ by a few percent.  Writes OUT (every line it prints, with the hash of the
library's sources)."""
import glob, hashlib, json, os, sys, tempfile
import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one
torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import rayrs_amd
from rayrs_amd import procedural, scenes

REPEATS = 10
SEEDS = 16
N_RAYS = 1 << 18
S_IRR, S_RAD, CHUNK, BOUNCES = 16, 4, 4, 50
PREAMBLE = """Light sampling (DESIGN.md 17): Scene.irradiance and Scene.radiance with lights=emitters(objs) against the same calls without
lights -- the rate, and at equal samples the per-ray variance and variance x time.
Every block below is one call of scripts/ubench/lit_bench.py CONFIG on one MI355X box; the lines are the script's own output (its
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


def run_set(scene, name, a, b, samples, bias, fast, lights):
    def call(lit, seed=0x5EED, queries=False):
        kw = dict(samples=samples, max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast, queries=queries, seed=seed,
                  lights=lights if lit else None)
        return scene.irradiance(a, b, bias=bias, **kw) if name == "irradiance" else scene.radiance(a, b, **kw)

    case = {"set": name, "walk": "fast" if fast else "default", "items": len(a), "samples": samples, "lights": len(lights)}
    rays = {lit: int(call(lit, queries=True)[1].to(torch.int64).sum()) for lit in (True, False)}
    ms_lit, ms_unlit, legs = abba(lambda: call(True), lambda: call(False))
    rate = lambda n, ms: round(n / ms / 1e3, 1)
    say({**case, "a": "rate", "lit_mray_s": rate(rays[True], ms_lit), "unlit_mray_s": rate(rays[False], ms_unlit),
         "lit_ms": round(ms_lit, 3), "unlit_ms": round(ms_unlit, 3), "lit_over_unlit_ms": round(ms_lit / ms_unlit, 3),
         "queries_per_path": {"lit": round(rays[True] / (len(a) * samples), 3), "unlit": round(rays[False] / (len(a) * samples), 3)},
         "legs_ms_ABBA": legs})
    var, finite_rays, mean = {}, {}, {}
    for lit in (True, False):
        runs = torch.stack([call(lit, seed=0xB0B + k) for k in range(SEEDS)])   # (SEEDS, n, 3)
        ok = torch.isfinite(runs).all(dim=2).all(dim=0)
        finite_rays[lit] = ok
        var[lit], mean[lit] = runs.var(dim=0, unbiased=True).sum(dim=1), runs.mean(dim=0)
    ok = finite_rays[True] & finite_rays[False]
    v_lit, v_unlit = float(var[True][ok].mean()), float(var[False][ok].mean())
    say({**case, "b": "variance at equal samples", "seeds": SEEDS, "rays_with_a_non_finite_answer": {"lit": int((~finite_rays[True]).sum()),
                                                                                                    "unlit": int((~finite_rays[False]).sum())},
         "rays_compared": int(ok.sum()), "mean_per_ray_variance": {"lit": v_lit, "unlit": v_unlit}, "variance_lit_over_unlit": round(v_lit / v_unlit, 4),
         "mean_radiance": {"lit": [round(float(x), 5) for x in mean[True][ok].mean(dim=0)], "unlit": [round(float(x), 5) for x in mean[False][ok].mean(dim=0)]},
         "variance_x_ms": {"lit": v_lit * ms_lit, "unlit": v_unlit * ms_unlit},
         "variance_x_time_lit_over_unlit": round(v_lit * ms_lit / (v_unlit * ms_unlit), 4)})


def bench(config, out):
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_{config}_{os.getuid()}.ply") if config in (3, 5) else None
    cam_args, objs, heur, spp, bounces = scenes.config(config, ply_path=ply) if ply else scenes.config(config)
    lights = rayrs_amd.emitters(objs)
    if not lights:
        raise SystemExit(f"config {config} has no emissive sphere or plane")
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
    say({"config": config, "aimed_rays": N_RAYS, "points": len(p), "repeats_per_leg": REPEATS, "n_prims": info["n_prims"], "lights": lights,
         "hot_count": info["hot_count"], "root_box_diagonal": round(diag, 4), "max_bounces": BOUNCES, "sample_chunk": CHUNK,
         "command": f"python scripts/ubench/lit_bench.py {config}", "source_hash": source_hash()})
    for fast in (False, True):
        run_set(scene, "irradiance", p, n, S_IRR, 1e-4 * diag, fast, lights)
        run_set(scene, "radiance", o, d, S_RAD, 0.0, fast, lights)
    fresh = not os.path.exists(out)
    with open(out, "a") as f:
        if fresh:
            f.write(PREAMBLE)
        f.write("\n".join(LINES) + "\n\n")


bench(int(sys.argv[1]) if len(sys.argv) > 1 else 3, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lit_rates.txt"))
