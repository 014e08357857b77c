"""SH probes (include/rayrs_hip.h SH PROBES) on config 3's scene (on the GPU box), on device tensors in the same run, timed with HIP
events on torch's current stream.
usage: python scripts/ubench/probes_bench.py [OUT]   (OUT: default profiles/probes_rates.txt)

The probes are rayrs_amd.probe_grid(scene, (16, 4, 16)): 1,024 points at the cell centres of the scene's root box, S = 256 samples
each, sample_chunk 16, max_bounces 50.  Four measurements, each on both walks:

  (a) Scene.probes (F, fused) against the route a user had before it (T, torch): the same number of directions, uniform over the
      sphere, made with torch on the device; Scene.radiance(samples=1) on the 262,144 rays; the nine harmonics and the projection
      as one torch einsum.  ms a call in F T T F order (each leg REPEATS calls between two events, after a warm-up call of each;
      the two legs of a side averaged), Mray/s by the queries made, T's ray generation (directions, origins and basis) timed on
      its own.  The two do not compute the same bits -- T's directions are not the library's keys' --, so the means of c_0 over
      the grid are printed side by side.
  (b) the projection alone (rayrs_lab_probe_project_ms: the two kernels between two HIP events, behind the same paths) and its share
      of the call, at sample_chunk 0, 16 and 1.
  (c) unlit against the lamp (direct=True) against the lamp and SKY: ms a call, queries a path, and the variance of every
      coefficient over SEEDS seeds at equal S -- per k its mean over probes and channels, relative to unlit's.
  (d) one lone probe (the grid's first) at S = 4,096, sample_chunk 0 and 64: the call and the projection alone.  With
      sample_chunk 0 the projection is ONE thread adding 4,096 samples in order.

Only comparisons within one run count; boxes differ by a few percent.  No figure is asserted.  The wave's thresholds
(rayrs_lab_radiance_tuning) are the radiance queries' defaults and were not swept for this item order.  Writes OUT (every line it
prints, with the hash of the library's sources)."""
import glob, hashlib, json, math, os, sys, tempfile
import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one
torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import rayrs_amd
from rayrs_amd import SKY, procedural, scenes

REPEATS = 10
SEEDS = 16
GRID = (16, 4, 16)
S, CHUNK, BOUNCES = 256, 16, 50
S_LONE = 4096
K = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
PREAMBLE = """SH probes (DESIGN.md 25): Scene.probes on a 16 x 4 x 16 grid of probes in config 3's root box, 256 samples each -- (a) against
making the rays with torch, calling Scene.radiance(samples=1) on them and projecting with one einsum, (b) the projection alone
and its share of the call, (c) unlit against the lamp against the lamp and the sky, with the variance of the coefficients over
16 seeds, (d) one lone probe of 4,096 samples.
Every block below is one call of scripts/ubench/probes_bench.py on one MI355X box; the lines are the script's own output (its
docstring says how the legs are ordered and how the variance is taken).

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


def leg_ms(fn, repeats=REPEATS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / repeats


def torch_rays(points, samples, gen):
    """Today's route, its first step: (origins (n * S, 3), directions (n * S, 3), basis (n, S, 9)) made on the device."""
    n = len(points)
    u = torch.rand((n, samples, 2), dtype=torch.float64, device="cuda:0", generator=gen)
    z = 1.0 - 2.0 * u[..., 0]
    r = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
    phi = (2.0 * math.pi) * u[..., 1]
    x, y = r * torch.cos(phi), r * torch.sin(phi)
    d = torch.stack([x, y, z], dim=-1).reshape(n * samples, 3).contiguous()
    o = points[:, None, :].expand(n, samples, 3).reshape(n * samples, 3).contiguous()
    Y = torch.stack([torch.full_like(x, K[0]), K[1] * y, K[1] * z, K[1] * x, K[2] * x * y, K[2] * y * z, K[3] * (3.0 * z * z - 1.0),
                     K[2] * x * z, K[4] * (x * x - y * y)], dim=-1)
    return o, d, Y


def torch_route(scene, points, samples, gen, fast, queries=False):
    o, d, Y = torch_rays(points, samples, gen)
    got = scene.radiance(o, d, samples=1, max_bounces=BOUNCES, fast_traversal=fast, queries=queries)
    L = (got[0] if queries else got).reshape(len(points), samples, 3)
    coeffs = torch.einsum("nsk,nsc->nkc", Y, L) * (4.0 * math.pi / samples)
    return (coeffs, got[1]) if queries else coeffs


def fused_against_torch(scene, points, fast):
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0x5EED)
    kw = dict(samples=S, max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast)
    f_coeffs, f_q = scene.probes(points, queries=True, **kw)
    t_coeffs, t_q = torch_route(scene, points, S, gen, fast, queries=True)
    rays = {"F": int(f_q.to(torch.int64).sum()), "T": int(t_q.to(torch.int64).sum())}
    calls = {"F": lambda: scene.probes(points, **kw), "T": lambda: torch_route(scene, points, S, gen, fast)}
    for c in calls.values():
        c()
    torch.cuda.synchronize()
    legs = [leg_ms(calls[s]) for s in "FTTF"]
    ms = {"F": (legs[0] + legs[3]) / 2.0, "T": (legs[1] + legs[2]) / 2.0}
    gen_ms = leg_ms(lambda: torch_rays(points, S, gen))
    say({"measurement": "a: fused against torch", "walk": "fast" if fast else "default", "probes": len(points), "samples": S,
         "sample_chunk": CHUNK, "F": "Scene.probes", "T": "torch rays + Scene.radiance(samples=1) + einsum",
         "ms": {s: round(v, 3) for s, v in ms.items()}, "legs_ms_FTTF": [round(x, 3) for x in legs],
         "T_ray_generation_ms": round(gen_ms, 3), "F_over_T": round(ms["F"] / ms["T"], 3),
         "queries_per_path": {s: round(rays[s] / (len(points) * S), 3) for s in rays},
         "mray_s": {s: round(rays[s] / ms[s] / 1e3, 1) for s in rays},
         "mean_c0": {"F": [round(float(x), 5) for x in f_coeffs[:, 0].mean(dim=0)], "T": [round(float(x), 5) for x in t_coeffs[:, 0].mean(dim=0)]}})


def projection_share(scene, points, fast):
    for chunk in (0, CHUNK, 1):
        kw = dict(samples=S, max_bounces=BOUNCES, sample_chunk=chunk, fast_traversal=fast)
        scene.probes(points, **kw)
        torch.cuda.synchronize()
        call = leg_ms(lambda: scene.probes(points, **kw))
        proj = scene.lab_probe_project_ms(len(points), S, chunk, REPEATS)
        say({"measurement": "b: the projection alone", "walk": "fast" if fast else "default", "probes": len(points), "samples": S,
             "sample_chunk": chunk, "call_ms": round(call, 3), "projection_ms": round(proj, 4), "projection_share": round(proj / call, 4)})


def lightings(scene, points, lamp, fast):
    sides = {"unlit": dict(), "lamp": dict(lights=lamp, direct=True), "lamp+sky": dict(lights=lamp + [SKY], direct=True)}
    kw = dict(samples=S, max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast)
    ms, qpp, var, mean = {}, {}, {}, {}
    for name, extra in sides.items():
        q = scene.probes(points, queries=True, **kw, **extra)[1]
        qpp[name] = int(q.to(torch.int64).sum()) / (len(points) * S)
        torch.cuda.synchronize()
        ms[name] = leg_ms(lambda: scene.probes(points, **kw, **extra))
        runs = torch.stack([scene.probes(points, seed=0xB0B + k, **kw, **extra) for k in range(SEEDS)])   # (SEEDS, n, 9, 3)
        ok = torch.isfinite(runs).all(dim=0).all(dim=2).all(dim=1)
        var[name] = runs[:, ok].var(dim=0, unbiased=True).mean(dim=(0, 2))    # (9,)
        mean[name] = runs[:, ok, 0].mean(dim=(0, 1))
    say({"measurement": "c: lightings", "walk": "fast" if fast else "default", "probes": len(points), "samples": S, "seeds": SEEDS,
         "ms": {k: round(v, 3) for k, v in ms.items()}, "queries_per_path": {k: round(v, 3) for k, v in qpp.items()},
         "coefficient_variance": {k: [float(f"{float(x):.4g}") for x in v] for k, v in var.items()},
         "variance_over_unlit": {k: [round(float(x), 4) for x in var[k] / var["unlit"]] for k in ("lamp", "lamp+sky")},
         "variance_x_time_over_unlit": {k: [round(float(x) * ms[k] / ms["unlit"], 4) for x in var[k] / var["unlit"]] for k in ("lamp", "lamp+sky")},
         "mean_c0": {k: [round(float(x), 5) for x in v] for k, v in mean.items()}})


def lone_probe(scene, points, fast):
    for chunk in (0, 64):
        kw = dict(samples=S_LONE, max_bounces=BOUNCES, sample_chunk=chunk, fast_traversal=fast)
        scene.probes(points[:1], **kw)
        torch.cuda.synchronize()
        call = leg_ms(lambda: scene.probes(points[:1], **kw))
        proj = scene.lab_probe_project_ms(1, S_LONE, chunk, REPEATS)
        say({"measurement": "d: one lone probe", "walk": "fast" if fast else "default", "samples": S_LONE, "sample_chunk": chunk,
             "call_ms": round(call, 3), "projection_ms": round(proj, 4), "projection_share": round(proj / call, 4)})


def bench(out):
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_3_{os.getuid()}.ply")
    cam_args, objs, heur, spp, bounces = scenes.config(3, ply_path=ply)
    lamp = rayrs_amd.emitters(objs)
    assert len(lamp) == 1
    scene = rayrs_amd.Scene(list(objs), 1e-6, 1e6, heur, procedural.make_hdri(64, 32), device=0)
    grid = rayrs_amd.probe_grid(scene, GRID)
    points = torch.from_numpy(grid).to("cuda:0")
    info = scene.info()
    say({"config": 3, "grid": list(GRID), "probes": len(points), "samples": S, "sample_chunk": CHUNK, "max_bounces": BOUNCES,
         "repeats_per_leg": REPEATS, "n_prims": info["n_prims"], "root_box": [round(float(x), 3) for x in info["root_box"]],
         "command": "python scripts/ubench/probes_bench.py", "source_hash": source_hash()})
    for fast in (False, True):
        fused_against_torch(scene, points, fast)
        projection_share(scene, points, fast)
        lightings(scene, points, lamp, fast)
        lone_probe(scene, points, fast)
    fresh = not os.path.exists(out)
    with open(out, "a") as fh:
        if fresh:
            fh.write(PREAMBLE)
        fh.write("\n".join(LINES) + "\n\n")


bench(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "probes_rates.txt"))
