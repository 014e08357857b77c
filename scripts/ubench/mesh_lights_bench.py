"""A mesh-light group as a light of direct lighting (include/rayrs_hip.h MESH LIGHTS) against what there was before it, on config 3's
scene (on the GPU box), on device tensors in the same run, timed with HIP events on torch's current stream.
usage: python scripts/ubench/mesh_lights_bench.py [OUT]   (OUT: default profiles/mesh_lights_rates.txt)

Two cases, each on both walks and on the two sets of profiles/lit_rates.txt (2^18 rays from a sphere around the scene's root box,
each aimed at a random point of the box; "irradiance": at the rays' first hits, S_IRR samples a point; "radiance": on the rays
themselves, S_RAD samples a ray; max_bounces 50, sample_chunk 4):

  "panel":     config 3 as it is, its 3 x 3 lamp a rectangle, under Scene.irradiance / Scene.radiance with lights=[lamp],
               direct=True (A), against config 3 with that lamp built as two emissive triangles, listed as a group, under the same
               calls with lights=[], mesh=group (B).  The same light in two representations: the cost of the table path.
  "icosphere": config 3 with a small emissive icosphere of 320 triangles as its lamp: the group (A) against the unlit calls (B),
               which find such a lamp by BSDF sampling alone -- what there was for a mesh lamp before.

Per case, set and walk: ms a call in A B B A order (each leg REPEATS calls between two events, after a warm-up call of each);
queries a path; the per-ray variance over SEEDS seeds, summed over the three channels, its mean over the rays whose answers are
finite under both; and variance x time, B's over A's.  The means are printed: both estimate the same light (the panel's two
scenes differ in the lamp's back face alone, which nothing sees).

Only comparisons within one run count; boxes differ by a few percent.  No figure is asserted.  The wave's thresholds
(rayrs_lab_radiance_tuning) are the radiance queries' defaults and were not swept for this wave.  Writes OUT (every line it
prints, with the hash of the library's sources)."""
import glob, hashlib, json, os, sys, tempfile
import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one
torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import rayrs_amd
from rayrs_amd import procedural, scenes
from rayrs_amd.api import Emission, Material, Object

REPEATS = 10
SEEDS = 16
N_RAYS = 1 << 18
S_IRR, S_RAD, CHUNK, BOUNCES = 16, 4, 4, 50
PREAMBLE = """Mesh lights (DESIGN.md 22): Scene.irradiance and Scene.radiance with mesh=scene.mesh_lights(...), direct=True -- the same lamp as
a rectangle of direct lighting and as a group of two triangles, and a 320-triangle icosphere lamp as a group against the unlit
calls -- ms a call, queries a path, and at equal samples the per-ray variance and variance x time.
Every block below is one call of scripts/ubench/mesh_lights_bench.py on one MI355X box; the lines are the script's own output (its
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


def run_set(case, sides, name, a, b, samples, bias, fast):
    """sides: {"A": (label, scene, kwargs), "B": ...}: the two calls compared."""
    def call(side, seed=0x5EED, queries=False):
        _, scene, extra = sides[side]
        kw = dict(samples=samples, max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast, queries=queries, seed=seed, **extra)
        return scene.irradiance(a, b, bias=bias, **kw) if name == "irradiance" else scene.radiance(a, b, **kw)

    head = {"case": case, "A": sides["A"][0], "B": sides["B"][0], "set": name, "walk": "fast" if fast else "default", "items": len(a),
            "samples": samples}
    rays = {s: int(call(s, queries=True)[1].to(torch.int64).sum()) for s in "AB"}
    ms_a, ms_b, legs = abba(lambda: call("A"), lambda: call("B"))
    ms = {"A": ms_a, "B": ms_b}
    var, finite, mean = {}, {}, {}
    for s in "AB":
        runs = torch.stack([call(s, seed=0xB0B + k) for k in range(SEEDS)])   # (SEEDS, n, 3)
        finite[s] = torch.isfinite(runs).all(dim=2).all(dim=0)
        var[s], mean[s] = runs.var(dim=0, unbiased=True).sum(dim=1), runs.mean(dim=0)
        del runs
    ok = finite["A"] & finite["B"]
    v = {s: float(var[s][ok].mean()) for s in "AB"}
    say({**head, "ms": {s: round(ms[s], 3) for s in "AB"}, "ms_A_over_B": round(ms["A"] / ms["B"], 3), "legs_ms_ABBA": legs,
         "queries_per_path": {s: round(rays[s] / (len(a) * samples), 3) for s in "AB"},
         "mray_s": {s: round(rays[s] / ms[s] / 1e3, 1) for s in "AB"}, "seeds": SEEDS,
         "rays_with_a_non_finite_answer": {s: int((~finite[s]).sum()) for s in "AB"}, "rays_compared": int(ok.sum()),
         "mean_per_ray_variance": v, "variance_A_over_B": round(v["A"] / v["B"], 4),
         "mean_radiance": {s: [round(float(x), 5) for x in mean[s][ok].mean(dim=0)] for s in "AB"},
         "variance_x_time_A_over_B": round(v["A"] * ms["A"] / (v["B"] * ms["B"]), 4)})


def bench(out):
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_3_{os.getuid()}.ply")
    cam_args, objs, heur, spp, bounces = scenes.config(3, ply_path=ply)
    lamp = rayrs_amd.emitters(objs)
    assert len(lamp) == 1 and objs[-1].kind == "plane"
    rect = objs[-1]
    hdri = procedural.make_hdri(64, 32)
    # the same lamp as two triangles (their normal faces down, as the rectangle's does)
    y, lo, hi = rect.pos, rect.umin, rect.umax
    quad = Object.from_triangles(np.array([(lo, y, lo), (hi, y, lo), (hi, y, hi), (lo, y, hi)], dtype=np.float64),
                                 np.array([(0, 1, 2), (0, 2, 3)], dtype=np.uint32), rect.mat, rect.emission)
    # a small emissive icosphere where the lamp was: the same power as the rectangle's one face, spread over its area
    v, f = procedural.icosphere(2)
    ball_area = 4.0 * np.pi * 0.35 ** 2
    ball = Object.from_triangles((v * 0.35 + (0.0, y - 0.5, 0.0)).astype(np.float32), f.astype(np.uint32), rect.mat,
                                 Emission.new(rect.emission.strength * (hi - lo) ** 2 / ball_area, rect.emission.color))
    built = {"rectangle": list(objs), "two_triangles": list(objs[:-1]) + quad, "icosphere": list(objs[:-1]) + ball}
    sc = {k: rayrs_amd.Scene(o, 1e-6, 1e6, heur, hdri, device=0) for k, o in built.items()}
    groups = {k: sc[k].mesh_lights(rayrs_amd.mesh_emitters(built[k])) for k in ("two_triangles", "icosphere")}
    assert len(groups["two_triangles"]) == 2 and len(groups["icosphere"]) == len(f)
    info = sc["rectangle"].info()
    box = torch.tensor(info["root_box"], dtype=torch.float64, device="cuda:0")
    lo_b, hi_b = box[0::2], box[1::2]
    centre, diag = (lo_b + hi_b) * 0.5, float((hi_b - lo_b).norm())
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0x5EED)
    o = (centre + unit_vectors(N_RAYS, gen) * (0.75 * diag)).contiguous()
    d = (lo_b + torch.rand((N_RAYS, 3), dtype=torch.float64, device="cuda:0", generator=gen) * (hi_b - lo_b) - o).contiguous()
    t, obj, nrm = sc["rectangle"].intersect(o, d, normals=True)
    hit = obj.view(torch.int32) != -1
    p = (o + d * t[:, None])[hit].contiguous()
    n = torch.where((nrm * d).sum(dim=1, keepdim=True) > 0.0, -nrm, nrm)[hit].contiguous()
    say({"config": 3, "aimed_rays": N_RAYS, "points": len(p), "repeats_per_leg": REPEATS, "n_prims": info["n_prims"],
         "hot_count": info["hot_count"], "root_box_diagonal": round(diag, 4), "max_bounces": BOUNCES, "sample_chunk": CHUNK,
         "group_sizes": {k: len(g) for k, g in groups.items()}, "group_areas": {k: g.total for k, g in groups.items()},
         "command": "python scripts/ubench/mesh_lights_bench.py", "source_hash": source_hash()})
    panel = {"A": ("rectangle lamp, direct", sc["rectangle"], dict(lights=lamp, direct=True)),
             "B": ("two-triangle group", sc["two_triangles"], dict(lights=[], direct=True, mesh=groups["two_triangles"]))}
    ico = {"A": ("320-triangle group", sc["icosphere"], dict(lights=[], direct=True, mesh=groups["icosphere"])),
           "B": ("unlit", sc["icosphere"], dict())}
    for case, sides in (("panel", panel), ("icosphere", ico)):
        for fast in (False, True):
            run_set(case, sides, "irradiance", p, n, S_IRR, 1e-4 * diag, fast)
            run_set(case, sides, "radiance", o, d, S_RAD, 0.0, fast)
    fresh = not os.path.exists(out)
    with open(out, "a") as fh:
        if fresh:
            fh.write(PREAMBLE)
        fh.write("\n".join(LINES) + "\n\n")


bench(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mesh_lights_rates.txt"))
