"""A mesh-light group chosen by a light tree (include/rayrs_hip.h LIGHT TREE) against the group drawn uniformly by area (MESH LIGHTS)
and against the unlit calls, on config 3's scene (on the GPU box), on device tensors in the same run, timed with HIP events on
torch's current stream.
usage: python scripts/ubench/tree_lights_bench.py [OUT]   (OUT: default profiles/tree_lights_rates.txt)

Two cases, each on both walks and on the two sets of profiles/lit_rates.txt (2^18 rays from a sphere around the scene's root box,
each aimed at a random point of the box; "irradiance": at the rays' first hits, S_IRR samples a point; "radiance": on the rays
themselves, S_RAD samples a ray; max_bounces 50, sample_chunk 4):

  "many lamps": config 3 with its rectangle lamp replaced by an 8 x 8 grid of emissive level-1 icospheres (80 triangles each,
                5,120 listed) half a unit below the rectangle's height, spread over the middle 80 % of the root box in x and z.
                The lamps alternate between emission e and 16 e, e chosen so that their total power is the rectangle's one
                face's.  What the tree is for: the near lamps and the bright ones matter, and uniform choice knows neither.
  "one lamp":   the single 320-triangle icosphere lamp of profiles/mesh_lights_rates.txt.  The tree can gain nothing on the
                selection here -- one compact lamp of one emission -- and pays for its descent; half the draws still land on the
                far side of the closed two-sided lamp.

Per case, set and walk, three legs: T the tree group, A the area group, U the unlit calls.  ms a call in T A U U A T order (each
leg REPEATS calls between two events, after a warm-up call of each; the two legs of a side averaged); queries a path; the per-ray
variance over SEEDS seeds, summed over the three channels, its mean over the rays whose answers are finite under all three; and
variance x time, each against the others.  The means of the three are printed with the standard error of their differences
(from the per-ray variances: sqrt(sum over rays of (v_X + v_Y) / SEEDS) / rays): all three estimate the same light.

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
from rayrs_amd.api import Emission, Object

REPEATS = 10
SEEDS = 16
N_RAYS = 1 << 18
S_IRR, S_RAD, CHUNK, BOUNCES = 16, 4, 4, 50
GRID, RADIUS = 8, 0.35
PREAMBLE = """Light tree (DESIGN.md 24): Scene.irradiance and Scene.radiance with mesh=scene.mesh_lights(..., tree=True), direct=True, against the
same group drawn uniformly by area (mesh=scene.mesh_lights(...)) and against the unlit calls -- (a) 64 icosphere lamps of two
emissions, 5,120 listed triangles, and (b) the one 320-triangle lamp of profiles/mesh_lights_rates.txt -- ms a call, queries a
path, and at equal samples the per-ray variance and variance x time.
Every block below is one call of scripts/ubench/tree_lights_bench.py on one MI355X box; the lines are the script's own output (its
docstring says how the rays are made, what T A U U A T means and how the variance is taken).

"""
LINES = []
SIDES = "TAU"


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


def run_set(case, sides, name, a, b, samples, bias, fast):
    """sides: {"T": (label, scene, kwargs), "A": ..., "U": ...}: the three calls compared."""
    def call(side, seed=0x5EED, queries=False):
        _, scene, extra = sides[side]
        kw = dict(samples=samples, max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast, queries=queries, seed=seed, **extra)
        return scene.irradiance(a, b, bias=bias, **kw) if name == "irradiance" else scene.radiance(a, b, **kw)

    head = {"case": case, **{s: sides[s][0] for s in SIDES}, "set": name, "walk": "fast" if fast else "default", "items": len(a),
            "samples": samples}
    rays = {s: int(call(s, queries=True)[1].to(torch.int64).sum()) for s in SIDES}
    for s in SIDES:
        call(s)
    torch.cuda.synchronize()
    order = SIDES + SIDES[::-1]   # T A U U A T
    legs = [leg_ms(lambda s=s: call(s)) for s in order]
    ms = {s: (legs[i] + legs[5 - i]) / 2.0 for i, s in enumerate(SIDES)}
    var, finite, mean = {}, {}, {}
    for s in SIDES:
        runs = torch.stack([call(s, seed=0xB0B + k) for k in range(SEEDS)])   # (SEEDS, n, 3)
        finite[s] = torch.isfinite(runs).all(dim=2).all(dim=0)
        var[s], mean[s] = runs.var(dim=0, unbiased=True), runs.mean(dim=0)
        del runs
    ok = finite["T"] & finite["A"] & finite["U"]
    n_ok = int(ok.sum())
    v = {s: float(var[s][ok].sum(dim=1).mean()) for s in SIDES}
    m = {s: mean[s][ok].mean(dim=0) for s in SIDES}
    pairs = (("T", "A"), ("T", "U"), ("A", "U"))
    se = {x + y: torch.sqrt(((var[x][ok] + var[y][ok]) / SEEDS).sum(dim=0)) / n_ok for x, y in pairs}
    say({**head, "ms": {s: round(ms[s], 3) for s in SIDES}, "legs_ms_TAUUAT": [round(x, 3) for x in legs],
         "ms_ratio": {x + "_over_" + y: round(ms[x] / ms[y], 3) for x, y in pairs},
         "queries_per_path": {s: round(rays[s] / (len(a) * samples), 3) for s in SIDES},
         "mray_s": {s: round(rays[s] / ms[s] / 1e3, 1) for s in SIDES}, "seeds": SEEDS,
         "rays_with_a_non_finite_answer": {s: int((~finite[s]).sum()) for s in SIDES}, "rays_compared": n_ok,
         "mean_per_ray_variance": v, "variance_ratio": {x + "_over_" + y: round(v[x] / v[y], 4) for x, y in pairs},
         "variance_x_time_ratio": {x + "_over_" + y: round(v[x] * ms[x] / (v[y] * ms[y]), 4) for x, y in pairs},
         "mean_radiance": {s: [round(float(x), 5) for x in m[s]] for s in SIDES},
         "mean_difference_over_its_standard_error": {x + "_minus_" + y: [round(float(q), 2) for q in (m[x] - m[y]) / se[x + y]]
                                                     for x, y in pairs}})


def bench(out):
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_3_{os.getuid()}.ply")
    cam_args, objs, heur, spp, bounces = scenes.config(3, ply_path=ply)
    lamp = rayrs_amd.emitters(objs)
    assert len(lamp) == 1 and objs[-1].kind == "plane"
    rect = objs[-1]
    hdri = procedural.make_hdri(64, 32)
    y, lo, hi = rect.pos, rect.umin, rect.umax
    power = rect.emission.strength * (hi - lo) ** 2   # (of the rectangle's one face, per unit of colour)
    ball_area = 4.0 * np.pi * RADIUS ** 2
    plain = rayrs_amd.Scene(list(objs), 1e-6, 1e6, heur, hdri, device=0)
    info = plain.info()
    box = np.array(info["root_box"], dtype=np.float64)
    # (a) 64 lamps of two emissions over the floor
    v1, f1 = procedural.icosphere(1)
    assert len(f1) == 80
    e = power / ((GRID * GRID // 2) * 17.0 * ball_area)
    xs = (box[0] + box[1]) * 0.5 + np.linspace(-0.4, 0.4, GRID) * (box[1] - box[0])
    zs = (box[4] + box[5]) * 0.5 + np.linspace(-0.4, 0.4, GRID) * (box[5] - box[4])
    lamps = []
    for i, x in enumerate(xs):
        for k, z in enumerate(zs):
            strength = e * (16.0 if (i + k) % 2 else 1.0)
            lamps += Object.from_triangles((v1 * RADIUS + (x, y - 0.5, z)).astype(np.float32), f1.astype(np.uint32), rect.mat,
                                           Emission.new(strength, rect.emission.color))
    # (b) the one lamp of profiles/mesh_lights_rates.txt
    v2, f2 = procedural.icosphere(2)
    ball = Object.from_triangles((v2 * RADIUS + (0.0, y - 0.5, 0.0)).astype(np.float32), f2.astype(np.uint32), rect.mat,
                                 Emission.new(power / ball_area, rect.emission.color))
    built = {"many lamps": list(objs[:-1]) + lamps, "one lamp": list(objs[:-1]) + ball}
    sc = {k: rayrs_amd.Scene(o, 1e-6, 1e6, heur, hdri, device=0) for k, o in built.items()}
    listed = {k: rayrs_amd.mesh_emitters(built[k]) for k in built}
    area = {k: sc[k].mesh_lights(listed[k]) for k in built}
    tree = {k: sc[k].mesh_lights(listed[k], tree=True) for k in built}
    assert len(tree["many lamps"]) == GRID * GRID * 80 and len(tree["one lamp"]) == len(f2)
    box_t = torch.tensor(box, dtype=torch.float64, device="cuda:0")
    lo_b, hi_b = box_t[0::2], box_t[1::2]
    centre, diag = (lo_b + hi_b) * 0.5, float((hi_b - lo_b).norm())
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0x5EED)
    o = (centre + unit_vectors(N_RAYS, gen) * (0.75 * diag)).contiguous()
    d = (lo_b + torch.rand((N_RAYS, 3), dtype=torch.float64, device="cuda:0", generator=gen) * (hi_b - lo_b) - o).contiguous()
    t, obj, nrm = plain.intersect(o, d, normals=True)
    hit = obj.view(torch.int32) != -1
    p = (o + d * t[:, None])[hit].contiguous()
    n = torch.where((nrm * d).sum(dim=1, keepdim=True) > 0.0, -nrm, nrm)[hit].contiguous()
    powers = {k: tree[k].powers() for k in built}
    say({"config": 3, "aimed_rays": N_RAYS, "points": len(p), "repeats_per_leg": REPEATS, "n_prims": {k: sc[k].info()["n_prims"] for k in built},
         "root_box": [round(float(x), 3) for x in box], "root_box_diagonal": round(diag, 4), "max_bounces": BOUNCES, "sample_chunk": CHUNK,
         "group_sizes": {k: len(g) for k, g in tree.items()}, "group_areas": {k: g.total for k, g in area.items()},
         "group_powers": {k: float(w.sum()) for k, w in powers.items()},
         "entry_power_max_over_min": {k: float(w.max() / w[w > 0.0].min()) for k, w in powers.items()},
         "tree_depth_max": {k: int(tree[k].paths()[1].max()) for k in built}, "rectangle_power": power * float(sum(rect.emission.color)),
         "command": "python scripts/ubench/tree_lights_bench.py", "source_hash": source_hash()})
    for case in built:
        sides = {"T": ("tree group", sc[case], dict(lights=[], direct=True, mesh=tree[case])),
                 "A": ("area group", sc[case], dict(lights=[], direct=True, mesh=area[case])),
                 "U": ("unlit", sc[case], dict())}
        for fast in (False, True):
            run_set(case, sides, "irradiance", p, n, S_IRR, 1e-4 * diag, fast)
            run_set(case, sides, "radiance", o, d, S_RAD, 0.0, fast)
    fresh = not os.path.exists(out)
    with open(out, "a") as fh:
        if fresh:
            fh.write(PREAMBLE)
        fh.write("\n".join(LINES) + "\n\n")


bench(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tree_lights_rates.txt"))
