"""Radiance-query rates on a BASELINE.json config's scene (on the GPU box): Scene.irradiance and Scene.radiance on device tensors,
timed with HIP events on torch's current stream.
usage: python scripts/ubench/radiance_bench.py [CONFIG [OUT]]   (CONFIG: default 5, the headline scene; OUT: default profiles/radiance_rates.txt)

Rays, as scripts/ubench/ao_bench.py makes its points: 2^18 rays from a sphere around the scene's root box (radius 1.5
half-diagonals), each aimed at a random point of the box.  Two sets, each on both walks, max_bounces 50:
  "irradiance": Scene.irradiance at the rays' first hits (the normal turned to face the ray that found it), S_IRR samples a point,
                sample_chunk 4, bias 1e-4 diagonals;
  "radiance":   Scene.radiance on the rays themselves, S_RAD samples a ray, sample_chunk 4.
Mray/s = the sum of the call's `queries` (every Bvh::intersect call of its paths) over the time of a call.  Per case, in one process:

  (a) the default thresholds;
  (b) the same kernel refilling only an empty wave and shading only when no lane walks: rayrs_lab_radiance_tuning(1, 64, 0),
      both extremes of the lab knobs;
  (c) rayrs_render of the same scene on the same walk in the same run (1024 x 1024, 4 samples a pixel), the production route's
      yardstick: its rays over its kernel time and over its total time.  Not the same rays: a yardstick, not a comparison of equals.

(a) against (b) in A B B A order (each leg REPEATS calls between two events, after a warm-up call of each).  Then a sweep: each of
refill_below, shade_at and leaf_min over SWEEP with the other two at their defaults, every setting timed in the order given and
again in the reverse order, the two legs averaged; and for (a), (b) and each swept setting the share of lane-turns spent walking
and shading, counted by the lab's instance of the kernel (rayrs_lab_radiance_turns, host buffers, never timed) on the first
TURN_ITEMS rays or points.  The last lines give, per knob and value, the geometric mean over the two sets and the two walks, and
the best: those are the kernel's defaults.  Only comparisons within one run count; boxes differ by a few percent.

On the mesh configs two more sets are measured beside them, never part of that choice: "off_floor_radiance", the rays that hit the
mesh of 2^18 aimed at the box around it, and "off_floor_irradiance", the points where they do -- paths that begin on geometry.

Writes OUT (every line it prints, with the hash of the library's sources)."""
import glob, hashlib, json, math, os, sys, tempfile
import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one
torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import rayrs_amd
from rayrs_amd import procedural, scenes

REPEATS = 20
N_RAYS = 1 << 18
S_IRR, S_RAD, CHUNK, BOUNCES = 16, 4, 4, 50
TURN_ITEMS = 1 << 15
SWEEP = [1, 16, 32, 48, 64]
KNOBS = ("refill_below", "shade_at", "leaf_min")
PREAMBLE = """Radiance queries (DESIGN.md 16): rates of Scene.irradiance and Scene.radiance at the default thresholds, of the same kernel refilling
only an empty wave and shading only when no lane walks, and of rayrs_render on the same scene; a sweep of the three thresholds; the
share of lane-turns spent walking and shading.
Every block below is one call of scripts/ubench/radiance_bench.py CONFIG on one MI355X box; the lines are the script's own output
(its docstring says how the rays are made, what A B B A means here and how the lane-turns are counted).

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


def turn_shares(scene, irradiance, a, b, samples, bias, fast, want_queries):
    """(share of lane-turns spent walking, shading) on host copies of the first TURN_ITEMS rays or points."""
    q, turns = np.zeros(len(a), dtype=np.uint32), np.zeros(3, dtype=np.uint64)
    rayrs_amd._ffi.check(scene._L.rayrs_lab_radiance_turns(scene._h, int(irradiance), a.ctypes.data, b.ctypes.data, len(a), samples, BOUNCES,
                                                            CHUNK, bias, 0x5EED, 0, int(fast), q.ctypes.data, turns.ctypes.data),
                         "rayrs_lab_radiance_turns")
    assert np.array_equal(q, want_queries), "the query counts differ under a threshold"
    return [round(float(turns[k]) / float(turns[0]), 4) if turns[0] else 0.0 for k in (1, 2)]


def run_set(scene, name, a, b, samples, bias, fast, geo, label=None):
    irr = name == "irradiance"

    def call(queries=False):
        if irr:
            return scene.irradiance(a, b, samples=samples, bias=bias, max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast, queries=queries)
        return scene.radiance(a, b, samples=samples, max_bounces=BOUNCES, sample_chunk=CHUNK, fast_traversal=fast, queries=queries)

    def extreme():
        scene.lab_radiance_tuning(1, 64, 0)
        call()
        scene.lab_radiance_tuning(0, 0, 0)

    rad, q = call(queries=True)
    rays = int(q.to(torch.int64).sum())
    rate = lambda ms: round(rays / ms / 1e3, 1)
    ha, hb, hq = a[:TURN_ITEMS].cpu().numpy(), b[:TURN_ITEMS].cpu().numpy(), q[:TURN_ITEMS].cpu().numpy()
    case = {"set": label or name, "walk": "fast" if fast else "default", "items": len(a), "samples": samples, "queries": rays,
            "queries_per_path": round(rays / (len(a) * samples), 3)}
    ms_a, ms_b, legs = abba(call, extreme)
    share_a = turn_shares(scene, irr, ha, hb, samples, bias, fast, hq)
    scene.lab_radiance_tuning(1, 64, 0)
    share_b = turn_shares(scene, irr, ha, hb, samples, bias, fast, hq)
    scene.lab_radiance_tuning(0, 0, 0)
    say({**case, "a_default_mray_s": rate(ms_a), "b_empty_wave_only_mray_s": rate(ms_b), "a_over_b": round(ms_b / ms_a, 3), "legs_ms_ABBA": legs,
         "a_lane_turns_walking_shading": share_a, "b_lane_turns_walking_shading": share_b})
    for k, knob in enumerate(KNOBS):
        ms = {v: [] for v in SWEEP}
        for order in (SWEEP, SWEEP[::-1]):
            for v in order:
                scene.lab_radiance_tuning(*[v if j == k else 0 for j in range(3)])
                call()
                ms[v].append(leg_ms(call))
        share = {}
        for v in SWEEP:
            scene.lab_radiance_tuning(*[v if j == k else 0 for j in range(3)])
            share[v] = turn_shares(scene, irr, ha, hb, samples, bias, fast, hq)
        scene.lab_radiance_tuning(0, 0, 0)
        for v in SWEEP:
            geo[knob][v].append(rays / (sum(ms[v]) / 2.0) / 1e3)
        say({**case, "sweep": knob, "mray_s": {str(v): rate(sum(ms[v]) / 2.0) for v in SWEEP},
             "legs_ms": {str(v): [round(x, 3) for x in ms[v]] for v in SWEEP}, "lane_turns_walking_shading": {str(v): share[v] for v in SWEEP}})


def bench(config, out):
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_{config}_{os.getuid()}.ply") if config in (3, 5) else None
    cam_args, objs, heur, spp, bounces = scenes.config(config, ply_path=ply) if ply else scenes.config(config)
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
    say({"config": config, "aimed_rays": N_RAYS, "points": len(p), "repeats_per_leg": REPEATS, "n_prims": info["n_prims"], "compact": info["compact"],
         "hot_count": info["hot_count"], "root_box_diagonal": round(diag, 4), "max_bounces": BOUNCES, "sample_chunk": CHUNK,
         "source_hash": source_hash()})
    geo = {knob: {v: [] for v in SWEEP} for knob in KNOBS}
    geo_off = {knob: {v: [] for v in SWEEP} for knob in KNOBS}
    off = None
    if config in (3, 5):
        # beside the sets the defaults are chosen on, as ao_bench.py's off_floor: rays aimed at the box around the hits that are not
        # the floor's, and the points where they meet the mesh -- paths that begin on geometry
        on_mesh = p[obj.view(torch.int32)[hit] > 0]
        m_lo, m_hi = on_mesh.min(dim=0).values, on_mesh.max(dim=0).values
        o2 = (centre + unit_vectors(N_RAYS, gen) * (0.75 * diag)).contiguous()
        d2 = (m_lo + torch.rand((N_RAYS, 3), dtype=torch.float64, device="cuda:0", generator=gen) * (m_hi - m_lo) - o2).contiguous()
        t2, obj2, nrm2 = scene.intersect(o2, d2, normals=True)
        hit2 = obj2.view(torch.int32) > 0
        off = (o2[hit2].contiguous(), d2[hit2].contiguous(), (o2 + d2 * t2[:, None])[hit2].contiguous(),
               torch.where((nrm2 * d2).sum(dim=1, keepdim=True) > 0.0, -nrm2, nrm2)[hit2].contiguous())
        say({"set": "off_floor", "aimed_rays": N_RAYS, "rays_and_points": len(off[0])})
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, 1024, 1024))
    for fast in (False, True):
        run_set(scene, "irradiance", p, n, S_IRR, 1e-4 * diag, fast, geo)
        run_set(scene, "radiance", o, d, S_RAD, 0.0, fast, geo)
        if off is not None:
            run_set(scene, "irradiance", off[2], off[3], S_IRR, 1e-4 * diag, fast, geo_off, "off_floor_irradiance")
            run_set(scene, "radiance", off[0], off[1], S_RAD, 0.0, fast, geo_off, "off_floor_radiance")
        rayrs_amd.render(scene, cam, 4, BOUNCES, sample_chunk=CHUNK, fast_traversal=fast)
        st = [rayrs_amd.render(scene, cam, 4, BOUNCES, sample_chunk=CHUNK, fast_traversal=fast)[1] for _ in range(3)]
        say({"c_render": "1024x1024x4", "walk": "fast" if fast else "default", "rays": st[0]["rays"],
             "mray_s_kernel_time": [round(s["rays"] / s["kernel_ms"] / 1e3, 1) for s in st],
             "mray_s_total_time": [round(s["rays"] / s["total_ms"] / 1e3, 1) for s in st]})
    best = {}
    for knob in KNOBS:
        g = {v: math.exp(sum(math.log(x) for x in geo[knob][v]) / len(geo[knob][v])) for v in SWEEP}
        best[knob] = max(SWEEP, key=lambda v: g[v])
        say({"sweep": knob, "geometric_mean_over_sets_and_walks_mray_s": {str(v): round(g[v], 1) for v in SWEEP}, "best": best[knob]})
        if off is not None:
            g = {v: math.exp(sum(math.log(x) for x in geo_off[knob][v]) / len(geo_off[knob][v])) for v in SWEEP}
            say({"sweep": knob, "off_floor_geometric_mean_over_sets_and_walks_mray_s": {str(v): round(g[v], 1) for v in SWEEP},
                 "off_floor_best": max(SWEEP, key=lambda v: g[v])})
    fresh = not os.path.exists(out)
    with open(out, "a") as f:
        if fresh:
            f.write(PREAMBLE)
        f.write("\n".join(LINES) + "\n\n")


bench(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "radiance_rates.txt"))
