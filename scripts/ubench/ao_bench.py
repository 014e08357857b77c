"""Ambient-occlusion rates on a BASELINE.json config's scene (on the GPU box): Scene.ambient_occlusion on device tensors, timed
with HIP events on torch's current stream.
usage: python scripts/ubench/ao_bench.py [CONFIG [OUT]]      (CONFIG: default 5, the headline scene; OUT: default profiles/ao_rates.txt)

Points, as scripts/ubench/query_bench.py makes its ray set (b): 2^18 rays from a sphere around the scene's root box (radius 1.5
half-diagonals), each aimed at a random point of the box; the points are their first hits, the normals FEATURES' normal turned to
face the ray that found it.  S = 16 samples a point, bias 1e-4 diagonals, once with t_max = None and once with a tenth of the
diagonal, on both walks.  Per case, in one process:

  (a) Scene.ambient_occlusion at the default refill_below;
  (b) the same kernel with rayrs_lab_ao_refill(1): a wave takes new items only when none of its lanes walks -- no refill within
      a batch of 64;
  (c) what a caller composes today: Scene.occluded on n x S device-resident cosine rays made with torch from the same points
      (the same distribution, not the same bits); the generation is timed on its own and is NOT in (c)'s rate.

(a) against (b) and (a) against (c) in A B B A order (each leg REPEATS calls between two events, after a warm-up call of each):
Mray/s = n x S rays over the mean of a side's two legs.  Then a sweep of refill_below over SWEEP, every setting timed in the
order given and again in the reverse order, the two legs averaged; and for every setting the share of lane-turns spent walking,
counted by the lab's instance of the kernel (rayrs_lab_ao_turns, host buffers, never timed): lane-turns in which a lane advanced
its walk over 64 x the wave's step turns; mean_steps_per_ray is those lane-turns over n x S (records visited + leaf groups tested
by a ray, the same under every setting).  Only comparisons within one run count; boxes differ by a few percent.

That set is "all_hits".  On the mesh configs a second set follows, "off_floor": the hits that are not the floor's of 2^20 rays
aimed at the box around such hits, whose rays meet geometry.  The last line gives, per threshold, the geometric mean of the two
sets' geometric means, and the best: that is the kernel's default.

Writes OUT (every line it prints, with the hash of the library's sources)."""
import glob, hashlib, json, math, os, sys, tempfile
import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one
torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import rayrs_amd
from rayrs_amd import procedural, scenes

REPEATS = 300
N_RAYS = 1 << 18
OFF_FLOOR_RAYS = 1 << 20
S = 16
SWEEP = [1, 16, 32, 48, 56, 64]   # 1 is the refill effectively off
PREAMBLE = """Ambient occlusion (DESIGN.md 15): rates of Scene.ambient_occlusion, of the same kernel without its refill, and of the composed path
(torch-made rays through Scene.occluded); a sweep of refill_below; the share of lane-turns spent walking.
Every block below is one call of scripts/ubench/ao_bench.py CONFIG on one MI355X box; the lines are the script's own output
(its docstring says how the points are made, what A B B A means here and how the lane-turns are counted).
The default refill_below (ao_kernels.h AO_REFILL_BELOW) is the threshold with the best geometric mean over BOTH point sets, the
block's last line.  On all_hits alone -- rays that leave an open floor: under one step a ray, 0.3 % occluded -- no threshold beats
(b), a wave that refills only when none of its lanes walks; on off_floor every threshold from 16 to 56 does.

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


def cosine_rays(p, n, bias, gen):
    """n x S cosine-distributed rays around the normals, with torch: the operation's distribution, not its bits."""
    pp, nn = p.repeat_interleave(S, dim=0), n.repeat_interleave(S, dim=0)
    u = torch.rand(len(pp), dtype=torch.float64, device="cuda:0", generator=gen)
    phi = 2.0 * math.pi * torch.rand(len(pp), dtype=torch.float64, device="cuda:0", generator=gen)
    first = nn[:, 0].abs() > nn[:, 1].abs()
    zero = torch.zeros_like(u)
    e1 = torch.where(first[:, None], torch.stack((nn[:, 2], zero, -nn[:, 0]), dim=1), torch.stack((zero, nn[:, 2], -nn[:, 1]), dim=1))
    e1 = e1 / e1.norm(dim=1, keepdim=True)
    e2 = torch.linalg.cross(nn, e1)
    e2 = e2 / e2.norm(dim=1, keepdim=True)
    su = u.sqrt()
    d = e1 * (phi.cos() * su)[:, None] + e2 * (phi.sin() * su)[:, None] + nn * (1.0 - u).sqrt()[:, None]
    return (pp + nn * bias).contiguous(), d.contiguous()


def walking_share(scene, p, n, t_max, bias, fast):
    cnt, turns = np.zeros(len(p), dtype=np.uint32), np.zeros(2, dtype=np.uint64)
    rayrs_amd._ffi.check(scene._L.rayrs_lab_ao_turns(scene._h, p.ctypes.data, n.ctypes.data, len(p), S, float("inf") if t_max is None else t_max,
                                                      bias, 0x5EED, 0, int(fast), cnt.ctypes.data, turns.ctypes.data), "rayrs_lab_ao_turns")
    return round(float(turns[1]) / float(turns[0]), 4) if turns[0] else 0.0, round(float(turns[1]) / (len(p) * S), 3), cnt


def aimed_points(scene, lo, hi, centre, diag, n_rays, gen, off_floor, aim_lo=None, aim_hi=None):
    """First hits of n_rays rays from a sphere around the root box, each aimed at a random point of it (or of the box aim_lo ..
    aim_hi), normals turned against the ray; off_floor: only those that are not object 0 (the mesh configs' floor)."""
    aim_lo, aim_hi = (lo, hi) if aim_lo is None else (aim_lo, aim_hi)
    o_a = (centre + unit_vectors(n_rays, gen) * (0.75 * diag)).contiguous()
    d_a = (aim_lo + torch.rand((n_rays, 3), dtype=torch.float64, device="cuda:0", generator=gen) * (aim_hi - aim_lo) - o_a).contiguous()
    t, obj, nrm = scene.intersect(o_a, d_a, normals=True)
    hit = (obj.view(torch.int32) > 0) if off_floor else (obj.view(torch.int32) != -1)
    p = (o_a + d_a * t[:, None])[hit].contiguous()
    return p, torch.where((nrm * d_a).sum(dim=1, keepdim=True) > 0.0, -nrm, nrm)[hit].contiguous()


def run_set(scene, name, p, n, diag, gen, compare):
    """Every case of a point set: (a) (b) (c) if compare, the sweep and the lane-turn shares.  Returns the sweep's rates per
    threshold, the geometric mean over the set's four cases."""
    bias, rays = 1e-4 * diag, len(p) * S
    hp, hn = p.cpu().numpy(), n.cpu().numpy()
    rate = lambda ms: round(rays / ms / 1e3, 1)
    sweep_rates = {r: [] for r in SWEEP}
    for t_max in (None, 0.1 * diag):
        for fast in (False, True):
            case = {"points_set": name, "t_max": "none" if t_max is None else round(t_max, 4), "walk": "fast" if fast else "default"}
            ao = lambda: scene.ambient_occlusion(p, n, samples=S, t_max=t_max, bias=bias, fast_traversal=fast)

            def ao_no_refill():
                scene.lab_ao_refill(1)
                scene.ambient_occlusion(p, n, samples=S, t_max=t_max, bias=bias, fast_traversal=fast)
                scene.lab_ao_refill(0)

            vis, cnt = scene.ambient_occlusion(p, n, samples=S, t_max=t_max, bias=bias, fast_traversal=fast, counts=True)
            if compare:
                ms_a, ms_b, legs = abba(ao, ao_no_refill)
                # (c): the rays once for the timed legs; their generation timed on its own
                o_c, d_c = cosine_rays(p, n, bias, gen)
                m_c = None if t_max is None else torch.full((rays,), t_max, dtype=torch.float64, device="cuda:0")
                torch.cuda.synchronize()
                gen_ms = leg_ms(lambda: cosine_rays(p, n, bias, gen))
                occ_c = scene.occluded(o_c, d_c, m_c, fast_traversal=fast)
                ms_a2, ms_c, legs2 = abba(ao, lambda: scene.occluded(o_c, d_c, m_c, fast_traversal=fast))
                say({**case, "occluded_fraction": round(float(cnt.double().sum()) / rays, 4),
                     "occluded_fraction_composed": round(float(occ_c.double().mean()), 4),
                     "a_ao_default_mray_s": rate(ms_a), "b_ao_no_refill_mray_s": rate(ms_b), "a_over_b": round(ms_b / ms_a, 3), "legs_ms_ABBA": legs,
                     "a_ao_default_mray_s_second_pair": rate(ms_a2), "c_composed_occluded_mray_s": rate(ms_c), "a_over_c": round(ms_c / ms_a2, 3),
                     "legs_ms_ABBA_second_pair": legs2, "c_ray_generation_ms": round(gen_ms, 3),
                     "c_with_generation_mray_s": rate(ms_c + gen_ms)})
            # the sweep: every setting forwards, then backwards
            ms = {r: [] for r in SWEEP}
            ao()
            torch.cuda.synchronize()
            for order in (SWEEP, SWEEP[::-1]):
                for r in order:
                    scene.lab_ao_refill(r)
                    ao()
                    ms[r].append(leg_ms(ao))
            scene.lab_ao_refill(0)
            share, steps = {}, 0.0
            for r in SWEEP:
                scene.lab_ao_refill(r)
                share[r], steps, c = walking_share(scene, hp, hn, t_max, bias, fast)
                assert np.array_equal(c, cnt.cpu().numpy()), ("counts differ at refill_below", r)
            scene.lab_ao_refill(0)
            for r in SWEEP:
                sweep_rates[r].append(rays / (sum(ms[r]) / 2.0) / 1e3)
            say({**case, "occluded_fraction": round(float(cnt.double().sum()) / rays, 4),
                 "sweep_refill_below_mray_s": {str(r): rate(sum(ms[r]) / 2.0) for r in SWEEP},
                 "sweep_legs_ms": {str(r): [round(x, 3) for x in ms[r]] for r in SWEEP},
                 "lane_turns_walking_share": {str(r): share[r] for r in SWEEP}, "mean_steps_per_ray": steps})
    geo = {r: math.exp(sum(math.log(x) for x in v) / len(v)) for r, v in sweep_rates.items()}
    say({"points_set": name, "sweep_geometric_mean_mray_s": {str(r): round(geo[r], 1) for r in SWEEP},
         "best_refill_below": max(SWEEP, key=lambda r: geo[r])})
    return geo


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
    p, n = aimed_points(scene, lo, hi, centre, diag, N_RAYS, gen, False)
    say({"config": config, "aimed_rays": N_RAYS, "points": len(p), "samples": S, "repeats_per_leg": REPEATS, "n_prims": info["n_prims"],
         "compact": info["compact"], "hot_count": info["hot_count"], "root_box_diagonal": round(diag, 4), "bias": 1e-4 * diag,
         "source_hash": source_hash()})
    geos = [run_set(scene, "all_hits", p, n, diag, gen, True)]
    if config in (3, 5):
        # beside the set the default is chosen on: the points on the mesh only, whose rays meet geometry
        # (the floor fills the root box: first find the rest with rays aimed at the root box, then aim at the box around it)
        p, n = aimed_points(scene, lo, hi, centre, diag, OFF_FLOOR_RAYS, gen, True)
        p, n = aimed_points(scene, lo, hi, centre, diag, OFF_FLOOR_RAYS, gen, True, p.min(dim=0).values, p.max(dim=0).values)
        say({"points_set": "off_floor", "aimed_rays": OFF_FLOOR_RAYS, "points": len(p)})
        geos.append(run_set(scene, "off_floor", p, n, diag, gen, True))
    both = {r: math.exp(sum(math.log(g[r]) for g in geos) / len(geos)) for r in SWEEP}
    say({"points_sets": len(geos), "sweep_geometric_mean_over_sets_mray_s": {str(r): round(both[r], 1) for r in SWEEP},
         "best_refill_below_over_sets": max(SWEEP, key=lambda r: both[r])})
    fresh = not os.path.exists(out)
    with open(out, "a") as f:
        if fresh:
            f.write(PREAMBLE)
        f.write("\n".join(LINES) + "\n\n")


bench(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ao_rates.txt"))
