"""Ray-query rates on a BASELINE.json config's scene (on the GPU box): rayrs_scene_intersect_launch against
rayrs_scene_occluded_launch on the same rays, device tensors on torch's current stream, timed with HIP events.
usage: python scripts/ubench/query_bench.py CONFIG [RAYS]      (RAYS: default 2^22 per set)

Ray set (a): origins on a sphere around the scene's root box (radius 1.5 half-diagonals), each aimed at a random point of the
box.  Ray set (b), ambient-occlusion style: origins are set (a)'s first hits pushed off the surface along the normal (turned to
face the ray that found it) by 1e-4 diagonals, directions uniform on the hemisphere around that normal, unit length, and t_max
a tenth of the root-box diagonal.  Per set, in one process and in A B B A order (intersect, occluded, occluded, intersect; each
leg REPEATS calls between two events, after one warm-up call of each): Mray/s of intersect, of occluded(t_max = inf) and, on
(b), of occluded with the finite t_max -- each against intersect ON THE SAME RAYS IN THE SAME RUN; nothing else is promised.
Both walks (fast_traversal 0 and 1).

How much of a wave idles: 64 consecutive rays share a wave, which runs as long as its slowest lane.  rayrs_lab_query_steps
(rayrs_amd/csrc/rayrs_lab.h) returns every ray's turns of the walk's loop; over the first 2^18 rays of a set,
idle = 1 - sum(steps) / sum over waves(64 * the wave's largest steps) -- lane-turns spent waiting for the wave's slowest ray
(the hot group's test, made by the whole wave at once, is not in it); mean_slowest_lane_steps is what a wave pays: the mean over
waves of the wave's largest steps.  With a NaN t_max no ray stops early: the closest-hit walk's figure on the same tree (on the
fast walk's tree: the closest-hit walk WITHOUT its culling, which rayrs_scene_intersect's fast walk does make).

Writes profiles/query_rates.txt (every line it prints, with the hash of the library's sources)."""
import glob, hashlib, json, os, sys, tempfile
import torch  # before the library is loaded: torch brings its own copy of the HIP runtime, and the two must share one
torch.cuda.set_device(0)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import rayrs_amd
from rayrs_amd import procedural, scenes

REPEATS = 100
PREAMBLE = """Ray queries (DESIGN.md 14): rates of rayrs_scene_intersect_launch and rayrs_scene_occluded_launch, and how much of a wave idles.
Every block below is one call of scripts/ubench/query_bench.py CONFIG on one MI355X box; the lines are the script's own output
(its docstring says how the ray sets are made, what A B B A means here and how idle is counted).

"""
STEP_RAYS = 1 << 18
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


def idle_share(scene, o, d, t_max, fast):
    n = len(o)
    occ, steps = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    rayrs_amd._ffi.check(scene._L.rayrs_lab_query_steps(scene._h, o.ctypes.data, d.ctypes.data, None if t_max is None else t_max.ctypes.data,
                                                         n, int(fast), occ.ctypes.data, steps.ctypes.data), "rayrs_lab_query_steps")
    waves = steps[: n // 64 * 64].reshape(-1, 64).astype(np.float64)
    paid = 64.0 * waves.max(axis=1).sum()
    return {"mean_steps": round(float(steps.mean()), 2), "mean_slowest_lane_steps": round(float(waves.max(axis=1).mean()), 2),
            "idle": round(1.0 - float(waves.sum()) / paid, 4) if paid else 0.0}


def bench(config, n):
    ply = os.path.join(tempfile.gettempdir(), f"film_bench_mesh_{config}_{os.getuid()}.ply") if config in (3, 5) else None
    cam_args, objs, heur, spp, bounces = scenes.config(config, ply_path=ply) if ply else scenes.config(config)
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(64, 32), device=0)
    info = scene.info()
    box = torch.tensor(info["root_box"], dtype=torch.float64, device="cuda:0")
    lo, hi = box[0::2], box[1::2]
    centre, diag = (lo + hi) * 0.5, float((hi - lo).norm())
    say({"config": config, "rays_per_set": n, "repeats_per_leg": REPEATS, "n_prims": info["n_prims"], "compact": info["compact"],
         "hot_count": info["hot_count"], "root_box_diagonal": round(diag, 4), "source_hash": source_hash()})
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0x5EED)
    o_a = (centre + unit_vectors(n, gen) * (0.75 * diag)).contiguous()
    target = lo + torch.rand((n, 3), dtype=torch.float64, device="cuda:0", generator=gen) * (hi - lo)
    d_a = (target - o_a).contiguous()
    for fast in (False, True):
        walk = "fast" if fast else "default"
        t, obj, nrm = scene.intersect(o_a, d_a, fast_traversal=fast, normals=True)
        hit = obj.view(torch.int32) != -1
        ms_i, ms_o, legs = abba(lambda: scene.intersect(o_a, d_a, fast_traversal=fast), lambda: scene.occluded(o_a, d_a, fast_traversal=fast))
        say({"set": "a", "walk": walk, "hit_fraction": round(float(hit.double().mean()), 4), "intersect_mray_s": round(n / ms_i / 1e3, 1),
             "occluded_inf_mray_s": round(n / ms_o / 1e3, 1), "occluded_inf_over_intersect": round(ms_i / ms_o, 3), "legs_ms_ABBA": legs})
        # set (b): from the hits of (a)
        facing = torch.where((nrm * d_a).sum(dim=1, keepdim=True) > 0.0, -nrm, nrm)[hit]
        o_b = ((o_a + d_a * t[:, None])[hit] + facing * (1e-4 * diag)).contiguous()
        d_b = unit_vectors(len(o_b), gen)
        d_b = torch.where((d_b * facing).sum(dim=1, keepdim=True) < 0.0, -d_b, d_b).contiguous()
        m_b = torch.full((len(o_b),), 0.1 * diag, dtype=torch.float64, device="cuda:0")
        nb = len(o_b)
        occ_b = scene.occluded(o_b, d_b, m_b, fast_traversal=fast)
        hit_b = scene.occluded(o_b, d_b, fast_traversal=fast)
        ms_i, ms_o, legs = abba(lambda: scene.intersect(o_b, d_b, fast_traversal=fast), lambda: scene.occluded(o_b, d_b, fast_traversal=fast))
        ms_i2, ms_f, legs2 = abba(lambda: scene.intersect(o_b, d_b, fast_traversal=fast), lambda: scene.occluded(o_b, d_b, m_b, fast_traversal=fast))
        say({"set": "b", "walk": walk, "rays": nb, "hit_fraction": round(float(hit_b.double().mean()), 4),
             "occluded_fraction_at_t_max": round(float(occ_b.double().mean()), 4), "intersect_mray_s": round(nb / ms_i / 1e3, 1),
             "occluded_inf_mray_s": round(nb / ms_o / 1e3, 1), "occluded_inf_over_intersect": round(ms_i / ms_o, 3), "legs_ms_ABBA": legs,
             "intersect_mray_s_second_pair": round(nb / ms_i2 / 1e3, 1), "occluded_t_max_mray_s": round(nb / ms_f / 1e3, 1),
             "occluded_t_max_over_intersect": round(ms_i2 / ms_f, 3), "legs_ms_ABBA_second_pair": legs2})
        # how much of a wave idles, in turns of the walk's loop
        k = min(STEP_RAYS, n, nb)
        ha, hd = o_a[:k].cpu().numpy(), d_a[:k].cpu().numpy()
        hb, hbd, hm = o_b[:k].cpu().numpy(), d_b[:k].cpu().numpy(), m_b[:k].cpu().numpy()
        nan = np.full(k, np.nan)
        say({"idle_lane_turns": walk, "rays": k,
             "a_closest_hit_walk": idle_share(scene, ha, hd, nan, fast), "a_occluded_inf": idle_share(scene, ha, hd, None, fast),
             "b_closest_hit_walk": idle_share(scene, hb, hbd, nan, fast), "b_occluded_inf": idle_share(scene, hb, hbd, None, fast),
             "b_occluded_t_max": idle_share(scene, hb, hbd, hm, fast)})
    out = os.path.join(ROOT, "profiles", "query_rates.txt")
    fresh = not os.path.exists(out)
    with open(out, "a") as f:
        if fresh:
            f.write(PREAMBLE)
        f.write("\n".join(LINES) + "\n\n")


bench(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 22)
