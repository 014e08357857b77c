"""Lightmap atlases (include/rayrs_hip.h LIGHTMAP ATLAS) on the GPU box: what the atlas costs, and what share of a lightmap job it is.
usage: python scripts/ubench/lightmap_bench.py [OUT]   (OUT: default profiles/lightmap_rates.txt)

Four measurements, one run each:

  (a) the headline mesh (procedural.blob_mesh(8): 1,310,720 triangles), unwrapped per triangle at cell = 4.  A = Lightmap(...): the
      whole call by the host's clock (the normals on the host, the uploads, the three passes, the list's length read back) and,
      inside it, the owner pass, the compaction (count and scan) and the record pass by HIP events (rayrs_lab_lightmap_ms); B = the
      vectorised numpy reading of the same input on the host (tests/_lightmap.py atlas_vector: the same expressions).  A B B A; A
      and B are compared bit for bit.
  (b) one triangle that fills a 4096 x 4096 atlas: the case a thread per triangle would walk alone.  Lightmap(...) and its split.
  (c) Lightmap.image on (a)'s atlas, three channels, dilate 0, 2 and 8: the whole call by the host's clock (values up, image and
      validity down).
  (d) config 3's mesh (81,920 triangles) end to end at cell = 8: the scene, the atlas, texels() and the Bake's creation, then
      bake_until(tau = 0.2, passes of 16, cap 256) and image(dilate = 2) -- unlit, and with the lamp direct-lit.

Only comparisons within one run count; boxes differ by a few percent.  No figure is asserted.  Not measured: hardware counters,
other cell sizes, other gutters, atlases above 4096 a side.  Writes OUT (every line it prints, with the hash of the library's
sources)."""
import ctypes as C
import glob, hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _lightmap as R
import rayrs_amd
from rayrs_amd import procedural, scenes

PREAMBLE = """Lightmap atlases (DESIGN.md 26): (a) Lightmap creation on the headline mesh, unwrapped per triangle at cell = 4, split into its
three passes, against the vectorised numpy reading on the host; (b) one triangle over a 4096 x 4096 atlas; (c) the assembly at
dilate 0, 2 and 8; (d) config 3's mesh baked end to end, unlit and direct-lit.
Every block below is one call of scripts/ubench/lightmap_bench.py on one MI355X box; the lines are the script's own output (its
docstring says what each figure is).

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


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def passes_ms(lm):
    ms = (C.c_double * 3)()
    assert lm._L.rayrs_lab_lightmap_ms(lm._h, ms) == 0
    return {"owner": round(ms[0], 3), "compaction": round(ms[1], 3), "records": round(ms[2], 3)}


def created(args):
    lm, ms = wall_ms(lambda: rayrs_amd.Lightmap(*args))
    return lm, {"call_ms": round(ms, 2), "passes_ms": passes_ms(lm)}


def headline():
    verts, idx = procedural.blob_mesh(8)
    uvs, W, H = rayrs_amd.unwrap_triangles(len(idx), cell=4)
    args = (verts, idx, uvs, W, H)
    rayrs_amd.Lightmap(verts[:3], idx[:0], uvs[:0], 4, 4).close()   # (the device's first touch is nobody's leg)
    legs, lm, want = [], None, None
    for side in "ABBA":
        if side == "A":
            if lm is not None:
                lm.close()
            lm, fig = created(args)
        else:
            want, ms = wall_ms(lambda: R.atlas_vector(verts, idx, uvs, W, H, small=4))
            fig = {"call_ms": round(ms, 1)}
        legs.append({side: fig})
    index, points, normals = lm.texels()
    same = bool(np.array_equal(lm.owner().astype(np.uint32), want[0]) and np.array_equal(index, want[1]) and R.same(points, want[2])
                and R.same(normals, want[3]) and R.same(lm.bary(), want[4]))
    a = [leg["A"]["call_ms"] for leg in legs if "A" in leg]
    b = [leg["B"]["call_ms"] for leg in legs if "B" in leg]
    say({"measurement": "a: the headline mesh at cell 4", "triangles": len(idx), "atlas": [W, H], "texels_owned": lm.n, "coverage": round(lm.coverage, 4),
         "A": "Lightmap(...) on the device", "B": "tests/_lightmap.py atlas_vector on the host", "legs_ABBA": legs,
         "ms": {"A": round(sum(a) / 2.0, 2), "B": round(sum(b) / 2.0, 1)}, "A_over_B": round(sum(a) / sum(b), 4), "bit_identical": same})
    return lm


def one_triangle():
    verts, idx = R._space(1, 1)
    uvs = np.array([[(-0.1, -0.1), (2.5, -0.1), (-0.1, 2.5)]])
    lm, fig = created((verts, idx, uvs, 4096, 4096))
    say({"measurement": "b: one triangle over 4096 x 4096", "texels_owned": lm.n, **fig})
    lm.close()


def assembly(lm):
    values = np.random.default_rng(1).uniform(size=(lm.n, 3))
    lm.image(values, dilate=1)
    for d in (0, 2, 8):
        (img, valid), ms = wall_ms(lambda: lm.image(values, dilate=d, return_valid=True))
        say({"measurement": "c: the assembly", "atlas": [lm.width, lm.height], "channels": 3, "dilate": d, "call_ms": round(ms, 2),
             "texels_valid": int(valid.sum())})


def end_to_end():
    _, objs, heur, _, _ = scenes.config(3)
    hdri = procedural.make_hdri(1024, 512)
    scene, scene_ms = wall_ms(lambda: rayrs_amd.Scene(objs, 1e-6, 1e6, heur, hdri, device=0))
    mesh = [o for o in rayrs_amd.api.flatten_objects(objs) if o.kind == "mesh"][0]
    for lit in (False, True):
        lighting = dict(lights=rayrs_amd.emitters(objs), direct=True) if lit else {}
        lm, fig = created((mesh.verts, mesh.idx) + rayrs_amd.unwrap_triangles(len(mesh.idx), cell=8))
        bake, bake_ms = wall_ms(lambda: lm.bake(scene, sample_chunk=4, bias=1e-6, **lighting))
        (st, reason), until_ms = wall_ms(lambda: rayrs_amd.bake_until(bake, tau=0.2, pass_samples=16, max_samples=256))
        values, read_ms = wall_ms(bake.values)
        img, image_ms = wall_ms(lambda: lm.image(values, dilate=2))
        atlas = fig["call_ms"] + image_ms
        total = atlas + bake_ms + until_ms + read_ms
        say({"measurement": "d: config 3's mesh end to end", "lighting": "lamp, direct" if lit else "unlit", "triangles": len(mesh.idx),
             "atlas": [lm.width, lm.height], "texels_owned": lm.n, "scene_ms": round(scene_ms, 1), "create": fig,
             "texels_and_bake_create_ms": round(bake_ms, 2), "bake_until_ms": round(until_ms, 1), "reason": reason,
             "point_samples": st["point_samples"], "rays": st["rays"], "values_ms": round(read_ms, 2), "image_ms": round(image_ms, 2),
             "atlas_share_of_job": round(atlas / total, 4), "finite": bool(np.isfinite(img).all())})
        bake.close()
        lm.close()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lightmap_rates.txt")
    say({"command": "python scripts/ubench/lightmap_bench.py", "source_hash": source_hash()})
    lm = headline()
    one_triangle()
    assembly(lm)
    lm.close()
    end_to_end()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(PREAMBLE + "\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
