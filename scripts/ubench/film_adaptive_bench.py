"""Measurements for adaptive film passes (profiles/film_adaptive.txt).  Run on a GPU box.

  python scripts/ubench/film_adaptive_bench.py plain <other_checkout> [config res spp]
      (a) the plain frame of this tree against another built checkout of the repository (the parent commit), same box,
      order A B B A, then this tree against itself A A A A: the harness's own run-to-run spread.  Each run is
      scripts/ubench/tune_sweep.py of the checkout it measures, in a fresh process; prints trace ms and the frame's sha.
  python scripts/ubench/film_adaptive_bench.py adaptive <config> <res> <tau> <cap> <pass>
      (b) render_until to the same tau and cap, uniform and adaptive: wall time, pixel-samples, active tiles per pass.
      Under `rocprofv3 --kernel-trace --stats -- python ... adaptive ...` the same run gives (c), the select kernels' time.
"""
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sweep(root, cfg, res, spp):
    env = dict(os.environ)
    env.pop("RAYRS_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "ubench", "tune_sweep.py"), cfg, res, spp, ""],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"tune_sweep.py in {root} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    rows = re.findall(r"trace\s+([0-9.]+) ms .*?sha ([0-9a-f]+)", r.stdout)
    return [float(ms) for ms, _ in rows], {sha for _, sha in rows}


def plain(other, cfg="5", res="2048", spp="1024"):
    results = {}
    for label, order in (("A B B A (this tree, other, other, this tree)", [ROOT, other, other, ROOT]), ("A A A A (this tree)", [ROOT] * 4)):
        print(label, flush=True)
        for root in order:
            ms, shas = sweep(root, cfg, res, spp)
            who = "this " if root == ROOT else "other"
            results.setdefault((label, who), []).extend(ms)
            print(f"  {who}: trace ms {' '.join(f'{v:8.1f}' for v in ms)}  sha {' '.join(sorted(shas))}", flush=True)
    ab = "A B B A (this tree, other, other, this tree)"
    mean = lambda v: sum(v) / len(v)
    this, prev, self_runs = results[(ab, "this ")], results[(ab, "other")], results[("A A A A (this tree)", "this ")]
    print(f"this tree {mean(this):.1f} ms, other {mean(prev):.1f} ms: {100.0 * (mean(this) / mean(prev) - 1.0):+.2f} %")
    print(f"this tree against itself: {min(self_runs):.1f} .. {max(self_runs):.1f} ms, spread "
          f"{100.0 * (max(self_runs) / min(self_runs) - 1.0):.2f} %")


def adaptive(cfg, res, tau, cap, step):
    sys.path.insert(0, ROOT)
    import rayrs_amd
    from rayrs_amd import procedural, scenes
    cam_args, objs, heur, _, mb = scenes.config(cfg)
    cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, res, res))
    scene = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, procedural.make_hdri(1024, 512), device=0)
    rayrs_amd.render(scene, cam, 4, mb, sample_chunk=0)  # warm
    print(f"config {cfg} at {res} x {res}, tau {tau}, cap {cap}, passes of {step}")
    for mode in (False, True, True, False):
        film = rayrs_amd.Film(scene, cam, sample_chunk=4, max_bounces=mb)
        per_pass = []
        t0 = time.perf_counter()
        st, why = rayrs_amd.render_until(film, tau, 0.0, pass_samples=step, max_samples=cap, adaptive=mode,
                                         on_pass=lambda f, s: per_pass.append(s.get("active_tiles")))
        wall = time.perf_counter() - t0
        pixel_samples = st.get("pixel_samples", st["samples"] * st["pixels"])
        print(f"  {'adaptive' if mode else 'uniform '}: {wall * 1e3:9.1f} ms  {why:11s} pixel-samples {pixel_samples:14d}  "
              f"samples max {st['samples']:5d}  unconverged {st['unconverged']:8d}  rays {st['rays']}"
              + (f"  active tiles per pass {per_pass}" if mode else f"  passes {len(per_pass)}"), flush=True)
        film.close()


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "plain":
        plain(os.path.abspath(sys.argv[2]), *sys.argv[3:6])
    elif len(sys.argv) == 7 and sys.argv[1] == "adaptive":
        adaptive(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    else:
        raise SystemExit(__doc__)
