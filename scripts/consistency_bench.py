"""What the filter-consistency mode (ekf_set_consistency) costs per step, and what it reports on the benchmark
frames.  Two engines hold the same map and step the same staged frames, alternated in one process, one with the mode on:
the wall time of a step (call + synchronise) as medians after a warm-up, at N = 200 (fp64) and N = 1000 (the benchmark's
default configuration, fp32 storage with the exact update), and the running totals of the engine with the mode on over
those frames -- total NIS / total rows, 1 for a consistent filter.

    python scripts/consistency_bench.py [--steps 60] [--warmup 10] [--out profiles/r09_consistency_bench.json]
    python scripts/consistency_bench.py --off-only        # one engine, mode off: the figure to compare with another build
                                                          # of the engine (EKF_ENGINE_LIB, scripts/build_variant.sh)
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/consistency_bench.py --steps 8 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from openekfmonoslam_amd import engine  # noqa: E402
from openekfmonoslam_amd.synth import SyntheticSequence  # noqa: E402

CASES = [(200, 0), (1000, 2)]  # (features, EKF_PRECISION_*): bench.py's n200_f64 and n1000_f32x


def run_case(nfeat, precision, steps, warmup, off_only):
    frames = steps + warmup
    seq = SyntheticSequence(nfeat, frames, width=640, height=480)
    eng = {}
    for name in (("off",) if off_only else ("on", "off")):
        e = engine.EkfEngine(seq.cam, seq.par, nfeat, max_keypoints=len(seq.frames[0][0]) + 64, precision=precision)
        e.upload_frames(seq.frames)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        if name == "on":
            e.set_consistency(True)
        eng[name] = e
    wall = {n: [] for n in eng}
    sizes = []
    for t in range(frames):
        for name, e in eng.items():  # alternated
            t0 = time.perf_counter()
            info = e.step_frame(t)
            e.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if t >= warmup:
                wall[name].append(dt)
                if name == "off":
                    sizes.append((info.n_inliers, info.n_rescued))
    out = {"N": nfeat, "precision": precision, "steps": steps, "warmup": warmup,
           "inliers_mean": float(np.mean([a for a, _ in sizes])), "rescued_mean": float(np.mean([b for _, b in sizes]))}
    for name in eng:
        out[name] = {"step_wall_ms_median": float(np.median(wall[name])), "step_wall_ms_min": float(np.min(wall[name]))}
    if "on" in eng:
        nis, rows, updates = eng["on"].consistency_totals()  # all frames, warm-up included
        out["totals"] = {"frames": frames, "updates": updates, "rows": rows, "nis": nis, "nis_per_row": nis / max(rows, 1)}
        out["on_minus_off_ms"] = out["on"]["step_wall_ms_median"] - out["off"]["step_wall_ms_median"]
    for e in eng.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"engine_lib": os.environ.get("EKF_ENGINE_LIB", ""), "cases": [run_case(n, p, a.steps, a.warmup, a.off_only) for n, p in CASES]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
