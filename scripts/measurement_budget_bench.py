"""What a measurement budget (ekf_set_measurement_budget) buys per step and what it costs in accuracy.  Engines
holding the same map step the same staged frames, alternated in one process, with the budget off and at K = N/2, N/4, N/8: the
wall time of a step (call + synchronise) as medians after a warm-up, at N = 1000 (the benchmark's configuration, fp32 storage with
the exact update) and N = 2000 (EKF_PRECISION_AUTO, 1280 x 720), and at the end of the frames the camera state of every
budgeted filter against the un-budgeted one and against the true trajectory -- a finding, not a gate.

    python scripts/measurement_budget_bench.py [--steps 30] [--warmup 5] [--out profiles/measurement_budget_bench.json]
    python scripts/measurement_budget_bench.py --off-only   # one engine, budget off: the figure to compare with another build
                                                            # of the engine (EKF_ENGINE_LIB, scripts/build_variant.sh)
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/measurement_budget_bench.py --steps 8 --warmup 2 --sizes 1000
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

CASES = {1000: (640, 480, 2), 2000: (1280, 720, 4)}  # features: (width, height, EKF_PRECISION_*) -- bench.py's n1000_f32x, n2000_auto


def run_case(nfeat, steps, warmup, off_only):
    width, height, precision = CASES[nfeat]
    frames = steps + warmup
    seq = SyntheticSequence(nfeat, frames, width=width, height=height)
    budgets = {"off": 0} if off_only else {"off": 0, "N/2": nfeat // 2, "N/4": nfeat // 4, "N/8": nfeat // 8}
    eng = {}
    for name, K in budgets.items():
        e = engine.EkfEngine(seq.cam, seq.par, nfeat, max_keypoints=len(seq.frames[0][0]) + 64, precision=precision)
        e.upload_frames(seq.frames)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        if K:
            e.set_measurement_budget(K)
        eng[name] = e
    wall = {n: [] for n in eng}
    sizes = {n: [] for n in eng}
    for t in range(frames):
        for name, e in eng.items():  # alternated
            t0 = time.perf_counter()
            info = e.step_frame(t)
            e.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if t >= warmup:
                wall[name].append(dt)
                sizes[name].append((info.n_predicted, info.n_matches, info.n_inliers, info.n_rescued))
    out = {"N": nfeat, "precision": eng["off"].precision, "steps": steps, "warmup": warmup}
    x_off = eng["off"].get_state(want_P=False)[0]
    r_true, q_true = seq.truth_r[frames], seq.truth_q[frames]
    for name, e in eng.items():
        s = np.array(sizes[name], dtype=float)
        x = e.get_state(want_P=False)[0]
        out[name] = {"K": budgets[name], "step_wall_ms_median": float(np.median(wall[name])), "step_wall_ms_min": float(np.min(wall[name])),
                     "predicted_mean": float(s[:, 0].mean()), "matches_mean": float(s[:, 1].mean()),
                     "inliers_mean": float(s[:, 2].mean()), "rescued_mean": float(s[:, 3].mean()),
                     "position_vs_unbudgeted": float(np.abs(x[0:3] - x_off[0:3]).max()),
                     "quaternion_vs_unbudgeted": float(np.abs(x[3:7] - x_off[3:7]).max()),
                     "position_error_vs_truth": float(np.abs(x[0:3] - r_true).max()),
                     "quaternion_error_vs_truth": float(np.abs(x[3:7] - q_true).max())}
        if name != "off":
            out[name]["speedup_vs_off"] = out["off"]["step_wall_ms_median"] / out[name]["step_wall_ms_median"]
    for e in eng.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=sorted(CASES))
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"engine_lib": os.environ.get("EKF_ENGINE_LIB", ""), "cases": [run_case(n, a.steps, a.warmup, a.off_only) for n in a.sizes]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
