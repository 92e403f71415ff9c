"""What a relocalisation costs (ekf_relocalise): the map is the point cloud of a synthetic sequence as depth
features, the frame is that sequence's frame 6 (K = 2 N keypoints: one per point plus as many distractors), and the camera state the
call starts from is 1 m and 40 degrees off -- which the call never looks at.

    python scripts/relocalise_timing.py [--sizes 1000,5000] [--hypotheses 256,1024,4096] [--warmup 3] [--reps 10] [--precision 2]

One JSON line per (N, H): ms per call from a host clock around the call (it synchronises: upload of the keypoints, four launches,
read-back of the result), min / median / max over --reps calls after --warmup untimed ones, and what the call found.  Nothing is
gated: figures only.  The split per kernel comes from a run of this script under rocprofv3 --kernel-trace --stats (a run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openekfmonoslam_amd import engine  # noqa: E402
from openekfmonoslam_amd.ekftypes import FEATURE_DEPTH  # noqa: E402
from openekfmonoslam_amd.synth import SyntheticSequence, angles_to_quat, initial_state_and_covariance, quat_mul  # noqa: E402

FRAME = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,5000")
    ap.add_argument("--hypotheses", default="256,1024,4096")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--precision", type=int, default=2, help="0 fp64, 2 EKF_PRECISION_F32_EXACT (the bench's default line)")
    args = ap.parse_args()
    for N in [int(s) for s in args.sizes.split(",")]:
        seq = SyntheticSequence(N, FRAME)
        fp = np.zeros((N, 6))
        fp[:, :3] = seq.points
        n = 13 + 3 * N
        P = np.zeros((n, n))
        P[:13, :13] = initial_state_and_covariance(seq.par)[1]
        P[np.arange(13, n), np.arange(13, n)] = 1e-4
        x = seq.x13.copy()
        x[0:3] = seq.truth_r[FRAME] + np.array([1.0, 0.0, 0.0])
        x[3:7] = quat_mul(seq.truth_q[FRAME], angles_to_quat(np.array([0.0, np.deg2rad(40.0), 0.0])))
        kps, desc = seq.frames[FRAME - 1]
        e = engine.EkfEngine(seq.cam, seq.par, N, max_keypoints=len(kps), precision=args.precision)
        e.set_state(x, fp, np.full(N, FEATURE_DEPTH, dtype=np.int32), seq.feature_desc, P)
        del P
        for H in [int(s) for s in args.hypotheses.split(",")]:
            ms, res = [], None
            for k in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                res = e.relocalise(kps, desc, hypotheses=H, min_inliers=8, seed=1)
                if k >= args.warmup:
                    ms.append(1e3 * (time.perf_counter() - t0))
            err = float(np.max(np.abs(res["r"] - seq.truth_r[FRAME])))
            print(json.dumps({"N": N, "K": len(kps), "H": H, "precision": e.precision, "ms_min": min(ms), "ms_median": float(np.median(ms)),
                              "ms_max": max(ms), "reps": args.reps, "found": res["found"], "candidates": res["n_candidates"],
                              "valid_hypotheses": res["n_valid_hypotheses"], "inliers": res["n_inliers"], "rms_px": res["rms_px"],
                              "position_error": err}), flush=True)
        e.close()


if __name__ == "__main__":
    main()
