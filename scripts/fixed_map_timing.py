"""What the fixed-map mode (ekf_set_fixed_map) buys per frame: the bench's own sequences, mode off and
mode on ALTERNATED in one process on one engine, every pass from the same uploaded state.

    python scripts/fixed_map_timing.py [--workloads n1000_f32x,n2000_auto,n5000_f64x] [--map-frames 12] [--rounds 3] [--warmup 3] [--steps 8]

The mode is for a map that exists: the first --map-frames frames are run with the mode off (mapping), the state behind them is
read back once, and every pass starts from it.  (--map-frames 0 starts every pass from the generator's fresh map instead: its
inverse depths are one sigma wide and are never corrected in the mode, so fewer matches pass the low-innovation gate, more are
rescued, and the second update of a frame has two to three times the rows -- a different frame, not a cheaper one.)

Per workload and mode one JSON line per round: ms per frame from a host clock around synchronised steps, and the engine's own
stage timers (ekf_timing_*: the two updates, the sweep inside them, the downdate's launches) over the same frames; then a summary
line with both means, their spread (min .. max over the rounds) and the ratio off / on.  Nothing is gated: figures only."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openekfmonoslam_amd import engine  # noqa: E402
from openekfmonoslam_amd.synth import SyntheticSequence  # noqa: E402

WORKLOADS = {  # bench.py's: features, width, height, precision
    "n200_f64": (200, 640, 480, 0),
    "n1000_f32x": (1000, 640, 480, 2),
    "n2000_auto": (2000, 1280, 720, 4),
    "n5000_f64x": (5000, 1920, 1080, 3),
}


def one_pass(e, seq, state, first, on, warmup, steps, on_path=0):
    e.set_state(state[0], state[1], seq.feature_type, state[3], state[2])
    e.set_fixed_map(on)
    e.set_update_path(on_path if on else 0)
    for t in range(first, first + warmup):
        e.step_frame(t)
    e.synchronize()
    e.timing(True)
    e.timing_reset()
    t0 = time.perf_counter()
    infos = [e.step_frame(t) for t in range(first + warmup, first + warmup + steps)]
    e.synchronize()
    dt = time.perf_counter() - t0
    tm, sw = e.timing_get(), e.sweep_timing()
    e.timing(False)
    return {
        "fixed_map": bool(on),
        "ms_per_frame": 1e3 * dt / steps,
        "update_li_ms": tm.update_li_ms / steps,
        "update_hi_ms": tm.update_hi_ms / steps,
        "sweep_ms": sw["ms"] / steps,
        "p_update_kernel_ms": tm.p_update_kernel_ms / steps,
        "p_update_launches": int(tm.p_update_launches),
        "inliers": [int(i.n_inliers) for i in infos],
        "rescued": [int(i.n_rescued) for i in infos],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="n1000_f32x,n2000_auto,n5000_f64x")
    ap.add_argument("--map-frames", type=int, default=12)
    ap.add_argument("--on-update-path", type=int, default=0, choices=[0, 1, 2],
                    help="ekf_set_update_path for the passes with the mode on (0: by size; 1: rows of B in the sweep; 2: inverse, no rows of B)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    for name in args.workloads.split(","):
        N, W, H, precision = WORKLOADS[name]
        seq = SyntheticSequence(N, args.map_frames + args.warmup + args.steps, width=W, height=H)
        e = engine.EkfEngine(seq.cam, seq.par, N, max_keypoints=len(seq.frames[0][0]) + 64, precision=precision)
        e.upload_frames(seq.frames)
        e.set_async_errors(True)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
        for t in range(args.map_frames):
            e.step_frame(t)
        state = e.get_state() + (e.get_map_features()[0],) if args.map_frames else (seq.x13, seq.feature_pos, seq.P0, seq.feature_desc)
        ms = {False: [], True: []}
        for r in range(args.rounds):
            for on in (False, True):
                rec = one_pass(e, seq, state, args.map_frames, on, args.warmup, args.steps, args.on_update_path)
                rec.update(workload=name, round=r, precision=e.precision, n=e.n, map_frames=args.map_frames, on_update_path=args.on_update_path)
                ms[on].append(rec["ms_per_frame"])
                print(json.dumps(rec), flush=True)
        off, on = sum(ms[False]) / len(ms[False]), sum(ms[True]) / len(ms[True])
        print(json.dumps({"workload": name, "summary": True, "rounds": args.rounds, "steps": args.steps, "map_frames": args.map_frames,
                          "off_ms_per_frame": off, "off_spread": [min(ms[False]), max(ms[False])],
                          "on_ms_per_frame": on, "on_spread": [min(ms[True]), max(ms[True])], "ratio_off_over_on": off / on}), flush=True)
        e.set_fixed_map(False)
        e.set_update_path(0)
        e.close()


if __name__ == "__main__":
    main()
