"""ekf_match_ncc with sub-pixel matches (ekf_set_subpixel_matches) against the integer matcher, on one scene per
size: 640x480, N = 1000 and 2000, one engine, the same predictions and frame for both modes.

  wall time:   EkfEngine.match_ncc() (launches, the read-back of the counters and of the match list), host clock around the
               call, median of --calls calls after --warmup; the two modes alternate in blocks of --calls + --warmup calls
  kernel time: from a profiler run of this script, merged into the same document with --kernel-trace:
      rocprofv3 --kernel-trace --output-format csv -d DIR -o ns -- python scripts/ncc_subpixel_bench.py
      python scripts/ncc_subpixel_bench.py --kernel-trace DIR/.../ns_kernel_trace.csv --merge-into profiles/ncc_subpixel_bench.json
  (k_ncc_match launches grouped by instantiation and grid size; median of the last --calls launches of each group)

--only-off times the integer matcher alone: with EKF_ENGINE_LIB pointing at a build of another commit this is the figure of
that commit (its library need not export the new calls).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def run(a):
    from openekfmonoslam_amd import engine
    from openekfmonoslam_amd.synth import SyntheticSequence

    rows = []
    for N in a.sizes:
        seq = SyntheticSequence(N, 2, width=640, height=480)
        e = engine.EkfEngine(seq.cam, seq.par, N + 8)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, None, seq.P0)
        e.upload_image(seq.render_image(0))
        e.capture_templates(np.arange(N), seq.pixel_positions(0).astype(np.float64))
        e.predict()
        preds, _, _ = e.predict_measurements()
        e.upload_image(seq.render_image(1))
        row = {"N": N, "width": 640, "height": 480, "predictions": len(preds)}
        for rep in range(a.repeats):  # off, on, off, on: the spread between repeats is the noise of the figure
            for mode in ("off",) if a.only_off else ("off", "on"):
                if not a.only_off:
                    e.set_subpixel_matches(mode == "on")
                med, lo, hi = median_ms(e.match_ncc, a.calls, a.warmup)
                row.setdefault(f"match_ncc_wall_ms_{mode}", []).append(med)
                row.setdefault(f"match_ncc_wall_ms_{mode}_min", []).append(lo)
                if rep == 0:
                    row[f"matches_{mode}"] = len(e.match_ncc())
                    if mode == "on":
                        row["axes_refined"], row["axes_integer"] = e.subpixel_counts()
        print(json.dumps(row), flush=True)
        rows.append(row)
        e.close()
    doc = {"what": "ekf_match_ncc, sub-pixel matches on / off", "calls": a.calls, "warmup": a.warmup, "repeats": a.repeats,
           "engine_lib": os.environ.get("EKF_ENGINE_LIB", "this build"), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def merge_trace(a):
    """k_ncc_match rows of a rocprofv3 kernel trace -> {"kernel_us": [{kernel, grid, launches, median_us, min_us, max_us}]}"""
    groups = {}
    with open(a.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_ncc_match" not in name:
                continue
            grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
            inst = "k_ncc_match<true>" if "<true>" in name else ("k_ncc_match<false>" if "<false>" in name else "k_ncc_match")
            groups.setdefault((inst, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for (inst, grid), us in sorted(groups.items(), key=lambda kv: (int(kv[0][1]) if kv[0][1].isdigit() else 0, kv[0][0])):
        last = us[-a.calls:]
        out.append({"kernel": inst, "grid_threads": grid, "launches": len(us), "median_us": statistics.median(last), "min_us": min(last),
                    "max_us": max(last)})
        print(json.dumps(out[-1]), flush=True)
    if a.merge_into:
        doc = json.load(open(a.merge_into)) if os.path.exists(a.merge_into) else {}
        doc[a.trace_key] = out
        with open(a.merge_into, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 2000])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--only-off", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 *_kernel_trace.csv of a run of this script: no GPU work, only the merge")
    ap.add_argument("--merge-into", default=None)
    ap.add_argument("--trace-key", default="kernel_us")
    a = ap.parse_args()
    if a.kernel_trace:
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
