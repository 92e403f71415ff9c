"""ekf_match_ncc with the distinctiveness test (ekf_set_ncc_distinct) against the matcher without it, on one scene:
640x480, N = 1000, one engine, the same predictions and frame for both modes.

  wall time:   EkfEngine.match_ncc() (launches, the read-back of the counters and of the match list), host clock around the
               call, median of --calls calls after --warmup; the two modes alternate in blocks of --calls + --warmup calls,
               --repeats times: the spread between the repeated blocks of one mode is the noise of the figure
  kernel time: from a profiler run of this script, merged into the same document with --kernel-trace:
      rocprofv3 --kernel-trace --output-format csv -d DIR -o ns -- python scripts/ncc_distinct_bench.py
      python scripts/ncc_distinct_bench.py --kernel-trace DIR/.../ns_kernel_trace.csv --merge-into profiles/ncc_distinct_bench.json
  (k_ncc_match launches grouped by instantiation; per group the median of every block of --calls launches, so that the blocks'
  medians show the run-to-run spread beside the figure)

--only-off times the matcher without the test alone: with EKF_ENGINE_LIB pointing at a build of the parent commit this is that
commit's figure for the off path (its library need not export the new calls); merge its trace with --trace-key kernel_us_parent.
"""
import argparse
import csv
import json
import os
import re
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
    return statistics.median(ts)


def run(a):
    from openekfmonoslam_amd import engine
    from openekfmonoslam_amd.synth import SyntheticSequence

    N = a.size
    seq = SyntheticSequence(N, 2, width=640, height=480)
    e = engine.EkfEngine(seq.cam, seq.par, N + 8)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, None, seq.P0)
    e.upload_image(seq.render_image(0))
    e.capture_templates(np.arange(N), seq.pixel_positions(0).astype(np.float64))
    e.predict()
    preds, _, _ = e.predict_measurements()
    e.upload_image(seq.render_image(1))
    row = {"N": N, "width": 640, "height": 480, "predictions": len(preds), "coef": a.coef}
    for rep in range(a.repeats):
        for mode in ("off",) if a.only_off else ("off", "on"):
            if not a.only_off:
                e.set_ncc_distinct(a.coef if mode == "on" else 0.0)
            row.setdefault(f"match_ncc_wall_ms_{mode}", []).append(median_ms(e.match_ncc, a.calls, a.warmup))
            if rep == 0:
                row[f"matches_{mode}"] = len(e.match_ncc())
                if mode == "on":
                    row["with_rival"], row["rejected"] = e.ncc_distinct_counts()
    print(json.dumps(row), flush=True)
    e.close()
    doc = {"what": "ekf_match_ncc, distinctiveness test on / off", "calls": a.calls, "warmup": a.warmup, "repeats": a.repeats,
           "engine_lib": os.environ.get("EKF_ENGINE_LIB", "this build"), "rows": [row]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def merge_trace(a):
    """k_ncc_match rows of a rocprofv3 kernel trace -> [{kernel, launches, block_median_us: [...], median_us}] under --trace-key"""
    groups = {}
    with open(a.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_ncc_match" not in name:
                continue
            m = re.search(r"k_ncc_match<[^>]*>", name)
            groups.setdefault(m.group(0) if m else "k_ncc_match", []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    per_block = a.calls + a.warmup
    for inst, us in sorted(groups.items()):
        blocks = [us[i + a.warmup:i + per_block] for i in range(0, len(us) - per_block + 1, per_block)]
        meds = [statistics.median(b) for b in blocks if b]
        out.append({"kernel": inst, "launches": len(us), "block_median_us": meds, "median_us": statistics.median(meds) if meds else None,
                    "spread_us": (max(meds) - min(meds)) if meds else None})
        print(json.dumps(out[-1]), flush=True)
    if a.merge_into:
        doc = json.load(open(a.merge_into)) if os.path.exists(a.merge_into) else {}
        doc[a.trace_key] = out
        with open(a.merge_into, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--coef", type=float, default=0.5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
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
