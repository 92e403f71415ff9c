"""Batch conversion (ekf_convert_all_inverse_depth_to_depth) against the route it replaces, on all-inverse-depth maps with the
linearity threshold at 1e9 (every feature converts).

  new     one ekf_convert_all_inverse_depth_to_depth: all N features
  single  one ekf_convert_inverse_depth_to_depth: ONE feature -- the existing cost per conversion (N of them do what `new` does)

Wall time: a host clock around the call, which ends synchronised, on a map that set_state and one prediction left (and a
synchronise behind them).  `fresh`: the call is the engine's first map operation (it allocates the second covariance buffer, either
route); `warm`: the same engine, seeded again.  Median over --reps fresh engines per route after --warmup more, the two routes in
turn.  At --step-size one full step() is timed on the map before and behind the conversion.  One JSON document in --out.

Kernel time comes from a profiler run of its own, merged into the same document:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o ca -- python scripts/convert_all_bench.py --only-new
    python scripts/convert_all_bench.py --kernel-trace DIR/.../ca_kernel_trace.csv --merge-into profiles/convert_all_bench.json
with the kernel's byte floor (n^2 + n'^2) sizeof(T) / 6.3 TB/s beside it.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12
ONLY_NEW_CALLS = 3  # per size and precision in the profiler run


def seeded(engine, seq, prec, e=None):
    if e is None:
        e = engine.EkfEngine(seq.cam, seq.par, seq.n_features, max_keypoints=4 * seq.n_features + 64, precision=prec)
    e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
    e.predict()
    e.synchronize()
    return e


def timed_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def run(a):
    from openekfmonoslam_amd import engine
    from openekfmonoslam_amd.synth import SyntheticSequence

    rows = []
    for N in a.sizes:
        seq = SyntheticSequence(N, 1)
        seq.par.inverseDepthLinearityIndexThreshold = 1e9
        for prec in a.precisions:
            w = 4 if prec else 8
            n, n_new = 13 + 6 * N, 13 + 3 * N
            row = {"N": N, "n": n, "n_new": n_new, "precision": prec, "P_bytes": n * n * w,
                   "kernel_floor_us": 1e6 * (n * n + n_new * n_new) * w / HBM_BYTES_PER_S}
            if a.only_new:
                e = seeded(engine, seq, prec)
                for _ in range(ONLY_NEW_CALLS):
                    assert len(e.convert_all_inverse_depth_to_depth()) == N
                    seeded(engine, seq, prec, e)
                e.close()
                rows.append(row)
                continue
            t = {"new_fresh": [], "new_warm": [], "single_fresh": [], "single_warm": []}
            for rep in range(a.warmup + a.reps):
                for route in ("new", "single"):
                    e = seeded(engine, seq, prec)
                    call = e.convert_all_inverse_depth_to_depth if route == "new" else e.convert_inverse_depth_to_depth
                    fresh, out = timed_ms(call)
                    assert (len(out) == N and e.n == n_new) if route == "new" else (out == 0 and e.n == n - 3)
                    seeded(engine, seq, prec, e)
                    warm, _ = timed_ms(call)
                    e.close()
                    if rep >= a.warmup:
                        t[route + "_fresh"].append(fresh)
                        t[route + "_warm"].append(warm)
            for k, v in t.items():
                row[k + "_ms"] = statistics.median(v)
                row[k + "_ms_min_max"] = [min(v), max(v)]
            row["new_over_single_fresh"] = row["new_fresh_ms"] / row["single_fresh_ms"]
            row["new_over_single_warm"] = row["new_warm_ms"] / row["single_warm_ms"]
            if N == a.step_size:
                e = seeded(engine, seq, prec)
                before, behind = [], []
                for rep in range(a.warmup + a.reps):
                    seeded(engine, seq, prec, e)
                    ms, info = timed_ms(lambda: (e.step(*seq.frames[0]), e.synchronize())[0])
                    seeded(engine, seq, prec, e)
                    e.convert_all_inverse_depth_to_depth()
                    ms2, info2 = timed_ms(lambda: (e.step(*seq.frames[0]), e.synchronize())[0])
                    if rep >= a.warmup:
                        before.append(ms)
                        behind.append(ms2)
                row.update(step_ms_before=statistics.median(before), step_ms_behind=statistics.median(behind),
                           step_inliers_before=info.n_inliers + info.n_rescued, step_inliers_behind=info2.n_inliers + info2.n_rescued)
                e.close()
            print(json.dumps(row), flush=True)
            rows.append(row)
        del seq
    if a.out and not a.only_new:
        with open(a.out, "w") as f:
            json.dump({"what": "ekf_convert_all_inverse_depth_to_depth (all N features) vs one ekf_convert_inverse_depth_to_depth (one feature)",
                       "reps": a.reps, "warmup": a.warmup, "rows": rows}, f, indent=1)
            f.write("\n")


def merge_trace(a):
    """the k_convert_all_P dispatches of a --only-new profiler run (per instantiation: ONLY_NEW_CALLS per size, sizes in order) ->
    kernel_us (median) and kernel_over_floor of the matching rows of --merge-into"""
    us = {4: [], 8: []}
    with open(a.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_convert_all_P" in name:
                us[4 if "<float>" in name or "IfE" in name else 8].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    doc = json.load(open(a.merge_into))
    for w, prec in ((4, 1), (8, 0)):
        rows = [r for r in doc["rows"] if r["precision"] == prec]
        assert len(us[w]) == ONLY_NEW_CALLS * len(rows), (w, len(us[w]), len(rows))
        for i, r in enumerate(rows):
            r["kernel_us"] = statistics.median(us[w][ONLY_NEW_CALLS * i:ONLY_NEW_CALLS * (i + 1)])
            r["kernel_over_floor"] = r["kernel_us"] / r["kernel_floor_us"]
            print(json.dumps({k: r[k] for k in ("N", "precision", "kernel_us", "kernel_floor_us", "kernel_over_floor")}), flush=True)
    with open(a.merge_into, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 1000, 2000])
    ap.add_argument("--precisions", type=int, nargs="+", default=[1, 0], help="1: fp32 storage, 0: fp64 storage")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-size", type=int, default=1000)
    ap.add_argument("--only-new", action="store_true", help="the profiler run: ONLY_NEW_CALLS new calls per size and precision, nothing written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_all_bench.json"))
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 *_kernel_trace.csv of an --only-new run: no GPU work, only the merge")
    ap.add_argument("--merge-into", default=os.path.join(ROOT, "profiles", "convert_all_bench.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
