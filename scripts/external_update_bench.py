"""External measurement update (ekf_update_external) against the two routes the engine offered for the
same job before it, on one scene per size and storage type.

  (a) EkfEngine.update_external with m = 1 (a distance row), 3 (a position fix) and 16 (random rows of 32 entries): wall time of
      the call (it synchronises the stream), the k_ext_downdate kernel time by HIP events (ekf_timing_enable: the bracket joins the
      P-update log) and its achieved bytes/s counted as 2 n^2 sizeof(T) -- P read once and written once
  (b) ekf_update with one match (2 rows) at the same N, behind the full ekf_predict_measurements it needs: the pair, and the
      update's own share of it
  (c) the round trip: get_state with all of P, set_state with it again (what fusing anything on the host costs before the host
      has computed anything)

Median over --calls calls after --warmup; one JSON line per (N, precision) on stdout and the document in --out.  The filter
is not meant to stay meaningful over 35 identical fixes: R is chosen large so that P barely moves and every call does the same
work."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from openekfmonoslam_amd import engine  # noqa: E402
from openekfmonoslam_amd.ekftypes import MATCH_DTYPE  # noqa: E402
from openekfmonoslam_amd.synth import SyntheticSequence  # noqa: E402

HBM_MEASURED = 6.29e12  # bytes/s of a float4 copy on an MI355X (8.0e12 by the data sheet)


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def rows_for(e, m, rng):
    n = e.n
    if m == 3:
        return (np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), np.ones(3)), np.full(3, 1e-4), np.eye(3)
    if m == 1:
        _, c = e.feature_layout()
        col = np.r_[c[0]:c[0] + 6, c[-1]:c[-1] + 6].astype(np.int32)
        return (np.array([0, 12], dtype=np.int32), col, 0.1 * rng.standard_normal(12)), np.array([1e-4]), np.eye(1)
    col = np.concatenate([np.sort(rng.choice(n, size=32, replace=False)) for _ in range(m)]).astype(np.int32)
    return (np.arange(0, 32 * m + 1, 32, dtype=np.int32), col, 0.1 * rng.standard_normal(32 * m)), np.full(m, 1e-4), 10.0 * np.eye(m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 1000, 5000])
    ap.add_argument("--precisions", type=int, nargs="+", default=[2, 0],
                    help="2: fp32 storage (EKF_PRECISION_F32_EXACT, bench.py's headline configuration), 0: fp64 storage")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--state-calls", type=int, default=None, help="calls of route (c) (default: --calls; it moves GBs at N = 5000)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    out = []
    for N in a.sizes:
        seq = SyntheticSequence(N, 1)
        for prec in a.precisions:
            e = engine.EkfEngine(seq.cam, seq.par, N, max_keypoints=4 * N + 64, precision=prec)
            e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
            e.step(*seq.frames[0])
            w = 4 if prec in (1, 2) else 8
            row = {"N": N, "n": e.n, "precision": prec, "downdate_bytes": 2 * e.n * e.n * w}
            e.timing(True)
            for m in (1, 3, 16):
                rows, residual, R = rows_for(e, m, rng)
                e.timing_reset()
                med, lo, hi = median_ms(lambda: e.update_external(rows, residual, R), a.calls, a.warmup)
                mm, ms = e.p_update_launches()
                assert len(ms) == a.calls + a.warmup and np.all(mm == m)
                k_ms = float(np.median(ms[a.warmup:]))
                row[f"m{m}"] = {"call_ms": med, "call_ms_min": lo, "call_ms_max": hi, "downdate_kernel_ms": k_ms,
                                "downdate_kernel_ms_min": float(ms[a.warmup:].min()),
                                "downdate_bytes_per_s": row["downdate_bytes"] / (1e-3 * k_ms),
                                "share_of_measured_hbm": row["downdate_bytes"] / (1e-3 * k_ms) / HBM_MEASURED}
            e.timing(False)
            # (b) the engine's own update with one match behind the full prediction it needs (ekf_update multiplies with the H P rows
            # of the last prediction, so a repeated update is only a filter step with a prediction in front of it); the update's
            # own share is timed inside the pair.  Dozens of identical matches are still not a meaningful filter: a failed
            # factorisation is let through and counted, the launches are the same
            failed = [0]
            preds, _, _ = e.predict_measurements()
            match = np.zeros(1, dtype=MATCH_DTYPE)
            match["featureIndex"], match["keypointIndex"], match["imagePos"] = preds["featureIndex"][0], -1, preds["imagePos"][0] + 0.1
            upd = []

            def predict_and_update():
                e.predict_measurements()
                t0 = time.perf_counter()
                failed[0] += 1 if e.update(match, allow_errors=(3, 4)) else 0
                upd.append(1e3 * (time.perf_counter() - t0))

            med, lo, hi = median_ms(predict_and_update, a.calls, a.warmup)
            row["predict_measurements_and_update_one_match"] = {"call_ms": med, "call_ms_min": lo, "call_ms_max": hi}
            row["ekf_update_one_match"] = {"call_ms": statistics.median(upd[a.warmup:]), "call_ms_min": min(upd[a.warmup:]),
                                           "call_ms_max": max(upd[a.warmup:]), "failed_factorisations": failed[0]}
            # (c) read everything back and upload it again
            P = np.zeros((e.n, e.n))
            t, _ = e.feature_layout()
            desc, _, _ = e.get_map_features()

            def round_trip():
                x, fp, _ = e.get_state(P_out=P)
                e.set_state(x, fp, t, desc, P)

            calls = a.state_calls or a.calls
            med, lo, hi = median_ms(round_trip, calls, min(a.warmup, calls))
            row["state_round_trip"] = {"call_ms": med, "call_ms_min": lo, "call_ms_max": hi, "calls": calls,
                                       "bytes_each_way": e.n * e.n * w}
            print(json.dumps(row), flush=True)
            out.append(row)
            e.close()
        del seq
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "ekf_update_external vs ekf_update with one match vs get_state + set_state", "calls": a.calls,
                       "warmup": a.warmup, "hbm_bytes_per_s_measured_copy": HBM_MEASURED, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
