"""Map export (ekf_get_map_points) against the route it replaces, on one scene per size.

  (a) EkfEngine.map_points(): one k_map_points launch + 216 bytes per feature over the bus (wall time, stream synchronised)
  (b) the route without it: EkfEngine.get_state() with all of P, then the numpy restatement tests/map_points_ref.py

Median over --calls calls after --warmup, per N and per storage precision; one JSON document on stdout and in --out.
Kernel time comes from a profiler run of its own (--only-export keeps that run to the export):
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/map_points_bench.py --only-export
"""
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

import map_points_ref as mp  # noqa: E402
from openekfmonoslam_amd import engine  # noqa: E402
from openekfmonoslam_amd.synth import SyntheticSequence  # noqa: E402


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 1000, 5000])
    ap.add_argument("--precisions", type=int, nargs="+", default=[1, 0], help="1: fp32 storage, 0: fp64 storage")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--state-calls", type=int, default=None, help="calls of route (b) (default: --calls; its read-back is GBs at N = 5000)")
    ap.add_argument("--only-export", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for N in a.sizes:
        seq = SyntheticSequence(N, 1)
        for prec in a.precisions:
            e = engine.EkfEngine(seq.cam, seq.par, N, max_keypoints=4 * N + 64, precision=prec)
            e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
            e.step(*seq.frames[0])
            row = {"N": N, "n": e.n, "precision": prec, "export_bytes": 216 * N, "P_bytes": e.n * e.n * (4 if prec else 8)}
            med, lo, hi = median_ms(e.map_points, a.calls, a.warmup)
            row.update(export_ms=med, export_ms_min=lo, export_ms_max=hi)
            if not a.only_export:
                t, c = e.feature_layout()
                P = np.zeros((e.n, e.n))

                def route_b():
                    x, fp, _ = e.get_state(P_out=P)
                    return mp.map_points_ref(x, fp, t, c, P)

                calls = a.state_calls or a.calls
                t0 = time.perf_counter()
                e.get_state(P_out=P)
                row["get_state_ms_once"] = 1e3 * (time.perf_counter() - t0)
                med, lo, hi = median_ms(route_b, calls, min(a.warmup, calls))
                row.update(state_route_ms=med, state_route_ms_min=lo, state_route_ms_max=hi, state_route_calls=calls)
            print(json.dumps(row), flush=True)
            rows.append(row)
            e.close()
        del seq
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "ekf_get_map_points vs ekf_get_state + numpy", "calls": a.calls, "warmup": a.warmup, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
