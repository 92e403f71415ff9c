"""Map blob (ekf_save_map / ekf_load_map) against the only route there was before it, on one scene per size.

  (a) EkfEngine.save_map() / .load_map(): P packed and checksummed on the device, one copy of n (n + 1) / 2 elements of the storage
      type, every per-feature table (templates, source patches, capture poses, patch normals) in the same buffer
  (b) the piecemeal route: get_state() + get_map_features() + feature_layout() out, set_state() in.  It moves P as n^2 doubles
      whatever the storage type -- and it CANNOT carry the templates, the source patches, the capture poses, the patch normals or the
      counters: what it restores is not the map that was saved.  It is timed for the part it does carry.

Wall time, stream synchronised (both routes synchronise); median over --calls calls after --warmup, per N and storage precision;
one JSON line per row on stdout and the document in --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

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
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 1000, 2000])
    ap.add_argument("--precisions", type=int, nargs="+", default=[2, 0], help="2: fp32 storage (F32_EXACT), 0: fp64 storage")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for N in a.sizes:
        seq = SyntheticSequence(N, 1)
        for prec in a.precisions:
            mk = lambda: engine.EkfEngine(seq.cam, seq.par, N, max_keypoints=4 * N + 64, precision=prec)  # noqa: E731
            e, target = mk(), mk()
            e.set_template_warp(True)
            e.set_patch_normals(True)
            e.set_state(seq.x13, seq.feature_pos, seq.feature_type, seq.feature_desc, seq.P0)
            e.step(*seq.frames[0])  # P bitwise symmetric: the packed triangle
            blob = e.save_map()
            info = engine.map_blob_info(blob)
            w = info["p_elem_bytes"]
            row = {"N": N, "n": e.n, "precision": prec, "blob_bytes": int(blob.size), "p_layout": info["p_layout"],
                   "p_section_bytes": e.n * (e.n + 1) // 2 * w, "get_state_P_bytes": e.n * e.n * 8}
            for name, fn in (("save_ms", e.save_map), ("load_ms", lambda: target.load_map(blob))):
                med, lo, hi = median_ms(fn, a.calls, a.warmup)
                row.update({name: med, name + "_min": lo, name + "_max": hi})

            def piecemeal_out():
                x, fp, P = e.get_state()
                d, tp, tm = e.get_map_features()
                t, _ = e.feature_layout()
                return x, fp, t, d, P

            med, lo, hi = median_ms(piecemeal_out, a.calls, a.warmup)
            row.update(get_state_route_ms=med, get_state_route_ms_min=lo, get_state_route_ms_max=hi)
            x, fp, t, d, P = piecemeal_out()
            med, lo, hi = median_ms(lambda: target.set_state(x, fp, t, d, P), a.calls, a.warmup)
            row.update(set_state_route_ms=med, set_state_route_ms_min=lo, set_state_route_ms_max=hi)
            print(json.dumps(row), flush=True)
            rows.append(row)
            e.close()
            target.close()
        del seq
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "ekf_save_map / ekf_load_map vs get_state + get_map_features / set_state (which carries no templates, "
                               "source patches, capture poses, normals or counters)", "calls": a.calls, "warmup": a.warmup, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
