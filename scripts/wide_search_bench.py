"""The NCC match with the wide search (ekf_set_ncc_wide_search) on and off, alternated in one process on the same
state and frame: EkfEngine.match_ncc() wall time (launches, the read-back of the counters and of the match list), median of
--calls calls after --warmup, the pair of modes repeated --repeats times (the spread between repeats is the noise).

Frames are blurred noise; every feature's gate is set through a diagonal covariance (direction uncertainty only), so the
regimes are exact:
  a     no gate wide (40 px): the price of having the mode on
  b1, b10, b100   1 %, 10 %, 100 % of the gates at a major semi-axis of about 150 px, the others at 40 px
  c     one gate larger than the frame (the tile-parallel latency case), the others at 40 px

Kernel times come from a profiler run of this script, merged into the same document:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ws -- python scripts/wide_search_bench.py --out X.json
    python scripts/wide_search_bench.py --kernel-trace DIR/.../ws_kernel_trace.csv --merge-into X.json
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

AXIS_PER_SIGMA = 2.0 * np.sqrt(5.9915)


def blurred_noise(h, w, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    return np.rint(sum(a[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0).astype(np.uint8)


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def regimes(n):
    out = {"a": np.full(n, 40.0)}
    for pct in (1, 10, 100):
        ax = np.full(n, 40.0)
        ax[: max(1, n * pct // 100)] = 150.0
        out[f"b{pct}"] = ax
    ax = np.full(n, 40.0)
    ax[0] = 20000.0
    out["c"] = ax
    return out


def run(a):
    from openekfmonoslam_amd import engine
    from openekfmonoslam_amd.ekftypes import FEATURE_INVERSE_DEPTH, s3_camera, s3_params
    from openekfmonoslam_amd.synth import initial_state_and_covariance, seed_map

    rows = []
    for (w, h) in a.frames:
        cam, par = s3_camera(w, h), s3_params()
        frame = blurred_noise(h, w, 7)
        for n in a.sizes:
            rng = np.random.default_rng(n)
            uv = np.stack([rng.uniform(0.1 * w, 0.9 * w, n), rng.uniform(0.1 * h, 0.9 * h, n)], axis=-1)
            x13, P13 = initial_state_and_covariance(par)
            fpos = np.concatenate([seed_map(cam, par, x13, P13, uv[i:i + 1])[0] for i in range(n)])
            ftype = np.full(n, FEATURE_INVERSE_DEPTH, dtype=np.int32)
            e = engine.EkfEngine(cam, par, n + 8)
            dim = 13 + 6 * n
            P = np.zeros((dim, dim))
            P[np.arange(13), np.arange(13)] = 2.22e-16
            first = True
            for name, axes in regimes(n).items():
                idx = 13 + 6 * np.arange(n)
                P[idx + 3, idx + 3] = (axes / AXIS_PER_SIGMA / cam.fx) ** 2
                P[idx + 4, idx + 4] = (axes / AXIS_PER_SIGMA / cam.fy) ** 2
                e.set_state(x13, fpos, ftype, None, P)
                if first:
                    e.upload_image(frame)
                    e.capture_templates(np.arange(n), uv)
                    first = False
                preds, _, _ = e.predict_measurements()
                row = {"frame": f"{w}x{h}", "N": n, "regime": name, "predictions": len(preds)}
                for rep in range(a.repeats):
                    for mode in ("off", "on"):
                        e.set_ncc_wide_search(mode == "on")
                        row.setdefault(f"match_ncc_wall_ms_{mode}", []).append(round(median_ms(e.match_ncc, a.calls, a.warmup), 4))
                        if rep == 0:
                            row[f"matches_{mode}"] = len(e.match_ncc())
                            if mode == "on":
                                row["wide_slots"], row["wide_candidates"] = e.ncc_wide_counts()
                print(json.dumps(row), flush=True)
                rows.append(row)
            e.close()
    doc = {"what": "ekf_match_ncc, wide search on / off", "calls": a.calls, "warmup": a.warmup, "repeats": a.repeats, "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def merge_trace(a):
    """NCC kernel rows of a rocprofv3 kernel trace, grouped by kernel and grid size -> launches, median / min / max in us"""
    groups = {}
    with open(a.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "k_ncc_" not in name:
                continue
            short = name[name.index("k_ncc_"):].split("(")[0]
            grid = "x".join(str(r.get(k, "?")) for k in ("Grid_Size_X", "Grid_Size_Y")) if "Grid_Size_X" in r else r.get("Grid_Size", "?")
            groups.setdefault((short, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = [{"kernel": k, "grid_threads": g, "launches": len(us), "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2),
            "max_us": round(max(us), 2)} for (k, g), us in sorted(groups.items())]
    for o in out:
        print(json.dumps(o), flush=True)
    if a.merge_into:
        doc = json.load(open(a.merge_into)) if os.path.exists(a.merge_into) else {}
        doc["kernel_us"] = out
        with open(a.merge_into, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--frames", type=lambda s: tuple(int(v) for v in s.split("x")), nargs="+", default=[(640, 480), (1920, 1080)])
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 *_kernel_trace.csv of a run of this script: no GPU work, only the merge")
    ap.add_argument("--merge-into", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
