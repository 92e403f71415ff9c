"""Image steps of the NCC matcher with patch normals (ekf_set_patch_normals) against the same steps with the
template warp alone, on one staged synthetic sequence per size: 640x480 at N = 200 and 1000.  Two engines hold the same map
and step the same staged frames, alternated in one process.  Per step: the wall time of the call and the engine's stage timers
("matching" holds the warp, which reads the estimates).  The estimator runs behind the step's last stage mark, so its cost is the
difference of the step wall times; as a stage of its own it is timed through ekf_refine_patch_normals on the last frame's
matches (launch + the counters' read-back).  The kernel's own time comes from a profiler run of the same script:

    python scripts/patch_normals_bench.py [--steps 24] [--warmup 4] [--out profiles/patch_normals_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/patch_normals_bench.py --steps 8
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


def stage_ms(t):
    return {k: getattr(t, k) for k in ("prediction_ms", "matching_ms", "ransac_ms", "update_li_ms", "rescue_ms", "update_hi_ms")}


def run_case(w, h, nfeat, steps, warmup):
    frames = steps + warmup
    seq = SyntheticSequence(nfeat, frames + 1, width=w, height=h)
    img0 = seq.render_image(0)
    imgs = [seq.render_image(t) for t in range(1, frames + 1)]
    uv0 = seq.pixel_positions(0).astype(np.float64)
    eng = {}
    for name in ("normals", "warp"):
        e = engine.EkfEngine(seq.cam, seq.par, nfeat + 8)
        e.set_template_warp(True)
        if name == "normals":
            e.set_patch_normals(True)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, None, seq.P0)
        e.upload_image(img0)
        e.capture_templates(np.arange(nfeat), uv0)
        e.upload_images(imgs)
        e.timing(True)
        eng[name] = e
    rec = {n: {"wall_ms": [], "stages": [], "matches": [], "counts": []} for n in eng}
    for t in range(frames):
        for name, e in eng.items():  # alternated
            e.timing_reset()
            t0 = time.perf_counter()
            info = e.step_staged_image(t)
            e.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if t < warmup:
                continue
            r = rec[name]
            r["wall_ms"].append(wall)
            r["stages"].append(stage_ms(e.timing_get()))
            r["matches"].append(info.n_matches)
            r["counts"].append(e.patch_normal_counts() if name == "normals" else (0, 0))
    # the estimator as a stage of its own: the last frame's matches, again and again (the estimates move; the work does not)
    e = eng["normals"]
    e.predict()
    e.predict_measurements()
    m = e.match_ncc()
    stage = []
    for i in range(steps + warmup):
        t0 = time.perf_counter()
        e.refine_patch_normals(m)
        if i >= warmup:
            stage.append((time.perf_counter() - t0) * 1e3)
    out = {"width": w, "height": h, "N": nfeat, "steps": steps, "warmup": warmup, "refine_matches": int(len(m)),
           "refine_call_ms_median": float(np.median(stage)), "refine_call_ms_min": float(np.min(stage))}
    for name, r in rec.items():
        st = {k: float(np.median([s[k] for s in r["stages"]])) for k in r["stages"][0]}
        out[name] = {"step_wall_ms_median": float(np.median(r["wall_ms"])), "step_wall_ms_min": float(np.min(r["wall_ms"])),
                     "stage_ms_median": st, "matches_mean": float(np.mean(r["matches"])),
                     "normals_updated_mean": float(np.mean([a for a, _ in r["counts"]])),
                     "normals_skipped_mean": float(np.mean([b for _, b in r["counts"]]))}
    for e in eng.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = []
    for n in (200, 1000):
        r = run_case(640, 480, n, a.steps, a.warmup)
        res.append(r)
        print(json.dumps({"N": n, "normals_step_ms": r["normals"]["step_wall_ms_median"], "warp_step_ms": r["warp"]["step_wall_ms_median"],
                          "normals_matching_ms": r["normals"]["stage_ms_median"]["matching_ms"],
                          "warp_matching_ms": r["warp"]["stage_ms_median"]["matching_ms"],
                          "refine_call_ms": r["refine_call_ms_median"], "refine_matches": r["refine_matches"],
                          "normals_updated_mean": r["normals"]["normals_updated_mean"], "normals_matches": r["normals"]["matches_mean"],
                          "warp_matches": r["warp"]["matches_mean"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
