"""Image steps with the keypoint matcher (device detector + BRIEF-32 + Hamming matcher) against image steps with the NCC
matcher, on staged synthetic sequences: 640x480 and 1920x1080 at N = 200 and 1000.  The two engines hold the same map and
step the same frames, alternated in one process.  Per step: the engine's stage timers (HIP events on its stream;
"matching" holds detection + descriptors + matching, or the NCC search) and the wall time of the call, after a warm-up.
Also the stand-alone detector (ekf_detect_keypoints, whole frame) and the keypoints detected per frame.

    python scripts/keypoint_image_bench.py [--steps 24] [--warmup 4] [--out profiles/r07_keypoint_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import keypoint_ref as kr  # noqa: E402
from openekfmonoslam_amd import engine  # noqa: E402
from openekfmonoslam_amd.synth import SyntheticSequence  # noqa: E402

RESPONSE = 1e10


def stage_ms(t):
    return {k: getattr(t, k) for k in ("prediction_ms", "matching_ms", "ransac_ms", "update_li_ms", "rescue_ms", "update_hi_ms")}


def run_case(w, h, nfeat, steps, warmup):
    frames = steps + warmup
    seq = SyntheticSequence(nfeat, frames + 1, width=w, height=h)
    img0 = seq.render_image(0)
    imgs = [seq.render_image(t) for t in range(1, frames + 1)]
    uv0 = seq.pixel_positions(0).astype(np.float64)
    desc0 = kr.describe(img0, uv0)
    eng = {}
    for name in ("keypoints", "ncc"):
        e = engine.EkfEngine(seq.cam, seq.par, nfeat + 8, max_keypoints=16384)
        e.set_state(seq.x13, seq.feature_pos, seq.feature_type, desc0, seq.P0)
        if name == "ncc":
            e.upload_image(img0)
            e.capture_templates(np.arange(nfeat), uv0)
        else:
            e.set_image_matcher(engine.IMAGE_MATCHER_KEYPOINTS, RESPONSE)
        e.upload_images(imgs)
        e.timing(True)
        eng[name] = e
    rec = {n: {"wall_ms": [], "stages": [], "matches": [], "inliers": []} for n in eng}
    kps = []
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
            r["inliers"].append(info.n_inliers + info.n_rescued)
            if name == "keypoints":
                kps.append(e.step_keypoints())
    # the detector alone on the last frame (whole frame, descriptors included, read-back included)
    e = eng["keypoints"]
    det = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        k, _ = e.detect_keypoints(RESPONSE, masked=False, capacity=16384)
        if i >= warmup:
            det.append((time.perf_counter() - t0) * 1e3)
    out = {"width": w, "height": h, "N": nfeat, "steps": steps, "warmup": warmup, "min_response": RESPONSE,
           "keypoints_detected_per_step": [a for a, _ in kps], "keypoints_kept_per_step": [b for _, b in kps],
           "whole_frame_keypoints": int(len(k)), "detect_keypoints_call_ms_median": float(np.median(det))}
    for name, r in rec.items():
        st = {k: float(np.median([s[k] for s in r["stages"]])) for k in r["stages"][0]}
        out[name] = {"step_wall_ms_median": float(np.median(r["wall_ms"])), "step_wall_ms_min": float(np.min(r["wall_ms"])),
                     "stage_ms_median": st, "matches_mean": float(np.mean(r["matches"])),
                     "inliers_mean": float(np.mean(r["inliers"]))}
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
    for w, h in ((640, 480), (1920, 1080)):
        for n in (200, 1000):
            r = run_case(w, h, n, a.steps, a.warmup)
            res.append(r)
            print(json.dumps({k: r[k] for k in ("width", "height", "N", "whole_frame_keypoints")}
                             | {"kp_step_ms": r["keypoints"]["step_wall_ms_median"], "ncc_step_ms": r["ncc"]["step_wall_ms_median"],
                                "kp_matching_ms": r["keypoints"]["stage_ms_median"]["matching_ms"],
                                "ncc_matching_ms": r["ncc"]["stage_ms_median"]["matching_ms"],
                                "kp_detected_mean": float(np.mean(r["keypoints_detected_per_step"]))}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
