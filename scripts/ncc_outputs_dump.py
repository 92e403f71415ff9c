"""Everything the NCC matcher's kernels produce on the small scenes of tests/, one .npz per mode combination, for a byte
comparison of two builds of the engine (a refactor of csrc/kernels_ncc.hip must not move a single byte):

    EKF_ENGINE_LIB=variants/libekf_engine_<tag>.so python scripts/ncc_outputs_dump.py --out DIR_A   # scripts/build_variant.sh
    python scripts/ncc_outputs_dump.py --out DIR_B
    python scripts/ncc_outputs_dump.py --compare DIR_A DIR_B      # np.array_equal on every array; exit status 1 on a difference

Scenes: tests/warp_scene.py (roll, approach, sideways; 40 features, 640 x 480), tests/tilted_scene.py (the orbit's frames 3 and
8 as tests/test_gpu_patch_normals.py drives them; 16 features, 320 x 240), tests/wide_scene.py (the displaced targets, and
gates larger than the frame).  Per match: the raw bytes of match_ncc()'s result, match_templates(), every mode's counters and,
with the patch normals on, patch_normals() before and after each estimator step."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tilted_scene as ts  # noqa: E402
import warp_scene as ws  # noqa: E402
import wide_scene as wsn  # noqa: E402
from ncc_wide_ref import blurred_noise  # noqa: E402
from openekfmonoslam_amd import engine  # noqa: E402
from openekfmonoslam_amd.ekftypes import MATCH_DTYPE  # noqa: E402
from test_template_warp_cpu import APPROACH_MARGIN, APPROACH_RATIO, IDENTITY, N_FEAT, ROLL_DEG  # noqa: E402

MODES = {  # name -> (warp, normals, subpix, wide)
    "off": (False, False, False, False),
    "warp": (True, False, False, False),
    "warp_normals": (True, True, False, False),
    "subpix": (False, False, True, False),
    "wide": (False, False, False, True),
    "wide_warp_subpix": (True, False, True, True),
}
WARP_SCENES = {"roll": (ROLL_DEG, 120.0), "approach": (APPROACH_RATIO, APPROACH_MARGIN), "sideways": (0.4, 120.0)}
WARP_FRAMES, WARP_AT = 10, (3, 6)
TILTED_AT = (3, 8)


def build_scenes():
    """rendered once, shared by every mode combination: name -> dict(cam, par, state, uv0, frame0, steps=[(n_predict, frame, truth)])"""
    out = {}
    plane = ws.PlaneScene()
    for kind, (amount, margin) in WARP_SCENES.items():
        poses = ws.trajectory(kind, WARP_FRAMES, amount)
        uv0, pts, fpos, ftype, x13, P = plane.seed_features(N_FEAT, margin=margin)
        v, w = ws.velocity(kind, WARP_FRAMES, amount)
        x13[7:10], x13[10:13] = v, np.where(w != 0, w, 2.22e-16)
        steps, done = [], 0
        for t in WARP_AT:
            steps.append((t - done, plane.render(poses[t], t), plane.true_pixels(poses[t], pts)[0]))
            done = t
        out["plane_" + kind] = dict(cam=plane.cam, par=plane.par, state=(x13, fpos, ftype, None, P), uv0=uv0,
                                    frame0=plane.render(IDENTITY, 0), steps=steps)
    tilted = ts.TiltedScene()
    poses = ts.orbit()
    uv0, pts, fpos, ftype, x13, P = tilted.seed_features()
    v, w = ts.orbit_velocity()
    x13[7:10], x13[10:13] = v, np.where(w != 0, w, 2.22e-16)
    steps, done = [], 0
    for t in TILTED_AT:
        steps.append((t - done, tilted.render(poses[t], t), tilted.true_pixels(poses[t], pts)[0]))
        done = t
    out["tilted"] = dict(cam=tilted.cam, par=tilted.par, state=(x13, fpos, ftype, None, P), uv0=uv0, frame0=tilted.render(poses[0], 0),
                         steps=steps)
    sc = wsn.DisplacedScene()
    out["wide_displaced"] = dict(cam=sc.cam, par=sc.par, state=(sc.x13, sc.fpos, sc.ftype, None, sc.P), uv0=sc.UV, frame0=sc.frame0,
                                 steps=[(0, sc.frame1, sc.target)])
    # a gate of about 2000 px (the box is the whole coarse level), one at the frame's corner, one narrow
    # (tests/test_gpu_ncc_wide.py::test_gate_larger_than_frame_and_off_frame, without its degenerate S)
    cam, par = wsn.s3_camera(wsn.W, wsn.H), wsn.s3_params()
    uv = np.array([[160.0, 120.0], [3.0, 3.0], [200.0, 60.0]])
    frame0, frame1 = blurred_noise(wsn.H, wsn.W, 51), blurred_noise(wsn.H, wsn.W, 52)
    frame1[8:72, 240:304] = frame0[88:152, 128:192]
    frame1[60:124, 40:104] = frame0[0:64, 0:64]
    frame1[28:92, 108:172] = frame0[28:92, 168:232]
    x13, fpos, ftype = wsn.seeded(cam, par, uv)
    P = wsn.diag_P(cam, 3, [2000.0, 88.0, 150.0], [2000.0, 88.0, 50.0])
    out["wide_frame"] = dict(cam=cam, par=par, state=(x13, fpos, ftype, None, P), uv0=uv, frame0=frame0,
                             steps=[(0, frame1, np.array([[272.0, 40.0], [43.0, 63.0], [140.0, 60.0]]))])
    return out


def normals_arrays(e, tag, rec):
    pn = e.patch_normals()
    for field in ("pq", "info", "updates", "normal"):
        rec[f"{tag}/normals_{field}"] = np.ascontiguousarray(pn[field])


def run(scene, name, mode, rec):
    warp, normals, subpix, wide = mode
    n = len(scene["uv0"])
    e = engine.EkfEngine(scene["cam"], scene["par"], n + 16)
    if warp:
        e.set_template_warp(True)
    if normals:
        e.set_patch_normals(True)
    e.set_subpixel_matches(subpix)
    e.set_ncc_wide_search(wide)
    e.set_state(*scene["state"])
    e.upload_image(scene["frame0"])
    e.capture_templates(np.arange(n), scene["uv0"])
    for s, (n_predict, frame, truth) in enumerate(scene["steps"]):
        tag = f"{name}/step{s}"
        for _ in range(n_predict):
            e.predict()
        preds, _, _ = e.predict_measurements()
        e.upload_image(frame)
        m = e.match_ncc()
        rec[f"{tag}/n_pred"] = np.array([len(preds)])
        rec[f"{tag}/matches"] = np.frombuffer(m.tobytes(), dtype=np.uint8)
        rec[f"{tag}/templates"] = e.match_templates(np.arange(n))
        rec[f"{tag}/counts"] = np.array(e.template_warp_counts() + e.subpixel_counts() + e.ncc_wide_counts() + e.patch_normal_counts())
        if normals:  # one estimator step at the rounded true pixels, then the match again: the warp now renders with the estimates
            anchors = np.zeros(n, dtype=MATCH_DTYPE)
            anchors["featureIndex"], anchors["imagePos"] = np.arange(n), np.rint(truth)
            normals_arrays(e, tag + "/before", rec)
            e.refine_patch_normals(anchors)
            normals_arrays(e, tag + "/after", rec)
            rec[f"{tag}/normal_counts"] = np.array(e.patch_normal_counts())
            m = e.match_ncc()
            rec[f"{tag}/matches_estimated"] = np.frombuffer(m.tobytes(), dtype=np.uint8)
            rec[f"{tag}/templates_estimated"] = e.match_templates(np.arange(n))
            rec[f"{tag}/counts_estimated"] = np.array(e.template_warp_counts())
    e.close()


def compare(dir_a, dir_b):
    bad = 0
    for mode in MODES:
        a, b = (np.load(os.path.join(d, mode + ".npz")) for d in (dir_a, dir_b))
        keys = sorted(set(a.files) | set(b.files))
        diff = [k for k in keys if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k])]
        nbytes = [sum(f[k].nbytes for k in f.files) for f in (a, b)]
        print(f"{mode}.npz: {len(keys)} arrays, {nbytes[0]} bytes" + (f" against {nbytes[1]}" if nbytes[1] != nbytes[0] else "") + ": " + ("equal" if not diff else "DIFFERENT: " + ", ".join(diff)))
        bad += len(diff)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if not a.out:
        ap.error("--out DIR or --compare DIR_A DIR_B")
    os.makedirs(a.out, exist_ok=True)
    scenes = build_scenes()
    for mode_name, mode in MODES.items():
        rec = {}
        for name, scene in scenes.items():
            run(scene, name, mode, rec)
        np.savez(os.path.join(a.out, mode_name + ".npz"), **rec)
        live = sum(int(v.any()) for v in rec.values())
        print(f"{mode_name}: {len(rec)} arrays, {live} not all zero", flush=True)


if __name__ == "__main__":
    main()
