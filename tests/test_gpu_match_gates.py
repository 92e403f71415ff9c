"""GPU: the descriptor matcher's gates at the boundary of the ellipse -- read from the table that the launch forming S_f (k_hp_rows)
fills for a full prediction of more than 256 features, or formed by k_match itself: on smaller maps, and whenever something
rewrote the prediction tables between the prediction and the matcher.

Scenes: tests/predict_ref.py's general pose with both feature types, every feature in view, N = 12 and N = 300, and a covariance
built here so that a dozen gates have the shapes that matter: a circle (aw == ah: the foci coincide; a covariance block that is
isotropic in the image), strongly elongated gates turned against the image axes (an XYZ feature uncertain along one world
direction, an inverse-depth feature uncertain in its angles), one of them partly outside the image; every other gate is the 8 x 7 pixel ellipse of the prediction's process noise.  The
covariance is representable in fp32, and the gates the keypoints are placed around are those of the engine's own predictions
(ekf_predict_measurements returns S_f in fp64), so the reference -- oracle.match on those predictions -- sees the ellipses the
device sees in either precision.

Keypoints: all descriptors are equal, so the gate alone decides.  A round of the test holds, per test gate, one keypoint at the
centre and ONE probe behind it in keypoint order: with equal distances the matcher returns the second candidate of a gate, i.e. the
probe if it is inside and the centre if it is not -- every probe decides its gate's match.  The probes of a gate, one per round:
along 8 rays through the centre the two float32 points on either side of the boundary (bisection on oracle.point_in_ellipse of
the float32-rounded point), four directions just inside and just outside the bounding circle of radius `major`, the centre
itself, and far away.  A probe that lands in another test gate, or on which oracle.match and oracle.point_in_ellipse disagree, is dropped (moved far away) before the reference is taken: the reference holds on its own.

The table is invalidated by a subset prediction between predict_measurements and match (it rewrites pred_uv and pred_S of its
features with the same numbers; ekf_rescue itself predicts nothing): k_match then forms its gates itself.  At N = 12 both cases
take that path (the table is written above 256 features only); at N = 300 "valid" reads the table."""
import numpy as np
import pytest

import predict_ref as pr
from openekfmonoslam_amd.ekftypes import KEYPOINT_DTYPE

pytestmark = pytest.mark.gpu

N_GATES = 12
RAYS = 8
FAR = (-5000.0, -5000.0)  # a keypoint in nobody's gate


@pytest.fixture(scope="module")
def eng_mod():
    from openekfmonoslam_amd import engine

    lib = engine.load_library()
    assert lib.ekf_device_count() >= 1, "no MI355X visible"
    return engine


def mixed_types(N):
    return np.where(np.arange(N) % 3 == 0, pr.FEATURE_INVERSE_DEPTH, pr.FEATURE_DEPTH).astype(np.int32)


def gate_features(s):
    """a dozen features whose predicted pixels are far from each other: greedy farthest-point choice from feature 0 (the scene's
    pixels are hashed over the frame), both types among them"""
    i = np.arange(s.n_features)
    uv = np.stack([40.0 + (s.cam.pixelsX - 80.0) * pr._hash01(i, 2), 40.0 + (s.cam.pixelsY - 80.0) * pr._hash01(i, 3)], -1)
    chosen = [0]
    while len(chosen) < min(N_GATES, s.n_features):
        d = np.min(np.linalg.norm(uv[:, None, :] - uv[None, chosen, :], axis=2), axis=1)
        chosen.append(int(np.argmax(d)))
    return chosen


def shaped_covariance(s, feats, Hf0):
    """1e-8 I, plus per test gate: feats[0] a block that is isotropic IN THE IMAGE (12 px: pinv(Hf) pinv(Hf)' with the feature's
    own measurement Jacobian Hf0 -- the circle), then alternately a rank-one block along a skew direction (XYZ: metres; inverse
    depth: the two angles) of growing size, every fourth left alone"""
    P = np.eye(s.n) * 1e-8
    for k, f in enumerate(feats):
        pos = int(s.covpos[f])
        inv = s.feature_type[f] == pr.FEATURE_INVERSE_DEPTH
        if k == 0:
            d = 6 if inv else 3
            Jp = np.linalg.pinv(Hf0[:, :d])
            P[pos:pos + d, pos:pos + d] += 12.0 ** 2 * Jp @ Jp.T
        elif k % 4 == 3:
            continue
        elif inv:
            v = np.zeros(6)
            v[3], v[4] = 1.0, 0.5
            P[pos:pos + 6, pos:pos + 6] += (0.01 * (1 + k % 3)) ** 2 * np.outer(v, v)
        else:
            v = np.array([1.0, 0.6, 0.1])
            v /= np.linalg.norm(v)
            P[pos:pos + 3, pos:pos + 3] += (0.05 * (1 + k % 3)) ** 2 * np.outer(v, v)
    P = 0.5 * (P + P.T)
    return P.astype(np.float32).astype(np.float64)


def ellipses(o, preds):
    """per prediction (aw, ah, angle, cx, cy) as the matcher forms them: float axes rounded half to even, float centre"""
    out = []
    for p in preds:
        ax, ang = o.ellipse(p["covarianceMatrix"])
        out.append((int(np.rint(ax[0])), int(np.rint(ax[1])), ang, np.float32(p["imagePos"][0]), np.float32(p["imagePos"][1])))
    return out


_SCENES = {}


def scene(oracle_lib, N):
    """(scene, P0, test features); the circle's block needs the feature's measurement Jacobian: the oracle's, here on the CPU"""
    if N not in _SCENES:
        s = pr.make_scene(mixed_types(N), vis=np.ones(N, dtype=bool), with_P0=False)
        feats = gate_features(s)
        o = oracle_lib.Oracle(s.cam, s.par, N + 8)
        o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, np.eye(s.n) * 1e-8)
        o.predict()
        preds, _, Hf = o.predict_measurements()
        k = int(np.nonzero(preds["featureIndex"] == feats[0])[0][0])
        _SCENES[N] = (s, shaped_covariance(s, feats, Hf[k]), feats)
    return _SCENES[N]


def boundary_pair(o, el, theta):
    """the last inside and the first outside float32 point along the ray from the centre at angle theta"""
    aw, ah, ang, cx, cy = el
    inside = lambda t: o.point_in_ellipse(float(np.float32(cx + t * np.cos(theta))), float(np.float32(cy + t * np.sin(theta))),
                                          float(cx), float(cy), aw, ah, ang)
    lo, hi = 0.0, float(max(aw, ah)) + 2.0
    assert inside(lo) and not inside(hi)
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if inside(mid):
            lo = mid
        else:
            hi = mid
    pt = lambda t: (float(np.float32(cx + t * np.cos(theta))), float(np.float32(cy + t * np.sin(theta))))
    return pt(lo), pt(hi)


def probes_of(o, el, k):
    """the probes of one gate (see the module docstring); k turns the rays so that the gates do not share directions"""
    aw, ah, ang, cx, cy = el
    major = float(max(aw, ah))
    out = []
    for r in range(RAYS):
        out.extend(boundary_pair(o, el, 2.0 * np.pi * (r + 0.37 * k / N_GATES) / RAYS))
    for r in range(4):  # the bounding circle: along and across the major axis, and in between
        th = ang + (0.0 if ah < aw else np.pi / 2) + r * np.pi / 4
        for rad in (major * (1.0 - 1e-6), major * (1.0 + 1e-6), major * (1.0 + 1e-3)):
            out.append((float(np.float32(cx + rad * np.cos(th))), float(np.float32(cy + rad * np.sin(th)))))
    out.append((float(cx), float(cy)))
    out.append(FAR)
    return out


def build_rounds(o, preds, feats):
    """([(keypoints, descriptors)] per round, probes dropped, probes kept, the test gates, their features); preds: the predictions
    the gates are taken from"""
    slot = {int(f): k for k, f in enumerate(preds["featureIndex"])}
    els = ellipses(o, preds)
    # a test gate whose centre lies inside another test gate (or that holds another's centre) would not be decided by its own probe:
    # it is left out (never the circle, feats[0])
    kept = []
    for f in feats:
        a = els[slot[f]]
        clash = any(o.point_in_ellipse(float(a[3]), float(a[4]), float(b[3]), float(b[4]), b[0], b[1], b[2]) or
                    o.point_in_ellipse(float(b[3]), float(b[4]), float(a[3]), float(a[4]), a[0], a[1], a[2])
                    for b in (els[slot[h]] for h in kept))
        if not clash:
            kept.append(f)
    feats = kept
    gates = [els[slot[f]] for f in feats]
    probes = [probes_of(o, g, k) for k, g in enumerate(gates)]
    n_rounds = max(len(p) for p in probes)
    G = len(gates)
    rounds, dropped, decided = [], 0, 0
    for r in range(n_rounds):
        kps = np.zeros(2 * G + 3, dtype=KEYPOINT_DTYPE)
        kps["x"], kps["y"] = FAR
        for g, el in enumerate(gates):
            kps["x"][g], kps["y"][g] = el[3], el[4]
            if r < len(probes[g]):
                kps["x"][G + g], kps["y"][G + g] = probes[g][r]
        desc = np.zeros((len(kps), 32), dtype=np.uint8)
        for attempt in range(2):
            want = {}
            for g, el in enumerate(gates):
                ins = [j for j in range(len(kps)) if o.point_in_ellipse(float(kps["x"][j]), float(kps["y"][j]), float(el[3]), float(el[4]),
                                                                         el[0], el[1], el[2])]
                want[feats[g]] = ins
            m = o.match(preds, kps, desc)
            got = {int(f): int(k) for f, k in zip(m["featureIndex"], m["keypointIndex"])}
            bad = []
            for g, f in enumerate(feats):
                ins = want[f]
                # the centre and at most the gate's own probe; equal distances: the second candidate wins
                clean = ins in ([g], [g, G + g])
                if not clean or got.get(f) != ins[-1]:
                    bad.append(g)
            if not bad:
                break
            assert attempt == 0, "a dropped probe cannot disagree again"
            drop = set()
            for b in bad:  # probes of other gates that landed in this one; without any, the gate's own probe is the disagreement
                foreign = [j - G for j in want[feats[b]] if j >= G and j != G + b]
                drop.update(foreign if foreign else [b])
            for g in drop:
                kps["x"][G + g], kps["y"][G + g] = FAR
            dropped += len(drop)
        decided += sum(1 for g in range(G) if kps["x"][G + g] != FAR[0])
        rounds.append((kps, desc))
    return rounds, dropped, decided, gates, feats


def check_shapes(s, gates):
    kinds = {"circle": False, "elongated": False, "off_image": False}
    for aw, ah, ang, cx, cy in gates:
        major, minor = max(aw, ah), min(aw, ah)
        kinds["circle"] |= aw == ah
        turned = min(abs(np.sin(ang)), abs(np.cos(ang))) > 0.2
        kinds["elongated"] |= major >= 3 * minor and turned
        kinds["off_image"] |= major >= 3 * minor and (cx - major < 0 or cy - major < 0 or cx + major > s.cam.pixelsX or cy + major > s.cam.pixelsY)
    assert all(kinds.values()), (kinds, gates)


@pytest.mark.parametrize("table", ["valid", "invalidated"])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("N", [12, 300])
def test_match_lists_at_the_gate_boundary_equal_the_oracle(eng_mod, oracle_lib, N, precision, table):
    s, P0, feats = scene(oracle_lib, N)
    e = eng_mod.EkfEngine(s.cam, s.par, N + 8, max_keypoints=64, precision=precision)
    o = oracle_lib.Oracle(s.cam, s.par, N + 8)
    e.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, P0)
    o.set_state(s.x13, s.feature_pos, s.feature_type, s.desc, P0)
    e.predict()
    preds, _, _ = e.predict_measurements()
    assert len(preds) == N
    assert {int(t) for t in s.feature_type[feats]} == {pr.FEATURE_INVERSE_DEPTH, pr.FEATURE_DEPTH}
    rounds, dropped, decided, gates, feats = build_rounds(o, preds, feats)
    assert len(feats) >= 10
    check_shapes(s, gates)
    assert decided >= 20 * len(feats) and dropped <= decided // 10, (decided, dropped)
    if table == "invalidated":
        sub = np.array(sorted(feats[::2]), dtype=np.int32)
        again, _, _ = e.predict_measurements(sub)
        lut = {int(p["featureIndex"]): p for p in preds}
        for p in again:  # the same numbers: only the table's validity changes
            assert p["imagePos"].tolist() == lut[int(p["featureIndex"])]["imagePos"].tolist()
            assert p["covarianceMatrix"].tolist() == lut[int(p["featureIndex"])]["covarianceMatrix"].tolist()
    probes_in = 0
    for r, (kps, desc) in enumerate(rounds):
        ref = o.match(preds, kps, desc)
        got = e.match(kps, desc)
        np.testing.assert_array_equal(got, ref, err_msg=f"round {r}")
        probes_in += int(np.sum(ref["keypointIndex"] >= len(feats)))
    assert probes_in >= 8 * len(feats)  # (both outcomes occur: about half of the probes are inside)
    e.close()
