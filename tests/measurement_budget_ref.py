"""numpy restatement of the measurement budget (ekf_set_measurement_budget) -- TEST INFRASTRUCTURE.

Of the features a step's full prediction sees, the K whose measurement carries most information about the state are measured.
The information of feature i is 0.5 ln(det S_i / det R) with S_i = H_i P H_i' + R its 2x2 innovation covariance; R = r I with
r = pixelErrorX for every feature, so the ranking is that of det S_i.

    scores(...)              S_i + (1 - r) I (what the engine keeps in its table: H_i P H_i' + I), key_i and gain_i
    rank_and_select(...)     rank_i = #{j : key_j > key_i, or equal and feature j < feature i}; selected = rank < K (all if np <= K)
    budgeted_oracle_step()   one EKF::step composed from the oracle's stages with the selection between prediction and matching
"""
import ctypes as C

import numpy as np

from openekfmonoslam_amd.ekftypes import FEATURE_INVERSE_DEPTH, KEYPOINT_DTYPE, EkfStepInfo


# the maps the device's ranks are checked on (tests/test_gpu_measurement_budget.py): (features, precision, features converted to
# depth first).  Every feature of a SyntheticSequence is in the frame, so np = N: 63 / 64 / 65 straddle a wavefront of the score
# kernel's workgroups, 255 / 256 / 257 a tile and a workgroup of the rank kernel (and the size up to which k_predict_features
# compacts its own list), 1030 is more than the 1024 threads of k_compact and several rank tiles.
RANK_MAPS = [(12, 0, 0), (63, 0, 0), (64, 0, 0), (65, 0, 0), (255, 0, 0), (256, 0, 0), (257, 0, 0), (1030, 1, 0), (50, 0, 5),
             (50, 1, 0), (50, 2, 0), (50, 3, 0)]


def budget_candidates(n_pred):
    return sorted(set([1, 2, n_pred // 2, n_pred - 1]))


def scores(P, feat_idx, ftype, covpos, Hs, Hf, pixel_error):
    """P [n, n]; feat_idx [np] the predicted features; ftype / covpos [N] the map layout; Hs [np, 2, 13] (columns 7..12 are
    structurally zero), Hf [np, 2, 6] -> (S_tab [np, 2, 2] = H_i P H_i' + I, key [np], gain [np]).  A key that is NaN or not
    positive becomes -1 and its gain 0."""
    P = np.asarray(P, dtype=np.float64)
    r = float(pixel_error)
    S_tab = np.zeros((len(feat_idx), 2, 2))
    key = np.zeros(len(feat_idx))
    for k, fi in enumerate(np.asarray(feat_idx, dtype=np.int64)):
        d = 6 if ftype[fi] == FEATURE_INVERSE_DEPTH else 3
        cols = np.concatenate([np.arange(7), covpos[fi] + np.arange(d)])
        H = np.concatenate([np.asarray(Hs[k])[:, :7], np.asarray(Hf[k])[:, :d]], axis=1)
        S_tab[k] = H @ P[np.ix_(cols, cols)] @ H.T + np.eye(2)
        S = S_tab[k] - np.eye(2) + r * np.eye(2)
        key[k] = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    bad = ~(key > 0)  # NaN too
    key[bad] = -1.0
    gain = np.zeros_like(key)
    gain[~bad] = 0.5 * np.log(key[~bad] / (r * r))
    return S_tab, key, gain


def clean_keys(keys):
    keys = np.array(keys, dtype=np.float64)
    keys[~(keys > 0)] = -1.0
    return keys


def rank_and_select(keys, feat_idx, K):
    """-> (rank [np] int, selected [np] bool).  The order the inputs come in does not matter: rank and selection belong to
    the (key, feature index) pairs."""
    keys = clean_keys(keys)
    feat_idx = np.asarray(feat_idx, dtype=np.int64)
    n = len(keys)
    order = sorted(range(n), key=lambda i: (-keys[i], feat_idx[i]))
    rank = np.zeros(n, dtype=np.int64)
    rank[order] = np.arange(n)
    selected = np.ones(n, dtype=bool) if n <= K else rank < K
    return rank, selected


def usable_budgets(keys, feat_idx, candidates, rel_gap=1e-9):
    """the K of `candidates` (0 < K < np) at which the keys of ranks K - 1 and K differ by at least rel_gap relative: there the
    selected set does not hang on the last bits of a key"""
    keys = clean_keys(keys)
    rank, _ = rank_and_select(keys, feat_idx, len(keys))
    by_rank = keys[np.argsort(rank)]
    out = []
    for K in candidates:
        if 0 < K < len(keys):
            a, b = by_rank[K - 1], by_rank[K]
            if abs(a - b) >= rel_gap * max(abs(a), abs(b)):
                out.append(K)
    return out


def _view(ptr, n, dtype):
    """a writable numpy view of n elements behind a ctypes pointer into the oracle's own memory"""
    return np.ctypeslib.as_array(ptr, (n,)) if n > 0 else np.zeros(0, dtype=dtype)


def budgeted_oracle_step(o, kps, desc, K, variant=0):
    """EKF::step of the oracle `o` (tests/oracle_lib.Oracle) with a measurement budget of K, composed from its stages in the
    order of orc_step: predict, predict_measurements of all features, the selection, match on the selected predictions, RANSAC,
    update, predict_measurements of the outliers, rescue, update, and the timesPredicted / timesMatched / descriptor
    bookkeeping for the selected only.  K <= 0 or K >= predicted features: nothing is left out and the result is o.step's,
    bit for bit.  -> (EkfStepInfo, feature indices predicted, feature indices selected, matches)"""
    import oracle_lib as ol

    kps = np.ascontiguousarray(kps, dtype=KEYPOINT_DTYPE)
    d = o._desc(desc)
    N = o.N
    info = EkfStepInfo()
    o.predict()
    preds, Hs, Hf = o.predict_measurements()
    predicted = preds["featureIndex"].astype(np.int64)
    if 0 < K < len(preds):
        _, keys, _ = scores(o.P(), predicted, o.feature_type(), o.feature_covpos(), Hs, Hf, o.cam.pixelErrorX)
        _, sel = rank_and_select(keys, predicted, K)
        preds, Hs, Hf = preds[sel], Hs[sel], Hf[sel]
    selected = preds["featureIndex"].astype(np.int64)
    info.n_predicted = len(preds)
    tp = _view(o.L.orc_feature_times_predicted(o.h), N, np.uint32)
    tm = _view(o.L.orc_feature_times_matched(o.h), N, np.uint32)
    fdesc = _view(o.L.orc_feature_desc(o.h), N * o.desc_bytes, np.uint8).reshape(N, o.desc_bytes)
    tp[selected] += 1

    def matched(sel_matches):
        for m in sel_matches:
            fi = int(m["featureIndex"])
            tm[fi] += 1
            fdesc[fi] = d[int(m["keypointIndex"])]

    matches = o.match(preds, kps, d)
    M = len(matches)
    info.n_matches = M
    mp, mHs, mHf = ol.align_to_matches(preds, Hs, Hf, matches) if M else (preds[:0], Hs[:0], Hf[:0])
    mask = np.zeros(max(M, 1), dtype=np.uint8)
    m_c, mp_c, mHs_c, mHf_c = (np.ascontiguousarray(a) for a in (matches, mp, mHs, mHf))
    info.n_hypotheses = o.L.orc_ransac(o.h, ol._p(mp_c), ol._p(mHs_c), ol._p(mHf_c), ol._p(m_c), M, ol._p(mask), None)
    mask = mask[:M].astype(bool)
    inl, outl = matches[mask], matches[~mask]
    info.n_inliers, info.n_outliers = len(inl), len(outl)
    matched(inl)
    status = o.update(inl, mp[mask], mHs[mask], mHf[mask], variant)
    no, nop, nr = len(outl), 0, 0
    if no > 0:
        mp2, mHs2, mHf2 = o.predict_measurements(outl["featureIndex"].astype(np.int32))
        nop = len(mp2)
        if 0 < nop < no:  # keep only the outlier matches whose prediction fell inside the frame (EKF.cpp:483-499)
            keep, j = [], 0
            for i in range(no):
                if j < nop and outl["featureIndex"][i] == mp2["featureIndex"][j]:
                    keep.append(i)
                    j += 1
            outl = outl[keep]
            no = len(outl)
        if no > 0 and nop > 0:
            rmask = o.rescue(outl, mp2[:no])
            resc = outl[rmask]
            nr = len(resc)
            matched(resc)
            if nr > 0:
                st = o.update(resc, mp2[:no][rmask], mHs2[:no][rmask], mHf2[:no][rmask], variant)
                status = st if st else status
    info.n_rescued = nr
    info.status = status
    return info, predicted, selected, matches
