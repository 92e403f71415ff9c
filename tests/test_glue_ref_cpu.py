"""CPU only: the reference of tests/test_gpu_glue_kernels.py (one RANSAC hypothesis restated from the prediction tables, the
re-projection in np.longdouble, the loop formed as it goes) against the oracle's own RANSAC, on the scenes and lists the GPU tests
use.  The engine is replaced by a stand-in that answers the same calls from the oracle."""
import numpy as np
import pytest

import test_gpu_glue_kernels as gk


def oracle_engine(ol):
    class OracleEngine:
        def __init__(self, cam, par, cap, max_keypoints=0, precision=0):
            self.o = ol.Oracle(cam, par, cap)

        def set_state(self, *a):
            self.o.set_state(*a)

        def predict(self):
            self.o.predict()

        def predict_measurements(self, idx=None):
            self.p = self.o.predict_measurements(idx, want_HP=True)
            return self.p[0], self.p[1], self.p[2]

        def get_state(self, want_P=True):
            return self.o.x13(), self.o.feature_pos(), None

        def feature_layout(self):
            return self.o.feature_type(), self.o.feature_covpos()

        def hp_rows(self, fs):
            row = {int(f): k for k, f in enumerate(self.p[0]["featureIndex"])}
            return np.stack([self.p[3][row[int(f)]] for f in fs]), None

        def ransac(self, m):
            if len(m) == 0:
                return np.zeros(0, dtype=bool), 0
            preds, Hs, Hf = self.p[0], self.p[1], self.p[2]
            seen = set(preds["featureIndex"].tolist())
            miss = [int(f) for f in m["featureIndex"] if int(f) not in seen]
            if miss:  # a match of an unpredicted feature: the oracle wants a row for it, which no hypothesis of these lists reads
                extra = np.zeros(len(miss), dtype=preds.dtype)
                extra["featureIndex"] = miss
                preds = np.concatenate([preds, extra])
                Hs = np.concatenate([Hs, np.zeros((len(miss), 2, 13))])
                Hf = np.concatenate([Hf, np.zeros((len(miss), 2, 6))])
            mp, mHs, mHf = ol.align_to_matches(preds, Hs, Hf, m)
            mask, counts = self.o.ransac(mp, mHs, mHf, m)
            return mask, len(counts)

        def close(self):
            pass

    class Module:
        EkfEngine = OracleEngine

    return Module


@pytest.mark.parametrize("N", [1, 63, 65, 257])
def test_reference_loop_equals_oracle(oracle_lib, N):
    gk.test_ransac_full_loop_by_match_count(oracle_engine(oracle_lib), N, gk.F64)


def test_reference_per_hypothesis_equals_oracle(oracle_lib):
    gk.test_ransac_support_mask_and_count_per_hypothesis(oracle_engine(oracle_lib), 65, gk.F64)


def test_reference_feature_behind_the_camera_equals_oracle(oracle_lib):
    gk.test_ransac_feature_behind_the_camera(oracle_engine(oracle_lib), gk.F64)
