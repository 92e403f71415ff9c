"""Scenes for the wide-search tests, 320 x 240, shared by test_ncc_wide_cpu.py and
test_gpu_ncc_wide.py.

The gates are set through the covariance: diag_P gives every feature an independent direction uncertainty (theta, phi of
its inverse-depth parameters) and nothing else, so that S = H P H' + R is close to diag(sig_u^2, sig_v^2) in pixels and
the gate's semi-axes are 2 sqrt(5.99) sig = 4.895 sig."""
import numpy as np

from ncc_wide_ref import blurred_noise
from openekfmonoslam_amd.ekftypes import FEATURE_INVERSE_DEPTH, s3_camera, s3_params
from openekfmonoslam_amd.synth import initial_state_and_covariance, seed_map

W, H = 320, 240
AXIS_PER_SIGMA = 2.0 * np.sqrt(5.9915)


def diag_P(cam, n_feat, axis_u, axis_v):
    """covariance whose gates have semi-axes of about axis_u, axis_v pixels (scalars or one value per feature)"""
    P = np.zeros((13 + 6 * n_feat, 13 + 6 * n_feat))
    P[np.arange(13), np.arange(13)] = 2.22e-16
    au, av = np.broadcast_to(axis_u, n_feat), np.broadcast_to(axis_v, n_feat)
    for i in range(n_feat):
        n0 = 13 + 6 * i
        P[n0 + 3, n0 + 3] = (au[i] / AXIS_PER_SIGMA / cam.fx) ** 2
        P[n0 + 4, n0 + 4] = (av[i] / AXIS_PER_SIGMA / cam.fy) ** 2
    return P


def seeded(cam, par, uv):
    """(x13, feature_pos, feature_type) of a camera at the origin with one inverse-depth feature per pixel of uv"""
    x13, P13 = initial_state_and_covariance(par)
    fpos, _ = seed_map(cam, par, x13, P13, uv)
    return x13, fpos, np.full(len(uv), FEATURE_INVERSE_DEPTH, dtype=np.int32)


class DisplacedScene:
    """Eight features seeded on frame0 (blurred noise); frame1 is other noise into which the 64 x 64 surroundings of every
    feature are pasted 100 px from where the resting camera predicts it.  Seeds and displacements are multiples of 4, so
    the pasted surroundings are the same bytes on all three pyramid levels and the true pixel scores exactly 1."""
    UV = np.array([[68, 44], [120, 124], [208, 56], [196, 124], [156, 192], [36, 104], [280, 196], [152, 44]], dtype=np.float64)
    SHIFT = np.array([[80, 60], [-80, -60], [80, 60], [60, 80], [-80, -60], [0, 100], [-100, 0], [60, 80]], dtype=np.float64)
    MAJOR = 150.0

    def __init__(self):
        self.cam, self.par = s3_camera(W, H), s3_params()
        self.n = len(self.UV)
        self.target = self.UV + self.SHIFT
        self.frame0 = blurred_noise(H, W, 31)
        self.frame1 = blurred_noise(H, W, 32)
        for (u, v), (tu, tv) in zip(self.UV.astype(int), self.target.astype(int)):
            assert 32 <= tu <= W - 32 and 32 <= tv <= H - 32
            self.frame1[tv - 32:tv + 32, tu - 32:tu + 32] = self.frame0[v - 32:v + 32, u - 32:u + 32]
        centres = self.target
        d = np.abs(centres[:, None, :] - centres[None, :, :]).max(axis=2) + 1000 * np.eye(self.n)
        assert d.min() >= 64, "pasted surroundings overlap"
        d = np.abs(self.UV[:, None, :] - self.UV[None, :, :]).max(axis=2) + 1000 * np.eye(self.n)
        assert d.min() >= 56, "a feature's coarse template lies in another feature's pasted surroundings"
        self.x13, self.fpos, self.ftype = seeded(self.cam, self.par, self.UV)
        self.P = diag_P(self.cam, self.n, self.MAJOR, self.MAJOR)

    def load(self, f):
        """state, frame0's templates, then frame1, into an engine or an oracle (the calls they share)"""
        f.set_state(self.x13, self.fpos, self.ftype, None, self.P)
        (f.upload_image if hasattr(f, "upload_image") else f.set_image)(self.frame0)
        f.capture_templates(np.arange(self.n), self.UV)
        (f.upload_image if hasattr(f, "upload_image") else f.set_image)(self.frame1)


def periodic_frame(period=32, seed=41):
    """a frame that repeats one period x period cell of blurred noise exactly; period is a multiple of 4, so levels 1 and
    2 repeat too (with period / 2 and period / 4)"""
    cell = blurred_noise(period, period, seed)
    return np.tile(cell, (H // period + 1, W // period + 1))[:H, :W].copy()
