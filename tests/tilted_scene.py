"""The textured plane of tests/warp_scene.py seen obliquely, for the patch-normal tests: the plane
passes through CENTRE = (0, 0, 4) and is tilted TILT_DEG about the y axis, so the camera of frame 0 (at the origin, identity
attitude) captures every feature at about 40 degrees to the surface.  Texture, camera model, noise and the inverse rendering
per pixel are PlaneScene's; only the ray / plane intersection and the texture's axes differ.

Trajectories: an orbit -- ORBIT_FRAMES frames over ORBIT_SPAN world units along x while the camera yaws to keep CENTRE on its
optical axis -- and a pure roll about the optical axis (no baseline: the image motion does not depend on the normal)."""
import numpy as np

import warp_scene as ws
from openekfmonoslam_amd.ekftypes import FEATURE_INVERSE_DEPTH
from openekfmonoslam_amd.synth import angles_to_quat, initial_state_and_covariance, quat_to_rot, seed_map, undistort

W, H = 320, 240
N_FEAT = 16
TILT_DEG = 40.0
CENTRE = np.array([0.0, 0.0, ws.PLANE_Z])
ORBIT_FRAMES, ORBIT_SPAN = 12, 1.2
ROLL_FRAMES, ROLL_DEG = 12, 20.0
_T = np.deg2rad(TILT_DEG)
E1 = np.array([np.cos(_T), 0.0, np.sin(_T)])   # texture x axis in the world: the plane is z = 4 + x tan(tilt)
E2 = np.array([0.0, 1.0, 0.0])                 # texture y axis
NORMAL = np.array([np.sin(_T), 0.0, -np.cos(_T)])  # unit normal, towards the cameras of both trajectories
IDENTITY = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))


def orbit(n_frames=ORBIT_FRAMES, span=ORBIT_SPAN):
    """poses [(r, q)] of frames 0..n_frames: r = (span t / n_frames, 0, 0), yaw about y so that CENTRE stays on the axis"""
    out = []
    for t in range(n_frames + 1):
        r = np.array([span * t / float(n_frames), 0.0, 0.0])
        yaw = np.arctan2(CENTRE[0] - r[0], CENTRE[2] - r[2])
        out.append((r, angles_to_quat(np.array([0.0, yaw, 0.0]))))
    return out


def roll(n_frames=ROLL_FRAMES, degrees=ROLL_DEG):
    return [(np.zeros(3), angles_to_quat(np.array([0.0, 0.0, np.deg2rad(degrees) * t / float(n_frames)]))) for t in range(n_frames + 1)]


def orbit_velocity(n_frames=ORBIT_FRAMES, span=ORBIT_SPAN):
    """(v, w) of the first orbit frame, for the filter's prior"""
    (r0, _), (r1, _) = orbit(n_frames, span)[:2]
    return r1 - r0, np.array([0.0, np.arctan2(CENTRE[0] - r1[0], CENTRE[2] - r1[2]), 0.0])


class TiltedScene(ws.PlaneScene):
    def __init__(self, width=W, height=H, seed=ws.SCENE_SEED, noise_sigma=1.0):
        super().__init__(width, height, seed, noise_sigma)

    def _lookup(self, X, Y):
        """PlaneScene's texture with its cells scaled to this frame size: CELL is "about 3 px at the seeding distance" at
        fx ~ 525 (640 x 480); at 320 x 240 the same cells would be 1.5 px (1.1 px along the tilt), and a texture that is
        point-sampled below two pixels per cell is aliased: its appearance changes with the sub-pixel phase, whatever the warp"""
        k = 640.0 / self.cam.pixelsX
        return super()._lookup((X + ws.TEX_HALF) / k - ws.TEX_HALF, (Y + ws.TEX_HALF) / k - ws.TEX_HALF)

    def _hit(self, r, d):
        """ray r + lam d against the tilted plane: (lam, texture coordinates)"""
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = float(NORMAL @ (CENTRE - r)) / (d @ NORMAL)
        P = r + lam[..., None] * d - CENTRE
        return lam, P @ E1, P @ E2

    def render(self, pose, frame_id=0):
        r, q = pose
        lam, a, b = self._hit(np.asarray(r, dtype=np.float64), self._rays @ quat_to_rot(q).T)
        ok = np.isfinite(lam) & (lam > 0)
        img = np.where(ok, self._lookup(np.where(ok, a, 0.0), np.where(ok, b, 0.0)), 118.0)
        rng = np.random.Generator(np.random.PCG64(self.seed * 1000 + frame_id))
        img = img + rng.normal(0.0, self.noise_sigma, img.shape)
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)

    def seed_features(self, n_features=N_FEAT, margin=80.0, seed=None, min_sep=16):
        """as PlaneScene.seed_features, the world points on the tilted plane"""
        rng = np.random.Generator(np.random.PCG64(self.seed + 17 if seed is None else seed))
        Wd, Ht = self.cam.pixelsX, self.cam.pixelsY
        uv0 = np.zeros((0, 2))
        while len(uv0) < n_features:
            c = np.array([rng.integers(int(margin), Wd - int(margin)), rng.integers(int(margin), Ht - int(margin))], dtype=np.float64)
            if len(uv0) == 0 or np.min(np.abs(uv0 - c).max(axis=1)) >= min_sep:
                uv0 = np.vstack([uv0, c])
        up = undistort(self.cam, uv0)
        ray = np.stack([(up[:, 0] - self.cam.cx) / self.cam.fx, (up[:, 1] - self.cam.cy) / self.cam.fy, np.ones(len(uv0))], axis=-1)
        lam, _, _ = self._hit(np.zeros(3), ray)
        pts = ray * lam[:, None]
        x13, P13 = initial_state_and_covariance(self.par)
        fpos, P = seed_map(self.cam, self.par, x13, P13, uv0)
        fpos[:, 5] = 1.0 / np.linalg.norm(pts, axis=1)
        ftype = np.full(n_features, FEATURE_INVERSE_DEPTH, dtype=np.int32)
        return uv0, pts, fpos, ftype, x13, P
