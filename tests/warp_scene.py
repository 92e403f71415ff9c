"""A textured plane seen by a moving camera, for the template-warp tests: unlike synth.SyntheticSequence.render_image
(which pastes the same upright patch in every frame) the appearance of a point changes with the viewpoint here.

World: the plane z = PLANE_Z carries one large random texture, smooth enough to have gradients (random values on a
grid of CELL world units, bilinearly interpolated, in the spirit of synth._textures).  The camera is the project's
model: pinhole + radial distortion.  A frame is rendered by the inverse mapping per pixel: distorted pixel ->
synth.undistort -> ray -> plane -> bilinear texture lookup.  Frame 0 (camera at the origin, identity attitude) seeds
the map; trajectories: a pure roll about the optical axis, a pure approach along it, a sideways translation."""
import numpy as np

from openekfmonoslam_amd.ekftypes import FEATURE_INVERSE_DEPTH, s3_camera, s3_params
from openekfmonoslam_amd.synth import angles_to_quat, initial_state_and_covariance, project, quat_to_rot, seed_map, undistort

PLANE_Z = 4.0
CELL = 0.0225         # world units per texture cell: ~3 px at the seeding distance (fx ~ 525)
TEX_HALF = 12.0       # the texture covers |X|, |Y| <= TEX_HALF
SCENE_SEED = 0x7A49


def texture(seed=SCENE_SEED):
    n = int(2 * TEX_HALF / CELL) + 2
    return np.random.Generator(np.random.PCG64(seed)).uniform(30.0, 225.0, (n, n))


def trajectory(kind, n_frames, amount):
    """poses [(r, q)] of frames 0..n_frames; the motion is uniform (constant velocity).
    roll: `amount` degrees about the optical axis in total; approach: the distance to the plane shrinks to
    PLANE_Z / amount; sideways: `amount` world units along x."""
    out = []
    for t in range(n_frames + 1):
        a = t / float(n_frames)
        r, w = np.zeros(3), np.zeros(3)
        if kind == "roll":
            w[2] = np.deg2rad(amount) * a
        elif kind == "approach":
            r[2] = PLANE_Z * (1.0 - 1.0 / amount) * a
        elif kind == "sideways":
            r[0] = amount * a
        else:
            raise ValueError(kind)
        out.append((r, angles_to_quat(w)))
    return out


def velocity(kind, n_frames, amount):
    """(v, w) per frame of the same motion, for the filter's prior"""
    (r0, _), (r1, _) = trajectory(kind, n_frames, amount)[:2]
    w = np.array([0.0, 0.0, np.deg2rad(amount) / n_frames]) if kind == "roll" else np.zeros(3)
    return r1 - r0, w


class PlaneScene:
    def __init__(self, width=640, height=480, seed=SCENE_SEED, noise_sigma=1.0):
        self.cam, self.par = s3_camera(width, height), s3_params()
        self.tex = texture(seed)
        self.seed, self.noise_sigma = seed, noise_sigma
        ys, xs = np.mgrid[0:height, 0:width]
        up = undistort(self.cam, np.stack([xs, ys], axis=-1).astype(np.float64))
        self._rays = np.stack([(up[..., 0] - self.cam.cx) / self.cam.fx, (up[..., 1] - self.cam.cy) / self.cam.fy,
                               np.ones((height, width))], axis=-1)

    def _lookup(self, X, Y):
        gx, gy = (X + TEX_HALF) / CELL, (Y + TEX_HALF) / CELL
        n = self.tex.shape[0]
        inside = (gx >= 0) & (gx < n - 1) & (gy >= 0) & (gy < n - 1)
        gx, gy = np.clip(gx, 0, n - 1.001), np.clip(gy, 0, n - 1.001)
        x0, y0 = gx.astype(np.int64), gy.astype(np.int64)
        ax, ay = gx - x0, gy - y0
        t = self.tex
        v = (1 - ay) * ((1 - ax) * t[y0, x0] + ax * t[y0, x0 + 1]) + ay * ((1 - ax) * t[y0 + 1, x0] + ax * t[y0 + 1, x0 + 1])
        return np.where(inside, v, 118.0)

    def render(self, pose, frame_id=0):
        """uint8 [H, W] gray frame seen from pose = (r, q)"""
        r, q = pose
        d = self._rays @ quat_to_rot(q).T
        lam = (PLANE_Z - r[2]) / d[..., 2]
        img = self._lookup(r[0] + lam * d[..., 0], r[1] + lam * d[..., 1])
        img = np.where(lam > 0, img, 118.0)
        rng = np.random.Generator(np.random.PCG64(self.seed * 1000 + frame_id))
        img = img + rng.normal(0.0, self.noise_sigma, img.shape)
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)

    def seed_features(self, n_features, margin=120.0, seed=None, min_sep=16):
        """n_features integer pixels of frame 0 (camera at the origin) inside the margin, their world points on the
        plane, and a map seeded like synth.seed_map with the inverse depth set to the truth.
        Returns (uv0 float [N, 2], points [N, 3], feature_pos [N, 6], feature_type [N], x13, P)."""
        rng = np.random.Generator(np.random.PCG64(self.seed + 17 if seed is None else seed))
        W, H = self.cam.pixelsX, self.cam.pixelsY
        uv0 = np.zeros((0, 2))
        while len(uv0) < n_features:  # integer pixels, at least min_sep px apart
            c = np.array([rng.integers(int(margin), W - int(margin)), rng.integers(int(margin), H - int(margin))], dtype=np.float64)
            if len(uv0) == 0 or np.min(np.abs(uv0 - c).max(axis=1)) >= min_sep:
                uv0 = np.vstack([uv0, c])
        up = undistort(self.cam, uv0)
        ray = np.stack([(up[:, 0] - self.cam.cx) / self.cam.fx, (up[:, 1] - self.cam.cy) / self.cam.fy, np.ones(len(uv0))], axis=-1)
        pts = ray * PLANE_Z
        x13, P13 = initial_state_and_covariance(self.par)
        fpos, P = seed_map(self.cam, self.par, x13, P13, uv0)
        fpos[:, 5] = 1.0 / np.linalg.norm(pts, axis=1)
        ftype = np.full(n_features, FEATURE_INVERSE_DEPTH, dtype=np.int32)
        return uv0, pts, fpos, ftype, x13, P

    def true_pixels(self, pose, pts):
        r, q = pose
        uv, h = project(self.cam, r, quat_to_rot(q), pts)
        return uv, h
