"""CPU-only checks of the map export (ekf_get_map_points): the numpy reference's Jacobians against finite
differences, its depth-feature case, the layout of EkfMapPoint on both sides of the ABI, and the exported symbol."""
import ctypes as C
import os
import subprocess

import numpy as np

import map_points_ref as mp
from openekfmonoslam_amd import build, engine, ekftypes
from openekfmonoslam_amd.synth import SyntheticSequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = {"xyz": 0, "cov": 24, "cam": 96, "cov_cam": 120, "linearity": 192, "type": 200, "covpos": 204,
           "times_predicted": 208, "times_matched": 212}


def central_difference(f, z):
    """d f / d z by central differences, step h = 1e-6 max(1, |component|): truncation ~h^2 and round-off ~u/h are both
    near 1e-10 relative"""
    z = np.asarray(z, dtype=np.float64)
    cols = []
    for k in range(len(z)):
        h = 1e-6 * max(1.0, abs(z[k]))
        zp, zm = z.copy(), z.copy()
        zp[k] += h
        zm[k] -= h
        cols.append((f(zp) - f(zm)) / (zp[k] - zm[k]))
    return np.stack(cols, axis=1)


def assert_rows_close(J, Jfd, rtol, what):
    scale = np.abs(J).max(axis=1, keepdims=True)  # relative to the largest entry of the Jacobian's row
    err = np.abs(J - Jfd) / scale
    assert err.max() <= rtol, (what, float(err.max()))


def jacobian_cases():
    seq = SyntheticSequence(50, 2)
    r, q = seq.x13[:3] + [0.3, -0.2, 0.1], seq.x13[3:7].copy()
    q = q + [0.0, 0.05, -0.11, 0.07]  # a camera that is neither at the origin nor axis-aligned
    q /= np.linalg.norm(q)
    cases = [("seq50[%d]" % i, seq.feature_pos[i].copy()) for i in (0, 17, 49)]
    y = seq.feature_pos[3].copy()
    y[3:5] = [1e-9, -2e-9]
    cases.append(("theta, phi near 0", y))
    y = seq.feature_pos[5].copy()
    y[5] = 0.02  # 50 m away.  1/rho makes the central difference's truncation (h / rho)^2 = 2.5e-9 relative here
    cases.append(("small rho", y))  # (h = 1e-6): still far inside rtol; at rho = 1e-3 the difference itself is only good to 1e-6
    return r, q, cases


def test_reference_jacobians_match_finite_differences():
    r, q, cases = jacobian_cases()
    I = mp.FEATURE_INVERSE_DEPTH
    for what, y in cases:
        _, Jw = mp.world_point(y, I)
        assert_rows_close(Jw, central_difference(lambda v: mp.world_point(v, I)[0], y), 1e-6, ("Jw", what))
        _, Jc = mp.camera_point(r, q, y, I)
        f = lambda z: mp.camera_point(z[:3], z[3:7], z[7:], I)[0]
        assert_rows_close(Jc, central_difference(f, np.r_[r, q, y]), 1e-6, ("Jc", what))
    # a depth feature: d = 3
    y = mp.world_point(cases[0][1], I)[0]
    _, Jc = mp.camera_point(r, q, y, mp.FEATURE_DEPTH)
    f = lambda z: mp.camera_point(z[:3], z[3:7], z[7:], mp.FEATURE_DEPTH)[0]
    assert Jc.shape == (3, 10)
    assert_rows_close(Jc, central_difference(f, np.r_[r, q, y]), 1e-6, "Jc depth")


def test_reference_depth_feature_is_the_stored_block():
    seq = SyntheticSequence(12, 1)
    # feature 4 as a depth feature: its rows 3..5 dropped from the state
    pos = 13 + 6 * 4
    keep = np.r_[0:pos + 3, pos + 6:len(seq.P0)]
    P = seq.P0[np.ix_(keep, keep)]
    ft = np.array(seq.feature_type, dtype=np.int32)
    ft[4] = mp.FEATURE_DEPTH
    covpos = 13 + np.r_[0, np.cumsum(np.where(ft == mp.FEATURE_INVERSE_DEPTH, 6, 3))[:-1]]
    fp = seq.feature_pos.copy()
    fp[4, :3] = mp.world_point(seq.feature_pos[4], mp.FEATURE_INVERSE_DEPTH)[0]
    fp[4, 3:] = 0.0
    ref = mp.map_points_ref(seq.x13, fp, ft, covpos, P)
    np.testing.assert_array_equal(ref["Jw"][4], np.eye(3))
    np.testing.assert_array_equal(ref["cov"][4], P[pos:pos + 3, pos:pos + 3])
    np.testing.assert_array_equal(ref["xyz"][4], fp[4, :3])
    assert ref["linearity"][4] == 1e300 and np.all(ref["linearity"][ft == mp.FEATURE_INVERSE_DEPTH] < 1e300)
    # an untouched inverse-depth neighbour reads the same block as before the removal
    np.testing.assert_array_equal(ref["cov"][5], ref["Jw"][5] @ seq.P0[pos + 6:pos + 12, pos + 6:pos + 12] @ ref["Jw"][5].T)
    assert np.all(ref["B"] >= np.abs(ref["cov"]) * (1 - 1e-15)) and np.all(ref["B_cam"] >= np.abs(ref["cov_cam"]) * (1 - 1e-15))


def test_map_point_layout_ctypes_and_numpy():
    assert C.sizeof(ekftypes.EkfMapPoint) == 216
    assert {n: getattr(ekftypes.EkfMapPoint, n).offset for n in OFFSETS} == OFFSETS
    dt = ekftypes.MAP_POINT_DTYPE
    assert dt.itemsize == 216 and {n: dt.fields[n][1] for n in OFFSETS} == OFFSETS
    assert dt["cov"].shape == (3, 3) and dt["cov_cam"].shape == (3, 3)


def test_map_point_layout_in_the_c_header(tmp_path):
    """the same numbers from include/ekf_types.h through the host C compiler (C99, as the ABI headers are)"""
    src = tmp_path / "layout.c"
    fields = ", ".join("(int)offsetof(EkfMapPoint, %s)" % n for n in OFFSETS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ekf_engine.h"\n'
                   'int main(void) { int o[] = {%s}; size_t i;\n'
                   '  printf("%%d", (int)sizeof(EkfMapPoint));\n'
                   '  for (i = 0; i < sizeof(o) / sizeof(o[0]); ++i) printf(" %%d", o[i]);\n'
                   '  printf("\\n"); return 0; }\n' % fields)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [216] + list(OFFSETS.values())


def test_library_exports_map_points():
    build.build_engine()
    lib = engine.load_library()
    assert "ekf_get_map_points" in engine.ABI
    restype, argtypes = engine.ABI["ekf_get_map_points"]
    assert restype is C.c_int and argtypes[1] == C.POINTER(ekftypes.EkfMapPoint)
    assert hasattr(lib, "ekf_get_map_points")
    n = C.c_int(-1)
    assert lib.ekf_get_map_points(None, None, 0, C.byref(n)) == 1  # EKF_ERR_INVALID_ARG: no engine
