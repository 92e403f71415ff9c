"""The C boundary of the fixed-map mode (include/ekf_engine.h) without a GPU: the built library exports the
three entry points, each refuses a NULL engine with EKF_ERR_INVALID_ARG, and the ABI version did not move."""
import ctypes as C

import pytest

from openekfmonoslam_amd import build, engine

INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    build.build_engine()
    return engine.load_library()


def test_library_exports_the_fixed_map_entry_points(lib):
    for name in ("ekf_update_fixed_map", "ekf_set_fixed_map", "ekf_get_fixed_map"):
        assert name in engine.ABI and hasattr(lib, name), name
    assert lib.ekf_abi_version() == 1


def test_null_engine_is_an_invalid_argument(lib):
    assert lib.ekf_update_fixed_map(None, None, 0) == INVALID_ARG
    assert lib.ekf_update_fixed_map(None, None, 3) == INVALID_ARG
    assert lib.ekf_set_fixed_map(None, 1) == INVALID_ARG
    assert lib.ekf_set_fixed_map(None, 0) == INVALID_ARG
    on, updates = C.c_int(7), C.c_int64(7)
    assert lib.ekf_get_fixed_map(None, C.byref(on), C.byref(updates)) == INVALID_ARG
    assert lib.ekf_get_fixed_map(None, None, None) == INVALID_ARG
    assert on.value == 7 and updates.value == 7  # nothing written


def test_wrapper_has_the_three_methods():
    for name in ("update_fixed_map", "set_fixed_map", "fixed_map"):
        assert callable(getattr(engine.EkfEngine, name))
