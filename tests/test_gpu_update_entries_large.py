"""The EKF update on either side of 2048 measurement rows, every entry of P and every component of the state under the bound of
tests/update_ref.py ("Stage tests of the update") -- the method of tests/test_gpu_update_entries.py, whose helpers are
reused, with the compiled long-double reference (tests/update_ref_fast.py) and C_ARITH_LARGE, measured at these cases
(tests/test_update_ref_fast_cpu.py).  No exclusion list, no outlier share.

Map: update_ref.case_map("large", 3157) -- 1032 features in view, 16 of them inverse-depth, n_pad = 3200 = 25 tiles of 128 with 85
live columns in the last.  M = 1024: m = 2048, 64 panels, the last size with the rows of B from digit planes inside the
(persistent) sweep, one full chunk of zero-piece masks in the downdate.  M = 1025: m = 2050, m_pad = 2080, 65 steps -- the second
mask chunk, parked in LDS, holds one step; the sweep factorises S alone in per-panel launches, inv(L) is formed and B comes from
k_b_gemm_i8p (exact configurations) or the fp64 GEMM.

Which bound.  Exact configurations: M = 1024 term (c) (rows of B from the planes in the sweep), M = 1025 term (d) (the int8 GEMM) on
every sweep mode of the default path.  EKF_UPDATE_PATH_SWEEP above 2048 rows (update_route.h: planes_b, gemm_planes and apriori all
false): the rows of B are fp64, dx = B'z is formed from them by k_dx_partial -- no digit term in the state -- and the downdate cuts
them into planes under MEASURED column scales: k_dx_partial leaves the largest exponent field of a column in Bexp (the rule of
k_col_exp) and k_slice_B shifts by 38 - (Bexp - 1022); terms (a) + (b) with those exponents, neither (c) nor (d)
(update_ref.with_bounds, exact="measured")."""
import numpy as np
import pytest

import update_ref as ur
from test_gpu_update_entries import WORST, check, eng_mod, fresh_engine, predicted_inputs, reference  # noqa: F401 (eng_mod: a fixture)

pytestmark = pytest.mark.gpu
PRECISIONS = (0, 2, 3)  # fp64, F32_EXACT, F64_EXACT
SWEEP = 1               # EKF_UPDATE_PATH_SWEEP
SINGLE, PAIRS = 1, 0    # EKF_SWEEP_SINGLE, EKF_SWEEP_PAIRS
N = ur.LARGE_N
COLUMN_BLOCKS = (N + 31) // 32


def run_large(eng_mod, M, precision, route, path=None, mode=None, dense=False, primed=True):
    e, cam = fresh_engine(eng_mod, "large", N, precision, path, mode, primed)
    if dense:
        e.dense_products(True)
    m, inputs = predicted_inputs(e, cam, M)
    assert np.array_equal(m["featureIndex"], np.arange(M)), "the first M features are the ones measured"
    exact = False
    if precision in (2, 3):  # (see the module docstring)
        exact = "measured" if path == SWEEP and M > 1024 else ("sweep" if M <= 1024 else "gemm")
    ref = reference(("large", N, M), inputs, precision, exact=exact, c_arith=ur.C_ARITH_LARGE)
    e.update(m)
    check(e, ref, inputs, f"large n = {N} M = {M}", precision, f"M{M} {route}")
    return e


def steps_and_zero_share(e, M):
    """plane0_pieces counts the bytes px_flag_plane0 writes: one per (32-column block, 16-row group) -- ceil(n / 32) x ceil(2 M / 16);
    a step of the downdate is 32 rows, two groups"""
    nz, total = e.plane0_pieces()
    groups = (2 * M + 15) // 16
    assert total == COLUMN_BLOCKS * groups, (total, groups)
    print(f"    plane 0: {nz} of {total} pieces hold anything; {(groups + 1) // 2} steps")
    return (groups + 1) // 2, (total - nz) / total


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("M", ur.LARGE_M)
def test_both_sides_of_the_row_boundary(eng_mod, M, precision):
    e = run_large(eng_mod, M, precision, "default")
    if precision in (2, 3):
        steps, zero = steps_and_zero_share(e, M)
        assert steps == (64 if M == 1024 else 65)
        assert zero >= 0.25  # the units take the step that skips zero pieces: at 65 steps, with parked masks


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("form", ["single", "pairs", "sweep-single"])
def test_routes_above_the_boundary(eng_mod, form, precision):
    path, mode = {"single": (None, SINGLE), "pairs": (None, PAIRS), "sweep-single": (SWEEP, SINGLE)}[form]
    e = run_large(eng_mod, 1025, precision, form, path, mode)
    if precision in (2, 3):
        assert steps_and_zero_share(e, 1025)[0] == 65


@pytest.mark.parametrize("precision", [2, 3])
def test_dense_products_above_the_boundary(eng_mod, precision):
    run_large(eng_mod, 1025, precision, "dense products", dense=True)


@pytest.mark.parametrize("precision", [2, 3])
def test_first_update_behind_an_upload_above_the_boundary(eng_mod, precision):
    """the averaging forms of the downdate: k_p_update_i8<true> in fp32 storage (65 steps without zero-piece masks), k_symmetrize_P
    in front of k_p_update_i8p in fp64 storage; B from k_b_gemm_i8p, whose units park their masks too"""
    run_large(eng_mod, 1025, precision, "first update", primed=False)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_state_only_update_above_the_boundary(eng_mod, precision):
    e, cam = fresh_engine(eng_mod, "large", N, precision)
    m, inputs = predicted_inputs(e, cam, 1025)
    ref = reference(("large", N, 1025), inputs, precision, update_cov=False, exact=False, c_arith=ur.C_ARITH_LARGE)
    e.update_only_state(m)
    check(e, ref, inputs, f"state only, n = {N} M = 1025", precision, "M1025 state only", update_cov=False)


def test_print_worst_ratios_of_the_large_cases():
    """(the table of DESIGN.md: worst |err| / tol per precision and route over the cases above)"""
    for (precision, route), w in sorted(WORST.items()):
        if route.startswith("M10"):
            print(f"precision {precision} route {route}:", {k: f"{v:.3f}" for k, v in sorted(w.items())})
