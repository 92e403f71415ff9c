"""tests/map_blob_ref.py, the numpy statement of the map blob's format, against itself and against numpy's own
triangle indexing: round trips in both layouts and element sizes at n on both sides of the kernels' 64-tile seams, the checksum's
sensitivity, the packed row offsets.  Everything is equality of bytes."""
import numpy as np
import pytest

import map_blob_ref as mb

SIZES = [13, 61, 67, 259, 514]


def types_for(n):
    """inverse-depth features, then XYZ ones, summing to n - 13"""
    r = n - 13
    n6 = r // 6 if r % 6 in (0, 3) else (r - 3) // 6
    while (r - 6 * n6) % 3:
        n6 -= 1
    return np.array([2] * n6 + [1] * ((r - 6 * n6) // 3), dtype=np.int32)


def blob_inputs(n, elem_bytes, symmetric, seed=0):
    rng = np.random.default_rng(seed + n)
    ft = types_for(n)
    N = ft.size
    A = rng.standard_normal((n, n))
    Pm = A @ A.T + n * np.eye(n) if symmetric else A + n * np.eye(n)
    if symmetric:
        Pm = np.triu(Pm) + np.triu(Pm, 1).T
    Pm = Pm.astype(np.float32 if elem_bytes == 4 else np.float64)
    x13 = rng.standard_normal(13)
    return dict(x13=x13, feat_pos=rng.standard_normal((N, 6)), feat_type=ft, desc=rng.integers(0, 256, (N, 32), dtype=np.uint8),
                times_predicted=rng.integers(0, 99, N).astype(np.uint32), times_matched=rng.integers(0, 99, N).astype(np.uint32), Pm=Pm,
                camera=rng.integers(0, 256, mb.CAMERA_BYTES, dtype=np.uint8).tobytes())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("elem_bytes", [4, 8])
@pytest.mark.parametrize("layout", [mb.TRIANGLE, mb.FULL])
def test_round_trip(n, elem_bytes, layout):
    inp = blob_inputs(n, elem_bytes, layout == mb.TRIANGLE)
    N = inp["feat_type"].size
    rng = np.random.default_rng(1)
    extra = dict(templates=rng.integers(0, 256, (N, 363), dtype=np.uint8), patch_normals=rng.integers(0, 256, (N, 48), dtype=np.uint8))
    blob = mb.build(**inp, p_elem_bytes=elem_bytes, p_layout=layout, desc_flags=0, **extra)
    p = mb.parse(blob)
    assert (p["N"], p["n"], p["p_elem_bytes"], p["p_layout"], p["total_bytes"]) == (N, n, elem_bytes, layout, blob.size)
    assert p["section_mask"] == mb.MASK_TEMPLATES | mb.MASK_PATCH_NORMALS
    assert mb.WARP_SOURCES not in p["sections"] and mb.WARP_POSES not in p["sections"]
    count = n * (n + 1) // 2 if layout == mb.TRIANGLE else n * n
    assert len(p["sections"][mb.P]) == count * elem_bytes
    back = mb.P_of(p)
    assert back.dtype == inp["Pm"].dtype and back.tobytes() == inp["Pm"].tobytes()  # pack -> unpack -> mirror reproduces P
    assert p["sections"][mb.X13] == inp["x13"].tobytes() and p["sections"][mb.TEMPLATES] == extra["templates"].tobytes()
    assert p["sections"][mb.CAMERA] == inp["camera"]
    assert mb.reassemble(p).tobytes() == blob.tobytes()
    for sid, sec in p["sections"].items():  # every section on a multiple of 64, gaps zero (parse checked them)
        off = int(np.frombuffer(blob[64 + 32 * sid + 8: 64 + 32 * sid + 16].tobytes(), "<u8")[0])
        assert off % 64 == 0 and blob[off:off + len(sec)].tobytes() == sec


def test_full_layout_keeps_both_triangles():
    inp = blob_inputs(67, 8, False)
    assert not np.array_equal(inp["Pm"], inp["Pm"].T)
    p = mb.parse(mb.build(**inp, p_elem_bytes=8, p_layout=mb.FULL, desc_flags=0))
    assert mb.P_of(p).tobytes() == inp["Pm"].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_row_offsets_against_triu_indices(n):
    rows, cols = np.triu_indices(n)
    first = np.flatnonzero(rows == cols)  # the diagonal entry opens every row of the packed triangle
    assert first.tolist() == [mb.tri_row(i, n) for i in range(n)]
    assert mb.tri_row(n, n) == n * (n + 1) // 2


def test_checksum_definition_and_sensitivity():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 4096, dtype=np.uint8)
    w = data.view("<u4")
    want = sum(int(v) * (2 * k + 1) for k, v in enumerate(w)) % (1 << 64)
    c0 = mb.checksum(data)
    assert c0 == want
    perm = rng.permutation(w.size)  # commutative: any order of summation
    assert sum(int(w[k]) * (2 * int(k) + 1) for k in perm) % (1 << 64) == c0
    flipped = data.copy()
    flipped[1234] ^= 0x10
    assert mb.checksum(flipped) != c0
    swapped = w.copy()
    assert swapped[10] != swapped[700]
    swapped[[10, 700]] = swapped[[700, 10]]
    assert mb.checksum(swapped.view(np.uint8)) != c0
    assert mb.checksum(data[:-4]) != c0
    assert mb.checksum(data[:5]) == mb.checksum(np.concatenate([data[:5], np.zeros(3, np.uint8)]))  # zero-padded to 4 bytes


def test_parse_refuses_corruption():
    inp = blob_inputs(61, 4, True)
    blob = mb.build(**inp, p_elem_bytes=4, p_layout=mb.TRIANGLE, desc_flags=0)
    mb.parse(blob)
    for at in (0, 9, 20, 30, 60, 100, 448, blob.size - 1, blob.size // 2):
        bad = blob.copy()
        bad[at] ^= 1
        with pytest.raises(ValueError):
            mb.parse(bad)
    for cut in (1, blob.size // 2, blob.size - 100):
        with pytest.raises(ValueError):
            mb.parse(blob[:-cut])
    with pytest.raises(ValueError):
        mb.parse(mb.reassemble(mb.parse(blob), n=64))
