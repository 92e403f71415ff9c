"""The map blob of ekf_save_map / ekf_load_map in numpy, written from the format's description and not from the
C++: builds blobs from plain arrays, parses them back, and recomputes checksums so that a test can hand the engine a blob that is
wrong in exactly one respect.

Little-endian.  Header: 64 bytes + 12 directory entries of 32 bytes = 448.  Sections in id order, each on a multiple of 64, gaps
zero, the blob ends with the last section.  Checksum of a byte range: sum of w_k (2 k + 1) mod 2^64 over its 32-bit words."""
import struct

import numpy as np

MAGIC = b"EKFMAP01"
HEADER_BYTES = 448
(X13, FEAT_POS, FEAT_TYPE, DESC, TIMES_PREDICTED, TIMES_MATCHED, P, TEMPLATES, WARP_SOURCES, WARP_POSES, PATCH_NORMALS,
 CAMERA) = range(12)
NAMES = ["X13", "FEAT_POS", "FEAT_TYPE", "DESC", "TIMES_PREDICTED", "TIMES_MATCHED", "P", "TEMPLATES", "WARP_SOURCES", "WARP_POSES",
         "PATCH_NORMALS", "CAMERA"]
TRIANGLE, FULL = 0, 1
MASK_TEMPLATES, MASK_WARP_SOURCES, MASK_PATCH_NORMALS = 1, 2, 4
TEMPLATE_BYTES, WARP_SOURCE_BYTES, PATCH_NORMAL_BYTES, CAMERA_BYTES = 363, 3 * 1681, 48, 104
_FIXED = "<8sIIQiiiiiiIIQ"  # magic version header_bytes total N n p_elem p_layout desc_bytes desc_flags mask zero checksum
_ENTRY = "<IIQQQ"           # id elem_bytes offset bytes checksum
assert struct.calcsize(_FIXED) == 64 and struct.calcsize(_ENTRY) == 32


def checksum(data):
    b = np.frombuffer(bytes(data), dtype=np.uint8)
    pad = (-b.size) % 4
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    w = b.view("<u4").astype(np.uint64)
    k = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int((w * (np.uint64(2) * k + np.uint64(1))).sum(dtype=np.uint64))


def tri_row(i, n):
    """first element of row i of the packed upper triangle"""
    return i * n - i * (i - 1) // 2


def pack_P(Pm, elem_bytes, layout):
    """n x n matrix -> the P section's elements (storage type, no averaging: the triangle takes the entries on and above the diagonal)"""
    dt = np.dtype("<f4") if elem_bytes == 4 else np.dtype("<f8")
    Pm = np.asarray(Pm)
    n = Pm.shape[0]
    flat = Pm[np.triu_indices(n)] if layout == TRIANGLE else Pm.reshape(-1)
    return np.ascontiguousarray(flat.astype(dt))


def unpack_P(sec, n, layout):
    """the P section's elements -> n x n matrix in the section's type; the triangle is mirrored"""
    if layout == FULL:
        return np.array(sec).reshape(n, n)
    M = np.zeros((n, n), dtype=sec.dtype)
    M[np.triu_indices(n)] = sec
    low = np.tril_indices(n, -1)
    M[low] = M.T[low]
    return M


def assemble(N, n, p_elem_bytes, p_layout, desc_bytes, desc_flags, sections):
    """sections: {id: bytes} of the present ones -> the blob (np.uint8), header and checksums computed here"""
    elem = [8, 8, 4, 1, 4, 4, p_elem_bytes, 1, 1, 8, PATCH_NORMAL_BYTES, CAMERA_BYTES]
    mask = ((MASK_TEMPLATES if TEMPLATES in sections else 0) | (MASK_WARP_SOURCES if WARP_SOURCES in sections else 0)
            | (MASK_PATCH_NORMALS if PATCH_NORMALS in sections else 0))
    body, entries, at = bytearray(), [], HEADER_BYTES
    for sid in range(12):
        if sid not in sections:
            entries.append(struct.pack(_ENTRY, sid, 0, 0, 0, 0))
            continue
        data = bytes(sections[sid])
        start = (at + 63) // 64 * 64
        body += bytes(start - at) + data
        entries.append(struct.pack(_ENTRY, sid, elem[sid], start, len(data), checksum(data)))
        at = start + len(data)

    def fixed(cs):
        return struct.pack(_FIXED, MAGIC, 1, HEADER_BYTES, at, N, n, p_elem_bytes, p_layout, desc_bytes, desc_flags, mask, 0, cs)

    head = fixed(0) + b"".join(entries)
    head = fixed(checksum(head)) + b"".join(entries)
    assert len(head) == HEADER_BYTES
    return np.frombuffer(head + bytes(body), dtype=np.uint8).copy()


def build(x13, feat_pos, feat_type, desc, times_predicted, times_matched, Pm, p_elem_bytes, p_layout, desc_flags, camera,
          templates=None, warp_sources=None, warp_poses=None, patch_normals=None):
    """arrays as the engine's getters return them -> blob.  Pm: n x n (any float type whose values the storage type holds
    exactly); camera: the 104 bytes of EkfCamera; the optional tables as raw bytes / arrays in map order"""
    ft = np.ascontiguousarray(feat_type, dtype="<i4").reshape(-1)
    N = ft.size
    n = int(np.asarray(Pm).shape[0])
    d = np.ascontiguousarray(desc).view(np.uint8).reshape(N, -1) if N else np.zeros((0, 32), np.uint8)
    secs = {
        X13: np.ascontiguousarray(x13, dtype="<f8").tobytes(),
        FEAT_POS: np.ascontiguousarray(feat_pos, dtype="<f8").reshape(-1)[: 6 * N].tobytes(),
        FEAT_TYPE: ft.tobytes(),
        DESC: d.tobytes(),
        TIMES_PREDICTED: np.ascontiguousarray(times_predicted, dtype="<u4").tobytes(),
        TIMES_MATCHED: np.ascontiguousarray(times_matched, dtype="<u4").tobytes(),
        P: pack_P(Pm, p_elem_bytes, p_layout).tobytes(),
        CAMERA: bytes(camera),
    }
    assert len(secs[CAMERA]) == CAMERA_BYTES
    for sid, t in ((TEMPLATES, templates), (WARP_SOURCES, warp_sources), (WARP_POSES, warp_poses), (PATCH_NORMALS, patch_normals)):
        if t is not None:
            secs[sid] = np.ascontiguousarray(t).tobytes()
    desc_bytes = d.shape[1] if N else 32
    return assemble(N, n, p_elem_bytes, p_layout, desc_bytes, desc_flags, secs)


def parse(blob):
    """blob -> dict(header fields, "sections": {id: bytes}); ValueError names what is wrong.  Checks what the format demands."""
    b = bytes(np.ascontiguousarray(blob, dtype=np.uint8))
    if len(b) < HEADER_BYTES:
        raise ValueError("truncated header")
    magic, version, hb, total, N, n, pe, pl, db, df, mask, zero, cs = struct.unpack_from(_FIXED, b, 0)
    if magic != MAGIC:
        raise ValueError("magic")
    if version != 1:
        raise ValueError("version")
    if hb != HEADER_BYTES:
        raise ValueError("header_bytes")
    if checksum(b[:56] + bytes(8) + b[64:HEADER_BYTES]) != cs:
        raise ValueError("header_checksum")
    if total != len(b):
        raise ValueError("total_bytes")
    if pe not in (4, 8) or pl not in (0, 1) or zero != 0 or mask & ~7 or N < 0 or n < 13 or db < 1:
        raise ValueError("header field out of range")
    pcount = n * (n + 1) // 2 if pl == TRIANGLE else n * n
    want = {X13: 104, FEAT_POS: 48 * N, FEAT_TYPE: 4 * N, DESC: N * db, TIMES_PREDICTED: 4 * N, TIMES_MATCHED: 4 * N, P: pcount * pe,
            CAMERA: CAMERA_BYTES}
    if mask & MASK_TEMPLATES:
        want[TEMPLATES] = N * TEMPLATE_BYTES
    if mask & MASK_WARP_SOURCES:
        want[WARP_SOURCES], want[WARP_POSES] = N * WARP_SOURCE_BYTES, N * 72
    if mask & MASK_PATCH_NORMALS:
        want[PATCH_NORMALS] = N * PATCH_NORMAL_BYTES
    secs, at = {}, HEADER_BYTES
    for sid in range(12):
        eid, elem, off, nb, scs = struct.unpack_from(_ENTRY, b, 64 + 32 * sid)
        if eid != sid:
            raise ValueError("directory id")
        if sid not in want:
            if (elem, off, nb, scs) != (0, 0, 0, 0):
                raise ValueError(f"absent section {NAMES[sid]} is not zero")
            continue
        if off % 64 or off < at or off + nb > len(b) or nb != want[sid]:
            raise ValueError(f"section {NAMES[sid]}: placement or size")
        if any(b[at:off]):
            raise ValueError("gap not zero")
        if checksum(b[off:off + nb]) != scs:
            raise ValueError(f"section {NAMES[sid]}: checksum")
        secs[sid] = b[off:off + nb]
        at = off + nb
    if at != len(b):
        raise ValueError("bytes behind the last section")
    ft = np.frombuffer(secs[FEAT_TYPE], dtype="<i4")
    if not np.isin(ft, (1, 2)).all() or 13 + int(np.where(ft == 2, 6, 3).sum()) != n:
        raise ValueError("FEAT_TYPE / n")
    return dict(version=version, total_bytes=total, N=N, n=n, p_elem_bytes=pe, p_layout=pl, desc_bytes=db, desc_flags=df,
                section_mask=mask, sections=secs)


def P_of(parsed):
    """the n x n matrix (section's type) of a parsed blob"""
    dt = "<f4" if parsed["p_elem_bytes"] == 4 else "<f8"
    return unpack_P(np.frombuffer(parsed["sections"][P], dtype=dt), parsed["n"], parsed["p_layout"])


def reassemble(parsed, replace=None, **header):
    """the blob of a parsed one with sections replaced ({id: bytes}) and header fields overridden, all checksums recomputed: wrong
    in exactly the respect asked for"""
    secs = dict(parsed["sections"])
    secs.update(replace or {})
    f = {k: header.get(k, parsed[k]) for k in ("N", "n", "p_elem_bytes", "p_layout", "desc_bytes", "desc_flags")}
    return assemble(f["N"], f["n"], f["p_elem_bytes"], f["p_layout"], f["desc_bytes"], f["desc_flags"], secs)


def refresh_header_checksum(blob):
    """recomputes the header checksum of a blob whose header bytes were edited in place"""
    b = np.array(blob, dtype=np.uint8)
    b[56:64] = 0
    b[56:64] = np.frombuffer(struct.pack("<Q", checksum(b[:HEADER_BYTES])), dtype=np.uint8)
    return b
