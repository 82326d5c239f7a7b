"""numpy oracle of the Z-order covering index (``index/zorder.py``, ``csrc/kernels/zorder.hip``):
order-preserving images, the bit allocation, Z-addresses, the stable row order, per-zone min/max
maps and the pruned range list.  Written bit by bit and zone by zone, nothing shared with the
code under test.

A column is ``(values, valid)``: numpy values in the device storage type (int8..int64, float32,
float64; date32 as int32, timestamps as int64, decimals of precision <= 15 as float64) and a
uint8 / bool validity array or None.
"""
from __future__ import annotations

import numpy as np

KEY_BITS = 63
MAX_COLS = 8


def image(values: np.ndarray) -> np.ndarray:
    """uint64 image whose unsigned order is the value order (floats: the bit total order,
    -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN; nothing canonicalised)."""
    v = np.ascontiguousarray(values)
    k, w = v.dtype.kind, v.dtype.itemsize * 8
    if k == "i":
        u = v.view(f"u{w // 8}").astype(np.uint64)
        return u ^ np.uint64(1 << (w - 1))
    if k == "f":
        b = v.view(f"u{w // 8}").astype(np.uint64)
        top = np.uint64(1 << (w - 1))
        mask = np.uint64((1 << w) - 1)
        return np.where(b & top != 0, ~b & mask, b | top)
    raise TypeError(f"no image for dtype {v.dtype}")


def _valid(col):
    vals, valid = col
    return np.ones(len(vals), bool) if valid is None else np.asarray(valid).astype(bool)


def column_range(col):
    """(min image, need bits) over the non-null rows; (0, 0) without one."""
    ok = _valid(col)
    if not ok.any():
        return 0, 0
    img = image(col[0])[ok]
    mn, mx = int(img.min()), int(img.max())
    return mn, (mx - mn).bit_length()


def bit_allocation(needs) -> list:
    """Bits per column: one bit per round to every column still short of its need, columns in
    declared order, until 63 bits are given or every column is satisfied."""
    b = [0] * len(needs)
    given = 0
    while given < KEY_BITS and any(x < y for x, y in zip(b, needs)):
        for j, need in enumerate(needs):
            if given < KEY_BITS and b[j] < need:
                b[j] += 1
                given += 1
    return b


def keys(cols) -> np.ndarray:
    """int64 Z-address of every row."""
    assert 1 <= len(cols) <= MAX_COLS
    n = len(cols[0][0])
    rng = [column_range(c) for c in cols]
    needs = [r[1] for r in rng]
    bits = bit_allocation(needs)
    codes = []
    for c, (mn, need), b in zip(cols, rng, bits):
        ok = _valid(c)
        img = image(c[0])
        code = np.zeros(n, dtype=np.uint64)
        if b:
            code[ok] = (img[ok] - np.uint64(mn)) >> np.uint64(need - b)
        codes.append(code)
    out = np.zeros(n, dtype=np.uint64)
    for level in range(max(bits) if bits else 0):
        for code, b in zip(codes, bits):
            if b > level:
                out = (out << np.uint64(1)) | ((code >> np.uint64(b - 1 - level)) & np.uint64(1))
    assert sum(bits) <= KEY_BITS
    return out.astype(np.int64)


def order(cols) -> np.ndarray:
    """Row permutation of the index: stable by key (ties keep input order)."""
    return np.argsort(keys(cols), kind="stable")


def zone_maps(cols, zone_rows: int):
    """(mn, mx, cnt): ``[K][NZ]`` uint64 / uint64 / int64; an all-null zone has mn = 2^64-1 and
    mx = 0."""
    n = len(cols[0][0])
    nz = -(-n // zone_rows)
    mn = np.full((len(cols), nz), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    mx = np.zeros((len(cols), nz), dtype=np.uint64)
    cnt = np.zeros((len(cols), nz), dtype=np.int64)
    for j, c in enumerate(cols):
        img, ok = image(c[0]), _valid(c)
        for z in range(nz):
            s = slice(z * zone_rows, min(n, (z + 1) * zone_rows))
            v = img[s][ok[s]]
            cnt[j, z] = len(v)
            if len(v):
                mn[j, z], mx[j, z] = v.min(), v.max()
    return mn, mx, cnt


def kept_zones(mn, mx, cnt, intervals) -> np.ndarray:
    """bool per zone.  ``intervals``: {column position: (lo image, hi image)}, inclusive."""
    keep = np.ones(mn.shape[1], dtype=bool)
    for j, (lo, hi) in intervals.items():
        for z in range(mn.shape[1]):
            keep[z] = keep[z] and cnt[j, z] > 0 and int(mx[j, z]) >= lo and int(mn[j, z]) <= hi
    return keep


def prune(mn, mx, cnt, n: int, zone_rows: int, intervals):
    """(ranges, kept zone count): ``ranges`` the ascending ``(start, len)`` list of kept zones,
    adjacent ones coalesced, the last zone clipped to ``n``."""
    keep = kept_zones(mn, mx, cnt, intervals)
    ranges = []
    z = 0
    nz = len(keep)
    while z < nz:
        if not keep[z]:
            z += 1
            continue
        e = z
        while e + 1 < nz and keep[e + 1]:
            e += 1
        ranges.append((z * zone_rows, min(n, (e + 1) * zone_rows) - z * zone_rows))
        z = e + 1
    return ranges, int(keep.sum())


def padded(ranges, nz: int):
    """``(rstart, rlen)`` int64 arrays of length ``nz``: live ranges first, then zero-length."""
    rs = np.zeros(nz, dtype=np.int64)
    rl = np.zeros(nz, dtype=np.int64)
    for i, (s, ln) in enumerate(ranges):
        rs[i], rl[i] = s, ln
    return rs, rl
