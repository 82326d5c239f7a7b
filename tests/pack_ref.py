"""Plain numpy reference of the row-packed layout (csrc/kernels/pack_rows.hip, exec/jit.py
``RowPack``).

A row is ``B`` bits (a multiple of 4, at most 64): column c's field ``(code - offs[c]) mod 2^32``
masked to ``bits[c]`` bits sits at bit ``pos[c]`` of the row, and row i starts at bit ``i * B`` of
a little-endian bit stream (so 8 rows fill exactly ``B / 4`` dwords).  The stream is padded with
zero rows to a whole number of 2048-row tiles, at least one.
"""
import numpy as np

TILE_ROWS = 2048


def padded_rows(n: int) -> int:
    return max(1, -(-n // TILE_ROWS)) * TILE_ROWS


def pack(cols, offs, pos, bits, B: int) -> np.ndarray:
    """uint32 dwords of the packed copy of integer code arrays ``cols``."""
    assert B % 4 == 0 and 4 <= B <= 64
    n = len(cols[0])
    npad = padded_rows(n)
    row = np.zeros(npad, np.uint64)
    for c, o, p, w in zip(cols, offs, pos, bits):
        assert 1 <= w <= 32 and 0 <= p and p + w <= B and len(c) == n
        f = ((np.asarray(c).astype(np.int64) - int(o)) & 0xFFFFFFFF) & ((1 << w) - 1)
        row[:n] |= f.astype(np.uint64) << np.uint64(p)
    # bit j of every row, row-major, then the stream's bytes
    shifts = np.arange(B, dtype=np.uint64)
    rb = ((row[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.packbits(rb.reshape(-1), bitorder="little").view(np.uint32).copy()


def unpack(words, n: int, offs, pos, bits, B: int):
    """int64 code arrays of the first ``n`` rows of packed dwords ``words``; a field that held
    ``(code - off) mod 2^32`` comes back as ``off + field`` (the code, when it lies in
    ``[off, off + 2^bits)``)."""
    rb = np.unpackbits(np.asarray(words, np.uint32).view(np.uint8), bitorder="little")
    rb = rb.reshape(-1, B)[:n].astype(np.uint64)
    out = []
    for o, p, w in zip(offs, pos, bits):
        f = np.zeros(n, np.uint64)
        for j in range(w):
            f |= rb[:, p + j] << np.uint64(j)
        out.append(f.astype(np.int64) + int(o))
    return out
