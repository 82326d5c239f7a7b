"""Z-order covering index: the config, the Z-address definition and the host builder.

A Z-order index holds the same columns as a covering index, but its rows are ordered by the
Morton interleave of *several* indexed columns and cut into ``numBuckets`` key-range files
(written with the bucket-file naming, the file number in the bucket position).  A filter on any
subset of the indexed columns then touches few zones of the resident table: the executor keeps
per-zone min/max maps and prunes zones on the device (``exec/zorder.py``).

Z-address.  For indexed column j of K (at most 8), over the whole build input:

  img_j(row)   the order-preserving unsigned image of the value (``hs_sortable``)
  min_j/max_j  over the non-null rows
  need_j       bit_length(max_j - min_j); 0 for a constant or all-null column
  b_j          bits granted: all start at 0; walk the columns in declared order giving one bit
               to each column with b_j < need_j, until 63 bits are given or all are satisfied
  code_j(row)  (img_j - min_j) >> (need_j - b_j), 0 for a null

The key takes, for level l = 0, 1, ..., bit b_j - 1 - l of code_j of every column (declared
order) with b_j > l, most significant first: Sum(b_j) <= 63 bits, a non-negative int64.  Rows are
ordered by the key with a stable sort (ties keep source order: files in listing order, rows in
file order), so the host and the device build write the same rows in the same order.  Queries
never depend on the key: pruning compares real per-zone min/max.
"""
from __future__ import annotations

import uuid
from typing import List, Optional, Sequence, Tuple

import numpy as np
import pyarrow as pa

from ..exceptions import HyperspaceException
from .config import IndexConfig

KEY_BITS = 63
MAX_INDEXED_COLUMNS = 8


class ZOrderCoveringIndexConfig(IndexConfig):
    """``IndexConfig`` whose rows are laid out in Z-order of up to 8 indexed columns."""

    def __init__(self, indexName: str, indexedColumns: Sequence[str],
                 includedColumns: Sequence[str] = ()):
        super().__init__(indexName, indexedColumns, includedColumns)
        if len(self.indexedColumns) > MAX_INDEXED_COLUMNS:
            raise ValueError(
                f"A Z-order index takes at most {MAX_INDEXED_COLUMNS} indexed columns.")

    __hash__ = IndexConfig.__hash__


def supported_indexed_type(t: pa.DataType) -> bool:
    """Types the Z-address is defined on: signed integers of 8-64 bits, date32, timestamps,
    float32 / float64, and decimals of precision <= 15 (float64 storage on the device)."""
    if pa.types.is_decimal(t):
        return t.precision <= 15
    return pa.types.is_signed_integer(t) or pa.types.is_date32(t) or pa.types.is_timestamp(t) \
        or pa.types.is_float32(t) or pa.types.is_float64(t)


def check_indexed_types(schema: pa.Schema, indexed: Sequence[str]) -> None:
    for c in indexed:
        t = schema.field(c).type
        if not supported_indexed_type(t):
            raise HyperspaceException(
                f"Column '{c}' of type {t} cannot be an indexed column of a Z-order index "
                "(supported: signed integers, date, timestamp, float, double, decimal of "
                "precision <= 15).")


def num_files(source_bytes: int, target_bytes: int) -> int:
    return max(1, -(-int(source_bytes) // max(1, int(target_bytes))))


def file_of_rank(n: int, nfiles: int) -> np.ndarray:
    """File number of every sorted position: file k holds positions [k * ceil(n / F),
    (k + 1) * ceil(n / F))."""
    per = max(1, -(-n // nfiles))
    return (np.arange(n, dtype=np.int64) // per).astype(np.int32)


# -- the Z-address ----------------------------------------------------------------------------
def sortable_images(values: np.ndarray) -> np.ndarray:
    """uint64 ``hs_sortable`` images of storage values (signed integers or floats)."""
    v = np.ascontiguousarray(values)
    size = v.dtype.itemsize
    top = np.uint64(1 << (8 * size - 1))
    if v.dtype.kind == "i":
        return v.view(f"u{size}").astype(np.uint64) ^ top
    if v.dtype.kind == "f":
        b = v.view(f"u{size}").astype(np.uint64)
        return np.where(b >= top, ~b & np.uint64((1 << (8 * size)) - 1), b | top)
    raise TypeError(f"no sortable image for {v.dtype}")


def allocate_bits(needs: Sequence[int]) -> List[int]:
    bits = [0] * len(needs)
    left = KEY_BITS
    while left > 0:
        short = [j for j, need in enumerate(needs) if bits[j] < need]
        if not short:
            break
        for j in short[:left]:
            bits[j] += 1
        left -= min(left, len(short))
    return bits


def key_plan(ranges: Sequence[Optional[Tuple[int, int]]]):
    """``(mins, shifts, bits)`` per column from its ``(min image, max image)`` over the non-null
    rows (None: no such row)."""
    mins = [0 if r is None else int(r[0]) for r in ranges]
    needs = [0 if r is None else (int(r[1]) - int(r[0])).bit_length() for r in ranges]
    bits = allocate_bits(needs)
    return mins, [need - b for need, b in zip(needs, bits)], bits


def host_keys(cols: Sequence[Tuple[np.ndarray, Optional[np.ndarray]]]) -> np.ndarray:
    """int64 Z-addresses of rows given as ``(storage values, validity or None)`` columns."""
    n = len(cols[0][0])
    imgs, oks, ranges = [], [], []
    for vals, valid in cols:
        img = sortable_images(vals)
        ok = None if valid is None else np.asarray(valid).astype(bool)
        live = img if ok is None else img[ok]
        ranges.append((int(live.min()), int(live.max())) if len(live) else None)
        imgs.append(img)
        oks.append(ok)
    mins, shifts, bits = key_plan(ranges)
    key = np.zeros(n, dtype=np.uint64)
    codes = []
    for img, ok, mn, sh, b in zip(imgs, oks, mins, shifts, bits):
        if not b:
            codes.append(None)
            continue
        code = (img - np.uint64(mn)) >> np.uint64(sh)
        codes.append(code if ok is None else np.where(ok, code, np.uint64(0)))
    one = np.uint64(1)
    for level in range(max(bits, default=0)):
        for code, b in zip(codes, bits):
            if b > level:
                key = (key << one) | ((code >> np.uint64(b - 1 - level)) & one)
    return key.view(np.int64)


# -- host builder -----------------------------------------------------------------------------
def host_build(session, table: pa.Table, indexed: List[str], nfiles: int, out_path: str,
               mode: str = "overwrite") -> List[str]:
    """Write ``table`` in Z-order of ``indexed`` as ``nfiles`` key-range files."""
    import os
    import shutil
    from ..exec.staging import fixed_width_numpy
    from ..io.writer import write_bucket_file
    from ..utils import path_utils as P
    from ..utils.conf import HyperspaceConf
    local = P.to_local(out_path)
    if mode == "overwrite" and os.path.exists(local):
        shutil.rmtree(local)
    if mode == "errorifexists" and os.path.exists(local):
        raise HyperspaceException(f"path {out_path} already exists")
    os.makedirs(local, exist_ok=True)
    n = table.num_rows
    if n == 0:
        return []
    keys = host_keys([fixed_width_numpy(table.column(c)) for c in indexed])
    t = table.take(pa.array(np.argsort(keys, kind="stable")))
    per = max(1, -(-n // nfiles))
    codec = HyperspaceConf.index_file_codec(session.conf)
    rg = HyperspaceConf.index_row_group_rows(session.conf)
    job = str(uuid.uuid4())
    return [write_bucket_file(t.slice(k * per, per), out_path, 0, job, k, codec, rg)
            for k in range(nfiles) if k * per < n]
