"""Device build of a data-skipping index's sketch rows (``index/dataskipping.py``).

The sketched columns of the source ride the index build's upload pipeline
(``device_build.upload_source_columns``: decode -> pinned -> HBM), file group by file group within the
build's HBM budget; each group is sketched by the kernels of ``csrc/kernels/sketch.hip`` and
released.  Per file only 3 words per MinMax sketch and one filter per Bloom sketch come back.

String columns arrive as codes over the group's sorted dictionary: MinMax reduces the codes and
maps min / max back through the dictionary on the host; Bloom hashes each dictionary entry once
on the device into an (h1, h2) table that the rows gather by code.

Columns the device cannot sketch exactly (decimals wider than float64's 15 digits, unsigned and
other storage the kernels do not take, columns the upload did not produce) and sources that are
not Parquet take the host builder; ``LAST_SKETCH_STATS`` records which path each column took.
"""
from __future__ import annotations

import time
from typing import Dict, List, Sequence

import numpy as np
import pyarrow as pa

from ..index import dataskipping as DS
from ..index.builder import source_format
from ..ops import _lib as NL
from ..ops import kernels as K
from . import device_build as DB
from .device_table import storage_numpy_dtype

# what the last sketch build did: path ("device" / "host"), columns {name: path}, upload_s,
# kernels_s, files, rows, groups
LAST_SKETCH_STATS: Dict[str, object] = {}

_KERNEL_TYPES = (NL.I8, NL.I16, NL.I32, NL.I64, NL.F32, NL.F64)
# files one ``hs_sketch_bloom`` launch takes (csrc/kernels/sketch.hip)
MAX_GROUP_FILES = 65535


def plan_groups(rows: List[int], row_bytes: int, group_budget: int) -> List[tuple]:
    """File ranges [a, b) uploaded and sketched together: within ``group_budget`` decoded bytes
    (``device_build.plan_file_groups``) and at most ``MAX_GROUP_FILES`` files each."""
    return [(i, min(i + MAX_GROUP_FILES, b))
            for a, b in DB.plan_file_groups(rows, row_bytes, group_budget)
            for i in range(a, b, MAX_GROUP_FILES)]


def _device_column_ok(t: pa.DataType) -> bool:
    if pa.types.is_dictionary(t):
        t = t.value_type
    if pa.types.is_decimal(t):
        return t.precision <= 15          # device storage is float64
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        return True
    return pa.types.is_signed_integer(t) or pa.types.is_floating(t) or pa.types.is_date(t) or \
        pa.types.is_timestamp(t)


def _typed(values: np.ndarray, counts: np.ndarray, atype: pa.DataType, dictionary) -> pa.Array:
    """Per-file min or max storage values as an array of the column's type, null where the
    file holds no non-null value."""
    mask = counts == 0
    t = DS.column_type(atype)
    if dictionary is not None:
        if not len(dictionary):
            return pa.nulls(len(values), t)
        codes = np.where(mask, 0, values).astype(np.int32)
        return dictionary.take(pa.array(codes, pa.int32(), mask=mask)).cast(t)
    if pa.types.is_date32(t):
        return pa.array(values.astype(np.int32), pa.int32(), mask=mask).view(t)
    if pa.types.is_date64(t) or pa.types.is_timestamp(t):
        return pa.array(values.astype(np.int64), pa.int64(), mask=mask).view(t)
    if pa.types.is_decimal(t):
        return pa.array(values, pa.float64(), mask=mask).cast(t)
    return pa.array(values, t, mask=mask)


def _with_empty_files(arrays: Dict[str, pa.Array], sketches, schema: pa.Schema, files, rows):
    """The device-built columns (one entry per file with rows) widened to every file: NULL
    min / max and an all-zero filter for a file without rows."""
    import pyarrow.compute as pc
    at, pos = [], 0
    for r in rows:
        at.append(pos if r > 0 else None)
        pos += r > 0
    take = pa.array(at, pa.int64())
    out = {}
    for s in sketches:
        if s["type"] == DS.MinMaxSketch.kind:
            for n in DS.minmax_names(s["column"]):
                src = arrays.get(n)
                out[n] = src.take(take) if src is not None else \
                    pa.nulls(len(files), schema.field(n).type)
        else:
            n = DS.bloom_name(s["column"])
            nw, k = DS.bloom_shape(s)
            empty = pa.scalar(DS.bloom_serialize(np.zeros(nw, np.uint64), k), pa.binary())
            src = arrays.get(n)
            out[n] = pc.fill_null(src.take(take), empty) if src is not None else \
                pa.array([empty.as_py()] * len(files), pa.binary())
    return out


def device_sketch_rows(session, rel, files: List[str], sketches: Sequence[dict],
                       lineage_ids: Dict[str, int]) -> pa.Table:
    import torch
    from .like import device_dictionary
    schema = DS.sketch_schema(sketches, rel.schema)
    LAST_SKETCH_STATS.clear()
    cols = list(dict.fromkeys(s["column"] for s in sketches))
    on_device = [c for c in cols if c in rel.data_schema.names and
                 _device_column_ok(rel.data_schema.field(c).type)] \
        if source_format(rel) == "parquet" and files else []
    paths = {c: ("device" if c in on_device else "host") for c in cols}
    data: Dict[str, list] = {}
    host_sk = [s for s in sketches if paths[s["column"]] == "host"]
    upload_s = kernels_s = 0.0
    rows_total = 0
    ngroups = 0
    if on_device:
        device = torch.device("cuda", torch.cuda.current_device())
        dev_sk = [s for s in sketches if paths[s["column"]] == "device"]
        for s in dev_sk:
            for n in (DS.minmax_names(s["column"]) if s["type"] == DS.MinMaxSketch.kind
                      else (DS.bloom_name(s["column"]),)):
                data[n] = []
        all_rows = DB.source_row_counts(files, on_device)
        rows_total = int(sum(all_rows))
        # a file without rows has nothing to upload: its sketches are known (NULL min / max, an
        # empty filter) and are filled in below
        all_files, files = files, [f for f, r in zip(files, all_rows) if r > 0]
        rows = [r for r in all_rows if r > 0]
        row_bytes = sum(storage_numpy_dtype(rel.data_schema.field(c).type).itemsize + 1
                        for c in on_device)
        groups = plan_groups(rows, row_bytes, max(DB._build_budget(session, device) // 4, 1))
        ngroups = len(groups)
        for a, b in groups:
            tu = time.perf_counter()
            up = DB.upload_source_columns(rel, files[a:b], on_device, device)
            torch.cuda.synchronize()
            tk = time.perf_counter()
            upload_s += tk - tu
            frows = rows[a:b]
            parts = {}
            for s in dev_sk:
                c = up[s["column"]]
                if c.dictionary is None and c.hs_type not in _KERNEL_TYPES:
                    raise RuntimeError(f"sketch: column {s['column']} reached the device as "
                                       f"{c.data.dtype}")
                if s["type"] == DS.MinMaxSketch.kind:
                    parts[id(s)] = (c, K.sketch_minmax(c, frows))
                else:
                    nw, k = DS.bloom_shape(s)
                    entries = None
                    if c.dictionary is not None:
                        # the group's dictionary is used once: uploaded, hashed, released
                        entries = K.sketch_hash_entries(
                            device_dictionary(c.dictionary, device, cache=False))
                    parts[id(s)] = (c, K.sketch_bloom(c, frows, nw, k, entries).cpu().numpy())
            torch.cuda.synchronize()
            kernels_s += time.perf_counter() - tk
            for s in dev_sk:
                c, res = parts[id(s)]
                if s["type"] == DS.MinMaxSketch.kind:
                    mn, mx, cnt = res
                    atype = rel.data_schema.field(s["column"]).type
                    lo, hi = DS.minmax_names(s["column"])
                    data[lo].append(_typed(mn, cnt, atype, c.dictionary))
                    data[hi].append(_typed(mx, cnt, atype, c.dictionary))
                else:
                    _, k = DS.bloom_shape(s)
                    words = res.view(np.uint64)
                    data[DS.bloom_name(s["column"])].append(
                        pa.array([DS.bloom_serialize(w, k) for w in words], pa.binary()))
            del up, parts
    arrays = {n: pa.concat_arrays(v) if len(v) != 1 else v[0] for n, v in data.items() if v}
    if on_device:
        arrays, files = _with_empty_files(arrays, dev_sk, schema, all_files, all_rows), all_files
    if host_sk or not on_device:
        ht = DS.host_sketch_rows(rel, files, host_sk if on_device else list(sketches),
                                 lineage_ids)
        for n in ht.column_names:
            arrays.setdefault(n, ht.column(n))
    arrays[schema.field(0).name] = pa.array([int(lineage_ids[f]) for f in files], pa.int64())
    LAST_SKETCH_STATS.update({"path": "device" if on_device else "host", "columns": paths,
                              "upload_s": upload_s, "kernels_s": kernels_s, "files": len(files),
                              "rows": rows_total, "groups": ngroups})
    return pa.Table.from_arrays(
        [arrays[f.name] if arrays[f.name].type.equals(f.type) else arrays[f.name].cast(f.type)
         for f in schema], schema=schema)
