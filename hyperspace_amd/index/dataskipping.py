"""Data-skipping indexes: per-source-file MinMax and Bloom-filter sketches.

A data-skipping index is a tiny table with one row per source file (``_data_file_id`` plus the
sketch columns).  At scan time ``prune`` drops the files whose sketches prove that no row can
satisfy the scan's filter; files the index does not know are always kept.

* ``DataSkippingIndexConfig`` / ``MinMaxSketch`` / ``BloomFilterSketch``: the public spec.
* ``host_sketch_rows``: the host builder (pyarrow + numpy per file) - the oracle, the CPU
  sessions' path and the multi-rank path; ``exec/device_sketch.py`` is the single-GPU path.
* ``prune``: numpy interval / membership tests over the cached sketch table.

The Bloom filter is intended to match Spark's ``BloomFilterImpl`` (Murmur3 double hashing, bit
``b`` in 64-bit word ``b >> 6``, big-endian serialization ``version, k, numWords, words``).
MinMax uses Spark's orderings: nulls ignored, NaN above +inf, -0.0 == 0.0 (stored as 0.0),
strings as unsigned UTF-8 bytes.
"""
from __future__ import annotations

import math
import struct
import uuid
from typing import Dict, List, Optional, Sequence

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from ..exceptions import HyperspaceException
from ..utils import murmur3
from ..utils import path_utils as P
from . import constants as C

KIND = "DataSkippingIndex"
MAX_BLOOM_BITS = 1 << 26          # 8 MiB per file
BLOOM_VERSION = 1

# what the last prune() did: {index, files, kept, unknown, kept_paths}
LAST_PRUNE: Dict[str, object] = {}


# ------------------------------------------------------------------------------------------------
# public spec
# ------------------------------------------------------------------------------------------------
class Sketch:
    kind = ""

    def __init__(self, column: str):
        if not column or not isinstance(column, str):
            raise ValueError("A sketch needs a column name.")
        self.column = column

    def key(self):
        return (self.kind, self.column.lower())

    def to_json_obj(self, column: Optional[str] = None) -> dict:
        return {"type": self.kind, "column": column or self.column}

    def __eq__(self, o):
        return isinstance(o, Sketch) and self.to_json_obj(self.column.lower()) == \
            o.to_json_obj(o.column.lower())

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return f"{self.kind}({self.column})"


class MinMaxSketch(Sketch):
    kind = "MinMax"


class BloomFilterSketch(Sketch):
    kind = "BloomFilter"

    def __init__(self, column: str, fpp: float, expectedDistinctCountPerFile: int):
        super().__init__(column)
        fpp = float(fpp)
        if not 0.0 < fpp < 1.0:
            raise ValueError("The false-positive probability of a Bloom filter sketch must be "
                             "between 0 and 1 (exclusive).")
        if int(expectedDistinctCountPerFile) < 1:
            raise ValueError("The expected distinct count of a Bloom filter sketch must be at "
                             "least 1.")
        self.fpp = fpp
        self.expected = int(expectedDistinctCountPerFile)

    def to_json_obj(self, column: Optional[str] = None) -> dict:
        num_bits, num_words, k = bloom_params(self.expected, self.fpp)
        return {"type": self.kind, "column": column or self.column, "fpp": self.fpp,
                "expectedDistinctCountPerFile": self.expected, "numBits": num_words * 64,
                "numHashFunctions": k}

    def __repr__(self):
        return f"{self.kind}({self.column}, {self.fpp}, {self.expected})"


class DataSkippingIndexConfig:
    def __init__(self, indexName: str, sketch: Sketch, *sketches: Sketch):
        if not indexName:
            raise ValueError("Empty index name is not allowed.")
        all_ = [sketch, *sketches]
        if sketch is None or any(not isinstance(s, Sketch) for s in all_):
            raise ValueError("A data-skipping index needs at least one sketch.")
        keys = [s.key() for s in all_]
        if len(set(keys)) < len(keys):
            raise ValueError("Duplicate sketches (same kind and column) are not allowed.")
        self.indexName = indexName
        self.sketches = all_

    @property
    def index_name(self):
        return self.indexName

    @property
    def indexedColumns(self) -> List[str]:
        out: List[str] = []
        for s in self.sketches:
            if s.column.lower() not in [c.lower() for c in out]:
                out.append(s.column)
        return out

    @property
    def includedColumns(self) -> List[str]:
        return []

    indexed_columns = indexedColumns
    included_columns = includedColumns

    def __eq__(self, o):
        return isinstance(o, DataSkippingIndexConfig) and \
            self.indexName.lower() == o.indexName.lower() and self.sketches == o.sketches

    def __hash__(self):
        return hash(tuple(s.key() for s in self.sketches))

    def __repr__(self):
        return f"[indexName: {self.indexName}; sketches: {', '.join(map(repr, self.sketches))}]"


def config_of(name: str, sketches: Sequence[dict]) -> DataSkippingIndexConfig:
    """The config that a log entry's ``properties.sketches`` came from."""
    out = []
    for s in sketches:
        if s["type"] == MinMaxSketch.kind:
            out.append(MinMaxSketch(s["column"]))
        elif s["type"] == BloomFilterSketch.kind:
            out.append(BloomFilterSketch(s["column"], s["fpp"], s["expectedDistinctCountPerFile"]))
        else:
            raise HyperspaceException(f"Unknown sketch type {s['type']}.")
    return DataSkippingIndexConfig(name, *out)


# ------------------------------------------------------------------------------------------------
# Bloom filter
# ------------------------------------------------------------------------------------------------
def bloom_params(n: int, p: float):
    """(numBits, numWords, k) of a filter for ``n`` expected items at false-positive rate ``p``."""
    num_bits = int(-n * math.log(p) / (math.log(2) ** 2))
    num_words = max(1, -(-num_bits // 64))
    k = max(1, int(round(num_bits / n * math.log(2))))
    return num_bits, num_words, k


def _hash_pairs(values) -> tuple:
    """(h1, h2) uint32 arrays of int64 values (numpy) or of strings (pyarrow array)."""
    if isinstance(values, pa.Array):
        n = len(values)
        h1 = np.asarray(murmur3.hash_strings(values, np.zeros(n, np.uint32)), dtype=np.uint32)
        h2 = np.asarray(murmur3.hash_strings(values, h1.copy()), dtype=np.uint32)
        return h1, h2
    v = np.asarray(values, dtype=np.int64)
    h1 = np.asarray(murmur3.hash_long(v, np.zeros(len(v), np.uint32)), dtype=np.uint32)
    h2 = np.asarray(murmur3.hash_long(v, h1), dtype=np.uint32)
    return h1, h2


def bloom_positions(h1: np.ndarray, h2: np.ndarray, num_words: int, k: int) -> np.ndarray:
    """``(len, k)`` bit positions."""
    bit_size = num_words * 64
    out = np.empty((len(h1), k), dtype=np.int64)
    with np.errstate(over="ignore"):
        for i in range(1, k + 1):
            c = (h1 + np.uint32(i) * h2).astype(np.uint32).view(np.int32)
            c = np.where(c < 0, ~c, c).astype(np.int64)
            out[:, i - 1] = c % bit_size
    return out


def bloom_words(values, num_words: int, k: int) -> np.ndarray:
    """The filter's ``num_words`` uint64 words over ``values`` (int64 numpy / pyarrow strings)."""
    bits = np.zeros(num_words * 64, dtype=np.uint8)
    if len(values):
        h1, h2 = _hash_pairs(values)
        bits[bloom_positions(h1, h2, num_words, k).reshape(-1)] = 1
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def bloom_serialize(words: np.ndarray, k: int) -> bytes:
    w = np.asarray(words).astype(np.uint64)
    return struct.pack(">iii", BLOOM_VERSION, int(k), len(w)) + w.astype(">u8").tobytes()


def bloom_deserialize(b: bytes):
    version, k, nw = struct.unpack(">iii", b[:12])
    if version != BLOOM_VERSION:
        raise HyperspaceException(f"Unsupported Bloom filter version {version}.")
    return np.frombuffer(b, dtype=">u8", count=nw, offset=12).astype(np.uint64), k


def _bloom_key_domain(t: pa.DataType) -> Optional[str]:
    if pa.types.is_dictionary(t):
        t = t.value_type
    if pa.types.is_uint64(t):
        return None                       # items hash as int64 values
    if pa.types.is_integer(t) or pa.types.is_date32(t) or pa.types.is_date64(t) or \
            pa.types.is_timestamp(t):
        return "int"
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        return "str"
    return None


def _minmax_supported(t: pa.DataType) -> bool:
    if pa.types.is_dictionary(t):
        t = t.value_type
    if pa.types.is_uint64(t):
        return False                      # min / max compare as int64 keys
    return pa.types.is_integer(t) or pa.types.is_date32(t) or pa.types.is_date64(t) or \
        pa.types.is_timestamp(t) or pa.types.is_float32(t) or pa.types.is_float64(t) or \
        pa.types.is_decimal(t) or pa.types.is_string(t) or pa.types.is_large_string(t)


def _plain(arr):
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks() if arr.num_chunks != 1 else arr.chunk(0)
    if pa.types.is_dictionary(arr.type):
        arr = arr.cast(arr.type.value_type)
    if pa.types.is_large_string(arr.type):
        arr = arr.cast(pa.string())
    return arr


def int_values(arr: pa.Array) -> np.ndarray:
    """Non-null values of an integer / date / timestamp array as int64."""
    arr = _plain(arr).drop_null()
    t = arr.type
    if pa.types.is_date32(t):
        arr = arr.view(pa.int32())
    elif pa.types.is_date64(t) or pa.types.is_timestamp(t):
        arr = arr.view(pa.int64())
    return np.asarray(arr.to_numpy(zero_copy_only=False)).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# sketch table
# ------------------------------------------------------------------------------------------------
def column_type(t: pa.DataType) -> pa.DataType:
    if pa.types.is_dictionary(t):
        t = t.value_type
    return pa.string() if pa.types.is_large_string(t) else t


def resolve_sketches(config: DataSkippingIndexConfig, resolved: Dict[str, str], schema: pa.Schema,
                     partition_names: Sequence[str]) -> List[dict]:
    """``properties.sketches`` of ``config`` over a source with ``schema``: column names as the
    source spells them, types checked."""
    out = []
    parts = {p.lower() for p in partition_names}
    for s in config.sketches:
        name = resolved[s.column]
        if name.lower() in parts:
            raise HyperspaceException(
                f"A sketch on partition column '{name}' is not supported: partition pruning "
                "already skips its files.")
        t = schema.field(name).type
        if isinstance(s, MinMaxSketch):
            if not _minmax_supported(t):
                raise HyperspaceException(f"MinMaxSketch does not support column '{name}' of "
                                          f"type {t}.")
        else:
            if _bloom_key_domain(t) is None:
                raise HyperspaceException(f"BloomFilterSketch does not support column '{name}' "
                                          f"of type {t}.")
            if bloom_params(s.expected, s.fpp)[1] * 64 > MAX_BLOOM_BITS:
                raise HyperspaceException(
                    f"The Bloom filter of column '{name}' needs more than {MAX_BLOOM_BITS} bits "
                    "per file; raise fpp or lower the expected distinct count.")
        out.append(s.to_json_obj(name))
    return out


def minmax_names(column: str):
    return f"MinMax_{column}__min", f"MinMax_{column}__max"


def bloom_name(column: str) -> str:
    return f"BloomFilter_{column}__bits"


def sketch_schema(sketches: Sequence[dict], source_schema: pa.Schema) -> pa.Schema:
    fields = [pa.field(C.DATA_FILE_NAME_ID, pa.int64(), False)]
    for s in sketches:
        if s["type"] == MinMaxSketch.kind:
            t = column_type(source_schema.field(s["column"]).type)
            lo, hi = minmax_names(s["column"])
            fields += [pa.field(lo, t), pa.field(hi, t)]
        else:
            fields.append(pa.field(bloom_name(s["column"]), pa.binary()))
    return pa.schema(fields)


def bloom_shape(s: dict):
    """(numWords, k) of a Bloom sketch's JSON."""
    return int(s["numBits"]) // 64, int(s["numHashFunctions"])


def host_minmax(arr) -> tuple:
    """(min, max) python values of one file's column, (None, None) without a non-null value."""
    arr = _plain(arr)
    t = arr.type
    if len(arr) == arr.null_count:
        return None, None
    if pa.types.is_floating(t):
        v = np.asarray(arr.drop_null().to_numpy(zero_copy_only=False))
        nan = np.isnan(v)
        rest = v[~nan] + v.dtype.type(0)          # -0.0 + 0.0 == +0.0
        mx = v.dtype.type(np.nan) if nan.any() else rest.max()
        mn = rest.min() if len(rest) else v.dtype.type(np.nan)
        return mn.item(), mx.item()
    if pa.types.is_string(t):
        u = pc.unique(arr.drop_null()).cast(pa.binary()).to_pylist()
        return min(u).decode("utf-8"), max(u).decode("utf-8")
    mm = pc.min_max(arr)
    return mm["min"].as_py(), mm["max"].as_py()


def host_sketch_rows(rel, files: List[str], sketches: Sequence[dict],
                     lineage_ids: Dict[str, int]) -> pa.Table:
    """The sketch table rows of ``files``, built on the host file by file."""
    from ..io.reader import read_files
    from .builder import source_format
    schema = sketch_schema(sketches, rel.schema)
    cols = list(dict.fromkeys(s["column"] for s in sketches))
    data: Dict[str, list] = {f.name: [] for f in schema}
    for f in files:
        t = read_files(source_format(rel), [f], rel.data_schema, rel.options,
                       rel.location.partition_spec, cols)
        data[C.DATA_FILE_NAME_ID].append(int(lineage_ids[f]))
        for s in sketches:
            arr = t.column(s["column"])
            if s["type"] == MinMaxSketch.kind:
                lo, hi = minmax_names(s["column"])
                mn, mx = host_minmax(arr)
                data[lo].append(mn)
                data[hi].append(mx)
            else:
                nw, k = bloom_shape(s)
                a = _plain(arr)
                vals = a.drop_null() if pa.types.is_string(a.type) else int_values(a)
                data[bloom_name(s["column"])].append(bloom_serialize(bloom_words(vals, nw, k), k))
    return pa.Table.from_arrays([pa.array(data[f.name], f.type) for f in schema], schema=schema)


def build_sketch_rows(session, rel, files: List[str], sketches: Sequence[dict],
                      lineage_ids: Dict[str, int]) -> pa.Table:
    """Sketch rows of ``files``: on the device in a single-GPU session, else on the host."""
    dist = getattr(session, "dist", None)
    world = dist.world if dist is not None else 1
    if session.device_kind() == "gpu" and world == 1:
        from ..exec.device_sketch import device_sketch_rows
        return device_sketch_rows(session, rel, files, sketches, lineage_ids)
    from ..exec.device_sketch import LAST_SKETCH_STATS
    out = host_sketch_rows(rel, files, sketches, lineage_ids)
    LAST_SKETCH_STATS.clear()
    LAST_SKETCH_STATS.update({"path": "host", "columns": {s["column"]: "host" for s in sketches},
                              "upload_s": 0.0, "kernels_s": 0.0, "files": len(files), "rows": 0,
                              "groups": 0})
    return out


def write_sketch_table(table: pa.Table, out_path: str) -> str:
    import os
    import pyarrow.parquet as pq
    local = P.to_local(out_path)
    os.makedirs(local, exist_ok=True)
    name = f"part-00000-{uuid.uuid4()}-c000.parquet"
    pq.write_table(table, os.path.join(local, name))
    return P.join(out_path, name)


def read_sketch_table(entry) -> pa.Table:
    import pyarrow.parquet as pq
    parts = [pq.read_table(P.to_local(f)) for f in sorted(entry.content.files)]
    if not parts:
        return entry.schema.empty_table()
    return pa.concat_tables(parts) if len(parts) > 1 else parts[0]


# ------------------------------------------------------------------------------------------------
# pruning
# ------------------------------------------------------------------------------------------------
def f64_image(v: np.ndarray) -> np.ndarray:
    """Order-preserving uint64 image of float64 values in Spark's total order."""
    v = np.asarray(v, dtype=np.float64).copy()
    v[v == 0.0] = 0.0
    b = v.view(np.uint64).copy()
    b[np.isnan(v)] = np.uint64(0x7FF8000000000000)
    top = np.uint64(1 << 63)
    return np.where(b & top, ~b, b | top)


def _exact_int(scalar: pa.Scalar, atype: pa.DataType) -> Optional[int]:
    """The int64 storage value of ``scalar`` as a date or timestamp of type ``atype``, or None
    when the conversion does not exist or is not exact: a timestamp with a time of day has no
    date image (the cast would drop the time, and ``date < timestamp`` compares in the wider
    type), so such a literal is not translatable and the file is kept."""
    try:
        c = scalar.cast(atype)
        if not c.is_valid or not c.cast(scalar.type).equals(scalar):
            return None
        return int(c.value)
    except (pa.ArrowInvalid, pa.ArrowNotImplementedError, AttributeError, TypeError, ValueError):
        return None


class _MinMaxCol:
    """One MinMax sketch in comparable form: ``mn`` / ``mx`` keys and the non-null mask."""

    def __init__(self, lo: pa.ChunkedArray, hi: pa.ChunkedArray):
        lo, hi = _plain(lo), _plain(hi)
        self.atype = t = lo.type
        self.valid = np.asarray(lo.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
        if pa.types.is_integer(t) or pa.types.is_date32(t) or pa.types.is_date64(t) or \
                pa.types.is_timestamp(t):
            self.domain = "int"
            st = pa.int32() if pa.types.is_date32(t) else pa.int64()
            conv = (lambda a: np.asarray((a.view(st) if not pa.types.is_integer(t) else a)
                                         .fill_null(0).to_numpy(zero_copy_only=False)).astype(np.int64))
        elif pa.types.is_floating(t) or pa.types.is_decimal(t):
            self.domain = "float"
            conv = (lambda a: f64_image(np.asarray(
                a.cast(pa.float64()).fill_null(0.0).to_numpy(zero_copy_only=False))))
        else:
            self.domain = "str"
            conv = (lambda a: np.array([b"" if x is None else x
                                        for x in a.cast(pa.binary()).to_pylist()], dtype=object))
        self.mn, self.mx = conv(lo), conv(hi)

    def key(self, scalar: pa.Scalar):
        """The literal in this column's key domain, or None when it has no exact image."""
        v = scalar.as_py()
        if v is None:
            return None
        if self.domain == "int":
            if isinstance(v, float):
                if v != v or v in (float("inf"), float("-inf")) or v != int(v):
                    return None
                v = int(v)
            if isinstance(v, bool):
                return None
            if isinstance(v, int):
                return v if -2 ** 63 <= v < 2 ** 63 and pa.types.is_integer(self.atype) else None
            return _exact_int(scalar, self.atype)
        if self.domain == "float":
            f = float(v)
            if f != f:
                return None
            return f64_image(np.array([f]))[0]
        if isinstance(v, str):
            return v.encode("utf-8")
        return None

    def test(self, op: str, k) -> np.ndarray:
        if op == "eq":
            m = (self.mn <= k) & (self.mx >= k)
        elif op == "lt":
            m = self.mn < k
        elif op == "le":
            m = self.mn <= k
        elif op == "gt":
            m = self.mx > k
        else:
            m = self.mx >= k
        return np.asarray(m, dtype=bool) & self.valid


class _BloomCol:
    def __init__(self, bits: pa.ChunkedArray, atype: pa.DataType):
        rows = _plain(bits).to_pylist()
        self.domain = _bloom_key_domain(atype)
        self.atype = column_type(atype)
        self.k = 0
        self.words = np.zeros((len(rows), 0), np.uint64)
        if rows:
            parsed = [bloom_deserialize(b) for b in rows]
            self.k = parsed[0][1]
            self.words = np.stack([w for w, _ in parsed])

    def might_contain(self, scalar: pa.Scalar) -> Optional[np.ndarray]:
        """Per file: may hold the literal; None when the literal has no hashed image."""
        v = scalar.as_py()
        if v is None or isinstance(v, bool):
            return None
        if self.domain == "str":
            if not isinstance(v, str):
                return None
            h1, h2 = _hash_pairs(pa.array([v], pa.string()))
        else:
            if isinstance(v, float):
                if v != v or v in (float("inf"), float("-inf")) or v != int(v):
                    return None
                v = int(v)
            if not isinstance(v, int):
                v = _exact_int(scalar, self.atype)
                if v is None:
                    return None
            elif not pa.types.is_integer(self.atype):
                return None
            if not -2 ** 63 <= v < 2 ** 63:
                return None
            h1, h2 = _hash_pairs(np.array([v], dtype=np.int64))
        nw = self.words.shape[1]
        if nw == 0:
            return np.ones(len(self.words), dtype=bool)
        pos = bloom_positions(h1, h2, nw, self.k)[0]
        hit = (self.words[:, pos >> 6] >> (pos & 63).astype(np.uint64)) & np.uint64(1)
        return hit.all(axis=1)


class SketchTable:
    """A data-skipping index's table in probe form."""

    def __init__(self, entry):
        t = read_sketch_table(entry)
        ids = np.asarray(t.column(C.DATA_FILE_NAME_ID).to_numpy(), dtype=np.int64)
        self.row_of_id = {int(v): i for i, v in enumerate(ids)}
        self.num_rows = t.num_rows
        self.minmax: Dict[str, _MinMaxCol] = {}
        self.bloom: Dict[str, _BloomCol] = {}
        src = {f.name: f.type for f in _source_schema(entry)}
        for s in entry.derived_dataset.sketches:
            c = s["column"]
            if s["type"] == MinMaxSketch.kind:
                lo, hi = minmax_names(c)
                self.minmax[c.lower()] = _MinMaxCol(t.column(lo), t.column(hi))
            else:
                self.bloom[c.lower()] = _BloomCol(t.column(bloom_name(c)), src.get(c, pa.int64()))
        tracker = {}
        for f in entry.source_file_info_set:
            tracker[(f.name, f.size, f.modified_time)] = f.id
        self.file_ids = tracker

    def column_type(self, name: str) -> Optional[pa.DataType]:
        c = self.minmax.get(name) or self.bloom.get(name)
        return c.atype if c is not None else None


def _source_schema(entry) -> pa.Schema:
    from ..plan.types import schema_from_json
    return schema_from_json(entry.relations[0].data_schema_json)


_TABLES: Dict[tuple, SketchTable] = {}


def sketch_table(entry) -> SketchTable:
    key = (entry.name.lower(), entry.id, tuple(sorted(entry.content.files)))
    hit = _TABLES.get(key)
    if hit is None:
        if len(_TABLES) > 64:
            _TABLES.clear()
        hit = _TABLES[key] = SketchTable(entry)
    return hit


_OPS = {"eq": "eq", "lt": "lt", "le": "le", "gt": "gt", "ge": "ge"}
_FLIPPED = {"eq": "eq", "lt": "gt", "le": "ge", "gt": "lt", "ge": "le"}


def _scalar_for(lit, target: pa.DataType) -> Optional[pa.Scalar]:
    from ..exec.arrow_eval import _coerce_literal
    if lit.value is None:
        return None
    try:
        return _coerce_literal(lit, target)
    except Exception:  # noqa: BLE001 - a literal that does not convert is not translatable
        return None


def _test_value(st: SketchTable, name: str, op: str, lit) -> Optional[np.ndarray]:
    """Files that may hold a row with ``name op lit``; None when not translatable."""
    mm, bf = st.minmax.get(name), st.bloom.get(name) if op == "eq" else None
    if mm is None and bf is None:
        return None
    scalar = _scalar_for(lit, st.column_type(name))
    if scalar is None:
        return None
    out = None
    try:
        if mm is not None:
            k = mm.key(scalar)
            if k is not None:
                out = mm.test(op, k)
        if bf is not None:
            m = bf.might_contain(scalar)
            if m is not None:
                out = m if out is None else out & m
    except Exception:  # noqa: BLE001
        return None
    return out


def _translate(st: SketchTable, e) -> Optional[np.ndarray]:
    from ..plan import expressions as E
    if isinstance(e, E.And):
        l, r = _translate(st, e.left), _translate(st, e.right)
        if l is None:
            return r
        return l if r is None else l & r
    if isinstance(e, E.Or):
        l, r = _translate(st, e.left), _translate(st, e.right)
        return None if l is None or r is None else l | r
    if isinstance(e, E.BinaryComparison) and getattr(e, "op", None) in _OPS:
        if isinstance(e.left, E.Attribute) and isinstance(e.right, E.Literal):
            return _test_value(st, e.left.name.lower(), e.op, e.right)
        if isinstance(e.right, E.Attribute) and isinstance(e.left, E.Literal):
            return _test_value(st, e.right.name.lower(), _FLIPPED[e.op], e.left)
        return None
    if isinstance(e, (E.In, E.InSet)) and isinstance(e.value, E.Attribute):
        if isinstance(e, E.In):
            if not all(isinstance(v, E.Literal) for v in e.values):
                return None
            lits = [v for v in e.values if v.value is not None]
        else:
            lits = [E.Literal(v) for v in e.hset if v is not None]
        name = e.value.name.lower()
        out = np.zeros(st.num_rows, dtype=bool)
        for lit in lits:
            m = _test_value(st, name, "eq", lit)
            if m is None:
                return None
            out |= m
        return out
    return None


def prune(entry, files: list, conjuncts: list) -> list:
    """The files of ``files`` (file statuses) that may hold a row passing every conjunct,
    judged by ``entry``'s sketches with the literals as they are now.  A file the index does
    not know (path, size, modification time) is kept."""
    st = sketch_table(entry)
    keep = np.ones(st.num_rows, dtype=bool)
    for c in conjuncts:
        m = _translate(st, c)
        if m is not None:
            keep &= m
    kept, unknown = [], 0
    for f in files:
        fid = st.file_ids.get((f.path, f.length, f.modification_time))
        row = st.row_of_id.get(fid) if fid is not None else None
        if row is None:
            unknown += 1
            kept.append(f)
        elif keep[row]:
            kept.append(f)
    LAST_PRUNE.clear()
    LAST_PRUNE.update({"index": entry.name, "files": len(files), "kept": len(kept),
                       "unknown": unknown, "kept_paths": [f.path for f in kept]})
    return kept
