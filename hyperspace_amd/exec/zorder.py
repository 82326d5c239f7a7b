"""Device side of Z-order covering indexes (``index/zorder.py``, ``csrc/kernels/zorder.hip``).

Build: the source columns are uploaded like a covering build, ``hs_zorder_keys`` computes one
int64 Z-address per row from the columns' ``hs_sortable`` images, the 64-bit stable radix sort
orders the rows, and the bucket-file writer cuts them into key-range files.

Query: a resident Z-order table keeps per-zone min/max maps of its indexed columns (built once,
``hs_zone_minmax``).  A filter's ``col op literal`` conjuncts on those columns become inclusive
image intervals (``ZoneSpec``), ``hs_zone_prune`` turns them into the row-range list the fused
scan kernels read.  Every predicate is still evaluated per row: the maps only skip zones.
"""
from __future__ import annotations

import numbers
import time
from typing import Dict, List, Optional, Tuple

import pyarrow as pa

from ..index import zorder as ZO
from ..ops import _lib as NL
from ..ops import kernels as K
from ..plan import expressions as E
from ..utils.conf import HyperspaceConf
from . import compile as CP
from .device_table import DeviceColumn


# -- build --------------------------------------------------------------------------------------
def device_keys(key_cols: List[DeviceColumn]):
    """int64 Z-addresses of device columns (min / max from the same ``hs_sortable`` images the
    key kernel reads, not the sketch kernel's canonicalised floats)."""
    mins, shifts, bits = ZO.key_plan(K.zorder_column_ranges(key_cols))
    return K.zorder_keys(key_cols, mins, shifts, bits)


# per row on top of the decoded columns: the int64 key, the int32 permutation and file ids, and
# the radix sort's key / permutation double buffers
KEY_SORT_ROW_BYTES = 8 + 4 + 4 + 24


def device_build_fits(session, rel, files: List[str], columns: List[str],
                      lineage_ids) -> bool:
    """Whether the one-pass device build of ``files`` fits the build's HBM budget
    (``spark.hyperspace.mi.build.hbmBudgetBytes``): the decoded columns and their sorted copy
    (``BUILD_SORT_FACTOR``, as the covering build plans) plus keys and sort buffers.  A build
    that does not fit takes the host builder."""
    import torch
    from ..index.builder import source_format
    from ..io.reader import output_schema
    from . import device_build as DB
    from .device_table import storage_numpy_dtype
    if not files:
        return True
    device = torch.device("cuda", torch.cuda.current_device())
    budget = DB._build_budget(session, device)
    if source_format(rel) == "parquet":
        schema = output_schema(rel.data_schema, rel.location.partition_spec, columns)
        rows = sum(DB.source_row_counts(files, list(schema.names)))
        row_bytes = sum(storage_numpy_dtype(f.type).itemsize + 1 for f in schema) + \
            (8 if lineage_ids is not None else 0)
        est = int(rows * (row_bytes * DB.BUILD_SORT_FACTOR + KEY_SORT_ROW_BYTES))
    else:
        import os
        from ..utils import path_utils as P
        est = int(sum(os.path.getsize(P.to_local(f)) for f in files) * 2 * DB.BUILD_SORT_FACTOR)
    DB.LAST_BUILD_STATS["zorder_build_estimate"] = (est, budget)
    return est <= budget


def device_build_zorder(session, rel, files: List[str], columns: List[str], indexed: List[str],
                        nfiles: int, out_path: str, lineage_ids: Optional[Dict[str, int]],
                        mode: str = "overwrite") -> List[str]:
    import torch
    from ..index.builder import source_format
    from . import device_build as DB
    device = torch.device("cuda", torch.cuda.current_device())
    DB._prepare_out_dir(out_path, mode, None)
    t0 = time.perf_counter()
    DB._T0[0] = t0
    DB.LAST_BUILD_STATS.clear()
    if source_format(rel) == "parquet":
        cols, names, schema = DB._upload_parquet(rel, files, columns, indexed, lineage_ids,
                                                 device, None)
    else:
        cols, names, schema = DB._upload_generic(rel, files, files, columns, indexed,
                                                 lineage_ids, device, None)
    n = len(cols[names[0]]) if names else 0
    if n == 0:
        return []
    t1 = time.perf_counter()
    keys = device_keys([cols[c] for c in indexed])
    perm = K.sort_permutation([DeviceColumn(keys, None, pa.int64())])
    # file k holds sorted positions [k * ceil(n / F), (k + 1) * ceil(n / F)): a source row's
    # file follows from its rank in the permutation
    per = max(1, -(-n // nfiles))
    file_id = torch.empty(n, dtype=torch.int32, device=device)
    file_id[perm.long()] = (torch.arange(n, dtype=torch.int64, device=device) // per).int()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    paths = DB._sort_and_write(session, cols, names, file_id, indexed, nfiles, out_path, schema,
                               0, perm=perm)
    DB.LAST_BUILD_STATS.update({"read_h2d_s": t1 - t0, "zorder_keys_sort_s": t2 - t1,
                                "total_s": time.perf_counter() - t0})
    return paths


# -- zone maps ----------------------------------------------------------------------------------
# zones of an automatically sized zone map: the scan's tile-prefix pass (hs_ranges_to_tiles) walks
# the NZ-entry range list with one wavefront, 64 entries per step, twice per query - at 29 301
# one-tile zones (60M rows) that walk cost more device time than the whole unpruned scan
AUTO_MAX_ZONES = 4096


def zone_rows_of(conf, num_rows: int = 0) -> int:
    """Rows per zone, always a multiple of the scan tile so kept ranges are whole, tile-aligned
    scan tiles: ``spark.hyperspace.mi.zorder.zoneRows`` when set; else (0) one tile, doubled
    until a table of ``num_rows`` rows has at most ``AUTO_MAX_ZONES`` zones."""
    tile = int(NL.lib().hs_scan_tile_rows())
    z = HyperspaceConf.zorder_zone_rows(conf)
    if z <= 0:
        z = tile
        while -(-int(num_rows) // z) > AUTO_MAX_ZONES:
            z *= 2
        return z
    if z % tile:
        # a bad tuning key must not break queries: the host executor answers instead
        raise CP.Unsupported(f"spark.hyperspace.mi.zorder.zoneRows must be a multiple of the "
                             f"scan tile ({tile} rows), got {z}")
    return z


def table_zone_maps(table, names: Tuple[str, ...], zone_rows: int):
    """``(mn, mx, cnt)`` zone maps of columns ``names`` of a resident table, built on first use
    and kept on the table as derived state."""
    from .device_cache import track_derived
    held = table.__dict__.setdefault("_hs_zone_maps", {})
    key = (names, zone_rows)
    maps = held.get(key)
    if maps is None:
        maps = K.zone_minmax([table.columns[c] for c in names], zone_rows)
        track_derived(maps[0]._base if maps[0]._base is not None else maps[0])
        held[key] = maps
    return maps


def resident_zone_maps(backend):
    """``(table, column names, zone rows, maps)`` of every zone map the backend's resident
    tables hold (diagnostics and benchmarks)."""
    out = []
    for table in backend.cache.tables():
        for (names, zone), maps in getattr(table, "_hs_zone_maps", {}).items():
            out.append((table, names, zone, maps))
    return out


# -- lowering -----------------------------------------------------------------------------------
class ZoneSpec:
    """The literal-dependent part of a pruned scan: inclusive image intervals per zone-map
    column.  Tagged apart from the range-search spec tuple of a key-sorted relation."""

    __slots__ = ("names", "constraints")

    def __init__(self, names: Tuple[str, ...], constraints: List[Tuple[int, int, int]]):
        self.names = names                  # zone-map columns, in indexed order
        self.constraints = constraints      # (position in names, lo image, hi image)


class LazyCount:
    """A device counter read on first use (never when the scan is submitted)."""

    __slots__ = ("_t", "_at", "_v")

    def __init__(self, t, at: int):
        self._t, self._at, self._v = t, at, None

    def __int__(self) -> int:
        if self._v is None:
            self._v = int(self._t[self._at].item())
            self._t = None
        return self._v

    __index__ = __int__

    def __eq__(self, o):
        return int(self) == o

    def __hash__(self):
        return hash(int(self))

    def __repr__(self):
        return str(int(self))


_IMG_MAX = (1 << 64) - 1


def _interval(leaf, kc):
    """Inclusive image interval of ``col op literal`` on column ``kc``, or None when the
    comparison is no interval of images."""
    op, v = leaf.op, leaf.value
    if v is None or isinstance(v, str) or kc.dictionary is not None:
        return None
    if op not in (NL.OP_EQ, NL.OP_LT, NL.OP_LE, NL.OP_GT, NL.OP_GE):
        return None
    if kc.is_float:
        return K.float_key_image_range(op, float(v), kc.hs_type)
    width = {NL.I8: 8, NL.I16: 16, NL.I32: 32, NL.I64: 64}.get(kc.hs_type)
    if width is None or isinstance(v, bool):
        return None
    if not isinstance(v, numbers.Integral):
        try:
            f = float(v)
        except (TypeError, ValueError):
            return None
        if not f.is_integer():
            return None     # stays a per-row predicate only
        v = int(f)
    v = int(v)
    lo_v, hi_v = -(1 << (width - 1)), (1 << (width - 1)) - 1
    # value bounds first (a literal outside the storage range must not wrap), then images
    lo, hi = lo_v, hi_v
    if op in (NL.OP_EQ, NL.OP_GE):
        lo = v
    if op in (NL.OP_EQ, NL.OP_LE):
        hi = v
    if op == NL.OP_GT:
        lo = v + 1
    if op == NL.OP_LT:
        hi = v - 1
    lo, hi = max(lo, lo_v), min(hi, hi_v)
    if lo > hi:
        return 1, 0
    return K.sortable_image(lo, kc.hs_type), K.sortable_image(hi, kc.hs_type)


def _in_interval(c, kc):
    """``col IN (literals)`` (``In`` or its ``InSet`` form) as the ``[min, max]`` interval of
    its list, or None."""
    if not isinstance(c.value, E.Attribute):
        return None
    values = c.values if isinstance(c, E.In) else [E.Literal(v) for v in c.hset]
    out = None
    for x in values:
        if not isinstance(x, E.Literal) or x.value is None:
            return None
        leaf = CP._leaf(E.EqualTo(c.value, x))
        if leaf.kind != "cmp_lit":
            return None
        iv = _interval(leaf, kc)
        if iv is None:
            return None
        if iv[0] > iv[1]:
            continue
        out = iv if out is None else (min(out[0], iv[0]), max(out[1], iv[1]))
    return out if out is not None else (1, 0)


def zone_spec(r, conds: list, conf) -> Optional[ZoneSpec]:
    """The ``ZoneSpec`` of a relation with ``zone_attrs`` under ``conds``, or None (full ranges)
    when no conjunct constrains an indexed column or pruning is switched off."""
    if not HyperspaceConf.zorder_prune_enabled(conf):
        return None
    pos = {a.expr_id: i for i, a in enumerate(r.zone_attrs)}
    names = tuple(r.colmap[a.expr_id] for a in r.zone_attrs)
    bounds: Dict[int, Tuple[int, int]] = {}
    for c in conds:
        attr = iv = None
        try:
            if isinstance(c, (E.In, E.InSet)):
                attr = c.value if isinstance(c.value, E.Attribute) else None
                if attr is not None and attr.expr_id in pos and not r.is_computed(attr):
                    iv = _in_interval(c, r.col(attr))
            elif isinstance(c, E.BinaryComparison) and not isinstance(c, E.NotEqual):
                leaf = CP._leaf(c)
                if leaf.kind == "cmp_lit" and leaf.attr.expr_id in pos and \
                        not r.is_computed(leaf.attr):
                    attr = leaf.attr
                    iv = _interval(leaf, r.col(attr))
        except CP.Unsupported:
            continue
        if iv is None or attr is None:
            continue
        j = pos[attr.expr_id]
        old = bounds.get(j)
        bounds[j] = iv if old is None else (max(old[0], iv[0]), min(old[1], iv[1]))
    if not bounds:
        return None
    cons = []
    for j, (lo, hi) in sorted(bounds.items()):
        if lo > hi:
            lo, hi = 1, 0       # one spelling of the empty interval, inside uint64
        cons.append((j, max(0, lo), min(_IMG_MAX, hi)))
    return ZoneSpec(names, cons)


def zone_ranges(table, spec: ZoneSpec, zone_rows: int, metrics: dict):
    """``(rstart, rlen, None)`` of the zones ``spec`` keeps; ``metrics`` gets ``scan_zones`` and
    the lazily read ``scan_zones_kept``."""
    maps = table_zone_maps(table, spec.names, zone_rows)
    rstart, rlen, counts = K.zone_prune(maps, table.num_rows, zone_rows, spec.constraints)
    metrics["scan_zones"] = int(maps[0].shape[1])
    metrics["scan_zones_kept"] = LazyCount(counts, 1)
    return rstart, rlen, None
