"""Window functions on the device (``WindowExec``; kernels in csrc/kernels/window.hip).

The rows of the plan below the planner's own Sort / Exchange are brought into (partition keys
ascending, order keys) order - by one device sort, or not at all when the relation is an index
bucketed on exactly the partition keys whose sort order starts with (partition keys, order keys):
a partition then lies inside one bucket, contiguous and ordered, so the table order is already
the window's.  ``hs_win_heads`` marks partition and peer-group starts, ``hs_win_rank`` gives the
ranking functions, ``hs_win_agg`` the running / whole-partition aggregates.  The result is a
relation of the child's columns plus the window columns; filters, projections, sorts and
aggregates above it take the usual paths.

Shapes the kernels do not cover raise ``Unsupported`` at submission (the host engine runs the
query): several ranks, an index streamed in bucket ranges, a bucket-union input, keys or arguments
that are expressions, float PARTITION BY keys, strings without a device dictionary, decimal
arguments."""
from __future__ import annotations

import numpy as np
import pyarrow as pa

from ..ops import _lib as NL, kernels as K
from ..plan import expressions as E, logical as L, physical as X
from ..utils.tracing import stage
from .arrow_eval import key
from .device_table import DeviceColumn, DeviceTable, is_string
from .gpu_common import _prefix_sorted, DRel, Unsupported

_INT_TYPES = (NL.I8, NL.I16, NL.I32, NL.I64, NL.BOOL, NL.U32)


def _input_plan(p: X.WindowExec) -> X.SparkPlan:
    """The plan below the planner's Sort(partition keys, order keys) <- Exchange: the device
    decides about the sort itself and has every row on one rank."""
    base = p.child
    if isinstance(base, X.SortExec) and not base.global_sort:
        base = base.child
    if isinstance(base, X.ShuffleExchangeExec):
        base = base.child
    return base


def _check_key(c: DeviceColumn, a: E.Attribute, partition: bool) -> None:
    if is_string(c.atype) and c.dictionary is None:
        raise Unsupported(f"window key {a.name}: a string column without a device dictionary")
    if partition and c.is_float:
        raise Unsupported(f"window PARTITION BY a float column ({a.name})")
    if c.hs_type == NL.U64:
        raise Unsupported(f"window key {a.name}: unsigned 64-bit column")


def _agg_kind(fn, c) -> int:
    """The ``hs_win_agg`` kind of one function over its argument column (None: count(*))."""
    if isinstance(fn, E.Count):
        return NL.WA_COUNT
    if c is None:
        raise Unsupported(f"window {fn.name} without an argument")
    if pa.types.is_decimal(c.atype):
        raise Unsupported(f"window {fn.name} over a decimal column")
    if c.hs_type == NL.U64:
        raise Unsupported(f"window {fn.name} over an unsigned 64-bit column")
    if isinstance(fn, (E.Sum, E.Avg)):
        if c.dictionary is not None or is_string(c.atype) or not (
                pa.types.is_integer(c.atype) or pa.types.is_floating(c.atype)):
            raise Unsupported(f"window {fn.name} over a {c.atype} column")
        if isinstance(fn, E.Avg) or c.is_float:
            return NL.WA_SUM_F64
        return NL.WA_SUM_I64
    if is_string(c.atype) and c.dictionary is None:
        raise Unsupported(f"window {fn.name} over a string column without a device dictionary")
    if c.is_float:
        return NL.WA_MIN_F64 if isinstance(fn, E.Min) else NL.WA_MAX_F64
    return NL.WA_MIN_I64 if isinstance(fn, E.Min) else NL.WA_MAX_I64


def window_rel(be, p: X.WindowExec) -> DRel:
    """The device relation of a ``WindowExec``: its child's columns plus the window columns."""
    import torch
    d = be._dist()
    if d is not None and d.world > 1:
        raise Unsupported("window functions on more than one rank")
    base = _input_plan(p)
    if getattr(be, "_bucket_chunk", None) is not None or be._stream_chunks(base) is not None:
        raise Unsupported("window functions over an index streamed in bucket ranges")
    orders = list(p.order_by)
    for e in p.partition_by + [o.child for o in orders]:
        if not isinstance(e, E.Attribute):
            raise Unsupported("window key that is an expression")
    fns = [a.child.function for a in p.window_exprs]
    for fn in fns:
        if isinstance(fn, E.AggregateFunction) and fn.child is not None and \
                not isinstance(fn.child, E.Attribute):
            raise Unsupported("window aggregate over an expression")
    r = be._rel(base)
    if r.parts:
        raise Unsupported("window functions over a bucket union")
    if r.split:
        raise Unsupported("window functions over a relation split across ranks")
    attrs = list(base.output)
    for a in p.partition_by:
        _check_key(r.col(a), a, True)
    for o in orders:
        _check_key(r.col(o.child), o.child, False)
    kinds = [None if isinstance(fn, E.RankingFunction) else
             _agg_kind(fn, r.col(fn.child) if fn.child is not None else None) for fn in fns]

    keys = list(p.partition_by) + [o.child for o in orders]
    bucket_names = [r.colmap.get(a.expr_id) for a in r.bucket_attrs]
    skip = bool(r.bucketed and p.partition_by and bucket_names and
                [r.colmap.get(a.expr_id) for a in p.partition_by] == bucket_names and
                all(o.ascending for o in orders) and _prefix_sorted(r, keys))
    be.metrics["window_sort_skipped"] = skip
    with stage("window.order"):
        if not skip and keys:
            # the device sort orders floats by their bits: -0.0 before 0.0, NaNs by payload.
            # Peers must tie there too (the next key decides their order), so a float order key
            # sorts through a copy with one zero and one NaN
            r = r.copy()
            sort_orders, hidden = [], []
            for o in orders:
                c = r.col(o.child)
                if not c.is_float:
                    sort_orders.append(o)
                    continue
                h = E.Attribute("__hs_wkey", o.child.data_type, True)
                name = f"__hs_wkey_{h.expr_id}"
                norm = DeviceColumn(torch.where(torch.isnan(c.data),
                                                torch.full_like(c.data, float("nan")),
                                                c.data + 0.0), c.valid, c.atype)
                norm.hs_transient = True
                r.colmap[h.expr_id] = name
                r.extra[name] = norm
                hidden.append(h)
                sort_orders.append(L.SortOrder(h, o.ascending))
            r = be._sort_rel(r, [L.SortOrder(a, True) for a in p.partition_by] + sort_orders,
                             True, attrs + hidden)
        if r.conds:
            # table order, filtered: the selected rows keep it (ascending row ids)
            got = be._materialize(r, attrs)
            n = len(next(iter(got.values()))) if got else 0
            off = np.array([0, n], dtype=np.int64)
            cols = {key(a): got[a.expr_id] for a in attrs}
            r = DRel(DeviceTable(cols, n, torch.from_numpy(off).to(be.device), off),
                     {a.expr_id: key(a) for a in attrs}, attrs)
    n = int(r.table.num_rows)
    out = r.copy(attrs=list(p.output))
    with stage("window.kernels"):
        part = [r.col(a) for a in p.partition_by]
        order = [r.col(o.child) for o in orders]
        flags = K.win_heads(part, order, n, be.device)
        ws = K.win_workspace(n, be.device)
        ranks = {}
        want = [any(isinstance(fn, t) for fn in fns)
                for t in (E.RowNumber, E.Rank, E.DenseRank)]
        if any(want):
            got = K.win_rank(flags, *want, ws=ws)
            ranks = dict(zip((E.RowNumber, E.Rank, E.DenseRank), got))
        ends = None
        for a, fn, kind in zip(p.window_exprs, fns, kinds):
            if kind is None:
                col = DeviceColumn(ranks[type(fn)], None, pa.int32())
            else:
                if ends is None:
                    ends = K.win_frame_ends(flags, whole=not orders, ws=ws)
                col = _aggregate(fn, kind, r.col(fn.child) if fn.child is not None else None,
                                 flags, ends, ws)
            col.hs_transient = True
            name = f"__hs_win_{a.expr_id}"
            out.colmap[a.expr_id] = name
            out.extra[name] = col
    return out


def _aggregate(fn, kind: int, c, flags, ends, ws) -> DeviceColumn:
    """One windowed aggregate as a device column of the function's result type."""
    import torch
    if isinstance(fn, E.Avg):
        vals, valid, cnt = K.win_agg(c, flags, ends, kind, ws, with_count=True)
        return DeviceColumn(vals / cnt.clamp(min=1).to(torch.float64), valid, pa.float64())
    vals, valid = K.win_agg(c, flags, ends, kind, ws)
    if isinstance(fn, E.Count):
        return DeviceColumn(vals, None, pa.int64())
    if isinstance(fn, E.Sum):
        return DeviceColumn(vals, valid, pa.float64() if kind == NL.WA_SUM_F64 else pa.int64())
    # min / max: the input's type (dictionary codes keep their dictionary); the kernel skips
    # NaN like the other aggregates and gives NaN for a frame that holds nothing else
    data = vals if vals.dtype == c.data.dtype else vals.to(c.data.dtype)
    return DeviceColumn(data, valid, c.atype, c.dictionary)
