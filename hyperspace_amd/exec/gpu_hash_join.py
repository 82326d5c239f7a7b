"""Broadcast hash joins on the device (``BroadcastHashJoinExec``): the join of a large relation
with a small one needs neither side bucketed or sorted - a hash table over the small ("build")
side (``K.hash_join_table``), the large ("stream") side probes it in one pass
(``K.hash_join_probe``, csrc/kernels/hash_join.hip), and both sides' columns are gathered by the
resulting row ids into a flat relation, the shape ``JoinOps._join_rel_pair`` returns.  The
preserved or filtered side of every join type the planner emits is the stream side.

Everything outside that - see ``HashJoinOps._hash_join_keys`` and ``_hash_join_rel`` - raises
``Unsupported`` and the query runs on the host with the same answer."""
from __future__ import annotations

from typing import List

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from ..ops import _lib as NL, kernels as K
from ..plan import expressions as E, physical as X
from ..utils.tracing import stage
from .arrow_eval import key
from .device_table import DeviceColumn, DeviceTable, is_string
from .gpu_common import DRel, Unsupported

# join types per build side (Planner._plan_join)
_JOIN_TYPES = {"right": ("inner", "left", "leftsemi", "leftanti"), "left": ("inner", "right")}


def _device_type(t: pa.DataType) -> bool:
    """Whether ``DeviceColumn.from_arrow`` holds a column of this Arrow type."""
    return (pa.types.is_integer(t) or pa.types.is_float32(t) or pa.types.is_float64(t) or
            pa.types.is_boolean(t) or pa.types.is_date(t) or pa.types.is_timestamp(t) or
            pa.types.is_decimal(t) or is_string(t))


class _LocalColumns(dict):
    """The device columns of a ``createDataFrame`` table by name.  A column whose type the device
    does not hold (lists, structs, binary, null, ...) is not uploaded; a query that never reads
    it is not affected, one that does is ``Unsupported`` with the type in the reason."""

    def __init__(self, cols, skipped):
        super().__init__(cols)
        self.skipped = skipped

    def __missing__(self, name):
        what = self.skipped.get(name)
        if what is None:
            raise KeyError(name)
        raise Unsupported(f"createDataFrame column {what} on the device")


class HashJoinOps:
    def _local_table_rel(self, p: X.LocalTableScanExec) -> DRel:
        """A ``createDataFrame`` table uploaded for this query (nothing is cached on it): the
        columns of ``p.output`` whose types the device holds (``_LocalColumns``)."""
        import torch
        d = self._dist()
        if d is not None and d.world > 1:
            # every rank holds the whole table: its rows would come back once per rank
            raise Unsupported("LocalTableScan on more than one rank")
        n = int(p.table.num_rows)
        cols, skipped, colmap = {}, {}, {}
        for a, arr in zip(p.output, p.table.columns):
            name = key(a)
            colmap[a.expr_id] = name
            if not _device_type(arr.type):
                skipped[name] = f"{a.name} of type {arr.type}"
                continue
            try:
                c = DeviceColumn.from_arrow(arr, self.device)
            except (TypeError, ValueError, KeyError, pa.ArrowInvalid,
                    pa.ArrowNotImplementedError) as e:
                skipped[name] = f"{a.name} of type {arr.type} ({type(e).__name__})"
                continue
            c.hs_transient = True
            cols[name] = c
        off = np.array([0, n], dtype=np.int64)
        table = DeviceTable(cols, n, torch.from_numpy(off).to(self.device), off)
        table.columns = _LocalColumns(cols, skipped)
        return DRel(table, colmap, list(p.output))

    # ------------------------------------------------------------------------------------------
    def _hash_join_key_pair(self, bc: DeviceColumn, sc: DeviceColumn):
        """(build, stream) columns of one key component whose values compare as int64.  String
        keys: the build side's codes are re-coded into the stream side's dictionary (one small
        lookup over the build rows; the stream column is read as it is) - a build string the
        stream dictionary lacks can match no stream row and becomes NULL, which is dropped from
        the table; that is the sorted-union remap of ``_string_join_keys`` restricted to the
        codes that can match."""
        import torch
        for c in (bc, sc):
            if pa.types.is_decimal(c.atype) or pa.types.is_floating(c.atype) or c.is_float:
                raise Unsupported("broadcast hash join on a float or decimal key")
            if c.hs_type == NL.U64:
                raise Unsupported("broadcast hash join on an unsigned 64-bit key")
            if is_string(c.atype) and c.dictionary is None:
                raise Unsupported("broadcast hash join on a string key without a device "
                                  "dictionary")
        bs, ss = bc.dictionary is not None, sc.dictionary is not None
        both_int = pa.types.is_integer(bc.atype) and pa.types.is_integer(sc.atype)
        if bs != ss or not (bs or both_int or bc.atype.equals(sc.atype)):
            raise Unsupported(f"broadcast hash join on keys of different types "
                              f"({bc.atype} and {sc.atype})")
        if not bs or bc.dictionary is sc.dictionary or bc.dictionary.equals(sc.dictionary):
            return bc, sc
        pos = pc.index_in(bc.dictionary.cast(pa.string()),
                          value_set=sc.dictionary.cast(pa.string()))
        found = torch.from_numpy(np.asarray(pos.is_valid().to_numpy(zero_copy_only=False),
                                            dtype=np.uint8)).to(self.device)
        remap = torch.from_numpy(np.asarray(pos.fill_null(0).to_numpy(zero_copy_only=False),
                                            dtype=np.int32)).to(self.device)
        if len(bc) and len(pos):
            data = K.lookup_i32(remap, bc.data)
            valid = K.gather_columns([DeviceColumn(found, None, pa.uint8())], bc.data,
                                     want_valid=False)[0].data
        else:
            data, valid = torch.zeros_like(bc.data), torch.zeros(len(bc), dtype=torch.uint8,
                                                                 device=self.device)
        if bc.valid is not None:
            valid = valid & (bc.valid != 0).to(torch.uint8)
        out = DeviceColumn(data, valid, sc.atype, sc.dictionary)
        out.hs_transient = True
        return out, sc

    def _hash_join_keys(self, build: DRel, stream: DRel, bks, sks):
        """(build key column, stream key column): one integer image per row, NULL where any
        component is.  Several columns pack into one int64 with the bases and widths of
        ``JoinOps._packed_join_keys`` (a plain tensor per side: there is no table to keep it
        on)."""
        import torch
        if not all(isinstance(k, E.Attribute) for k in list(bks) + list(sks)):
            raise Unsupported("broadcast hash join on expression keys")
        pairs = [self._hash_join_key_pair(build.col(bk), stream.col(sk))
                 for bk, sk in zip(bks, sks)]
        if len(pairs) == 1:
            return pairs[0]
        spans = []
        for bc, sc in pairs:
            if bc.dictionary is not None:
                doms = [(0, max(len(sc.dictionary), 1))]
            else:
                doms = [d for d in (self._local_domain(c) for c in (bc, sc)) if d[1] > 0]
            lo = min((d[0] for d in doms), default=0)
            hi = max((d[0] + d[1] - 1 for d in doms), default=0)
            spans.append((lo, max(1, int(hi - lo + 2).bit_length())))
        if sum(b for _, b in spans) > 62:
            raise Unsupported("broadcast hash join: the key columns do not pack into 62 bits")

        def pack(cols: List[DeviceColumn], null_code: int) -> DeviceColumn:
            n = len(cols[0])
            packed = torch.zeros(n, dtype=torch.int64, device=self.device)
            valid = None
            for c, (lo, bits) in zip(cols, spans):
                code = c.data.long() - (lo - 2)
                if c.valid is not None:
                    ok = c.valid != 0
                    code = torch.where(ok, code, torch.full_like(code, null_code))
                    valid = ok if valid is None else (valid & ok)
                packed = (packed << bits) | code
            out = DeviceColumn(packed, valid.to(torch.uint8) if valid is not None else None,
                               pa.int64())
            out.hs_transient = True
            return out
        return pack([b for b, _ in pairs], 1), pack([s for _, s in pairs], 0)

    # ------------------------------------------------------------------------------------------
    def _hash_join_rel(self, p: X.BroadcastHashJoinExec) -> DRel:
        """The joined rows as a flat relation over ``p.output``: each side's pending filters
        become row-id lists, the build side's keys go into the hash table, the stream side
        probes it - pairs (inner), pairs plus padded unmatched rows (left / right: the stream
        side is the preserved one) or match marks (left semi / anti) - and the output columns
        are gathered by the row ids.  ``metrics["hash_join"]`` describes the join."""
        import torch
        jt, side = p.join_type, p.build_side
        if jt not in _JOIN_TYPES.get(side, ()):
            raise Unsupported(f"broadcast hash join: {jt} join building the {side} side")
        if p.condition is not None and jt != "inner":
            raise Unsupported(f"broadcast hash join: residual condition on a {jt} join")
        d = self._dist()
        if d is not None and d.world > 1:
            raise Unsupported("broadcast hash join on more than one rank")
        lp, rp = p.left, p.right
        if isinstance(lp, X.BroadcastExchangeExec):
            lp = lp.child
        if isinstance(rp, X.BroadcastExchangeExec):
            rp = rp.child
        splan = lp if side == "right" else rp
        if getattr(self, "_bucket_chunk", None) is not None or \
                self._stream_chunks(splan) is not None:
            raise Unsupported("broadcast hash join over an index streamed in bucket ranges")
        left, right = self._rel(lp), self._rel(rp)
        if left.parts or right.parts:
            raise Unsupported("broadcast hash join over a bucket union")
        if left.split or right.split:
            raise Unsupported("broadcast hash join over a relation split across ranks")
        build, stream = (right, left) if side == "right" else (left, right)
        bks, sks = (p.right_keys, p.left_keys) if side == "right" else \
            (p.left_keys, p.right_keys)
        bkey, skey = self._hash_join_keys(build, stream, list(bks), list(sks))

        with stage("join.hash_build"):
            brows = self._selected_rows(build) if build.conds else None
            table = K.hash_join_table(bkey, brows)
        with stage("join.hash_probe"):
            srows = self._selected_rows(stream) if stream.conds else None
            nprobe = int(srows.numel()) if srows is not None else len(skey)
            if jt in ("leftsemi", "leftanti"):
                mark = K.hash_join_probe(table, skey, srows, how="mark")
                pos = torch.arange(nprobe, dtype=torch.int64, device=self.device)
                pos = K.select_marked(pos, mark, 1 if jt == "leftsemi" else 0)
                sid = srows.index_select(0, pos) if srows is not None else pos
                bid = None
            else:
                sid, bid = K.hash_join_probe(table, skey, srows,
                                             how="pairs" if jt == "inner" else "preserve")
        n = int(sid.numel())
        self.metrics["hash_join"] = {
            "build_rows": table.nbuild, "keys": table.nkeys, "slots": table.slots,
            "unique": table.unique, "probe_rows": nprobe, "pairs": n, "build_side": side}

        out_attrs = list(p.output)
        sset = {a.expr_id for a in splan.output}
        sattrs = [a for a in out_attrs if a.expr_id in sset]
        battrs = [a for a in out_attrs if a.expr_id not in sset] if bid is not None else []
        with stage("join.hash_gather"):
            sg = K.gather_columns([stream.col(a) for a in sattrs], sid) if sattrs else []
            bg = K.gather_columns([build.col(a) for a in battrs], bid,
                                  padded=jt in ("left", "right")) if battrs else []
        cols = {}
        for a, c in list(zip(sattrs, sg)) + list(zip(battrs, bg)):
            c.hs_transient = True
            cols[key(a)] = c
        off = np.array([0, n], dtype=np.int64)
        out = DRel(DeviceTable(cols, n, torch.from_numpy(off).to(self.device), off),
                   {a.expr_id: key(a) for a in out_attrs}, out_attrs)
        if p.condition is not None:
            # an inner join's residual: pending predicates of the joined rows
            out = self._unary(X.FilterExec(p.condition, p), out)
        return out


__all__ = ["HashJoinOps"]
