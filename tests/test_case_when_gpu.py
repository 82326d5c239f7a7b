"""CASE WHEN on the device.

Kernel level: guarded aggregates (``agg(CASE WHEN g THEN v [ELSE c] END)``: the guard is a CNF of
Pred entries behind the row filter's, ``AggSpec.pad`` places it) in the generated scan kernels -
strided and vectorised, full width and compact, ungrouped, LDS-grouped and in hash mode - and in
the generated join kernels, against the fp64 numpy reference of tests/case_ref.py.  Counts,
MIN / MAX and integer-valued sums are exact; a float sum is within ``2 * k * 2**-53 * sum(|x|)``
over its k contributing rows (the bound of tests/test_window_kernels_gpu.py).  Every case is
launched twice and the two results must be bit-equal; the grouped kernels add float sums with
atomics, so their bit-equal cases sum integer-valued doubles and a further grouped run checks
the inexact columns against the bound alone.

End to end: conditional aggregates through covering indexes against the host engine, fused and as
a hidden computed column, CASE in select / WHERE / GROUP BY, literal-only resubmission, Hybrid
Scan and a bucket-range streamed run.
"""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import case_ref as CR
import scan_ref as R
from hyperspace_amd import Hyperspace, IndexConfig, Session, col, count, sum_, when
from hyperspace_amd.exec import compile as CP
from hyperspace_amd.ops import _lib as NL
from hyperspace_amd.utils import murmur3

from test_gpu_e2e import _both, _close

pytestmark = pytest.mark.gpu

T1, T2 = 1024, 2048          # rows of a strided / a vectorised scan tile (BLOCK * items)
N = 3 * T2 + 17
# 1, 63, 64, 65, each tile boundary -1 / 0 / +1, three tiles + 17
COUNTS = [1, 63, 64, 65, T1 - 1, T1, T1 + 1, T2 - 1, T2, T2 + 1, 3 * T1 + 17, 3 * T2 + 17]
GG = CP.GUARD_GROUP


def _pad(first, count, has_else=False, never=False):
    return CP.G_ON | (CP.G_ELSE if has_else else 0) | (CP.G_NEVER if never else 0) | \
        (first << 8) | (count << 16)


class Table:
    def __init__(self, device):
        import torch
        rng = np.random.default_rng(31)
        c = {}
        c["f"] = rng.integers(0, 100, N).astype(np.int32)            # the row filter's column
        c["x"] = np.round(rng.random(N) * 1e4, 2)                    # value (decimal: compact)
        c["y"] = rng.integers(0, 11, N) / 100.0
        c["q"] = rng.integers(1, 51, N).astype(np.int64)             # integer-valued sums
        c["xi"] = rng.integers(0, 100_000, N).astype(np.float64)     # doubles with exact sums
        c["yi"] = rng.integers(0, 11, N).astype(np.float64)
        c["lane"] = (np.arange(N) % 2).astype(np.int32)              # alternating by lane
        last = np.zeros(N, np.int32)
        last[T1 - 1::T1] = 1                                         # last row of every tile
        last[N - 1] = 1
        c["last"] = last
        c["own"] = rng.integers(0, 100, N).astype(np.int32)          # a column of the guard's own
        mm = rng.normal(size=N) * 50
        c["mm"] = np.where(rng.random(N) < 0.1, np.nan, mm)          # NaN under min / max
        c["g3"] = rng.integers(0, 3, N).astype(np.int32)
        c["g257"] = rng.integers(0, 257, N).astype(np.int32)
        self.V = (rng.random(N) >= 0.15).astype(np.uint8)
        self._np = c
        hs = {v: k for k, v in R.NP_TYPE.items()}
        self._type = {n: hs[a.dtype.type] for n, a in c.items()}
        self._dev = {n: torch.from_numpy(a).to(device) for n, a in c.items()}
        self._vdev = torch.from_numpy(self.V).to(device)
        self.device = device
        self._compact = {}

    def col(self, name):
        b = name.rstrip("?")
        return (self._np[b], self.V if name.endswith("?") else None, self._type[b])

    def desc(self, name):
        b = name.rstrip("?")
        return NL.ColDesc(self._dev[b].data_ptr(), self._vdev.data_ptr() if name.endswith("?") else 0,
                          self._type[b], 0)

    def compact(self, name):
        if name not in self._compact:
            from hyperspace_amd.exec.device_table import DeviceColumn
            from hyperspace_amd.exec.encoding import encode
            b = name.rstrip("?")
            self._compact[name] = encode(DeviceColumn(
                self._dev[b], self._vdev if name.endswith("?") else None,
                pa.from_numpy_dtype(self._np[b].dtype)))
        return self._compact[name]

    def params(self, cols, preds, gpreds, aggs, group):
        """``aggs``: (kind, terms, guard) with guard None or (first, count, const, else_) over
        the guard predicates ``gpreds`` (indices relative to them)."""
        p = NL.ScanParams()
        for s, n in cols.items():
            p.cols[s] = self.desc(n)
        for i, (kind, op, c, c2, grp, ilit, flit, _) in enumerate(list(preds) + list(gpreds)):
            p.preds[i] = NL.Pred(kind, op, c, c2, grp, 0, int(ilit), float(flit), None)
        p.npreds = len(preds)
        for i, (kind, terms, guard) in enumerate(aggs):
            a = NL.AggSpec()
            a.kind, a.nterms = kind, len(terms)
            for t, (c, al, be) in enumerate(terms):
                a.col[t], a.alpha[t], a.beta[t] = c, al, be
            if guard is not None:
                first, cnt, const, else_ = guard
                if not terms:
                    a.alpha[0] = const
                if else_ is not None:
                    a.alpha[NL.MAX_TERMS - 1] = else_
                a.pad = _pad(len(preds) + first, cnt, else_ is not None)
            p.aggs[i] = a
        p.naggs = len(aggs)
        p.group_col, p.num_groups, p.group_base = group
        return p


_TABLE = []


@pytest.fixture
def T(device):
    if not _TABLE:
        _TABLE.append(Table(device))
    return _TABLE[0]


def _p(kind, op=0, c=0, group=0, ilit=0, flit=0.0):
    return (kind, op, c, 0, group, ilit, flit, None)


def _ref_aggs(aggs, gpreds):
    out = []
    for kind, terms, guard in aggs:
        if guard is None:
            out.append((kind, terms, None))
        else:
            first, cnt, const, else_ = guard
            out.append((kind, terms, (gpreds[first:first + cnt], const, else_)))
    return out


def _compare(ref, got, aggs, G, tag, int_sums=()):
    s, c, mn, mx = (x.reshape(G, len(aggs)) for x in got)
    for a, (kind, terms, _) in enumerate(aggs):
        assert np.array_equal(c[:, a], ref.count[:, a]), (tag, "count", a, c[:, a], ref.count[:, a])
        if kind == R.AK_SUM:
            if a in int_sums:
                assert np.array_equal(s[:, a], ref.sum[:, a]), (tag, "int sum", a)
            else:
                bound = 2.0 * ref.count[:, a] * 2.0 ** -53 * ref.abs_sum[:, a]
                err = np.abs(s[:, a] - ref.sum[:, a])
                assert (err <= bound).all(), (tag, "sum", a, err.max(), bound)
        elif kind == R.AK_MIN:
            assert np.array_equal(mn[:, a], ref.mn[:, a]), (tag, "min", a, mn[:, a], ref.mn[:, a])
        elif kind == R.AK_MAX:
            assert np.array_equal(mx[:, a], ref.mx[:, a]), (tag, "max", a, mx[:, a], ref.mx[:, a])


def _run(T, cols, preds, gpreds, aggs, group, ranges, int_sums=(), compact=(False, True),
         bit_equal=True):
    """Every generated scan form over ``ranges``, each twice, against the reference."""
    import torch
    from hyperspace_amd.exec import jit
    p = T.params(cols, preds, gpreds, aggs, group)
    assert jit.has_guards(p) == any(g is not None for _, _, g in aggs)
    ref = CR.scan_guarded({s: T.col(n) for s, n in cols.items()}, preds, _ref_aggs(aggs, gpreds),
                          *group, ranges=ranges)
    rstart = torch.tensor([s for s, _ in ranges], dtype=torch.int64, device=T.device)
    rlen = torch.tensor([ln for _, ln in ranges], dtype=torch.int64, device=T.device)
    G = group[1] if group[0] >= 0 else 1
    for comp in compact:
        cm = None
        if comp:
            cm = {s: e for s, e in ((s, T.compact(n)) for s, n in cols.items()) if e is not None}
            assert cm
            assert jit.scan_pack_layout(p, cm, 8) is None      # the row-packed form declines
        for nrows in (0, N):
            if nrows:
                assert jit.scan_vec(p, cm, nrows) != 0
            a = [t.cpu().numpy().copy() for t in jit.scan_agg(p, rstart, rlen, None, cm, nrows)]
            b = [t.cpu().numpy().copy() for t in jit.scan_agg(p, rstart, rlen, None, cm, nrows)]
            for x, y in zip(a, b):
                assert not bit_equal or x.tobytes() == y.tobytes(), "two launches differ"
            _compare(ref, a, aggs, G, (ranges[:2], comp, nrows), int_sums)
            _compare(ref, b, aggs, G, (ranges[:2], comp, nrows, "again"), int_sums)
    return ref


# slots: 0 f, 1 x, 2 y, 3 q, 4 guard column A (int32), 5 guard column B (int32, nullable),
# 6 mm, 7 x? (nullable value), 8 group
COLS = {0: "f", 1: "x", 2: "y", 3: "q", 4: "lane", 5: "own?", 6: "mm", 7: "x?"}
FILTER = [_p(R.PK_INT_LIT, R.OP_GE, 0, 0, ilit=10)]


def _guards(a_lit, a_col=4):
    """guard 0: A >= a_lit; guard 1: B < 50 (NULL B takes the ELSE side); guard 2: f < 50 (the
    filter's own column); guard 3: x > 5000 (an aggregate input)."""
    return [_p(R.PK_INT_LIT, R.OP_GE, a_col, GG, ilit=a_lit),
            _p(R.PK_INT_LIT, R.OP_LT, 5, 2 * GG, ilit=50),
            _p(R.PK_INT_LIT, R.OP_LT, 0, 3 * GG, ilit=50),
            _p(R.PK_FLT_LIT, R.OP_GT, 1, 4 * GG, flit=5000.0)]


AGGS = [(R.AK_SUM, [(1, 0.0, 1.0), (2, 1.0, -1.0)], (0, 1, None, 0.0)),   # sum(x*(1-y)) ELSE 0
        (R.AK_COUNT, [], (1, 1, 1.0, None)),                              # count(THEN 1)
        (R.AK_SUM, [(3, 0.0, 1.0)], (2, 1, None, None)),                  # int sum, no ELSE
        (R.AK_MIN, [(6, 0.0, 1.0)], (0, 1, None, None)),                  # NaN under min
        (R.AK_MAX, [(7, 0.0, 1.0)], (3, 1, None, -1.0)),                  # NULL value, ELSE -1
        (R.AK_SUM, [(1, 0.0, 1.0)], None),                                # unguarded beside them
        (R.AK_MAX, [(6, 0.0, 1.0)], (2, 1, None, None)),                  # NaN under max
        (R.AK_COUNT_STAR, [], None)]
STAR = len(AGGS) - 1


@pytest.mark.parametrize("n", COUNTS)
def test_guarded_scan_row_counts(T, n):
    """One range of ``n`` rows from an unaligned start; half the rows take guard 0."""
    start = 5 if n + 5 <= N else 0
    ref = _run(T, COLS, FILTER, _guards(1), AGGS, (-1, 1, 0), [(start, n)], int_sums=(2,))
    assert ref.count[0, STAR] == len(ref.rows)


def test_guarded_scan_disjoint_ranges(T):
    ranges = [(3, T1 + 1), (T1 + 70, 0), (T2 + 9, 63), (2 * T2 - 1, T2 + 2), (N - 1, 1)]
    _run(T, COLS, FILTER, _guards(1), AGGS, (-1, 1, 0), ranges, int_sums=(2,))


@pytest.mark.parametrize("lit,what", [(0, "all true"), (2, "all false"), (1, "alternating")])
def test_guard_all_true_all_false_alternating(T, lit, what):
    """The same kernels (literals are arguments): sum(.. ELSE 0) is 0 with a count when no row
    takes the guard, min without ELSE has no row then."""
    ref = _run(T, COLS, FILTER, _guards(lit), AGGS, (-1, 1, 0), [(0, N)], int_sums=(2,))
    nrows = len(ref.rows)
    assert ref.count[0, 0] == nrows                      # ELSE 0: every passing row counts
    if lit == 2:
        assert ref.sum[0, 0] == 0.0 and ref.count[0, 3] == 0 and ref.mn[0, 3] == np.inf
    if lit == 0:
        assert ref.count[0, 3] == nrows                  # (NaN is a value: it counts)


def test_guard_true_only_in_last_row_of_a_tile(T):
    cols = dict(COLS)
    cols[4] = "last"
    ref = _run(T, cols, [], _guards(1), AGGS, (-1, 1, 0), [(0, N)], int_sums=(2,))
    assert 0 < ref.count[0, 3] <= N // T1 + 1


@pytest.mark.parametrize("G,gcol", [(3, "g3"), (257, "g257")])
def test_guarded_scan_lds_grouped(T, G, gcol):
    """The LDS-grouped kernels add a group's float sums with atomics, in an order that varies
    from launch to launch (guarded or not, as before): two launches are bit-equal when the sums
    are exact in every order.  So the grouped cases sum integer-valued doubles - every sum is
    then held exactly - and the inexact ones are summed ungrouped above."""
    cols = dict(COLS)
    cols.update({1: "xi", 2: "yi", 7: "xi?", 8: gcol})
    _run(T, cols, FILTER, _guards(1), AGGS, (8, G, 0), [(7, N - 7)], int_sums=(0, 2, 5))
    # the inexact columns, grouped: each launch within the float-sum bound (not bit-equal)
    cols = dict(COLS)
    cols[8] = gcol
    _run(T, cols, FILTER, _guards(1), AGGS, (8, G, 0), [(7, N - 7)], int_sums=(2,),
         bit_equal=False)


@pytest.mark.parametrize("ranges", [[(5, N - 5)], [(3, T1 + 1), (T2 + 9, 63), (2 * T2 - 1, T2 + 2)]],
                         ids=["one", "disjoint"])
def test_guarded_scan_hash_mode(T, ranges):
    """The hash-mode scan (``hk`` / ``htab``: groups keyed in a device hash table) with the same
    guards: every group of the table against the reference, strided and vectorised, full width
    and compact, each launched twice into a fresh table.  The table's sums are float atomics,
    so - as in the LDS-grouped case - the summed columns are integer-valued doubles."""
    import torch
    import types
    from hyperspace_amd.exec import hash_agg as H, jit
    cols = dict(COLS)
    cols.update({1: "xi", 2: "yi", 7: "xi?", 8: "g257"})
    group = (-1, 1, 0)
    p = T.params(cols, FILTER, _guards(1), AGGS, group)
    ref = CR.scan_guarded({s: T.col(n) for s, n in cols.items()}, FILTER,
                          _ref_aggs(AGGS, _guards(1)), 8, 257, 0, ranges=ranges)
    live = np.flatnonzero(ref.count[:, STAR] > 0)
    assert len(live) > 200
    kc = types.SimpleNamespace(hs_type=NL.I32, valid=None, dictionary=None, offsets=None,
                               atype=pa.int32())
    own = tuple(kind != R.AK_COUNT_STAR for kind, _, _ in AGGS)
    hk = H.plan_keys([(8, None, kc, (0, 257, None))], own, True)
    assert hk.mode == "packed"
    rstart = torch.tensor([s for s, _ in ranges], dtype=torch.int64, device=T.device)
    rlen = torch.tensor([ln for _, ln in ranges], dtype=torch.int64, device=T.device)
    NA = len(AGGS)
    for comp in (False, True):
        cm = None
        if comp:
            cm = {s: e for s, e in ((s, T.compact(n)) for s, n in cols.items()) if e is not None}
        for nrows in (0, N):
            outs = []
            for _ in range(2):
                t = H.HashTable(1024, NA, True, T.device)
                jit.scan_agg(p, rstart, rlen, None, cm, nrows, hk=hk, htab=t)
                g = t.extract(STAR)
                G, over = g.count()
                assert not over and G == len(live), (G, len(live))
                h = g.to_host()
                keys = hk.unpack(h["keys"], h["nulls"])[0].to_numpy(zero_copy_only=False)
                order = np.argsort(keys)
                assert np.array_equal(keys[order], live)
                outs.append(tuple(h[k][order] for k in ("sums", "cnts", "mins", "maxs")))
            for x, y in zip(*outs):
                assert x.tobytes() == y.tobytes(), "two launches differ"
            s_, c_, mn_, mx_ = outs[0]
            tag = (comp, nrows)
            for a, (kind, terms, _) in enumerate(AGGS):
                assert np.array_equal(c_[:, a], ref.count[live, a]), (tag, "count", a)
                if kind == R.AK_SUM:
                    assert np.array_equal(s_[:, a], ref.sum[live, a]), (tag, "sum", a)
                elif kind == R.AK_MIN:
                    assert np.array_equal(mn_[:, a], ref.mn[live, a]), (tag, "min", a)
                elif kind == R.AK_MAX:
                    assert np.array_equal(mx_[:, a], ref.mx[live, a]), (tag, "max", a)


def test_unguarded_shape_and_source_do_not_change(T):
    """A guard is part of the shape key and of the source; without one both are what they were."""
    from hyperspace_amd.exec import jit
    plain = [(k, t, None) for k, t, _ in AGGS]
    p0 = T.params(COLS, FILTER, [], plain, (-1, 1, 0))
    p1 = T.params(COLS, FILTER, _guards(1), AGGS, (-1, 1, 0))
    p2 = T.params(COLS, FILTER, _guards(7), AGGS, (-1, 1, 0))
    assert jit.scan_agg_shape(p1) == jit.scan_agg_shape(p2) != jit.scan_agg_shape(p0)
    assert all(len(e) == 3 for e in jit.scan_agg_shape(p0)[3])
    assert "a.E0" in jit.gen_scan_agg(p1).src and "a.E0" not in jit.gen_scan_agg(p0).src


# -- joins ------------------------------------------------------------------------------------------
def test_guarded_join_kernels(device):
    """Generic tiled join, merge join (full width and compact; the run-keyed form declines) and
    the grouped form: guards on a left column, on a right column and an unguarded aggregate."""
    import torch
    from hyperspace_amd.exec import jit, jit_runs
    from hyperspace_amd.exec.device_table import DeviceColumn
    from hyperspace_amd.exec.encoding import encode
    from hyperspace_amd.ops import kernels as K
    rng = np.random.default_rng(9)
    B = 8
    rk = np.arange(0, 6000, dtype=np.int64) * 3                      # unique right keys
    lk = np.concatenate([np.repeat(rk[::2], rng.integers(1, 6, len(rk[::2]))),
                         rng.integers(0, 20_000, 3000)])
    rb, lb = murmur3.bucket_ids([pa.array(rk)], B), murmur3.bucket_ids([pa.array(lk)], B)
    ro = np.lexsort((rk, rb)); rk, rb = rk[ro], rb[ro]
    lo_ = np.lexsort((lk, lb)); lk, lb = lk[lo_], lb[lo_]
    loff = np.searchsorted(lb, np.arange(B + 1)).astype(np.int64)
    roff = np.searchsorted(rb, np.arange(B + 1)).astype(np.int64)
    ldate = rng.integers(0, 1000, len(lk)).astype(np.int32)
    lprice = np.round(rng.random(len(lk)) * 100, 2)
    rpri = rng.integers(0, 5, len(rk)).astype(np.int32)
    rnull = rng.random(len(rk)) < 0.1
    rgrp = rng.integers(0, 3, len(rk)).astype(np.int32)
    cl = [DeviceColumn.from_arrow(pa.array(x), device) for x in (lk, ldate, lprice)]
    cr = [DeviceColumn.from_arrow(pa.array(rk), device),
          DeviceColumn.from_arrow(pa.array(rpri, mask=rnull), device),
          DeviceColumn.from_arrow(pa.array(rgrp), device)]
    p = NL.JoinParams()
    for i, c in enumerate(cl):
        p.cols[i] = c.desc()
    for i, c in enumerate(cr):
        p.cols[8 + i] = c.desc()
    p.preds[0] = NL.Pred(NL.PK_INT_LIT, NL.OP_GT, 1, 0, 0, 0, 100, 0.0, None)        # ldate > 100
    p.preds[1] = NL.Pred(NL.PK_INT_LIT, NL.OP_LE, 9, 0, GG, 0, 1, 0.0, None)         # g0: rpri <= 1
    p.preds[2] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 1, 0, 2 * GG, 0, 500, 0.0, None)   # g1: ldate < 500
    p.nlp, p.npreds = 1, 1
    a0 = NL.AggSpec(); a0.kind, a0.nterms = NL.AK_SUM, 1
    a0.col[0], a0.alpha[0], a0.beta[0] = 2, 0.0, 1.0
    a0.pad = _pad(1, 1, True)                                  # sum(CASE g0 THEN lprice ELSE 0)
    a1 = NL.AggSpec(); a1.kind, a1.nterms = NL.AK_COUNT, 0
    a1.alpha[0] = 1.0
    a1.pad = _pad(2, 1)                                        # count(CASE g1 THEN 1)
    a2 = NL.AggSpec(); a2.kind, a2.nterms = NL.AK_SUM, 1
    a2.col[0], a2.alpha[0], a2.beta[0] = 2, 0.0, 1.0           # sum(lprice)
    a3 = NL.AggSpec(); a3.kind, a3.nterms = NL.AK_COUNT_STAR, 0
    for i, a in enumerate((a0, a1, a2, a3)):
        p.aggs[i] = a
    p.naggs, p.lkey, p.rkey, p.key_is_float = 4, 0, 8, 0
    assert jit.has_guards(p) and not jit_runs.applies(p)
    # reference
    rrow = {int(k): i for i, k in enumerate(rk)}
    j = np.array([rrow.get(int(k), -1) for k in lk])
    m = (j >= 0) & (ldate > 100)
    jm = j[m]
    g0 = (~rnull[jm]) & (rpri[jm] <= 1)
    g1 = ldate[m] < 500
    price = lprice[m]
    rstart, rlen, rbk = K.full_ranges(loff, device)
    roff_t = torch.from_numpy(roff).to(device)
    mt = K.join_max_tiles(len(lk), B)
    # grouped: a group's float sums are added in an order that varies between launches, so the
    # grouped runs sum integer-valued doubles (exact in every order) and stay bit-equal
    lwhole = np.floor(lprice * 100)
    cwhole = DeviceColumn.from_arrow(pa.array(lwhole), device)
    for grp in (-1, 10):
        p.group_col, p.num_groups, p.group_base = grp, 3, 0
        G = 3 if grp >= 0 else 1
        gid = rgrp[jm] if grp >= 0 else np.zeros(len(jm), np.int32)
        if grp >= 0:
            cl[2], price = cwhole, lwhole[m]
            p.cols[2] = cwhole.desc()
        allc = dict(enumerate(cl))
        allc.update({8 + i: c for i, c in enumerate(cr)})
        comp = {s: e for s, e in ((s, encode(c)) for s, c in allc.items()) if e is not None}
        assert 0 in comp and 8 in comp
        assert jit._with_runs(p, comp)[1] is None

        def run(which, cm):
            if which == "tiled":
                return jit.join_agg(p, rstart, rlen, rbk, roff_t, mt, cm)
            return jit.merge_join_agg(p, rstart, rlen, rbk, roff_t, cm, nrows=len(lk), rdup=False)
        for which in ("tiled", "merge"):
            for cm in (None, comp):
                a = [t.cpu().numpy().copy() for t in run(which, cm)]
                b = [t.cpu().numpy().copy() for t in run(which, cm)]
                for x, y in zip(a, b):
                    assert x.tobytes() == y.tobytes(), (which, "two launches differ")
                s, c = a[0].reshape(G, 4), a[1].reshape(G, 4)
                for g in range(G):
                    sel = gid == g
                    tag = (which, cm is None, grp, g)
                    assert c[g, 3] == sel.sum() and c[g, 0] == sel.sum(), tag
                    assert c[g, 1] == (sel & g1).sum(), tag
                    assert c[g, 2] == sel.sum(), tag
                    for k, vals in ((0, price[sel & g0]), (2, price[sel])):
                        bound = 2.0 * max(len(vals), 1) * 2.0 ** -53 * np.abs(vals).sum()
                        assert abs(s[g, k] - float(np.sum(vals.astype(np.longdouble)))) <= bound, tag


# -- end to end ----------------------------------------------------------------------------------------
@pytest.fixture
def tpch(tmp_path, device):
    rng = np.random.default_rng(17)
    n_ord = 12_000
    okeys = rng.permutation(np.arange(1, n_ord + 1, dtype=np.int64) * 4)
    pri = np.array(["1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"])
    od = pa.table({"o_orderkey": okeys,
                   "o_orderdate": pa.array(rng.integers(8000, 10500, n_ord).astype(np.int32)).view(pa.date32()),
                   "o_orderpriority": pa.array(pri[rng.integers(0, 5, n_ord)]),
                   "o_shippriority": rng.integers(0, 3, n_ord).astype(np.int32)})
    lk = np.repeat(okeys, rng.integers(1, 8, n_ord))
    n = len(lk)
    types = np.array(["PROMO BRUSHED", "PROMO PLATED", "STANDARD TIN", "ECONOMY STEEL", "LARGE BRASS"])
    qn = rng.random(n) < 0.1
    li = pa.table({"l_orderkey": lk,
                   "l_quantity": pa.array(rng.integers(1, 51, n).astype(np.float64), mask=qn),
                   "l_extendedprice": np.round(rng.random(n) * 1e5, 2),
                   "l_discount": rng.integers(0, 11, n) / 100.0,
                   "l_shipdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32)).view(pa.date32()),
                   "l_shipmode": pa.array(np.array(["MAIL", "SHIP", "AIR", "RAIL"])[rng.integers(0, 4, n)]),
                   "l_type": pa.array(types[rng.integers(0, 5, n)]),
                   "l_linenumber": rng.integers(1, 8, n).astype(np.int32)})
    assert n <= 60_000
    for name, t, parts in (("lineitem", li, 3), ("orders", od, 2)):
        os.makedirs(tmp_path / name)
        step = (t.num_rows + parts - 1) // parts
        for i in range(parts):
            pq.write_table(t.slice(i * step, step), tmp_path / name / f"part-{i}.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.numBuckets": "8",
                      "spark.sql.autoBroadcastJoinThreshold": "-1",
                      "spark.sql.shuffle.partitions": "8",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    hs = Hyperspace(s)
    lpath, opath = str(tmp_path / "lineitem"), str(tmp_path / "orders")
    hs.createIndex(s.read.parquet(lpath), IndexConfig(
        "li_ok", ["l_orderkey"], ["l_quantity", "l_extendedprice", "l_discount", "l_shipdate",
                                  "l_shipmode", "l_type", "l_linenumber"]))
    hs.createIndex(s.read.parquet(lpath), IndexConfig(
        "li_ship", ["l_shipdate"], ["l_quantity", "l_extendedprice", "l_discount", "l_shipmode",
                                    "l_type"]))
    hs.createIndex(s.read.parquet(opath), IndexConfig(
        "od_ok", ["o_orderkey"], ["o_orderdate", "o_orderpriority", "o_shippriority"]))
    Hyperspace.enable(s)
    s.read.parquet(lpath).createOrReplaceTempView("lineitem")
    s.read.parquet(opath).createOrReplaceTempView("orders")
    return s, lpath, opath


def _native(s, q, cond_agg=None, index=()):
    plan = q.queryExecution.executed_plan.tree_string()
    for name in index:
        assert f"Name: {name}" in plan, plan
    g, c, path = _both(s, q)
    assert path == "native", s.backend().fallback_reason
    _close(g, c)
    if cond_agg is not None:
        assert s.backend().metrics.get("cond_agg") == cond_agg, s.backend().metrics.get("cond_agg")
    return g


Q6 = ("SELECT sum(CASE WHEN l_discount >= 0.05 THEN l_extendedprice * l_discount ELSE 0 END) rev, "
      "count(CASE WHEN l_quantity < 24 THEN 1 END) small, "
      "avg(CASE WHEN l_shipmode = 'MAIL' THEN l_quantity ELSE 0 END) aq, "
      "min(CASE WHEN l_type LIKE 'PROMO%' THEN l_extendedprice END) mn, "
      "sum(l_extendedprice) tot, count(*) n "
      "FROM lineitem WHERE l_shipdate >= DATE '1994-01-01' AND l_shipdate < DATE '1997-01-01'")
Q12 = ("SELECT l_shipmode, "
       "sum(CASE WHEN o_orderpriority IN ('1-URGENT', '2-HIGH') THEN 1 ELSE 0 END) high, "
       "sum(CASE WHEN o_orderpriority <> '1-URGENT' AND o_orderpriority <> '2-HIGH' THEN 1 ELSE 0 END) low "
       "FROM orders JOIN lineitem ON o_orderkey = l_orderkey "
       "WHERE l_shipmode IN ('MAIL', 'SHIP') AND l_linenumber < 6 GROUP BY l_shipmode")
Q14 = ("SELECT 100.0 * sum(CASE WHEN l_type LIKE 'PROMO%' THEN l_extendedprice * (1 - l_discount) "
       "ELSE 0 END) / sum(l_extendedprice * (1 - l_discount)) promo "
       "FROM lineitem JOIN orders ON l_orderkey = o_orderkey WHERE o_orderdate >= DATE '1995-01-01'")


def test_q6_style_fused_ungrouped(tpch):
    s, _, _ = tpch
    g = _native(s, s.sql(Q6), "fused", ["li_ship"])
    assert g.num_rows == 1 and g.column("small")[0].as_py() > 0


RIGHT = ("sum(CASE WHEN o_orderpriority IN ('1-URGENT', '2-HIGH') THEN 1 ELSE 0 END) high, "
         "sum(CASE WHEN o_orderpriority = '5-LOW' THEN l_extendedprice ELSE 0 END) lowrev, "
         "count(CASE WHEN o_orderpriority LIKE '%HIGH' OR o_orderpriority LIKE '3-%' THEN 1 END) k, "
         "min(CASE WHEN o_shippriority > 0 THEN l_discount END) md, count(*) n "
         "FROM lineitem JOIN orders ON l_orderkey = o_orderkey WHERE l_linenumber < 6")


@pytest.mark.parametrize("grouped", [False, True], ids=["ungrouped", "grouped"])
def test_guards_on_the_right_side_of_the_merge_join(tpch, grouped):
    """lineitem is the join's left input (no side is 64 times smaller, so the kernel does not
    swap them): the guards read dictionary (=, IN, LIKE) and integer columns of the right input,
    orders, and are bound behind the right side's predicates."""
    s, _, _ = tpch
    text = f"SELECT l_shipmode, {RIGHT} GROUP BY l_shipmode" if grouped else f"SELECT {RIGHT}"
    q = s.sql(text)
    plan = q.queryExecution.executed_plan.tree_string()
    assert "SortMergeJoin" in plan and plan.index("Name: li_ok") < plan.index("Name: od_ok"), plan
    g = _native(s, q, "fused", ["li_ok", "od_ok"])
    assert g.num_rows == (4 if grouped else 1)
    row = g.to_pylist()[0]
    assert 0 < row["high"] < row["n"] and 0 < row["k"] < row["n"] and row["lowrev"] > 0


def test_q12_and_q14_style_join_guards(tpch):
    """Guards on a dictionary string (IN, <>, LIKE) on the left input of the merge join, grouped
    and ungrouped (the right input: ``test_guards_on_the_right_side_of_the_merge_join``)."""
    s, _, _ = tpch
    g = _native(s, s.sql(Q12), "fused", ["li_ok", "od_ok"])
    assert g.num_rows == 2
    _native(s, s.sql(Q14), "fused", ["li_ok", "od_ok"])


def test_guard_on_the_build_side_of_a_broadcast_join(tpch, tmp_path):
    s, lpath, _ = tpch
    dim = pa.table({"d_ln": np.arange(1, 8, dtype=np.int32),
                    "d_class": (np.arange(1, 8) % 3).astype(np.int32),
                    "d_w": pa.array(np.linspace(0.0, 1.0, 7), mask=np.arange(7) == 2)})
    os.makedirs(tmp_path / "dim")
    pq.write_table(dim, tmp_path / "dim" / "part-0.parquet")
    s.conf.set("spark.sql.autoBroadcastJoinThreshold", str(10 << 20))
    li, d = s.read.parquet(lpath), s.read.parquet(str(tmp_path / "dim"))
    q = li.filter(col("l_orderkey") < 30000).join(d, li["l_linenumber"] == d["d_ln"]).agg(
        sum_(when(col("d_class") == 1, col("l_extendedprice")).otherwise(0)).alias("c1"),
        count(when(col("d_w") > 0.5, 1)).alias("heavy"), count("*").alias("n"))
    assert "BroadcastHashJoin" in q.queryExecution.executed_plan.tree_string()
    g = _native(s, q, "fused")
    assert 0 < g.column("heavy")[0].as_py() < g.column("n")[0].as_py()


def test_guard_semantics_against_the_host(tpch):
    """All-false guards: sum(.. ELSE 0) is 0, without ELSE it is NULL; count is 0; avg(.. ELSE 0)
    divides by every row that passes the filter; a NULL guard takes the ELSE side."""
    s, _, _ = tpch
    q = s.sql("SELECT sum(CASE WHEN l_discount > 5 THEN l_extendedprice ELSE 0 END) z, "
              "sum(CASE WHEN l_discount > 5 THEN l_extendedprice END) nul, "
              "count(CASE WHEN l_shipmode = 'NOPE' THEN 1 END) c0, "
              "avg(CASE WHEN l_quantity < 10 THEN l_quantity ELSE 0 END) a, "
              "sum(CASE WHEN l_quantity >= 0 THEN 0 ELSE 1 END) nullq, count(*) n "
              "FROM lineitem WHERE l_linenumber < 4")
    g = _native(s, q, "fused")
    row = g.to_pylist()[0]
    assert row["z"] == 0.0 and row["nul"] is None and row["c0"] == 0 and row["nullq"] > 0


def test_fused_switch_off_takes_the_column_route_with_equal_results(tpch):
    s, _, _ = tpch
    text = ("SELECT l_linenumber, sum(CASE WHEN l_discount >= 0.05 THEN l_extendedprice ELSE 0 END) r, "
            "count(CASE WHEN l_quantity < 24 THEN 1 END) c FROM lineitem "
            "WHERE l_shipdate < DATE '1996-06-01' GROUP BY l_linenumber")
    fused = _native(s, s.sql(text), "fused")
    s.conf.set("spark.hyperspace.mi.condAgg.fused", "false")
    try:
        column = _native(s, s.sql(text), "column")
    finally:
        s.conf.set("spark.hyperspace.mi.condAgg.fused", "true")
    _close(fused, column)


def test_multi_branch_case_takes_the_column_route_natively(tpch):
    s, _, _ = tpch
    q = s.sql("SELECT sum(CASE WHEN l_quantity < 10 THEN 1 WHEN l_quantity < 30 THEN 2 ELSE 3 END) w, "
              "sum(2 * CASE WHEN l_discount > 0.05 THEN l_extendedprice ELSE 0 END) d, "
              "count(CASE WHEN l_shipmode = 'AIR' THEN 1 END) air "      # stays a fused guard

              "FROM lineitem WHERE l_linenumber < 5")
    _native(s, q, "column")


def test_string_valued_case_falls_back_with_its_reason(tpch):
    s, _, _ = tpch
    q = s.sql("SELECT max(CASE WHEN l_quantity < 10 THEN l_shipmode ELSE 'none' END) m FROM lineitem")
    g, c, path = _both(s, q)
    _close(g, c)
    assert path != "native" and s.backend().fallback_reason


def test_case_in_select_where_and_group_by(tpch):
    s, lpath, _ = tpch
    li = s.read.parquet(lpath)
    sel = li.filter(col("l_orderkey") < 4000).select(
        "l_orderkey", when(col("l_quantity") < 10, col("l_extendedprice"))
        .when(col("l_quantity").isNull(), -1.0).otherwise(col("l_discount")).alias("v"),
        when(col("l_shipdate") < "1995-01-01", col("l_shipdate")).alias("d"))
    _native(s, sel)
    _native(s, s.sql("SELECT count(*) n, sum(l_extendedprice) t FROM lineitem "
                     "WHERE CASE WHEN l_quantity < 10 THEN l_discount ELSE 0.0 END > 0.04"))
    _native(s, s.sql("SELECT CASE WHEN l_quantity < 25 THEN 0 ELSE 1 END b, count(*) n, "
                     "sum(l_extendedprice) t FROM lineitem "
                     "GROUP BY CASE WHEN l_quantity < 25 THEN 0 ELSE 1 END"))


def test_hash_mode_group_with_guards(tpch):
    """A nullable float group key runs the hash-mode aggregate."""
    s, _, _ = tpch
    q = s.sql("SELECT l_quantity, sum(CASE WHEN l_discount >= 0.05 THEN l_extendedprice ELSE 0 END) r, "
              "count(CASE WHEN l_shipmode = 'AIR' THEN 1 END) c, "
              "max(CASE WHEN l_linenumber > 3 THEN l_discount END) m, count(*) n "
              "FROM lineitem GROUP BY l_quantity")
    be = s.backend()
    be.htables.sizes.clear()
    g = _native(s, q, "fused")
    assert g.num_rows == 51
    assert len(be.htables.sizes) == 1, "the hash-mode aggregate ran (its table size is kept)"
    # and over the merge join, the guard on the right input
    from hyperspace_amd.exec import jit
    jit.LAST_MJ_PATH[0] = None
    j = s.sql("SELECT l_quantity, sum(CASE WHEN o_orderpriority = '1-URGENT' THEN l_extendedprice "
              "ELSE 0 END) r, count(CASE WHEN o_shippriority > 0 THEN 1 END) c, count(*) n "
              "FROM lineitem JOIN orders ON l_orderkey = o_orderkey GROUP BY l_quantity")
    gj = _native(s, j, "fused", ["li_ok", "od_ok"])
    assert gj.num_rows == 51 and jit.LAST_MJ_PATH[0] == "hash"


def test_literal_only_resubmission_compiles_nothing(tpch):
    s, _, _ = tpch
    from hyperspace_amd.exec import jit
    text = ("SELECT sum(CASE WHEN l_discount >= {d} THEN l_extendedprice * l_discount ELSE {e} END) r, "
            "count(CASE WHEN l_linenumber < {k} THEN 1 END) c FROM lineitem "
            "WHERE l_orderkey >= 1000 AND l_orderkey < {y}")      # a range of the index key
    _native(s, s.sql(text.format(d=0.05, e=0.0, k=3, y=30000)), "fused", ["li_ok"])
    _native(s, s.sql(text.format(d=0.05, e=0.0, k=3, y=30000)), "fused")
    size = len(jit._KERNELS)
    be = s.backend()

    def replays():
        return sum(g.replays for g in be.graphs._lru.values())
    assert len(be.graphs) >= 1, "the guarded scan over a key range is graph-eligible"
    before = replays()
    for d, e, k, y in ((0.02, 1.5, 5, 41000), (0.07, 0.0, 2, 20000)):
        _native(s, s.sql(text.format(d=d, e=e, k=k, y=y)), "fused")
    assert len(jit._KERNELS) == size
    assert replays() > before


def test_hybrid_scan_with_appended_files(tpch, tmp_path):
    s, lpath, _ = tpch
    rng = np.random.default_rng(3)
    n = 500
    extra = pa.table({"l_orderkey": rng.integers(1, 40_000, n).astype(np.int64),
                      "l_quantity": pa.array(rng.integers(1, 51, n).astype(np.float64)),
                      "l_extendedprice": np.round(rng.random(n) * 1e5, 2),
                      "l_discount": rng.integers(0, 11, n) / 100.0,
                      "l_shipdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32)).view(pa.date32()),
                      "l_shipmode": pa.array(np.array(["MAIL", "TRUCK"])[rng.integers(0, 2, n)]),
                      "l_type": pa.array(np.array(["PROMO NEW", "SMALL TIN"])[rng.integers(0, 2, n)]),
                      "l_linenumber": rng.integers(1, 8, n).astype(np.int32)})
    pq.write_table(extra, os.path.join(lpath, "part-appended.parquet"))
    s.conf.set("spark.hyperspace.index.hybridscan.enabled", "true")
    s.read.parquet(lpath).createOrReplaceTempView("lineitem")
    q = s.sql("SELECT sum(CASE WHEN l_shipmode = 'TRUCK' THEN l_extendedprice ELSE 0 END) t, "
              "count(CASE WHEN l_type LIKE 'PROMO%' THEN 1 END) p, count(*) n "
              "FROM lineitem WHERE l_orderkey < 30000")
    g = _native(s, q, "fused", index=["li_ok"])
    assert g.column("t")[0].as_py() > 0


def test_bucket_range_streamed_guarded_aggregate(tpch):
    s, _, _ = tpch
    s.conf.set("spark.hyperspace.mi.deviceCacheBytes", str(64 << 10))
    try:
        g = _native(s, s.sql(Q6), "fused", ["li_ship"])
        assert s.backend().last_stream_passes > 1
    finally:
        s.conf.unset("spark.hyperspace.mi.deviceCacheBytes")
    assert g.num_rows == 1
