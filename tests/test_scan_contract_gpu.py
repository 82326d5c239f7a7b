"""The scan predicate / aggregate contract (csrc/kernels/hs_scan.h) on every device path against
the numpy reference in tests/scan_ref.py.

``run_all`` drives one query through the interpreter kernels (``K.scan_agg`` at several grids,
``K.scan_select``, ``K.scan_bitmap``) and the generated kernels (``jit.scan_agg`` strided and
vectorised, each over full-width and over compact columns); every result is compared with the
reference, never with another device path.

Comparison: counts, MIN, MAX, row ids and bitmap words exactly; a sum against the reference's
``math.fsum`` within ``(n_pass + 4 * nterms + 2) * 2**-52 * sum(|product|)`` - the bound of any
summation order plus the roundings of a product and the 1-ulp reciprocal decode of compact
decimals.

One table of N rows (four and a bit interpreter tiles) is built per module.  The row ranges
start off every alignment, have lengths 0, 1, 2, 2047, 2048, 2049, two of them are adjacent
and the last one ends at the table's last row.  Rows outside every range ("poison") are valid,
carry an aggregate input ~100x any in-range one and, in the geometry column, a passing value:
a read outside a range shows in count and sum.

The generated kernels compile once per shape (column types, kinds and ops; literals are
arguments), about half a second each.  A literal-leaf case therefore runs the interpreter paths
on every column type x validity, and the generated paths on one or two of them, rotating with the
op: types and ops are independent textual substitutions in the generator (``(i64)x OP lit``),
and over the ops of a kind every type x validity is generated at least once.
"""
import numpy as np
import pytest

import scan_ref as R
from hyperspace_amd.ops import _lib as NL

pytestmark = pytest.mark.gpu

N = 9211
TILE = 2048
RANGES = [(37, 2049), (2086, 1), (2500, 0), (2600, 2047), (4711, 2048), (6800, 2),
          (7003, N - 7003)]
GRIDS = (1, 3, None)
OPS = [R.OP_EQ, R.OP_NE, R.OP_LT, R.OP_LE, R.OP_GT, R.OP_GE]
OPNAME = {R.OP_EQ: "EQ", R.OP_NE: "NE", R.OP_LT: "LT", R.OP_LE: "LE", R.OP_GT: "GT", R.OP_GE: "GE"}
STRETCH = (2600 + 1024, 512)     # rows of one group key, 64-aligned within every path's tile
NAN, INF = float("nan"), float("inf")
COUNT_SUM = [(R.AK_COUNT_STAR, []), (R.AK_SUM, [(14, 0.0, 1.0)])]     # slot 14 = x


def _in_range():
    m = np.zeros(N, bool)
    for s, ln in RANGES:
        m[s:s + ln] = True
    return m


class Table:
    """Host columns (name -> (values, valid, hs_type)) and their device copies.  ``name?`` and
    ``name?2`` are the column ``name`` under the validity masks V and V2."""

    def __init__(self, device):
        import torch
        self.device = device
        rng = np.random.default_rng(20)
        inr = _in_range()

        def ints(lo, hi, dt):
            return rng.integers(lo, hi + 1, N).astype(dt)

        c = {}
        c["i8"] = ints(-100, 100, np.int8)
        c["i16"] = ints(-3000, 3000, np.int16)
        c["i16"][200:203] = (-1000, -809, -808)      # around the last bit of test_leaf_bitmap
        c["i32"] = ints(-30000, 30000, np.int32)                 # compact: 2 bytes
        c["i64"] = 10 ** 12 + ints(0, 3_000_000_000, np.int64)   # compact: 4 bytes
        c["c1"] = ints(1000, 1200, np.int32)                     # compact: 1 byte
        c["u32"] = (2 ** 31 + ints(-1000, 1000, np.int64)).astype(np.uint32)
        c["b"] = ints(0, 1, np.uint8)
        c["i64s"] = (c["i16"].astype(np.int64) + ints(-1, 1, np.int64))
        f = np.round(rng.normal(size=N) * 100, 1)
        sp = rng.random(N)
        for k, v in enumerate((-0.0, 0.0, INF, -INF, NAN)):
            f[(sp >= 0.01 * k) & (sp < 0.01 * (k + 1))] = v
        c["f64"] = f
        c["f32"] = f.astype(np.float32)
        c["f64b"] = np.where(rng.random(N) < 0.5, c["f32"].astype(np.float64), f)
        c["f64i"] = c["i32"].astype(np.float64) + rng.choice([0.0, 0.5, -0.5], N)
        # exact decimals of k digits (compact scale 10^k) and doubles that are none
        c["d0"] = ints(-500, 500, np.int64).astype(np.float64)
        c["d1"] = ints(-1200, 1200, np.int64) / 10.0
        c["d2"] = ints(0, 10, np.int64) / 100.0
        c["d3"] = ints(0, 10 ** 6, np.int64) / 1000.0
        c["d4"] = ints(-30000, 30000, np.int64) / 10000.0
        c["fr"] = rng.random(N)
        # aggregate inputs: x * (1 - y) * (1 + z)
        x = np.round(rng.random(N) * 1e5, 2)
        x[~inr] = 9e6 + 0.25
        c["x"] = x
        c["y"] = np.where(inr, ints(0, 10, np.int64) / 100.0, 0.0)
        c["z"] = np.where(inr, ints(0, 8, np.int64) / 100.0, 0.0)
        c["i64n"] = ints(-5_000_000, 5_000_000, np.int64)
        c["f32m"] = rng.normal(size=N).astype(np.float32)
        # group keys: 17 never occurs; one key over the whole STRETCH
        gk = ints(-3, 40, np.int64)
        gk[gk == 17] = 18
        gk[STRETCH[0]:STRETCH[0] + STRETCH[1]] = 5
        gk[100] = gk[101] = 5
        c["g8"], c["g64"] = gk.astype(np.int8), gk
        g300 = ints(-5, 310, np.int32)
        g300[STRETCH[0]:STRETCH[0] + STRETCH[1]] = 5
        c["g32"] = g300
        # MIN / MAX inputs with NaN: scattered; the whole STRETCH (group 5) after that group's
        # extremes at rows 100 / 101; every row of group 9
        mm = rng.normal(size=N) * 50
        c["mm"] = mm
        c["mmn"] = np.where(rng.random(N) < 0.05, NAN, mm)
        mms = mm.copy()
        mms[STRETCH[0]:STRETCH[0] + STRETCH[1]] = NAN
        mms[100], mms[101] = -1e6, 1e6
        c["mms"] = mms
        c["mma"] = np.where(gk == 9, NAN, c["mmn"])
        # geometry: in-range rows pass (500) or fail (50), poison rows pass
        gd = np.where(rng.random(N) < 0.5, 500, 50).astype(np.int32)
        gd[~inr] = 1000
        gd[2085], gd[2086], gd[6800:6802], gd[N - 1] = 500, 50, 500, 500
        c["gd"] = gd
        c["rid"] = np.arange(N, dtype=np.int32)
        c["key"] = 10 ** 9 + 3 * np.arange(N, dtype=np.int64)     # unique, ascending (join side)
        self.V = (rng.random(N) >= 0.1).astype(np.uint8)
        self.V2 = (rng.random(N) >= 0.1).astype(np.uint8)
        self.V[~inr] = 1
        self.V2[~inr] = 1
        self.V[100:102] = 1
        self._np = c
        hs = {v: k for k, v in R.NP_TYPE.items()}
        self._type = {n: hs[a.dtype.type] for n, a in c.items()}
        self._dev = {n: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
                     for n, a in c.items()}
        self._vdev = {"?": torch.from_numpy(self.V).to(device),
                      "?2": torch.from_numpy(self.V2).to(device)}
        self._compact = {}
        self._keep = []

    @staticmethod
    def _split(name):
        for suf in ("?2", "?"):
            if name.endswith(suf):
                return name[:-len(suf)], suf
        return name, ""

    def col(self, name):
        b, suf = self._split(name)
        return (self._np[b], {"": None, "?": self.V, "?2": self.V2}[suf], self._type[b])

    def valid_values(self, name):
        v, m, _ = self.col(name)
        return v if m is None else v[m.astype(bool)]

    def desc(self, name):
        b, suf = self._split(name)
        return NL.ColDesc(self._dev[b].data_ptr(), self._vdev[suf].data_ptr() if suf else 0,
                          self._type[b], 0)

    def compact(self, name):
        if name not in self._compact:
            import pyarrow as pa
            from hyperspace_amd.exec.device_table import DeviceColumn
            from hyperspace_amd.exec.encoding import encode
            b, suf = self._split(name)
            e = None
            if self._np[b].dtype != np.uint32:
                e = encode(DeviceColumn(self._dev[b], self._vdev[suf] if suf else None,
                                        pa.from_numpy_dtype(self._np[b].dtype)))
            self._compact[name] = e
        return self._compact[name]

    def dev_i64(self, values):
        import torch
        t = torch.from_numpy(np.asarray(values).astype(np.int64)).to(self.device)
        self._keep.append(t)
        return t

    def params(self, cols, preds, aggs, group, cls=NL.ScanParams):
        p = cls()
        for s, n in cols.items():
            p.cols[s] = self.desc(n)
        for i, (kind, op, c, c2, grp, ilit, flit, pset) in enumerate(preds):
            sp, sl = None, 0
            if pset is not None:
                sp, sl = self.dev_i64(pset).data_ptr(), len(pset)
            p.preds[i] = NL.Pred(kind, op, c, c2, grp, sl, int(ilit), float(flit), sp)
        p.npreds = len(preds)
        for i, (kind, terms) in enumerate(aggs):
            a = NL.AggSpec()
            a.kind, a.nterms = kind, len(terms)
            for t, (c, al, be) in enumerate(terms):
                a.col[t], a.alpha[t], a.beta[t] = c, al, be
            p.aggs[i] = a
        p.naggs = len(aggs)
        p.group_col, p.num_groups, p.group_base = group
        return p

    def ranges(self, ranges):
        import torch
        rs = torch.tensor([s for s, _ in ranges], dtype=torch.int64, device=self.device)
        rl = torch.tensor([ln for _, ln in ranges], dtype=torch.int64, device=self.device)
        return rs, rl


_TABLE = []


@pytest.fixture
def T(device):
    """The module's one table (built on first use; ``device`` is a per-test fixture)."""
    if not _TABLE:
        _TABLE.append(Table(device))
    return _TABLE[0]


def _host(out):
    return tuple(t.cpu().numpy().copy() for t in out)


def run_all(T, cols, preds, aggs, group=(-1, 1, 0), ranges=RANGES, grids=GRIDS, gen=True,
            full_width=True, compact_slots=None):
    """Every device path that accepts the query, keyed by path name.  ``gen``: include the
    generated kernels; ``full_width``: include their full-width forms beside the compact ones;
    ``compact_slots``: the slots read in compact form (default: every slot that has one)."""
    from hyperspace_amd.exec import jit, kernel_config
    from hyperspace_amd.ops import kernels as K
    p = T.params(cols, preds, aggs, group)
    rstart, rlen = T.ranges(ranges)
    tp = K.ranges_to_tiles(rlen)
    out = {}
    for g in grids:
        out[f"aot grid={g}"] = _host(K.scan_agg(p, rstart, rlen, tp, grid=g))
    ntiles = sum(-(-ln // TILE) for _, ln in ranges)
    out["select"] = K.scan_select(p, rstart, rlen, tp, max_tiles=ntiles + 1).cpu().numpy()
    pb = T.params({**cols, 15: "rid"}, preds, aggs, group)
    out["bitmap"] = K.scan_bitmap(pb, rstart, rlen, tp, 15, 0, N).cpu().numpy()
    if not gen:
        return out
    comp = {s: T.compact(n) for s, n in cols.items()
            if compact_slots is None or s in compact_slots}
    comp = {s: e for s, e in comp.items() if e is not None}
    forms = [("jit compact", comp, 0), ("jit compact vec", comp, N)] if comp else []
    if full_width or not comp:
        forms += [("jit", None, 0), ("jit vec", None, N)]
    for name, cm, nrows in forms:
        if nrows:
            assert jit.scan_vec(p, cm, nrows) != 0, "the vectorised form must be the one that runs"
        for g in grids:
            over = {"scan_grid": g} if g else {}
            with kernel_config.use(**over):
                out[f"{name} grid={g}"] = _host(jit.scan_agg(p, rstart, rlen, None, cm, nrows))
    return out


def _words(rows):
    bits = np.zeros((N + 63) // 64 * 64, np.uint8)
    bits[rows] = 1
    return np.packbits(bits, bitorder="little").view(np.int64)


def compare(ref, got, aggs, G, tag):
    s, c, mn, mx = (x.reshape(G, len(aggs)) for x in got)
    for a, (kind, terms) in enumerate(aggs):
        assert np.array_equal(c[:, a], ref.count[:, a]), (tag, "count", a, c[:, a], ref.count[:, a])
        if kind == R.AK_SUM:
            bound = (ref.count[:, a] + 4 * len(terms) + 2) * 2.0 ** -52 * ref.abs_sum[:, a]
            err = np.abs(s[:, a] - ref.sum[:, a])
            assert (err <= bound).all(), (tag, "sum", a, err.max(), s[:, a], ref.sum[:, a])
        elif kind == R.AK_MIN:
            assert np.array_equal(mn[:, a], ref.mn[:, a]), (tag, "min", a, mn[:, a], ref.mn[:, a])
        elif kind == R.AK_MAX:
            assert np.array_equal(mx[:, a], ref.mx[:, a]), (tag, "max", a, mx[:, a], ref.mx[:, a])


def check(T, cols, preds, aggs=COUNT_SUM, group=(-1, 1, 0), ranges=RANGES, tag=None, **kw):
    cols = dict(cols)
    if any(c == 14 for _, terms in aggs for c, _, _ in terms):
        cols.setdefault(14, "x")
    ref = R.scan({s: T.col(n) for s, n in cols.items()}, preds, aggs, *group, ranges=ranges)
    got = run_all(T, cols, preds, aggs, group, ranges, **kw)
    G = group[1] if group[0] >= 0 else 1
    for path, r in got.items():
        if path == "select":
            assert np.array_equal(r, ref.rows), (tag, path, len(r), len(ref.rows))
        elif path == "bitmap":
            assert np.array_equal(r, _words(ref.rows)), (tag, path)
        else:
            compare(ref, r, aggs, G, (tag, path))
    return ref, got


def _p(kind, op=0, col=0, col2=0, group=0, ilit=0, flit=0.0, pset=None):
    return (kind, op, col, col2, group, ilit, flit, pset)


# ------------------------------------------------------------------------------------------------
# Tile and range geometry
# ------------------------------------------------------------------------------------------------
def test_geometry_ranges_tiles_and_poison(T):
    preds = [_p(R.PK_INT_LIT, R.OP_GE, 0, ilit=100)]
    aggs = [(R.AK_COUNT_STAR, []), (R.AK_SUM, [(14, 0.0, 1.0)]), (R.AK_MAX, [(14, 0.0, 1.0)])]
    ref, _ = check(T, {0: "gd"}, preds, aggs, tag="geometry")
    # the reference sees passing rows in every tile but the one-row range's, which has none
    passing = set(ref.rows.tolist())
    tiles = [[r for r in range(s + o, min(s + ln, s + o + TILE)) if r in passing]
             for s, ln in RANGES for o in range(0, ln, TILE)]
    assert len(tiles) == 8
    assert [bool(t) for t in tiles] == [True, True, False, True, True, True, True, True]
    # a poison row passes the predicate and would dominate the sum and the maximum
    gd, x = T.col("gd")[0], T.col("x")[0]
    inr = _in_range()
    assert (gd[~inr] >= 100).all() and x[~inr].min() > 50 * x[inr].max()
    assert ref.mx[0, 2] < 1e6 and ref.rows[-1] == N - 1


@pytest.mark.parametrize("ranges", [[(37, 2049)], [(2086, 1)], [(2500, 0)], [(2600, 2047)],
                                    [(4711, 2048)], [(6800, 2)], [(2500, 0), (6800, 2), (2600, 0)]],
                         ids=lambda r: "+".join(f"{s}x{ln}" for s, ln in r))
def test_geometry_single_ranges(T, ranges):
    check(T, {0: "gd"}, [_p(R.PK_INT_LIT, R.OP_GE, 0, ilit=100)], ranges=ranges, tag=ranges)


def test_bitmap_window(T):
    """``scan_bitmap`` with a non-zero base and fewer bits than keys: keys outside set nothing."""
    from hyperspace_amd.ops import kernels as K
    cols = {0: "gd", 15: "rid"}
    preds = [_p(R.PK_INT_LIT, R.OP_GE, 0, ilit=100)]
    p = T.params(cols, preds, [], (-1, 1, 0))
    rstart, rlen = T.ranges(RANGES)
    lo, nbits = 2000, 3001
    w = K.scan_bitmap(p, rstart, rlen, K.ranges_to_tiles(rlen), 15, lo, nbits).cpu().numpy()
    rows = R.scan({s: T.col(n) for s, n in cols.items()}, preds, [], ranges=RANGES).rows
    rows = rows[(rows >= lo) & (rows < lo + nbits)] - lo
    assert len(rows) > 100 and np.array_equal(w, _words(rows)[:len(w)])


# ------------------------------------------------------------------------------------------------
# Leaves: one case per (kind, op)
# ------------------------------------------------------------------------------------------------
def _rot(combos, op, k=2):
    """The k of ``combos`` whose generated kernels this op's case compiles (see module doc)."""
    return {combos[(k * op + j) % len(combos)] for j in range(k)}


@pytest.mark.parametrize("op", OPS, ids=OPNAME.get)
def test_leaf_int_lit(T, op):
    combos = [n + m for n in ("i8", "i16", "i32", "i64", "u32", "b") for m in ("", "?")]
    gen = _rot(combos, op)
    for name in combos:
        v = T.valid_values(name).astype(np.int64)
        for lit in (v.min(), v.max(), v.min() - 1, v.max() + 1, int(np.median(v)), 2 ** 62,
                    -2 ** 62):
            check(T, {0: name}, [_p(R.PK_INT_LIT, op, 0, ilit=int(lit))], tag=(name, int(lit)),
                  gen=name in gen, compact_slots=(0, 1))


@pytest.mark.parametrize("op", OPS, ids=OPNAME.get)
def test_leaf_flt_lit(T, op):
    combos = [n + m for n in ("f32", "f64", "i32") for m in ("", "?")]
    gen = {combos[op]}
    for name in combos:
        v = T.valid_values(name).astype(np.float64)
        v = v[np.isfinite(v)]
        lits = [v.min(), v.max(), np.nextafter(v.min(), -INF), np.nextafter(v.max(), INF),
                float(np.median(v)), 0.0, -0.0, INF, -INF, NAN, 2.0 ** 62, -2.0 ** 62]
        for lit in lits:
            check(T, {0: name}, [_p(R.PK_FLT_LIT, op, 0, flit=float(lit))], tag=(name, lit),
                  gen=name in gen, compact_slots=(0, 1))


@pytest.mark.parametrize("op", OPS, ids=OPNAME.get)
def test_leaf_int_col(T, op):
    """I16 against I64, nulls on neither, the first, the second and both sides."""
    combos = [("i16", "i64s"), ("i16?", "i64s"), ("i16", "i64s?2"), ("i16?", "i64s?2"),
              ("i64s?", "i16?2"), ("i64s", "i16")]
    gen = {combos[op]}
    for a, b in combos:
        check(T, {0: a, 1: b}, [_p(R.PK_INT_COL, op, 0, 1)], tag=(a, b), gen=(a, b) in gen,
              compact_slots=(0, 1))


@pytest.mark.parametrize("op", OPS, ids=OPNAME.get)
def test_leaf_flt_col(T, op):
    """F32 against F64 and I32 against F64 (with -0.0, +-inf and NaN on the float sides)."""
    combos = [(a + m, b + m2) for a, b in (("f32", "f64b"), ("i32", "f64i"), ("f64", "f32"))
              for m, m2 in (("", ""), ("?", ""), ("", "?2"), ("?", "?2"))]
    gen = _rot(combos, op)
    for a, b in combos:
        check(T, {0: a, 1: b}, [_p(R.PK_FLT_COL, op, 0, 1)], tag=(a, b), gen=(a, b) in gen,
              compact_slots=(0, 1))


@pytest.mark.parametrize("kind", [R.PK_IS_NULL, R.PK_NOT_NULL], ids=["IS_NULL", "NOT_NULL"])
def test_leaf_null_tests(T, kind):
    for name in ("i32", "i32?", "f64?2", "b"):
        check(T, {0: name}, [_p(kind, col=0)], tag=name, compact_slots=(0,))


@pytest.mark.parametrize("op", [R.OP_EQ, R.OP_NE], ids=OPNAME.get)
def test_leaf_in_set(T, op):
    """Sets of 1, 2 and 7 members taken from the column: the data holds both ends of each set,
    values between members, below the first and above the last."""
    u = np.unique(T.col("i32")[0]).astype(np.int64)
    for name in ("i32", "i32?"):
        for k in (1, 2, 7):
            members = u[np.linspace(len(u) // 4, 3 * len(u) // 4, k).astype(int)]
            assert u[0] < members[0] and members[-1] < u[-1]
            check(T, {0: name}, [_p(R.PK_IN_SET, op, 0, pset=sorted(members.tolist()))],
                  tag=(name, k))


@pytest.mark.parametrize("op", [R.OP_EQ, R.OP_NE], ids=OPNAME.get)
def test_leaf_bitmap(T, op):
    """A three-word bitmap (no power of two) at base -1000 over a column in [-3000, 3000]:
    values below the base and at or past base + 192 find nothing."""
    rng = np.random.default_rng(6)
    words = rng.integers(-2 ** 63, 2 ** 63 - 1, 3)
    words[2] |= -2 ** 63                # bit 191, the last one
    v = T.col("i16")[0]
    assert (v < -1000).any() and (v >= -1000 + 192).any() and (v == -1000 + 191).any()
    for name in ("i16", "i16?"):
        ref, _ = check(T, {0: name}, [_p(R.PK_BITMAP, op, 0, ilit=-1000, pset=words.tolist())],
                       tag=name)
        assert len(ref.rows) > 0
    # a one-word bitmap whose base sits above every value, and one far below
    for base in (5000, -2 ** 40):
        check(T, {0: "i16?"}, [_p(R.PK_BITMAP, op, 0, ilit=base, pset=[-1])], tag=base)


def test_leaf_true(T):
    ref, _ = check(T, {}, [_p(R.PK_TRUE)], tag="true")
    assert len(ref.rows) == sum(ln for _, ln in RANGES)


# ------------------------------------------------------------------------------------------------
# CNF
# ------------------------------------------------------------------------------------------------
def test_cnf_unknown_or_true(T):
    """(f64? < 0 OR i8 >= -100): the first leaf is unknown on null rows, the second always true."""
    preds = [_p(R.PK_FLT_LIT, R.OP_LT, 0, group=0, flit=0.0),
             _p(R.PK_INT_LIT, R.OP_GE, 1, group=0, ilit=-100)]
    ref, _ = check(T, {0: "f64?", 1: "i8"}, preds, tag="unknown-or-true")
    assert len(ref.rows) == sum(ln for _, ln in RANGES)
    # and the other way round with AND: the unknown leaf decides
    preds = [_p(R.PK_FLT_LIT, R.OP_NE, 0, group=0, flit=0.0),
             _p(R.PK_INT_LIT, R.OP_GE, 1, group=1, ilit=-100)]
    check(T, {0: "f64?", 1: "i8"}, preds, tag="ne-and-true")


def test_cnf_ne_against_null_rows(T):
    v = T.col("i32?")
    lit = int(v[0][(v[1] == 0) & _in_range()][0])     # the stored value of a null row
    ref, _ = check(T, {0: "i32?"}, [_p(R.PK_INT_LIT, R.OP_NE, 0, ilit=lit)], tag="ne-null")
    assert not (set(ref.rows.tolist()) & set(np.nonzero(v[1] == 0)[0].tolist()))


def test_cnf_group_false_for_every_row(T):
    preds = [_p(R.PK_INT_LIT, R.OP_GE, 0, group=0, ilit=100),
             _p(R.PK_INT_LIT, R.OP_GT, 1, group=1, ilit=30000),
             _p(R.PK_IS_NULL, col=0, group=1),
             _p(R.PK_TRUE, group=2)]
    aggs = COUNT_SUM + [(R.AK_MIN, [(14, 0.0, 1.0)]), (R.AK_MAX, [(14, 0.0, 1.0)])]
    ref, _ = check(T, {0: "gd", 1: "i32"}, preds, aggs, tag="false-group")
    assert len(ref.rows) == 0


def test_cnf_sixteen_leaves_in_five_groups(T):
    cols = {0: "i8", 1: "i16?", 2: "i32", 3: "f64?2", 4: "f32", 5: "b", 6: "u32?", 7: "i64s"}
    u = np.unique(T.col("i32")[0]).astype(np.int64)
    preds = [_p(R.PK_INT_LIT, R.OP_GT, 0, group=0, ilit=-60),
             _p(R.PK_INT_LIT, R.OP_LT, 1, group=0, ilit=-2000),
             _p(R.PK_IS_NULL, col=1, group=0),
             _p(R.PK_FLT_LIT, R.OP_LE, 3, group=1, flit=50.0),
             _p(R.PK_FLT_LIT, R.OP_GE, 4, group=1, flit=120.0),
             _p(R.PK_INT_COL, R.OP_EQ, 1, 7, group=1),
             _p(R.PK_IN_SET, R.OP_EQ, 2, group=1, pset=u[::3].tolist()),
             _p(R.PK_INT_LIT, R.OP_EQ, 5, group=2, ilit=1),
             _p(R.PK_INT_LIT, R.OP_GE, 6, group=2, ilit=2 ** 31),
             _p(R.PK_NOT_NULL, col=3, group=2),
             _p(R.PK_FLT_COL, R.OP_NE, 3, 4, group=3),
             _p(R.PK_INT_LIT, R.OP_NE, 2, group=3, ilit=int(u[5])),
             _p(R.PK_BITMAP, R.OP_NE, 0, group=4, ilit=-100, pset=[0x5555555555555555, 3]),
             _p(R.PK_INT_LIT, R.OP_LE, 7, group=4, ilit=-2500),
             _p(R.PK_FLT_LIT, R.OP_GT, 2, group=4, flit=29000.5),
             _p(R.PK_TRUE, group=4)]
    assert len(preds) == NL.MAX_PREDS
    ref, _ = check(T, cols, preds, tag="16 leaves")
    assert 500 < len(ref.rows) < sum(ln for _, ln in RANGES) - 500
    # without the always-true leaf the last group filters too
    ref, _ = check(T, cols, preds[:-1], tag="15 leaves")
    assert 100 < len(ref.rows)


def test_cnf_zero_predicates(T):
    aggs = COUNT_SUM + [(R.AK_COUNT, [(0, 0.0, 1.0)])]
    ref, _ = check(T, {0: "i32?"}, [], aggs, tag="no predicate")
    assert len(ref.rows) == sum(ln for _, ln in RANGES) > ref.count[0, 2]


# ------------------------------------------------------------------------------------------------
# Aggregates
# ------------------------------------------------------------------------------------------------
PASS_HALF = [_p(R.PK_INT_LIT, R.OP_GE, 0, ilit=100)]        # on gd


@pytest.mark.parametrize("yname", ["y", "y?"])
def test_sums_of_one_two_and_three_terms(T, yname):
    """x, x * (1 - y), x * (1 - y) * (1 + z) and a scaled form; ``y?`` is null in places while
    x and z never are, so only the aggregates that read it lose those rows."""
    aggs = [(R.AK_SUM, [(14, 0.0, 1.0)]),
            (R.AK_SUM, [(14, 0.0, 1.0), (1, 1.0, -1.0)]),
            (R.AK_SUM, [(14, 0.0, 1.0), (1, 1.0, -1.0), (2, 1.0, 1.0)]),
            (R.AK_SUM, [(14, 0.25, -3.0), (2, -0.5, 7.0)]),
            (R.AK_COUNT, [(1, 0.0, 1.0)]), (R.AK_COUNT_STAR, [])]
    ref, _ = check(T, {0: "gd", 1: yname, 2: "z"}, PASS_HALF, aggs, tag=yname)
    assert (ref.count[0, 0] > ref.count[0, 1]) == (yname == "y?")
    assert ref.count[0, 4] == ref.count[0, 1] and ref.count[0, 5] == ref.count[0, 0]


def test_min_max_over_i64_f32_f64_and_nothing_passing(T):
    aggs = [(R.AK_MIN, [(1, 0.0, 1.0)]), (R.AK_MAX, [(1, 0.0, 1.0)]),
            (R.AK_MIN, [(2, 0.0, 1.0)]), (R.AK_MAX, [(2, 0.0, -2.0)]),
            (R.AK_MIN, [(3, 0.0, 0.5)]), (R.AK_MAX, [(3, 0.0, 1.0)])]
    cols = {0: "gd", 1: "i64n", 2: "f32m?", 3: "mm"}
    ref, _ = check(T, cols, PASS_HALF, aggs, tag="minmax")
    assert ref.mn[0, 0] < 0 and ref.count[0, 2] < ref.count[0, 0]
    ref, _ = check(T, cols, [_p(R.PK_INT_LIT, R.OP_GT, 0, ilit=5000)], aggs, tag="minmax empty")
    assert ref.count.sum() == 0 and ref.mn[0, 0] == INF and ref.mx[0, 1] == -INF


def test_eight_aggregates_at_once(T):
    aggs = [(R.AK_SUM, [(14, 0.0, 1.0), (1, 1.0, -1.0), (2, 1.0, 1.0)]), (R.AK_COUNT_STAR, []),
            (R.AK_MIN, [(3, 0.0, 1.0)]), (R.AK_MAX, [(3, 0.0, 1.0)]), (R.AK_COUNT, [(1, 0.0, 1.0)]),
            (R.AK_SUM, [(1, 0.0, 1.0)]), (R.AK_MAX, [(14, 0.0, 1.0)]), (R.AK_MIN, [(4, 0.0, 1.0)])]
    assert len(aggs) == NL.MAX_AGGS
    cols = {0: "gd", 1: "y?", 2: "z", 3: "mm", 4: "i64n"}
    check(T, cols, PASS_HALF, aggs, tag="8 global")
    check(T, {**cols, 5: "g8"}, PASS_HALF, aggs, (5, 37, 0), tag="8 grouped")


GROUP_AGGS = [(R.AK_SUM, [(14, 0.0, 1.0), (1, 1.0, -1.0)]), (R.AK_MIN, [(2, 0.0, 1.0)]),
              (R.AK_MAX, [(2, 0.0, 1.0)]), (R.AK_COUNT_STAR, [])]


@pytest.mark.parametrize("gname,G,base", [
    ("g8", 1, 5), ("g8", 37, 0), ("g8?", 37, 0), ("g64", 37, -2), ("g64?", 37, 3),
    ("g32", 300, 0), ("g32?2", 300, -4), ("g32", 37, 270)],
    ids=lambda v: str(v))
def test_grouped_aggregates(T, gname, G, base):
    """Dense group domains [base, base + G) over I8 / I32 / I64 keys with null keys and keys
    on both sides outside the domain; key 17 receives no row; STRETCH holds one key."""
    cols = {0: "gd", 1: "y", 2: "mm", 3: gname}
    ref, _ = check(T, cols, PASS_HALF, GROUP_AGGS, (3, G, base), tag=(gname, G, base))
    keys = T.valid_values(gname).astype(np.int64)
    assert (keys < base).any() and (keys >= base + G).any()
    assert ref.count[:, 3].sum() < len(ref.rows)
    if gname.startswith(("g8", "g64")) and base <= 17 < base + G:
        assert ref.count[17 - base, 3] == 0 and ref.mn[17 - base, 1] == INF
    # the same with every row passing, so STRETCH is 64 consecutive rows of one slot in a wave
    check(T, cols, [], GROUP_AGGS, (3, G, base), tag=(gname, G, base, "all rows"))


# ------------------------------------------------------------------------------------------------
# NaN in MIN / MAX inputs: skipped, as np.fmin / np.fmax (and exec/window.py) do
# ------------------------------------------------------------------------------------------------
NAN_AGGS = [(R.AK_MIN, [(1, 0.0, 1.0)]), (R.AK_MAX, [(1, 0.0, 1.0)]), (R.AK_COUNT_STAR, [])]


def test_nan_scattered_global_and_grouped(T):
    ref, _ = check(T, {0: "gd", 1: "mmn"}, PASS_HALF, NAN_AGGS, tag="nan global")
    assert np.isfinite(ref.mn[0, 0]) and np.isnan(T.col("mmn")[0][ref.rows]).any()
    ref, _ = check(T, {0: "gd", 1: "mmn", 2: "g8"}, PASS_HALF, NAN_AGGS, (2, 37, 0),
                   tag="nan grouped")
    assert np.isfinite(ref.mn[np.arange(37) != 17, 0]).all()


def test_nan_stretch_of_one_group_keeps_its_extremes(T):
    """Group 5: its minimum and maximum (rows 100 / 101), then 512 consecutive NaN rows of that
    group alone (every lane of whole waves), then ordinary values.  The NaN must not displace
    the extremes already accumulated."""
    s0, sl = STRETCH
    g, v = T.col("g8")[0], T.col("mms")[0]
    assert (s0 - 2600) % 1024 == 0 and (g[s0:s0 + sl] == 5).all()
    assert np.isnan(v[s0:s0 + sl]).all() and ((g[s0 + sl:] == 5) & _in_range()[s0 + sl:]).sum() > 20
    for grids in ((1,), GRIDS):
        ref, _ = check(T, {1: "mms", 2: "g8"}, [], NAN_AGGS, (2, 37, 0), tag="nan stretch",
                       grids=grids)
        assert ref.mn[5, 0] == -1e6 and ref.mx[5, 1] == 1e6
    check(T, {1: "mms"}, [], NAN_AGGS, tag="nan stretch global")


def test_nan_only_group_agrees_on_every_path(T):
    """Group 9 holds NaN only.  The contract fixes no answer for it, so this is the one check
    that compares device paths with each other: they must all give the same.
    Every device path answers (+inf, -inf) for (MIN, MAX) with the group's row count - the
    identities, as np.fmin / np.fmax with an initial value do; the CPU session's answer for the
    same query (pyarrow min / max over a float column holding only NaN) is NaN."""
    cols = {1: "mma", 2: "g8"}
    ref = R.scan({s: T.col(n) for s, n in cols.items()}, [], NAN_AGGS, 2, 37, 0, ranges=RANGES)
    assert ref.count[9, 2] > 20
    got = run_all(T, cols, [], NAN_AGGS, (2, 37, 0))
    keep = np.arange(37) != 9
    answers = set()
    for path, r in got.items():
        if path in ("select", "bitmap"):
            continue
        s, c, mn, mx = (x.reshape(37, 3) for x in r)
        assert np.array_equal(c, ref.count), path
        assert np.array_equal(mn[keep, 0], ref.mn[keep, 0]), path
        assert np.array_equal(mx[keep, 1], ref.mx[keep, 1]), path
        answers.add((repr(float(mn[9, 0])), repr(float(mx[9, 1]))))
    print("all-NaN group (MIN, MAX) on every path:", answers)
    assert len(answers) == 1, answers


# ------------------------------------------------------------------------------------------------
# Compact columns
# ------------------------------------------------------------------------------------------------
COMPACT_FORMS = {"c1": (1, None), "i32": (2, None), "i64": (4, None), "i32?": (2, None),
                 "d0": (2, 1.0), "d1": (2, 10.0), "d2": (1, 100.0), "d3": (4, 1000.0),
                 "d4": (2, 10000.0), "x?": (4, 100.0), "x": (4, 100.0)}


def test_compact_forms_are_the_expected_ones(T):
    for name, (width, scale) in COMPACT_FORMS.items():
        e = T.compact(name)
        assert e is not None and (e.width, e.scale) == (width, scale), name
    for name in ("fr", "f64", "i16", "i8", "mmn"):       # not exact decimals / not narrower
        assert T.compact(name) is None, name


@pytest.mark.parametrize("op", OPS, ids=OPNAME.get)
def test_compact_flt_lit_on_decimal_columns(T, op):
    """Literal compares on decimal-scaled codes with host-computed integer bounds
    (``int_bounds`` / ``code_bounds``) against the double compare of the decoded value."""
    names = ["d0", "d1", "d2", "d3", "d4", "x?"]
    gen = _rot(names, op)
    for name in names:
        scale = COMPACT_FORMS[name][1]
        v = T.valid_values(name)
        q = float(np.median(v))
        lits = [v.min(), v.max(), q, q + 0.5 / scale, np.nextafter(q, INF), np.nextafter(q, -INF),
                0.05, 0.07, -0.0, INF, -INF, NAN, 1e22, 1e300, 1.7976931348623157e308,
                -1.7976931348623157e308]
        for lit in lits:
            check(T, {0: name}, [_p(R.PK_FLT_LIT, op, 0, flit=float(lit))], tag=(name, lit),
                  gen=name in gen, full_width=False)


@pytest.mark.parametrize("op", OPS, ids=OPNAME.get)
def test_compact_int_lit_on_integer_codes(T, op):
    names = ["c1", "i32", "i64", "i32?"]
    gen = _rot(names, op)
    for name in names:
        e = T.compact(name)
        lits = [e.lo, e.hi, e.lo - 1, e.hi + 1, (e.lo + e.hi) // 2, e.base - 2 ** 31,
                e.base + 2 ** 31, e.base + 2 ** 31 - 1, e.base - 2 ** 31 - 1]
        for lit in lits:
            check(T, {0: name}, [_p(R.PK_INT_LIT, op, 0, ilit=int(lit))], tag=(name, lit),
                  gen=name in gen, full_width=False)


def test_compact_sum_inputs_decode_with_a_reciprocal(T):
    """x, y, z compact (4 / 1 / 1 bytes): SUM-only slots decode approximately, the MIN / MAX
    and predicate slots exactly; y? is a nullable decimal."""
    aggs = [(R.AK_SUM, [(14, 0.0, 1.0), (1, 1.0, -1.0), (2, 1.0, 1.0)]), (R.AK_COUNT_STAR, []),
            (R.AK_MIN, [(3, 0.0, 1.0)]), (R.AK_MAX, [(3, 0.0, 1.0)]), (R.AK_SUM, [(4, 0.0, 1.0)])]
    cols = {0: "d2", 1: "y?", 2: "z", 3: "d3", 4: "d4"}
    preds = [_p(R.PK_FLT_LIT, R.OP_GE, 0, group=0, flit=0.05),
             _p(R.PK_FLT_LIT, R.OP_LE, 0, group=1, flit=0.07)]
    for s, n in list(cols.items()) + [(14, "x")]:
        assert T.compact(n) is not None, n
    check(T, cols, preds, aggs, tag="compact sums")
    check(T, {**cols, 5: "g8"}, preds, aggs, (5, 37, 0), tag="compact sums grouped")


# ------------------------------------------------------------------------------------------------
# The join side, reduced: the table joined with itself 1:1 on a unique key, so the reference is
# the scan reference over the row pairing (left row i, right row i).  Slots >= 8 are the right row.
# ------------------------------------------------------------------------------------------------
JOIN_OFF = [0, 2303, 4606, 6909, N]                              # 4 buckets, rows in key order
JOIN_RANGES = [(JOIN_OFF[b] + 3, JOIN_OFF[b + 1] - JOIN_OFF[b] - 8) for b in range(4)]
JOIN_AGGS = [(R.AK_COUNT_STAR, []), (R.AK_SUM, [(2, 0.0, 1.0), (10, 1.0, -1.0)]),
             (R.AK_COUNT, [(10, 0.0, 1.0)])]
JOIN_COLS = {0: "key", 1: "gd", 2: "x", 8: "key", 10: "y?2"}
LEFT_PRED = _p(R.PK_INT_LIT, R.OP_GE, 1, group=0, ilit=100)


def run_join(T, cols, preds, nlp, aggs, group=(-1, 1, 0)):
    """K.join_agg, jit.join_agg and jit.merge_join_agg, the generated ones over full-width and
    over compact columns, keyed by path name."""
    import torch
    from hyperspace_amd.exec import jit
    from hyperspace_amd.ops import kernels as K
    p = T.params(cols, preds, aggs, group, NL.JoinParams)
    p.nlp, p.lkey, p.rkey, p.key_is_float = nlp, 0, 8, 0
    rstart, rlen = T.ranges(JOIN_RANGES)
    rbk = torch.arange(4, dtype=torch.int32, device=T.device)
    roff = torch.tensor(JOIN_OFF, dtype=torch.int64, device=T.device)
    mt = K.join_max_tiles(N, 4)
    out = {"aot join": _host(K.join_agg(p, rstart, rlen, rbk, roff, mt))}
    comp = {s: T.compact(n) for s, n in cols.items()}
    comp = {s: e for s, e in comp.items() if e is not None}
    assert 0 in comp and 8 in comp and 10 in comp
    for tag, cm in (("", None), (" compact", comp)):
        out["jit join" + tag] = _host(jit.join_agg(p, rstart, rlen, rbk, roff, mt, cm))
        assert jit.merge_join_ok(p, cm, N, N)
        out["jit merge join" + tag] = _host(jit.merge_join_agg(p, rstart, rlen, rbk, roff, cm,
                                                               nrows=N))
    return out


def check_join(T, cols, preds, nlp, aggs=JOIN_AGGS, group=(-1, 1, 0), tag=None):
    ref = R.scan({s: T.col(n) for s, n in cols.items()}, preds, aggs, *group, ranges=JOIN_RANGES)
    G = group[1] if group[0] >= 0 else 1
    for path, r in run_join(T, cols, preds, nlp, aggs, group).items():
        compare(ref, r, aggs, G, (tag, path))
    return ref


def _join_cases():
    rng = np.random.default_rng(6)
    words = rng.integers(-2 ** 63, 2 ** 63 - 1, 3).tolist()
    return {
        "INT_LIT": ({9: "i32?"}, _p(R.PK_INT_LIT, R.OP_LT, 9, group=1, ilit=1000)),
        "FLT_LIT": ({9: "f64?"}, _p(R.PK_FLT_LIT, R.OP_GE, 9, group=1, flit=-20.0)),
        "INT_COL": ({9: "i16?", 11: "i64s"}, _p(R.PK_INT_COL, R.OP_LE, 9, 11, group=1)),
        "FLT_COL": ({9: "f32?", 11: "f64b"}, _p(R.PK_FLT_COL, R.OP_NE, 9, 11, group=1)),
        "IS_NULL": ({9: "i32?"}, _p(R.PK_IS_NULL, col=9, group=1)),
        "NOT_NULL": ({9: "f64?"}, _p(R.PK_NOT_NULL, col=9, group=1)),
        "IN_SET": ({9: "i32?"}, _p(R.PK_IN_SET, R.OP_NE, 9, group=1,
                                   pset=list(range(-30000, 30001, 7)))),
        "BITMAP": ({9: "i16?"}, _p(R.PK_BITMAP, R.OP_EQ, 9, group=1, ilit=-1000, pset=words)),
        "TRUE": ({}, _p(R.PK_TRUE, group=1)),
    }


@pytest.mark.parametrize("kind", ["INT_LIT", "FLT_LIT", "INT_COL", "FLT_COL", "IS_NULL", "NOT_NULL",
                                  "IN_SET", "BITMAP", "TRUE"])
def test_join_right_side_leaf(T, kind):
    """Every kind once as a per-match predicate on a nullable right-side slot, beside a left
    predicate; the SUM multiplies a left column with a nullable right one."""
    extra, pred = _join_cases()[kind]
    ref = check_join(T, {**JOIN_COLS, **extra}, [LEFT_PRED, pred], 1, tag=kind)
    assert 0 < ref.count[0, 2] < ref.count[0, 0] < sum(ln for _, ln in JOIN_RANGES)


def test_join_left_against_right_column_and_right_group(T):
    """A ``*_COL`` leaf comparing a left column with a right one (so it belongs to the per-match
    predicates, after ``nlp``), an aggregate term and the group key on the right side."""
    cols = {**JOIN_COLS, 3: "i16?", 9: "i64s", 11: "f64b", 4: "f32?2", 12: "g8?"}
    preds = [LEFT_PRED, _p(R.PK_NOT_NULL, col=3, group=1),
             _p(R.PK_INT_COL, R.OP_GE, 3, 9, group=2),
             _p(R.PK_FLT_COL, R.OP_LT, 11, 4, group=2)]
    aggs = JOIN_AGGS + [(R.AK_MIN, [(11, 0.0, 1.0)]), (R.AK_MAX, [(4, 0.0, 1.0)])]
    ref = check_join(T, cols, preds, 2, aggs, tag="left vs right")
    assert 0 < ref.count[0, 0] < sum(ln for _, ln in JOIN_RANGES) // 2
    ref = check_join(T, cols, preds, 2, aggs, (12, 37, 0), tag="left vs right, grouped")
    assert ref.count[17, 0] == 0 and ref.count[:, 0].sum() > 0
