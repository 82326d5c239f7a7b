"""The window kernels (csrc/kernels/window.hip: hs_win_heads, hs_win_rank, hs_win_frame_ends,
hs_win_agg) against a numpy reference, over row counts around the wavefront, block and tile sizes
and partition layouts that put heads on, before and after tile edges.

The numpy reference is checked on the CPU first (against a plain Python loop).  Ranking functions,
counts, int64 sums, min / max and fp64 sums of integer-valued doubles compare exactly; a general
fp64 running sum is compared with ``numpy.cumsum`` per partition under the analytic bound for two
summation orders, ``|got - ref| <= 2 k 2^-53 sum|x|`` over the k rows of the frame.  Every call
is made twice and the outputs compared bitwise."""
import functools

import numpy as np
import pyarrow as pa
import pytest

gpu = pytest.mark.gpu

T = 2048          # hs_win_tile_rows(); test_tile_rows_is_what_the_layouts_assume checks it
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3)
LAYOUTS = ("one", "own", "m64", "m64pm1", "tile", "tilepm1", "span3", "rand5", "rand700")
PEERS = ("ties", "single", "all")
KINDS = ("sum_i64", "sum_f64", "count", "min_i64", "max_i64", "min_f64", "max_f64")


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def part_heads(n: int, layout: str, seed: int = 0) -> np.ndarray:
    """bool[n]: rows that start a partition (row 0 always)."""
    h = np.zeros(n, dtype=bool)
    if n == 0:
        return h
    rng = np.random.default_rng(seed + n)
    if layout == "own":
        h[:] = True
    elif layout == "m64":
        h[::64] = True
    elif layout == "m64pm1":
        for k in range(64, n + 2, 64):
            for j in (k - 1, k + 1):
                if 0 < j < n:
                    h[j] = True
    elif layout == "tile":
        h[::T] = True
    elif layout == "tilepm1":
        for k in range(T, n + 2, T):
            for j in (k - 1, k + 1):
                if 0 < j < n:
                    h[j] = True
    elif layout == "span3":
        h[min(n, 2 * T + 500):] = True      # one partition over three tiles, then singletons
    elif layout in ("rand5", "rand700"):
        mean = 5 if layout == "rand5" else 700
        pos = np.cumsum(rng.geometric(1.0 / mean, size=n // mean + 2))
        h[pos[pos < n]] = True
    h[0] = True
    return h


def make_case(n: int, layout: str, peers: str) -> dict:
    """Key and value columns of one case.  Partition key: int64 partition number, NULL for
    partition 1.  Order key: int32, position in the partition // 3 ("ties": peer groups of three
    rows, which straddle tile edges as 2048 % 3 != 0), the position ("single") or a constant
    ("all").  Values: ~20 % NULL, all NULL in partition 2."""
    rng = np.random.default_rng(1000 + n)
    ph = part_heads(n, layout)
    pid = np.cumsum(ph) - 1 if n else np.zeros(0, np.int64)
    start = np.maximum.accumulate(np.where(ph, np.arange(n), 0)) if n else np.zeros(0, np.int64)
    pos = np.arange(n) - start
    okey = {"ties": pos // 3, "single": pos, "all": np.zeros(n, np.int64)}[peers].astype(np.int32)
    valid = (rng.random(n) >= 0.2) & (pid != 2)
    ints = rng.integers(-1000, 1000, n).astype(np.int64)
    return {"n": n, "pkey": pid.astype(np.int64), "pvalid": (pid != 1).astype(np.uint8),
            "okey": okey, "valid": valid.astype(np.uint8), "ints": ints,
            "int_doubles": ints.astype(np.float64), "doubles": rng.normal(size=n) * 1e3}


def nan_case(n: int) -> dict:
    """Partitions of mean length 5 whose float values are ~30 % NaN (both signs) and ~20 % NULL;
    every third partition holds NaN and NULL only.  Peer groups of two rows."""
    rng = np.random.default_rng(77 + n)
    ph = part_heads(n, "rand5", seed=3)
    pid = np.cumsum(ph) - 1
    x = rng.normal(size=n) * 10
    x[rng.random(n) < 0.3] = np.nan
    x[rng.random(n) < 0.1] = -np.nan
    x[pid % 3 == 1] = np.nan
    valid = rng.random(n) >= 0.2
    start = np.maximum.accumulate(np.where(ph, np.arange(n), 0))
    okey = ((np.arange(n) - start) // 2).astype(np.int32)
    flags = ref_flags([(pid, None)], [(okey, None)], n)
    return {"x": x, "valid": valid.astype(np.uint8), "flags": flags}


# ------------------------------------------------------------------------------------------------
# the numpy reference
# ------------------------------------------------------------------------------------------------
def ref_differs(v: np.ndarray, valid) -> np.ndarray:
    n = len(v)
    d = np.zeros(n, dtype=bool)
    if n < 2:
        return d
    same = v[1:] == v[:-1]
    if v.dtype.kind == "f":
        same |= np.isnan(v[1:]) & np.isnan(v[:-1])
    if valid is None:
        d[1:] = ~same
    else:
        a, b = valid[:-1].astype(bool), valid[1:].astype(bool)
        d[1:] = ~((a & b & same) | (~a & ~b))
    return d


def ref_flags(part_cols, order_cols, n: int) -> np.ndarray:
    p = np.zeros(n, dtype=bool)
    if n:
        p[0] = True
    for v, valid in part_cols:
        p |= ref_differs(v, valid)
    q = p.copy()
    for v, valid in order_cols:
        q |= ref_differs(v, valid)
    return (p.astype(np.uint8) | (q.astype(np.uint8) << 1)).astype(np.uint8)


def ref_rank(flags: np.ndarray):
    n = len(flags)
    i = np.arange(n)
    if n == 0:
        z = np.zeros(0, np.int32)
        return z, z, z
    ph = np.maximum.accumulate(np.where(flags & 1, i, 0))
    qh = np.maximum.accumulate(np.where(flags & 2, i, 0))
    cnt = np.cumsum((flags >> 1) & 1)
    return ((i - ph + 1).astype(np.int32), (qh - ph + 1).astype(np.int32),
            (cnt - cnt[ph] + 1).astype(np.int32))


def ref_ends(flags: np.ndarray, whole: bool) -> np.ndarray:
    n = len(flags)
    heads = np.flatnonzero(flags & (1 if whole else 2))
    if n == 0:
        return np.zeros(0, np.int64)
    bounds = np.append(heads, n)
    return np.repeat(bounds[1:] - 1, np.diff(bounds)).astype(np.int64)


def ref_agg(x, valid, flags, whole: bool, kind: str):
    """(values, valid) of one windowed aggregate: per partition a numpy accumulate, read at the
    frame's last row.  ``x`` None: count(*)."""
    n = len(flags)
    valid = np.ones(n, bool) if valid is None else valid.astype(bool)
    floating = kind.endswith("f64")
    scan = np.zeros(n, np.float64 if floating else np.int64)
    cnt = np.zeros(n, np.int64)
    bounds = np.append(np.flatnonzero(flags & 1), n) if n else np.zeros(1, np.int64)
    # one-row partitions at once (their scan is the row itself), the others one by one
    single = bounds[:-1][np.diff(bounds) == 1]
    cnt[single] = valid[single]
    if kind != "count" and len(single):
        ident = 0 if kind.startswith("sum") else (
            (np.inf if floating else np.iinfo(np.int64).max) if kind.startswith("min") else
            (-np.inf if floating else np.iinfo(np.int64).min))
        scan[single] = np.where(valid[single], x[single], ident)
    longer = np.diff(bounds) > 1
    for s, e in zip(bounds[:-1][longer], bounds[1:][longer]):
        m = valid[s:e]
        cnt[s:e] = np.cumsum(m)
        if kind == "count":
            continue
        seg = x[s:e]
        if kind.startswith("sum"):
            scan[s:e] = np.cumsum(np.where(m, seg, 0))
        elif kind.startswith("min"):
            ident = np.inf if floating else np.iinfo(np.int64).max
            scan[s:e] = (np.fmin if floating else np.minimum).accumulate(np.where(m, seg, ident))
        else:
            ident = -np.inf if floating else np.iinfo(np.int64).min
            scan[s:e] = (np.fmax if floating else np.maximum).accumulate(np.where(m, seg, ident))
    ends = ref_ends(flags, whole)
    c = cnt[ends] if n else cnt
    if kind == "count":
        return c, np.ones(n, bool)
    out = np.where(c > 0, scan[ends] if n else scan, 0)
    if floating and not kind.startswith("sum") and n and np.isnan(x).any():
        # NaN is skipped like a NULL; a frame whose non-NULL inputs are all NaN is NaN
        some, _ = ref_agg(None, valid & ~np.isnan(x), flags, whole, "count")
        out = np.where((some == 0) & (c > 0), np.nan, out)
    return out, c > 0


def test_reference_against_a_python_loop():
    for layout, peers in (("rand5", "ties"), ("m64", "single"), ("one", "all")):
        c = make_case(300, layout, peers)
        n = c["n"]
        flags = ref_flags([(c["pkey"], c["pvalid"])], [(c["okey"], None)], n)
        rn, rk, dr = ref_rank(flags)
        # the loop: partitions by (key, is-null), peers by the order key
        part = [(int(k) if v else None) for k, v in zip(c["pkey"], c["pvalid"])]
        start = 0
        for i in range(n):
            if i and part[i] != part[i - 1]:
                start = i
            assert bool(flags[i] & 1) == (i == start)
            peer_start = i
            while peer_start > start and c["okey"][peer_start - 1] == c["okey"][i]:
                peer_start -= 1
            assert bool(flags[i] & 2) == (i == peer_start)
            assert rn[i] == i - start + 1 and rk[i] == peer_start - start + 1
            assert dr[i] == len(set(c["okey"][start:peer_start + 1].tolist()))
        for whole in (False, True):
            ends = ref_ends(flags, whole)
            for kind, x in (("sum_i64", c["ints"]), ("count", None), ("min_i64", c["ints"]),
                            ("max_f64", c["doubles"]), ("sum_f64", c["int_doubles"])):
                got, ok = ref_agg(x, c["valid"], flags, whole, kind)
                for i in range(n):
                    s = i
                    while not flags[s] & 1:
                        s -= 1
                    e = i
                    while e + 1 < n and not flags[e + 1] & (1 if whole else 2):
                        e += 1
                    assert ends[i] == e
                    vals = [x[j] if x is not None else 1 for j in range(s, e + 1) if c["valid"][j]]
                    if kind == "count":
                        assert got[i] == len(vals)
                    elif not vals:
                        assert not ok[i]
                    else:
                        want = {"sum": sum, "min": min, "max": max}[kind[:3]](vals)
                        assert ok[i] and got[i] == want, (kind, i)
    assert (ref_agg(np.zeros(0), None, np.zeros(0, np.uint8), True, "sum_f64")[0]).size == 0
    # NaN inputs of a float min / max
    c = nan_case(300)
    for whole in (False, True):
        for kind in ("min_f64", "max_f64"):
            got, ok = ref_agg(c["x"], c["valid"], c["flags"], whole, kind)
            for i in range(300):
                s = i
                while not c["flags"][s] & 1:
                    s -= 1
                e = i
                while e + 1 < 300 and not c["flags"][e + 1] & (1 if whole else 2):
                    e += 1
                vals = [c["x"][j] for j in range(s, e + 1) if c["valid"][j]]
                nums = [v for v in vals if v == v]
                assert bool(ok[i]) == bool(vals)
                if nums:
                    assert got[i] == (min(nums) if kind == "min_f64" else max(nums))
                elif vals:
                    assert np.isnan(got[i])
    assert np.isnan(ref_agg(c["x"], c["valid"], c["flags"], True, "min_f64")[0]).any()


# ------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------
def _col(device, v: np.ndarray, valid=None, atype=None, dictionary=None):
    import torch
    from hyperspace_amd.exec.device_table import DeviceColumn
    atype = atype or pa.from_numpy_dtype(v.dtype)
    return DeviceColumn(torch.from_numpy(np.ascontiguousarray(v)).to(device),
                        None if valid is None else
                        torch.from_numpy(np.ascontiguousarray(valid.astype(np.uint8))).to(device),
                        atype, dictionary)


def _twice(fn):
    """``fn()``'s outputs as numpy arrays, after a second call gave the same bits."""
    a = [None if x is None else x.cpu().numpy() for x in fn()]
    b = [None if x is None else x.cpu().numpy() for x in fn()]
    for x, y in zip(a, b):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()
    return a


@functools.lru_cache(maxsize=None)
def _case(n: int, layout: str, peers: str):
    c = make_case(n, layout, peers)
    c["flags"] = ref_flags([(c["pkey"], c["pvalid"])], [(c["okey"], None)], n)
    return c


@gpu
def test_tile_rows_is_what_the_layouts_assume(device):
    from hyperspace_amd.ops import _lib as NL, kernels as K
    assert K.win_tile_rows() == T
    for n in (0, 1, T, 5 * T + 3):
        assert NL.lib().hs_win_workspace_bytes(n) >= 24 * n


def _key_cases(n: int):
    """name -> (partition columns, order columns) as (values, valid, arrow type, dictionary)."""
    rng = np.random.default_rng(7 + n)
    runs = np.sort(rng.integers(0, max(n // 4, 1) + 1, n))
    sub = np.sort(rng.integers(0, 3, n))
    nullable = rng.random(n) < 0.3
    f = np.sort(rng.integers(-2, 3, n)).astype(np.float64)
    f[rng.random(n) < 0.3] *= -1.0            # -0.0 beside 0.0, and broken runs elsewhere
    f = np.where(rng.random(n) < 0.15, np.nan, f)
    if n > 4:
        f[1:3] = np.array([0x7FF8000000000001, 0xFFF8000000000000], np.uint64).view(np.float64)
    d = pa.array([f"w{i:03d}" for i in range(max(n // 4, 1) + 1)])
    return {
        "int32": ([(runs.astype(np.int32), None, None, None)], []),
        "int64_order_int32": ([(runs.astype(np.int64), None, None, None)],
                              [(sub.astype(np.int32), None, None, None)]),
        "dictionary_codes": ([(runs.astype(np.int32), None, pa.string(), d)],
                             [(sub.astype(np.int32), None, None, None)]),
        "float_order_key": ([(runs.astype(np.int64), None, None, None)],
                            [(f, None, None, None)]),
        "float32_order_key": ([], [(f.astype(np.float32), None, None, None)]),
        "nullable_keys": ([(runs.astype(np.int64), ~nullable, None, None)],
                          [(sub.astype(np.int32), rng.random(n) >= 0.3, None, None)]),
        "two_partition_keys": ([(runs.astype(np.int64), None, None, None),
                                (sub.astype(np.int16), ~nullable, None, None)],
                               [(f, rng.random(n) >= 0.2, None, None)]),
    }


@gpu
@pytest.mark.parametrize("n", (0, 1, 2, 65, 257, T + 1, 2 * T + 1))
def test_heads_over_key_types(device, n):
    from hyperspace_amd.ops import kernels as K
    for name, (part, order) in _key_cases(n).items():
        want = ref_flags([(v, ok) for v, ok, _, _ in part], [(v, ok) for v, ok, _, _ in order], n)
        pc = [_col(device, *x) for x in part]
        oc = [_col(device, *x) for x in order]
        got, = _twice(lambda: (K.win_heads(pc, oc, n, device),))
        assert got.dtype == np.uint8 and got.tolist() == want.tolist(), name
        if n:
            assert got[0] == 3 and not ((got & 1) & ~(got >> 1)).any()    # bit 0 implies bit 1


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_rank_and_aggregates(device, n, layout):
    import torch
    from hyperspace_amd.ops import _lib as NL, kernels as K
    peers = PEERS[(SIZES.index(n) + LAYOUTS.index(layout)) % len(PEERS)]
    c = _case(n, layout, peers)
    flags = c["flags"]
    got_flags, = _twice(lambda: (K.win_heads(
        [_col(device, c["pkey"], c["pvalid"])], [_col(device, c["okey"])], n, device),))
    assert got_flags.tolist() == flags.tolist()
    dflags = torch.from_numpy(flags).to(device)
    ws = K.win_workspace(n, device)

    for want, got in zip(ref_rank(flags), _twice(lambda: K.win_rank(dflags, ws=ws))):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    only_dense = _twice(lambda: K.win_rank(dflags, False, False, True))
    assert only_dense[0] is None and only_dense[1] is None
    assert np.array_equal(only_dense[2], ref_rank(flags)[2])

    valid = c["valid"]
    cols = {"sum_i64": c["ints"], "min_i64": c["ints"], "max_i64": c["ints"], "count": c["ints"],
            "sum_f64": c["int_doubles"], "min_f64": c["doubles"], "max_f64": c["doubles"]}
    for whole in (False, True):
        ends, = _twice(lambda: (K.win_frame_ends(dflags, whole, ws),))
        assert np.array_equal(ends, ref_ends(flags, whole))
        dends = torch.from_numpy(ends).to(device)
        for kind in KINDS:
            col = _col(device, cols[kind], valid)
            got, ok = _twice(lambda: K.win_agg(col, dflags, dends, getattr(NL, "WA_" + kind.upper()),
                                               ws))
            want, wok = ref_agg(cols[kind], valid, flags, whole, kind)
            assert np.array_equal(ok.astype(bool), wok), (kind, whole)
            assert got.dtype == want.dtype
            assert np.array_equal(got[wok], want[wok]), (kind, whole)       # exact, fp64 too
        # count(*) and a column without a validity mask
        got, ok = _twice(lambda: K.win_agg(None, dflags, dends, NL.WA_COUNT, ws))
        assert np.array_equal(got, ref_agg(None, None, flags, whole, "count")[0]) and ok.all()
        col = _col(device, c["ints"].astype(np.int32))
        got, ok = _twice(lambda: K.win_agg(col, dflags, dends, NL.WA_SUM_I64, ws))
        assert np.array_equal(got, ref_agg(c["ints"], None, flags, whole, "sum_i64")[0])
        # a general fp64 sum: another summation order than numpy's, within the analytic bound
        col = _col(device, c["doubles"], valid)
        got, ok = _twice(lambda: K.win_agg(col, dflags, dends, NL.WA_SUM_F64, ws))
        want, wok = ref_agg(c["doubles"], valid, flags, whole, "sum_f64")
        mass, _ = ref_agg(np.abs(c["doubles"]), valid, flags, whole, "sum_f64")
        start = np.maximum.accumulate(np.where(flags & 1, np.arange(n), 0)) if n else ends
        k = ends - start + 1
        bound = 2.0 * k * 2.0 ** -53 * mass
        assert np.array_equal(ok.astype(bool), wok)
        assert (np.abs(got - want)[wok] <= bound[wok]).all(), float(
            (np.abs(got - want)[wok] / np.maximum(bound[wok], 1e-300)).max())


@gpu
@pytest.mark.parametrize("n", (65, 2 * T + 1))
def test_float_min_max_skip_nan_and_counts_come_with_the_values(device, n):
    import torch
    from hyperspace_amd.ops import _lib as NL, kernels as K
    c = nan_case(n)
    dflags = torch.from_numpy(c["flags"]).to(device)
    for whole in (False, True):
        dends = K.win_frame_ends(dflags, whole)
        for dtype in (np.float64, np.float32):
            x = c["x"].astype(dtype)
            col = _col(device, x, c["valid"])
            for kind in ("min_f64", "max_f64"):
                got, ok = _twice(lambda: K.win_agg(col, dflags, dends,
                                                   getattr(NL, "WA_" + kind.upper())))
                want, wok = ref_agg(x.astype(np.float64), c["valid"], c["flags"], whole, kind)
                assert np.array_equal(ok.astype(bool), wok)
                assert np.array_equal(got[wok], want[wok], equal_nan=True), (kind, whole)
                assert np.isnan(want[wok]).any() and not np.isinf(got[wok]).any()
        # the count a sum carries is the count scan's (what avg divides by)
        col = _col(device, c["x"], c["valid"])
        _, ok, cnt = _twice(lambda: K.win_agg(col, dflags, dends, NL.WA_SUM_F64,
                                              with_count=True))
        want = ref_agg(None, c["valid"], c["flags"], whole, "count")[0]
        assert cnt.dtype == np.int64 and np.array_equal(cnt, want)
        assert np.array_equal(ok.astype(bool), want > 0)
