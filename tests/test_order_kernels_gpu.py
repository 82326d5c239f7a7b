"""The kernels that consume the order-preserving key image - radix sort, run merge, range search,
key probes, the exclusive scans and bucket offsets under them - against the independent numpy
reference in tests/order_ref.py.  Every comparison is exact.  GPU-only."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from order_ref import (SPECIAL_F32, SPECIAL_F64, ref_image, ref_probe, ref_ranges,
                       ref_sort_perm)

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def _dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _dcol(values, nulls, atype, device, dictionary=None):
    """A device column straight from arrays: ``values`` is stored as it is, garbage under the
    null slots included; ``nulls`` None = no validity mask."""
    from hyperspace_amd.exec.device_table import DeviceColumn
    valid = None if nulls is None else _dev((~np.asarray(nulls, bool)).astype(np.uint8), device)
    return DeviceColumn(_dev(values, device), valid, atype, dictionary)


def _garbage(values, nulls):
    """``values`` with the extremes of its type (NaN for floats) under the null slots, so a key
    range or a comparison that looked at invalid rows would show."""
    v = values.copy()
    idx = np.nonzero(nulls)[0]
    if v.dtype.kind == "f":
        v[idx] = np.nan
    elif v.dtype == np.uint8:
        v[idx] = 1
    else:
        info = np.iinfo(v.dtype)
        v[idx] = np.where(np.arange(len(idx)) % 2 == 0, info.min, info.max)
    return v


# ------------------------------------------------------------------------------------------------
# Radix sort
# ------------------------------------------------------------------------------------------------
def _i_full(dtype):
    def gen(rng, n):
        info = np.iinfo(dtype)
        v = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        if n >= 2:
            v[rng.choice(n, 2, replace=False)] = [info.min, info.max]
        return v
    return gen


def _floats(special):
    def gen(rng, n):
        v = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)).astype(special.dtype)
        pick = rng.random(n) < 0.4
        v[pick] = rng.choice(special, int(pick.sum()))
        return v
    return gen


_DICT = pa.array(sorted(f"s{i:03d}" for i in range(50)))
SORT_TYPES = {
    "i8": (_i_full(np.int8), pa.int8(), None),
    "i16": (_i_full(np.int16), pa.int16(), None),
    "i32": (_i_full(np.int32), pa.int32(), None),
    "i64": (_i_full(np.int64), pa.int64(), None),
    "bool": (lambda rng, n: rng.integers(0, 2, n).astype(np.uint8), pa.bool_(), None),
    "f32": (_floats(SPECIAL_F32), pa.float32(), None),
    "f64": (_floats(SPECIAL_F64), pa.float64(), None),
    "date32": (lambda rng, n: rng.integers(-3000, 20000, n).astype(np.int32), pa.date32(), None),
    "timestamp": (lambda rng, n: rng.integers(-2**40, 2**52, n).astype(np.int64),
                  pa.timestamp("us"), None),
    "dictionary": (lambda rng, n: rng.integers(0, 50, n).astype(np.int32), pa.string(), _DICT),
}
SORT_ROWS = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 40_000)


def _null_modes(rng, n):
    """(name, null mask or None): no mask, a mask without a null, 3 % nulls (at least one), all."""
    some = rng.random(n) < 0.03
    some[rng.integers(0, n)] = True
    return (("none", None), ("nullable", np.zeros(n, bool)), ("3pct", some),
            ("all", np.ones(n, bool)))


@pytest.mark.parametrize("tname", sorted(SORT_TYPES))
def test_sort_single_key_every_type_and_row_count(device, tname):
    from hyperspace_amd.ops import kernels as K
    gen, atype, dictionary = SORT_TYPES[tname]
    rng = np.random.default_rng(sorted(SORT_TYPES).index(tname))
    for n in SORT_ROWS:
        base = gen(rng, n)
        for mode, nulls in _null_modes(rng, n):
            vals = base if nulls is None else _garbage(base, nulls)
            col = _dcol(vals, nulls, atype, device, dictionary)
            got = K.sort_permutation([col]).cpu().numpy()
            want = ref_sort_perm([(vals, nulls)])
            assert np.array_equal(got, want), (tname, n, mode, np.nonzero(got != want)[0][:5])


SPANS = {
    np.int32: [("const", 7, 0), ("255", -100, 255), ("256", -100, 256), ("257", -100, 257),
               ("65535", -40000, 65535), ("65536", -40000, 65536),
               ("2^32-1", I32_MIN, 2**32 - 1)],
    np.int64: [("const", -7, 0), ("255", -100, 255), ("256", -100, 256), ("257", -100, 257),
               ("2^32-1", -2**31 - 5, 2**32 - 1), ("2^32", -2**31 - 5, 2**32),
               ("2^32+1", -2**31 - 5, 2**32 + 1), ("full", I64_MIN, 2**64 - 1)],
}


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_sort_span_edges(device, dtype):
    """A constant column (no pass at all), spans across the 8-bit pass boundaries, across the
    32- to 64-bit key switch, and the full int64 range, at a row count one past a tile."""
    from hyperspace_amd.ops import kernels as K
    rng = np.random.default_rng(20)
    n = 4097
    atype = pa.int32() if dtype == np.int32 else pa.int64()
    for name, lo, span in SPANS[dtype]:
        off = rng.integers(0, span, n, dtype=np.uint64, endpoint=True)
        off[rng.choice(n, 2, replace=False)] = [0, span]
        # lo + off modulo 2^64, so the full int64 range needs no wider type
        base = (np.uint64(lo & (2**64 - 1)) + off).view(np.int64).astype(dtype)
        assert int(base.max()) - int(base.min()) == span
        for mode, nulls in _null_modes(rng, n):
            if mode == "all":
                continue
            if nulls is not None:
                nulls[[np.argmin(base), np.argmax(base)]] = False    # the span stays the span
            vals = base if nulls is None else _garbage(base, nulls)
            got = K.sort_permutation([_dcol(vals, nulls, atype, device)]).cpu().numpy()
            want = ref_sort_perm([(vals, nulls)])
            assert np.array_equal(got, want), (name, mode, np.nonzero(got != want)[0][:5])


def test_sort_multi_key_stability_leading_and_init_perm(device):
    import torch
    from hyperspace_amd.ops import kernels as K
    rng = np.random.default_rng(21)
    n = 8193
    a = rng.integers(-3, 3, n).astype(np.int64)
    an = rng.random(n) < 0.1
    a = _garbage(a, an)
    f = rng.choice(np.concatenate([SPECIAL_F64[[1, 5, 6, 11]], [2.5, -2.5]]), n)
    fn = rng.random(n) < 0.1
    f = _garbage(f, fn)
    c = rng.integers(-2, 2, n).astype(np.int16)
    bucket = rng.integers(0, 5, n).astype(np.int32)
    cols = [_dcol(a, an, pa.int64(), device), _dcol(f, fn, pa.float64(), device),
            _dcol(c, None, pa.int16(), device)]
    keys = [(a, an), (f, fn), (c, None)]
    # heavy duplicates in the leading keys: the order of ties is the input order
    got = K.sort_permutation(cols).cpu().numpy()
    assert np.array_equal(got, ref_sort_perm(keys))
    lead = (_dev(bucket, device), 8)
    got = K.sort_permutation(cols, extra_leading=lead).cpu().numpy()
    assert np.array_equal(got, ref_sort_perm(keys, leading=bucket))
    # init_perm: the rows are taken in that order, and the argument is left alone
    p = rng.permutation(n).astype(np.int32)
    dp = _dev(p, device)
    got = K.sort_permutation(cols, init_perm=dp).cpu().numpy()
    assert np.array_equal(got, ref_sort_perm(keys, init=p))
    got = K.sort_permutation(cols, init_perm=dp, extra_leading=lead).cpu().numpy()
    assert np.array_equal(got, ref_sort_perm(keys, leading=bucket, init=p))
    assert torch.equal(dp.cpu(), torch.from_numpy(p))
    # only the last key decides: two constant keys in front
    k0 = np.full(n, 9, np.int32)
    got = K.sort_permutation([_dcol(k0, None, pa.int32(), device),
                              _dcol(k0, np.zeros(n, bool), pa.int32(), device), cols[2]])
    assert np.array_equal(got.cpu().numpy(), ref_sort_perm([(c, None)]))


# ------------------------------------------------------------------------------------------------
# Merge of sorted runs
# ------------------------------------------------------------------------------------------------
# run lengths per group: 1, 2, 3 and 5 runs; empty runs first, in the middle and last; the
# lengths around MP_ITEMS (8) and around one block's 2048 outputs
MERGE_GROUPS = [[2049], [7], [0, 7], [8, 0], [2047, 2049], [1, 1], [9, 0, 2048], [2048, 7, 8],
                [1, 9, 0], [2047, 1, 0, 2049, 9], [0, 8, 7, 1, 0], [2048, 2048, 2047, 2049, 8]]


def _run_layout():
    lens = [m for g in MERGE_GROUPS for m in g]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    grp = np.array([gi for gi, g in enumerate(MERGE_GROUPS) for _ in g], np.int64)
    return off, grp


def _sort_runs(keys, off):
    """``keys`` with every run put in the reference order."""
    out = [(v.copy(), None if m is None else m.copy()) for v, m in keys]
    for s, e in zip(off[:-1], off[1:]):
        if e - s < 2:
            continue
        p = s + ref_sort_perm([(v[s:e], None if m is None else m[s:e]) for v, m in keys])
        for (v, m), (v0, m0) in zip(out, keys):
            v[s:e] = v0[p]
            if m is not None:
                m[s:e] = m0[p]
    return out


def _merge_case(name, rng, n):
    if name == "i64_nullable_i32":
        a = rng.integers(-4, 4, n).astype(np.int64)
        an = rng.random(n) < 0.1
        return [(_garbage(a, an), an), (rng.integers(0, 3, n).astype(np.int32), None)], \
            [pa.int64(), pa.int32()]
    if name == "f64_64bit":
        f = rng.normal(size=n)
        pick = rng.random(n) < 0.5
        f[pick] = rng.choice(SPECIAL_F64, int(pick.sum()))
        return [(f, None)], [pa.float64()]
    # 31 bits + (1 null bit + 32 bits) = 64; the optional null bit on the first key makes 65
    a = rng.choice(np.array([0, 5, 2**31 - 1], np.int32), n)
    a[:2] = [0, 2**31 - 1]
    b = rng.integers(I32_MIN, I32_MAX, n, dtype=np.int32, endpoint=True)
    bn = rng.random(n) < 0.1
    bn[:2] = False
    b[:2] = [I32_MIN, I32_MAX]
    b = _garbage(b, bn)
    an = np.zeros(n, bool) if name == "composite_65" else None
    return [(a, an), (b, bn)], [pa.int32(), pa.int32()]


@pytest.mark.parametrize("case", ["i64_nullable_i32", "f64_64bit", "composite_64"])
def test_merge_runs_equals_reference_sort(device, case):
    """Ties across runs go to the left run: the merge is the stable (group, keys) sort."""
    from hyperspace_amd.ops import kernels as K
    off, grp = _run_layout()
    n = int(off[-1])
    rng = np.random.default_rng(30)
    keys, atypes = _merge_case(case, rng, n)
    keys = _sort_runs(keys, off)
    cols = [_dcol(v, m, t, device) for (v, m), t in zip(keys, atypes)]
    total = sum(K._sortable_range(c)[1] + (c.valid is not None) for c in cols)
    assert total == {"i64_nullable_i32": 3 + 1 + 2, "f64_64bit": 64, "composite_64": 64}[case]
    perm = K.merge_runs_permutation(cols, off, grp)
    assert perm is not None
    got = perm.cpu().numpy()
    want = ref_sort_perm(keys, leading=np.repeat(grp, np.diff(off)))
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    # one run per group: nothing to merge
    one = K.merge_runs_permutation(cols, np.array([0, 5, n]), np.array([0, 1]))
    assert np.array_equal(one.cpu().numpy(), np.arange(n))


def test_merge_runs_declines_what_it_cannot_merge(device):
    from hyperspace_amd.ops import _lib as NL, kernels as K
    off, grp = _run_layout()
    n = int(off[-1])
    rng = np.random.default_rng(31)
    # a composite key of 65 bits
    keys, atypes = _merge_case("composite_65", rng, n)
    keys = _sort_runs(keys, off)
    cols = [_dcol(v, m, t, device) for (v, m), t in zip(keys, atypes)]
    assert sum(K._sortable_range(c)[1] + (c.valid is not None) for c in cols) == 65
    assert K.merge_runs_permutation(cols, off, grp) is None
    # more key columns than the kernel's key table holds (constant columns: 0 bits in all)
    const = _dcol(np.zeros(n, np.int32), None, pa.int32(), device)
    assert K.merge_runs_permutation([const] * NL.MERGE_MAX_KEYS, off, grp) is not None
    assert K.merge_runs_permutation([const] * (NL.MERGE_MAX_KEYS + 1), off, grp) is None
    # a run that is not sorted: one swap inside the longest run
    a = np.sort(rng.integers(0, 50, n)).astype(np.int64)
    keys = _sort_runs([(a, None)], off)
    assert K.merge_runs_permutation([_dcol(keys[0][0], None, pa.int64(), device)],
                                    off, grp) is not None
    bad = keys[0][0].copy()
    s = int(off[np.argmax(np.diff(off))])
    bad[s], bad[s + 2048] = 60, -1
    assert K.merge_runs_permutation([_dcol(bad, None, pa.int64(), device)], off, grp) is None


# ------------------------------------------------------------------------------------------------
# Range search and key probes
# ------------------------------------------------------------------------------------------------
# non-null rows per bucket: the 32-lane tail alone (<= 32), one 32-ary step (33, 34), two steps
# from 32 * 33 = 1056 on, and a large bucket
RANGE_SIZES = (0, 1, 31, 32, 33, 34, 1056, 1057, 1090, 40_000)
RANGE_KEYS = {
    "i32": (np.int32, pa.int32(), 1),
    "i64": (np.int64, pa.int64(), 2**33),
    "f64": (np.float64, pa.float64(), 0.25),
    "date32": (np.int32, pa.date32(), 1),
}


def _range_table(kname, prefix, rng):
    """(values, nulls or None, bucket_off, literals).  Keys are even multiples of the type's
    step in [-20000, 20000] steps (so an odd multiple lies between two present values), sorted
    per bucket with many duplicates, behind ``prefix`` null rows ("whole": every row null;
    None: no validity mask)."""
    dtype, _, step = RANGE_KEYS[kname]
    vals, nulls = [], []
    for m in RANGE_SIZES:
        k = np.sort(rng.integers(-10000, 10001, m)) * 2
        if m == 40_000:
            k[:3], k[-3:] = -20000, 20000        # the extremes, as runs of duplicates
            k[20000:20010] = k[20000]
        k = (k * step).astype(dtype)
        npre = 0 if prefix in (None, "whole") else prefix
        vals.append(np.concatenate([np.zeros(npre, dtype), k]))
        nulls.append(np.concatenate([np.ones(npre, bool), np.full(m, prefix == "whole")]))
    off = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.int64)
    vals, nulls = np.concatenate(vals), np.concatenate(nulls)
    vals = _garbage(vals, nulls)
    big = vals[off[-2]:][~nulls[off[-2]:]]
    dup = big[20000] if len(big) else dtype(0)
    lits = [dtype(-20001 * step), dtype(-20000 * step), dup, dtype(dup + step),
            dtype(20000 * step), dtype(20001 * step)]
    return vals, (None if prefix is None else nulls), off, lits


BUCKET_SETS = (None, [7], [9, 2, 2, 5], [9, 3, 3, 0, 6])    # 10, 1, 4 and 5 ranges: RANGE_WAVES = 4


@pytest.mark.parametrize("prefix", [None, 0, 1, 33, "whole"])
@pytest.mark.parametrize("kname", sorted(RANGE_KEYS))
def test_range_search_both_entry_points_equal_reference(device, kname, prefix):
    """Every pair of (none, inclusive, exclusive) bounds with literals below, at, inside and
    above the keys (lo > hi included), over bucket sizes on the edges of the 32-ary search;
    K.range_search and hs_range_search_dev agree with each other and with np.searchsorted."""
    import torch
    from hyperspace_amd.exec.graphs import range_bounds
    from hyperspace_amd.ops import _lib as NL, kernels as K
    rng = np.random.default_rng(40)
    kind = {"i32": "I32", "i64": "I64", "f64": "F64", "date32": "I32"}[kname]
    vals, nulls, off, lits = _range_table(kname, prefix, rng)
    imgs = [int(i) for i in ref_image(np.array(lits), kind)]
    col = _dcol(vals, nulls, RANGE_KEYS[kname][1], device)
    doff = _dev(off, device)
    calls = []
    for lo_mode in (None, True, False):
        for hi_mode in (None, True, False):
            for lo in (imgs if lo_mode is not None else [None]):
                for hi in (imgs if hi_mode is not None else [None]):
                    calls.append((lo, bool(lo_mode), hi, bool(hi_mode),
                                  BUCKET_SETS[len(calls) % len(BUCKET_SETS)]))
    assert len(calls) == 1 + 4 * 6 + 4 * 36
    dsets = {i: None if b is None else _dev(np.array(b, np.int32), device)
             for i, b in enumerate(BUCKET_SETS)}
    params = _dev(np.array([range_bounds(lo, li, hi, hi_) for lo, li, hi, hi_, _ in calls],
                           np.int64), device)
    kd = col.desc()
    L = NL.lib()
    out_a, out_b = [], []
    for i, (lo, li, hi, hi_, _) in enumerate(calls):
        db = dsets[i % len(BUCKET_SETS)]
        out_a.append(K.range_search(col, doff, db, lo, li, hi, hi_))
        nb = len(RANGE_SIZES) if db is None else db.numel()
        rs = torch.full((nb,), -1, dtype=torch.int64, device=device)
        rl, rb = torch.full_like(rs, -1), torch.full((nb,), -1, dtype=torch.int32, device=device)
        NL.check(L.hs_range_search_dev(C.byref(kd), NL.ptr(doff), NL.ptr(db), nb,
                                       C.c_void_p(params.data_ptr() + 48 * i), NL.ptr(rs),
                                       NL.ptr(rl), NL.ptr(rb), NL.stream_ptr()),
                 "hs_range_search_dev")
        out_b.append((rs, rl, rb))
    host = [[torch.cat([o[j] for o in out]).cpu().numpy() for j in range(3)]
            for out in (out_a, out_b)]
    want = [ref_ranges(vals, nulls, off, b, lo, li, hi, hi_) for lo, li, hi, hi_, b in calls]
    pos = 0
    for call, w in zip(calls, want):
        k = len(w[0])
        for which, h in zip(("range_search", "range_search_dev"), host):
            for j, what in enumerate(("rstart", "rlen", "rbucket")):
                got = h[j][pos:pos + k]
                assert np.array_equal(got, w[j]), (which, what, call, got, w[j])
        assert (host[0][1][pos:pos + k] >= 0).all()
        pos += k
    assert pos == len(host[0][0])
    if prefix != "whole":
        # the cases are what they claim: some range is empty, some is a whole bucket
        lens = np.concatenate([w[1] for w in want])
        assert (lens == 0).any() and (lens == 40_000).any() and (lens >= 10).any()


@pytest.mark.parametrize("kname", ["i32", "i64", "f64"])
def test_probe_ranges_equal_reference(device, kname):
    """Probes for keys present once, as a run of duplicates, absent, below and above a bucket's
    keys, into empty and single-row buckets, behind a null prefix."""
    from hyperspace_amd.ops import kernels as K
    rng = np.random.default_rng(41)
    kind = {"i32": "I32", "i64": "I64", "f64": "F64"}[kname]
    dtype, atype, step = RANGE_KEYS[kname]
    vals, nulls, off, lits = _range_table(kname, 33, rng)
    col = _dcol(vals, nulls, atype, device)
    doff = _dev(off, device)
    nb = len(RANGE_SIZES)
    for np_ in (1, 4, 5, 1000):
        pb = rng.integers(0, nb, np_).astype(np.int32)
        pb[:3] = [9, 0, 1][:np_]                  # the large, the empty and the one-row bucket
        keys = np.empty(np_, dtype)
        for i, b in enumerate(pb):
            s, e = off[b] + 33, off[b + 1]
            how = i % 5
            if how < 2 and e > s:
                keys[i] = vals[rng.integers(s, e)]                    # present
            elif how == 2:
                keys[i] = dtype((2 * rng.integers(-10000, 10000) + 1) * step)   # absent
            else:
                keys[i] = lits[0] if how == 3 else lits[5]            # below / above
        if np_ == 1000:
            keys[0] = lits[2]                      # the run of 10 duplicates in the large bucket
        img = ref_image(keys, kind)
        rs, rl, rb = K.probe_ranges(col, doff, _dev(pb, device), _dev(img.view(np.int64), device))
        want = ref_probe(vals, nulls, off, pb, img)
        for got, w, what in zip((rs, rl, rb), want, ("rstart", "rlen", "rbucket")):
            assert np.array_equal(got.cpu().numpy(), w), (np_, what)
        if np_ == 1000:
            assert want[1][0] >= 10 and (want[1] == 0).any() and (want[1] == 1).any()


# ------------------------------------------------------------------------------------------------
# Scans, bucket offsets, tiles
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 2048 * 2048, 2048 * 2048 + 1])
def test_exclusive_scan_i64_one_two_and_three_levels(device, n):
    from hyperspace_amd.ops import kernels as K
    rng = np.random.default_rng(n)
    x = rng.integers(-2**40, 2**40, n)          # sums far beyond 32 bits, both signs
    got = K.exclusive_scan_i64(_dev(x, device)).cpu().numpy()
    want = np.concatenate([[0], np.cumsum(x)[:-1]])
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]


def test_bucket_offsets_from_sorted_equal_searchsorted(device):
    from hyperspace_amd.ops import kernels as K
    rng = np.random.default_rng(50)
    cases = [(np.sort(rng.integers(0, 200, 100_003)), 200),
             (np.sort(rng.choice([1, 2, 5, 6], 5000)), 8),      # empty first, middle and last
             (np.zeros(777), 1), (np.full(777, 3), 5), (np.zeros(0), 4), (np.zeros(0), 1),
             (np.arange(300), 300), (np.sort(rng.integers(0, 1000, 50)), 1000)]
    for ids, B in cases:
        ids = ids.astype(np.int32)
        got = K.bucket_offsets_from_sorted(_dev(ids, device), B).cpu().numpy()
        assert np.array_equal(got, np.searchsorted(ids, np.arange(B + 1))), (len(ids), B)


@pytest.mark.parametrize("R", [1, 63, 64, 65, 200])
def test_ranges_to_tiles_equal_ceil_div_cumsum(device, R):
    from hyperspace_amd.ops import _lib as NL, kernels as K
    rng = np.random.default_rng(R)
    tile = int(NL.lib().hs_scan_tile_rows())
    for tr in (None, 7, 1):
        t = tr or tile
        rlen = rng.integers(0, 5 * t, R)
        rlen[rng.random(R) < 0.3] = 0
        mult = rng.random(R) < 0.3
        rlen[mult] = rng.integers(1, 6, int(mult.sum())) * t      # exact multiples of the tile
        rlen[-1] = 3 * t
        got = K.ranges_to_tiles(_dev(rlen.astype(np.int64), device), tr).cpu().numpy()
        want = np.concatenate([[0], np.cumsum((rlen + t - 1) // t)])
        assert np.array_equal(got, want), (R, t)
    z = K.ranges_to_tiles(_dev(np.zeros(R, np.int64), device)).cpu().numpy()
    assert np.array_equal(z, np.zeros(R + 1, np.int64))
