"""The level-2 kernels of COUNT(DISTINCT x) (csrc/kernels/distinct_agg.hip) against a numpy
reference: the dense (LDS + slab) regroup and the hash regroup over dense level-1 groups built on
the host.  Sums are integer valued, so every comparison is exact.

The numpy reference is checked on the CPU first (against a plain Python loop)."""
import itertools

import numpy as np
import pytest

from hyperspace_amd.exec import hash_agg as H

gpu = pytest.mark.gpu

_U = np.uint64
_FULL = 0xFFFFFFFFFFFFFFFF
SIZES = (0, 1, 63, 64, 65, 1000)


# ------------------------------------------------------------------------------------------------
# inputs and the reference
# ------------------------------------------------------------------------------------------------
def make_rows(n: int, A: int, pattern: str, outer_bits: int, x_nullable: bool, seed: int,
              integer: bool = True) -> dict:
    """Dense level-1 groups: key = outer | xcode << outer_bits.  Patterns: "one" every row in
    outer group 5 % slots (the contention case), "own" row i in outer group i, "mixed" a few
    outer groups, one of them (outer 1) holding only NULL-x rows when x is nullable."""
    rng = np.random.default_rng(seed)
    slots = 1 << outer_bits
    if pattern == "one":
        outer = np.full(n, 5 % slots, dtype=np.uint64)
    elif pattern == "own":
        assert n <= slots
        outer = np.arange(n, dtype=np.uint64)
    else:
        outer = rng.integers(0, min(slots, 7), n).astype(np.uint64)
    # level-1 rows are distinct (outer, x): give row i the x code i + 1 (or 0 = NULL)
    code = np.arange(1, n + 1, dtype=np.uint64)
    if x_nullable:
        code[outer == 1] = 0
        code[rng.random(n) < 0.2] = 0
    keys = outer | (code << _U(outer_bits))
    vals = rng.integers(-50, 50, (n, A)).astype(np.float64) if integer else \
        rng.normal(size=(n, A)) * 1e3
    return {"keys": keys, "nulls": np.zeros(n, np.uint8), "sums": vals,
            "cnts": rng.integers(0, 9, (n, A)).astype(np.int64),
            "mins": rng.integers(-99, 99, (n, A)).astype(np.float64),
            "maxs": rng.integers(-99, 99, (n, A)).astype(np.float64)}


def fields(outer_bits: int, x_nullable: bool) -> H.DistinctFields:
    return H.DistinctFields((1 << outer_bits) - 1, outer_bits, x_nullable, False)


def ref_regroup(host: dict, A: int, f: H.DistinctFields, minmax: bool) -> dict:
    """{outer key: (sums[A + 2], cnts[A + 2], mins[A + 2], maxs[A + 2])} in numpy."""
    keys = host["keys"]
    n = len(keys)
    if f.raw:
        outer = np.zeros(n, np.uint64)
        nonnull = host["nulls"] == 0
    else:
        outer = keys & _U(f.outer_mask)
        code = keys >> _U(f.x_shift) if f.x_shift < 64 else np.zeros(n, np.uint64)
        nonnull = (code != 0) | (not f.x_nullable)
    out = {}
    for k in np.unique(outer):
        m = outer == k
        sums, cnts = np.zeros(A + 2), np.zeros(A + 2, np.int64)
        mins, maxs = np.full(A + 2, np.inf), np.full(A + 2, -np.inf)
        sums[:A] = host["sums"][m].sum(axis=0)
        cnts[:A] = host["cnts"][m].sum(axis=0)
        cnts[A] = int((m & nonnull).sum())
        cnts[A + 1] = int(m.sum())
        if minmax:
            mins[:A] = host["mins"][m].min(axis=0)
            maxs[:A] = host["maxs"][m].max(axis=0)
        out[int(k)] = (sums, cnts, mins, maxs)
    return out


def dense_fits(slots: int, A: int, minmax: bool) -> bool:
    """The bound the kernel file states: slots * NA2 * 8 * (2 + 2 * minmax) <= 64 KiB."""
    return slots * (A + 2) * 8 * (2 + (2 if minmax else 0)) <= 64 * 1024


def test_reference_against_a_python_loop():
    A = 2
    for xn, pattern in itertools.product((False, True), ("one", "mixed")):
        host = make_rows(200, A, pattern, 4, xn, 1)
        f = fields(4, xn)
        want = {}
        for i in range(200):
            k = int(host["keys"][i])
            o, code = k & 15, k >> 4
            e = want.setdefault(o, [[0.0] * A, [0] * A, [np.inf] * A, [-np.inf] * A, 0, 0])
            for a in range(A):
                e[0][a] += host["sums"][i, a]
                e[1][a] += int(host["cnts"][i, a])
                e[2][a] = min(e[2][a], host["mins"][i, a])
                e[3][a] = max(e[3][a], host["maxs"][i, a])
            e[4] += 1 if (code != 0 or not xn) else 0
            e[5] += 1
        got = ref_regroup(host, A, f, True)
        assert set(got) == set(want)
        for o, e in want.items():
            s, c, mn, mx = got[o]
            assert s[:A].tolist() == e[0] and c[:A].tolist() == e[1]
            assert mn[:A].tolist() == e[2] and mx[:A].tolist() == e[3]
            assert (c[A], c[A + 1]) == (e[4], e[5]) and c[A + 1] >= 1
            assert s[A] == s[A + 1] == 0 and np.isinf(mn[A:]).all() and np.isinf(mx[A:]).all()
        if xn and pattern == "mixed":
            assert got[1][1][A] == 0 and got[1][1][A + 1] > 0     # only NULL-x rows
    # raw keys: one outer group, NULL in the nulls byte
    host = make_rows(10, 1, "one", 0, False, 2)
    host["nulls"][3] = 1
    got = ref_regroup(host, 1, H.DistinctFields(raw=True), False)
    assert list(got) == [0] and got[0][1][1] == 9 and got[0][1][2] == 10


# ------------------------------------------------------------------------------------------------
# device helpers
# ------------------------------------------------------------------------------------------------
def _upload(host: dict, A: int, minmax: bool, device) -> H.Groups:
    return H.Groups.from_host(host, A, minmax, device)


def _as_dict(host: dict) -> dict:
    return {int(k): (host["sums"][i], host["cnts"][i], host["mins"][i], host["maxs"][i])
            for i, k in enumerate(host["keys"])}


def _same(got: dict, want: dict, minmax: bool):
    assert set(got) == set(want)
    for k, (s, c, mn, mx) in want.items():
        gs, gc, gmn, gmx = got[k]
        assert np.array_equal(gs, s) and np.array_equal(gc, c), k
        if minmax:
            assert np.array_equal(gmn, mn) and np.array_equal(gmx, mx), k


def run_dense(host: dict, A: int, f: H.DistinctFields, minmax: bool, device) -> dict:
    n = len(host["keys"])
    out = H.distinct_regroup_dense(_upload(host, A, minmax, device), n, f).to_host(f.slots)
    assert out["keys"].tolist() == list(range(f.slots))          # one row per outer code
    live = out["cnts"][:, A + 1] > 0
    dead = {k: v[~live] for k, v in out.items()}
    assert not dead["sums"].any() and not dead["cnts"].any()     # untouched codes stay zero
    return _as_dict({k: v[live] for k, v in out.items()})


def run_hash(host: dict, A: int, f: H.DistinctFields, minmax: bool, device, M: int = 0):
    n = len(host["keys"])
    M = M or H.next_pow2(max(16, 4 * n))
    table = H.HashTable(M, A + 2, minmax, device)
    out = H.distinct_regroup(_upload(host, A, minmax, device), n, f, table)
    G, over = out.count()
    return _as_dict(out.to_host(G)), over, table


DENSE_CASES = [(n, pattern, mm, xn)
               for n, pattern, mm, xn in itertools.product(SIZES, ("one", "own", "mixed"),
                                                           (False, True), (False, True))
               if pattern != "own" or dense_fits(H.next_pow2(max(n, 1)), 1, mm)]


@gpu
def test_dense_bound_is_the_documented_formula(device):
    for slots, A, mm in itertools.product((1, 2, 64, 256, 1024, 1365, 1366, 4096), (1, 2, 5),
                                          (False, True)):
        f = H.DistinctFields(slots - 1, 0, False, False)
        assert H.distinct_dense_fits(f, A, mm) == dense_fits(slots, A, mm), (slots, A, mm)


@gpu
@pytest.mark.parametrize("n,pattern,minmax,x_nullable", DENSE_CASES)
def test_dense_regroup(device, n, pattern, minmax, x_nullable):
    A = 1 if pattern == "own" else 3
    bits = max(n - 1, 0).bit_length() if pattern == "own" else 3
    host = make_rows(n, A, pattern, bits, x_nullable, 10 + n)
    f = fields(bits, x_nullable)
    assert H.distinct_dense_fits(f, A, minmax)
    _same(run_dense(host, A, f, minmax, device), ref_regroup(host, A, f, minmax), minmax)


@gpu
@pytest.mark.parametrize("n,pattern,minmax,x_nullable",
                         list(itertools.product(SIZES, ("one", "own", "mixed"), (False, True),
                                                (False, True))))
def test_hash_regroup(device, n, pattern, minmax, x_nullable):
    A = 3
    bits = 12 if pattern == "own" else 3
    host = make_rows(n, A, pattern, bits, x_nullable, 20 + n)
    f = fields(bits, x_nullable)
    got, over, table = run_hash(host, A, f, minmax, device)
    assert not over
    _same(got, ref_regroup(host, A, f, minmax), minmax)
    assert int(table.flag[0].item()) == 0
    assert bool((table.keys[:table.M] == -1).all())              # extract left the table clean


@gpu
@pytest.mark.parametrize("minmax", (False, True))
def test_hash_regroup_outer_key_equal_to_the_empty_pattern(device, minmax):
    """x has no bits of its own (one non-null value): the whole key is the outer key, and the
    all-ones key is the table's EMPTY pattern (direct slot M)."""
    A, n = 2, 65
    host = make_rows(n, A, "one", 0, False, 31)
    rng = np.random.default_rng(32)
    host["keys"] = rng.integers(0, 1 << 62, n).astype(np.uint64)
    host["keys"][[0, 17, 64]] = _U(_FULL)
    host["keys"][[3, 4]] = _U(0)
    f = H.DistinctFields(_FULL, 64, False, False)
    assert not H.distinct_dense_fits(f, A, minmax)
    got, over, _ = run_hash(host, A, f, minmax, device)
    assert not over
    want = ref_regroup(host, A, f, minmax)
    assert want[_FULL][1][A + 1] == 3 and want[_FULL][1][A] == 3
    _same(got, want, minmax)


@gpu
@pytest.mark.parametrize("kind", ("raw_int", "raw_float"))
@pytest.mark.parametrize("n", (1, 64, 65, 1000))
def test_raw_modes_with_the_null_row(device, kind, n):
    A = 2
    host = make_rows(n, A, "one", 0, False, 40 + n)
    rng = np.random.default_rng(41)
    if kind == "raw_int":
        host["keys"] = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64).view(np.uint64)
    else:
        host["keys"] = (rng.normal(size=n) * 1e6).view(np.uint64)
    host["nulls"][n // 2] = 1                                    # the NULL key's row
    f = H.DistinctFields(raw=True)
    want = ref_regroup(host, A, f, True)
    assert want[0][1][A] == n - 1 and want[0][1][A + 1] == n
    _same(run_dense(host, A, f, True, device), want, True)
    got, over, _ = run_hash(host, A, f, True, device)
    assert not over
    _same(got, want, True)


@gpu
def test_hash_regroup_overflow_sets_the_flag_and_returns(device):
    """16 outer groups into a table of 4 slots: the probe budget runs out, the kernel flags it
    and returns; extract reports and clears the flag and leaves the table empty."""
    A = 1
    host = make_rows(16, A, "own", 4, False, 50)
    f = fields(4, False)
    got, over, table = run_hash(host, A, f, False, device, M=4)
    assert over
    assert len(got) <= 4
    assert int(table.flag[0].item()) == 0
    assert bool((table.keys[:4] == -1).all())
    # the same table object takes a query that fits afterwards
    small = make_rows(3, A, "own", 4, False, 51)
    out = H.distinct_regroup(_upload(small, A, False, device), 3, f, table)
    G, over = out.count()
    assert (G, over) == (3, False)
    _same(_as_dict(out.to_host(G)), ref_regroup(small, A, f, False), False)
    # and a large enough table holds all 16
    got, over, _ = run_hash(host, A, f, False, device, M=64)
    assert not over
    _same(got, ref_regroup(host, A, f, False), False)


@gpu
@pytest.mark.parametrize("pattern,bits", (("one", 0), ("mixed", 3)))
def test_dense_regroup_is_bitwise_reproducible(device, pattern, bits):
    """Non-integer sums: two runs over the same input give the same bits (no atomics, a fixed
    reduction order), close to the float64 reference."""
    A, n = 3, 5000
    host = make_rows(n, A, pattern, bits, True, 60, integer=False)
    f = fields(bits, True)
    g = _upload(host, A, True, device)
    a = H.distinct_regroup_dense(g, n, f).to_host(f.slots)
    b = H.distinct_regroup_dense(g, n, f).to_host(f.slots)
    for k in ("sums", "cnts", "mins", "maxs"):
        assert a[k].tobytes() == b[k].tobytes(), k
    want = ref_regroup(host, A, f, True)
    for o, (s, c, _, _) in want.items():
        assert np.array_equal(a["cnts"][o], c)
        # n partial sums of magnitude ~1e3 each: |error| <= n * eps * sum|v|
        bound = n * np.finfo(np.float64).eps * np.abs(host["sums"]).sum()
        assert np.all(np.abs(a["sums"][o] - s) <= bound)
