"""The numpy key-order reference (tests/order_ref.py) against hand-written ladders, the host
mirror ``K.sortable_image`` and Python's ``sorted``.  No GPU."""
import numpy as np
import pytest

from order_ref import (SPECIAL_F32, SPECIAL_F64, ref_image, ref_probe, ref_ranges,
                       ref_sort_perm)

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max

# strictly ascending in the key order, written by hand
LADDERS = {
    "I8": np.array([-128, -127, -1, 0, 1, 126, 127], np.int8),
    "I16": np.array([-32768, -32767, -256, -1, 0, 1, 255, 256, 32766, 32767], np.int16),
    "I32": np.array([-2**31, -2**31 + 1, -65536, -1, 0, 1, 65535, 2**31 - 2, 2**31 - 1], np.int32),
    "I64": np.array([I64_MIN, I64_MIN + 1, -2**32, -2**31, -1, 0, 1, 2**31, 2**32, I64_MAX - 1,
                     I64_MAX], np.int64),
    "BOOL": np.array([0, 1], np.uint8),
    "U32": np.array([0, 1, 2**31 - 1, 2**31, 2**32 - 1], np.uint32),
    "F32": SPECIAL_F32,
    "F64": SPECIAL_F64,
}


@pytest.mark.parametrize("kind", sorted(LADDERS))
def test_ref_image_strictly_monotone_on_ladder(kind):
    img = ref_image(LADDERS[kind], kind)
    assert img.dtype == np.uint64
    assert all(int(a) < int(b) for a, b in zip(img[:-1], img[1:])), img


def test_special_floats_are_what_they_claim():
    for sp, tiny, big in ((SPECIAL_F64, 5e-324, np.finfo(np.float64).max),
                          (SPECIAL_F32, np.float32(1e-45), np.finfo(np.float32).max)):
        assert len(sp) == 13
        assert np.isnan(sp[[0, 1, 11, 12]]).all() and not np.isnan(sp[2:11]).any()
        assert np.signbit(sp[[0, 1]]).all() and not np.signbit(sp[[11, 12]]).any()
        assert sp[2] == -np.inf and sp[10] == np.inf
        assert sp[3] == -big and sp[9] == big
        assert sp[4] == -tiny and sp[7] == tiny and sp[4] != 0 and sp[7] != 0
        assert sp[5] == 0 and np.signbit(sp[5]) and sp[6] == 0 and not np.signbit(sp[6])
        assert sp[8] == 1.5
        # between the two zeros and apart from NaN the key order is the numeric order
        assert (np.diff(sp[2:11].astype(np.float64)) >= 0).all()


@pytest.mark.parametrize("kind", sorted(LADDERS))
def test_ref_image_equals_host_mirror_on_literals(kind):
    from hyperspace_amd.ops import _lib as NL, kernels as K
    rng = np.random.default_rng(1)
    vals = LADDERS[kind]
    if kind in ("F32", "F64"):
        more = rng.normal(size=50) * 10.0 ** rng.integers(-30, 30, 50)
    elif kind == "BOOL":
        more = np.zeros(0)
    else:
        info = np.iinfo(vals.dtype)
        more = rng.integers(info.min, info.max, 50, dtype=vals.dtype, endpoint=True)
    vals = np.concatenate([vals, more.astype(vals.dtype)])
    img = ref_image(vals, kind)
    for v, i in zip(vals, img):
        lit = float(v) if kind in ("F32", "F64") else int(v)
        assert K.sortable_image(lit, getattr(NL, kind)) == int(i), (kind, v)


def test_ref_sort_perm_equals_sorted_tuples():
    rng = np.random.default_rng(2)
    n = 500
    bucket = rng.integers(0, 3, n).astype(np.int32)
    a = rng.integers(-3, 3, n).astype(np.int64)
    an = rng.random(n) < 0.2
    a[an] = I64_MIN                       # garbage under nulls must not matter
    f = rng.choice(np.concatenate([SPECIAL_F64, [2.5, -2.5]]), n)
    fn = rng.random(n) < 0.1
    c = rng.integers(-2, 2, n).astype(np.int8)
    ia, if_, ic = ref_image(a, "I64"), ref_image(f, "F64"), ref_image(c, "I8")

    def tup(r):
        return (int(bucket[r]), not an[r], 0 if an[r] else int(ia[r]), not fn[r],
                0 if fn[r] else int(if_[r]), True, int(ic[r]))

    want = sorted(range(n), key=lambda r: tup(r) + (r,))
    got = ref_sort_perm([(a, an), (f, fn), (c, None)], leading=bucket)
    assert got.tolist() == want
    # init: ties keep the order of the given permutation
    p = rng.permutation(n)
    pos = np.empty(n, np.int64)
    pos[p] = np.arange(n)
    want = sorted(range(n), key=lambda r: tup(r) + (int(pos[r]),))
    assert ref_sort_perm([(a, an), (f, fn), (c, None)], leading=bucket, init=p).tolist() == want
    # without nulls or a leading key it is numpy's stable argsort
    assert ref_sort_perm([(c, None)]).tolist() == np.argsort(c, kind="stable").tolist()


def test_ref_ranges_and_probe_against_a_row_loop():
    rng = np.random.default_rng(3)
    sizes = [0, 1, 5, 40, 0, 17]
    off = np.concatenate([[0], np.cumsum(sizes)])
    vals, nulls = [], []
    for m in sizes:
        k = int(rng.integers(0, m + 1)) if m else 0
        vals.append(np.concatenate([np.full(k, 99, np.int32),
                                    np.sort(rng.integers(-5, 6, m - k)).astype(np.int32)]))
        nulls.append(np.arange(m) < k)
    vals, nulls = np.concatenate(vals), np.concatenate(nulls)
    buckets = [5, 0, 3, 3, 2]
    for lo in (None, -7, -5, 0, 3, 5, 7):
        for hi in (None, -7, -5, 0, 3, 5, 7):
            for li in (True, False):
                for hi_ in (True, False):
                    rs, rl, rb = ref_ranges(vals, nulls, off, buckets,
                                            None if lo is None else ref_image([lo], "I32")[0], li,
                                            None if hi is None else ref_image([hi], "I32")[0], hi_)
                    assert rb.tolist() == buckets and (rl >= 0).all()
                    for s, ln, b in zip(rs, rl, rb):
                        m = np.zeros(len(vals), bool)
                        m[off[b]:off[b + 1]] = True
                        m &= ~nulls
                        if lo is not None:
                            m &= (vals >= lo) if li else (vals > lo)
                        if hi is not None:
                            m &= (vals <= hi) if hi_ else (vals < hi)
                        assert ln == m.sum()
                        if ln:
                            assert np.nonzero(m)[0].tolist() == list(range(s, s + ln))
                        else:
                            assert off[b] <= s <= off[b + 1]
    pk = ref_image(np.array([0, -6, 9, 2], np.int32), "I32")
    rs, rl, rb = ref_probe(vals, nulls, off, [3, 3, 5, 0], pk)
    for s, ln, b, k in zip(rs, rl, rb, [0, -6, 9, 2]):
        m = np.zeros(len(vals), bool)
        m[off[b]:off[b + 1]] = True
        m &= ~nulls & (vals == k)
        assert ln == m.sum() and (not ln or np.nonzero(m)[0][0] == s)
