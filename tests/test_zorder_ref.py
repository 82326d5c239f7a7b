"""Self-checks of the Z-order oracle (tests/zorder_ref.py) and its agreement with the host
builder's vectorised Z-address (index/zorder.py)."""
import numpy as np
import pytest

import zorder_ref as R
from hyperspace_amd.index import zorder as ZO


def test_single_column_key_order_is_plain_sort_order():
    rng = np.random.default_rng(1)
    v = rng.integers(-10 ** 6, 10 ** 6, 5000).astype(np.int32)
    valid = rng.random(5000) > 0.1
    got = R.order([(v, valid)])
    # nulls (code 0) tie with the minimum; among the non-null rows the order is the value order
    nn = got[valid[got]]
    assert (np.diff(v[nn].astype(np.int64)) >= 0).all()
    want = np.argsort(np.where(valid, v.astype(np.int64), v[valid].min()), kind="stable")
    assert (got == want).all()


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64])
def test_key_is_monotone_in_each_column(dtype):
    rng = np.random.default_rng(2)
    n = 400
    if np.dtype(dtype).kind == "f":
        x = np.sort(rng.standard_normal(n).astype(dtype))
    else:
        info = np.iinfo(dtype)
        x = np.sort(rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True))
    fixed = np.full(n, 12345, dtype=np.int32)
    spread = np.array([0, 99999], dtype=np.int32)     # gives the fixed column bits of its own
    for cols in ([(np.concatenate([x, x[:2]]), None), (np.concatenate([fixed, spread]), None)],
                 [(np.concatenate([fixed, spread]), None), (np.concatenate([x, x[:2]]), None)]):
        k = R.keys(cols)[:n]
        assert (np.diff(k) >= 0).all()
        assert (k >= 0).all()


def test_bit_allocation_hand_cases():
    assert R.bit_allocation([3, 3]) == [3, 3]
    assert R.bit_allocation([0, 5]) == [0, 5]
    assert R.bit_allocation([64]) == [63]
    assert R.bit_allocation([40, 40]) == [32, 31]            # 63 bits, first column first
    assert R.bit_allocation([2, 64, 64]) == [2, 31, 30]      # unequal needs
    assert R.bit_allocation([64] * 8) == [8, 8, 8, 8, 8, 8, 8, 7]
    assert R.bit_allocation([0, 0]) == [0, 0]
    for needs in ([3, 3], [0, 5], [64], [40, 40], [2, 64, 64], [64] * 8, [1, 20, 64, 7]):
        assert ZO.allocate_bits(needs) == R.bit_allocation(needs)
        assert sum(R.bit_allocation(needs)) <= 63


def test_interleave_hand_case():
    # a: need 2 (0..3), b: need 1 (0..1): bits a1 b0 a0
    a = np.array([0, 1, 2, 3, 3], dtype=np.int8)
    b = np.array([0, 1, 0, 1, 0], dtype=np.int8)
    assert R.keys([(a, None), (b, None)]).tolist() == [0b000, 0b011, 0b100, 0b111, 0b101]
    # a null contributes code 0 and does not move min / max
    valid = np.array([1, 1, 1, 1, 0], dtype=np.uint8)
    assert R.keys([(a, valid), (b, None)]).tolist() == [0b000, 0b011, 0b100, 0b111, 0b000]


def test_shifted_columns_and_all_null_and_constant():
    rng = np.random.default_rng(3)
    n = 1000
    wide = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64)
    f = rng.standard_normal(n)
    f[:6] = [np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf]
    const = np.full(n, 7, dtype=np.int16)
    nulls = (np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8))
    cols = [(wide, None), (f, None), (const, None), nulls]
    k = R.keys(cols)
    assert (k >= 0).all()
    assert (k == R.keys([(wide, None), (f, None)])).all()    # need 0 columns add no bits
    assert (ZO.host_keys(cols) == k).all()


def test_host_keys_equal_reference_on_mixed_columns():
    rng = np.random.default_rng(4)
    n = 3000
    cols = [(rng.integers(0, 10 ** 6, n).astype(np.int32), rng.random(n) > 0.1),
            (rng.integers(0, 2500, n).astype(np.int32), None),
            (rng.standard_normal(n).astype(np.float32), rng.random(n) > 0.5),
            (rng.integers(-5, 5, n).astype(np.int8), None)]
    assert (ZO.host_keys(cols) == R.keys(cols)).all()


def test_zone_maps_and_prune():
    n, zr = 1000, 128                       # 8 zones, the last one partial
    a = np.arange(n, dtype=np.int32)
    valid = np.ones(n, dtype=np.uint8)
    valid[256:384] = 0                      # zone 2 all null
    mn, mx, cnt = R.zone_maps([(a, valid)], zr)
    assert cnt[0].tolist() == [128, 128, 0, 128, 128, 128, 128, 104]
    assert mn[0, 2] > mx[0, 2]
    img = lambda v: int(R.image(np.array([v], dtype=np.int32))[0])      # noqa: E731
    ranges, kept = R.prune(mn, mx, cnt, n, zr, {0: (img(100), img(600))})
    assert ranges == [(0, 256), (384, 256)] and kept == 4               # zone 2 dropped
    ranges, kept = R.prune(mn, mx, cnt, n, zr, {0: (img(900), img(5000))})
    assert ranges == [(896, 104)] and kept == 1                         # clipped to n
    assert R.prune(mn, mx, cnt, n, zr, {0: (5, 4)}) == ([], 0)
    assert R.prune(mn, mx, cnt, n, zr, {}) == ([(0, 1000)], 8)
