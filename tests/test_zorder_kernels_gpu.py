"""The Z-order kernels (csrc/kernels/zorder.hip) through ``K.zorder_keys`` / ``K.zone_minmax`` /
``K.zone_prune`` against the numpy oracle of tests/zorder_ref.py (checked on the CPU in
test_zorder_ref.py), bit for bit: row counts around the wave and the block, 1 to 8 columns of
every supported storage type, nulls, all-null and constant columns, keys that need the shifts,
zone counts around the wave and the 256-zone block, every range-list shape."""
import decimal

import numpy as np
import pyarrow as pa
import pytest

import zorder_ref as R

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 2047, 2049, 70_001]


def _col(values, valid, device, atype=None):
    import torch
    from hyperspace_amd.exec.device_table import DeviceColumn
    a = np.ascontiguousarray(values)
    v = torch.from_numpy(np.ascontiguousarray(valid).astype(np.uint8)).to(device) \
        if valid is not None else None
    return DeviceColumn(torch.from_numpy(a.copy()).to(device), v,
                        atype or pa.from_numpy_dtype(a.dtype))


def _floats(rng, n, dtype):
    v = (rng.standard_normal(n) * 1e3).astype(dtype)
    special = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf], dtype=dtype)
    if n >= 12:
        v[rng.choice(n, 6, replace=False)] = special
    elif n:
        v[0] = special[n % 6]
    return v


def _full(rng, n, dtype):
    info = np.iinfo(dtype)
    v = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    if n >= 2:
        v[[0, n - 1]] = [info.max, info.min]
    return v


def _decimal(rng, n):
    cents = rng.integers(-10 ** 7, 10 ** 7, n)
    arr = pa.array([decimal.Decimal(int(c)) / 100 for c in cents], pa.decimal128(10, 2))
    return np.asarray(arr.cast(pa.float64()))


# (name, values(rng, n), has nulls, arrow type or None)
POOL = [
    ("i32_nulls", lambda r, n: r.integers(0, 10 ** 6, n).astype(np.int32), True, None),
    ("f64_special", lambda r, n: _floats(r, n, np.float64), False, None),
    ("i64_full", lambda r, n: _full(r, n, np.int64), False, None),
    ("date32", lambda r, n: r.integers(8000, 10_500, n).astype(np.int32), False, pa.date32()),
    ("i8", lambda r, n: _full(r, n, np.int8), True, None),
    ("timestamp", lambda r, n: r.integers(0, 2 ** 50, n), False, pa.timestamp("us")),
    ("f32_special_nulls", lambda r, n: _floats(r, n, np.float32), True, None),
    ("i16", lambda r, n: _full(r, n, np.int16), False, None),
    ("decimal_10_2", _decimal, True, pa.decimal128(10, 2)),
    ("all_null", lambda r, n: np.zeros(n, dtype=np.int32), "all", None),
    ("constant", lambda r, n: np.full(n, -7, dtype=np.int16), False, None),
]


def _make(entry, n, seed):
    name, gen, nulls, atype = entry
    rng = np.random.default_rng(seed)
    vals = gen(rng, n)
    valid = None
    if nulls == "all":
        valid = np.zeros(n, dtype=np.uint8)
    elif nulls:
        valid = (rng.random(n) > 0.2).astype(np.uint8)
    return vals, valid, atype


def _column_sets(k):
    m = len(POOL)
    if k == 8:
        return [list(range(8)), list(range(m - 8, m))]
    return [[(s + i) % m for i in range(k)] for s in range(0, m, k)]


def _check_keys(cols, device):
    from hyperspace_amd.exec.zorder import device_keys
    want = R.keys([(v, valid) for v, valid, _ in cols])
    got = device_keys([_col(v, valid, device, at) for v, valid, at in cols]).cpu().numpy()
    assert got.dtype == np.int64 and (got >= 0).all()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("n", ROWS)
def test_keys_equal_reference(device, n, k):
    for at in _column_sets(k):
        _check_keys([_make(POOL[i], n, 1000 * k + i) for i in at], device)


def test_keys_with_shifts_and_uneven_levels(device):
    """Sum(need) > 63 (every column is shifted) and columns of 3, 8 and 20 bits that leave the
    interleave at different levels."""
    from hyperspace_amd.index import zorder as ZO
    n = 5000
    wide = [_make(POOL[i], n, 77 + i) for i in (2, 1, 5)]          # int64 full, f64, timestamp
    needs = [R.column_range((v, valid))[1] for v, valid, _ in wide]
    bits = R.bit_allocation(needs)
    assert sum(needs) > 63 and sum(bits) == 63 and all(b < x for b, x in zip(bits, needs))
    _check_keys(wide, device)
    rng = np.random.default_rng(5)
    uneven = [(rng.integers(0, 8, n).astype(np.int8), None, None),
              (rng.integers(0, 2 ** 20, n).astype(np.int32), None, None),
              (rng.integers(-128, 128, n).astype(np.int16), (rng.random(n) > 0.3), None)]
    needs = [R.column_range((v, valid))[1] for v, valid, _ in uneven]
    assert needs == [3, 20, 8] and R.bit_allocation(needs) == needs
    assert ZO.allocate_bits(needs) == needs
    _check_keys(uneven, device)


def test_key_wrapper_refuses_bad_input(device):
    from hyperspace_amd.ops import kernels as K
    c = _col(np.arange(10, dtype=np.int32), None, device)
    with pytest.raises(ValueError):
        K.zorder_keys([c] * 9, [0] * 9, [0] * 9, [1] * 9)
    with pytest.raises(ValueError):
        K.zorder_keys([c, c], [0, 0], [0, 0], [32, 32])           # 64 bits
    with pytest.raises(ValueError):
        K.zorder_keys([c, _col(np.arange(9, dtype=np.int32), None, device)], [0, 0], [0, 0],
                      [4, 4])


# -- zone maps ---------------------------------------------------------------------------------
def _maps_np(maps):
    return tuple(m.cpu().numpy().view(t) for m, t in zip(maps, (np.uint64, np.uint64, np.int64)))


@pytest.mark.parametrize("n,zone", [(1000, 128), (2048, 256), (100, 256), (70_001, 2048), (0, 64),
                                    (1, 1)])
def test_zone_minmax_equals_numpy(device, n, zone):
    from hyperspace_amd.ops import kernels as K
    cols = [_make(POOL[i], n, 31 + i) for i in (0, 1, 2, 6, 4, 7, 9)]
    if n >= 3 * zone:
        cols[0][1][zone:2 * zone] = 0                      # zone 1 of column 0: all null
    want = R.zone_maps([(v, valid) for v, valid, _ in cols], zone)
    got = _maps_np(K.zone_minmax([_col(v, valid, device, at) for v, valid, at in cols], zone))
    nz = -(-n // zone)
    for g, w in zip(got, want):
        assert g.shape == (len(cols), nz)
        assert (g == w).all()
    if n >= 3 * zone:
        assert got[2][0, 1] == 0 and got[0][0, 1] > got[1][0, 1]
    if nz:
        assert (got[2][6] == 0).all() and (got[0][6] > got[1][6]).all()      # all-null column


def test_column_ranges_use_sortable_images(device):
    """NaN and -0.0 keep their own images (nothing canonicalised), nulls do not count."""
    from hyperspace_amd.ops import kernels as K
    f = np.array([1.5, -np.nan, np.nan, -0.0, 0.0, 7.0], dtype=np.float64)
    valid = np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8)
    i = np.array([5, -3, 9, 0, 2, 100], dtype=np.int16)
    got = K.zorder_column_ranges([_col(f, valid, device), _col(i, valid, device),
                                  _col(i, np.zeros(6, np.uint8), device)])
    img = R.image(f)[:5]
    assert got[0] == (int(img.min()), int(img.max()))
    assert got[0][0] == int(R.image(np.array([-np.nan]))[0])
    assert got[1] == (int(R.image(np.array([-3], np.int16))[0]),
                      int(R.image(np.array([9], np.int16))[0]))
    assert got[2] is None


# -- zone pruning ------------------------------------------------------------------------------
ZR = 4


def _prune_table(nz):
    """Columns whose zone maps are easy to aim at: per zone z, a = z, b = z % 2, c = (z // 3) % 2,
    d..h spread rows; the last zone is partial and zone 2 of ``a`` is all null."""
    n = nz * ZR - 1
    z = np.arange(n) // ZR
    rng = np.random.default_rng(nz)
    cols = [(z.astype(np.int32), np.ones(n, np.uint8)),
            ((z % 2).astype(np.int8), None),
            (((z // 3) % 2).astype(np.int16), None),
            (z.astype(np.float64) * 0.5, None),
            (rng.integers(0, 100, n), None),
            ((z * 1000 + rng.integers(0, 1000, n)).astype(np.int64), None),
            (rng.standard_normal(n).astype(np.float32), None),
            ((nz - z).astype(np.int32), None)]
    if nz > 2:
        cols[0][1][2 * ZR:3 * ZR] = 0
    return n, cols


def _img(v, dtype):
    return int(R.image(np.array([v], dtype=dtype))[0])


def _prune_cases(nz):
    i32 = lambda v: _img(v, np.int32)           # noqa: E731
    full = lambda j, dt: (j, _img(np.iinfo(dt).min, dt), _img(np.iinfo(dt).max, dt))   # noqa: E731
    cases = {
        "nothing": [(0, i32(nz + 10), i32(nz + 20))],
        "everything": [(1, _img(0, np.int8), _img(1, np.int8))],
        "unconstrained": [],
        "alternating": [(1, _img(1, np.int8), _img(1, np.int8))],
        "runs_of_three": [(2, _img(1, np.int16), _img(1, np.int16))],
        "last_zone_clipped": [(0, i32(nz - 1), i32(nz + 5))],
        "null_zone_dropped": [(0, i32(0), i32(nz))],
        "empty_interval": [(0, i32(3), i32(2))],
        "across_wave_and_block": [(0, i32(60), i32(70)), (7, i32(0), i32(nz))],
        "block_edge_run": [(0, i32(250), i32(260))],
        "two_columns": [(0, i32(1), i32(max(1, nz - 2))), (1, _img(0, np.int8), _img(0, np.int8))],
        "eight_columns": [
            (0, i32(0), i32(nz)), full(1, np.int8), (2, _img(0, np.int16), _img(0, np.int16)),
            (3, _img(1.0, np.float64), _img(1e9, np.float64)), full(4, np.int64),
            (5, _img(3000, np.int64), _img(2 ** 62, np.int64)),
            (6, _img(-np.inf, np.float32), _img(np.inf, np.float32)),
            (7, i32(2), i32(nz))],
    }
    return cases


@pytest.mark.parametrize("nz", [5, 64, 65, 1025])
def test_zone_prune_equals_reference(device, nz):
    from hyperspace_amd.ops import kernels as K
    n, cols = _prune_table(nz)
    want_maps = R.zone_maps(cols, ZR)
    maps = K.zone_minmax([_col(v, valid, device) for v, valid in cols], ZR)
    assert all((g == w).all() for g, w in zip(_maps_np(maps), want_maps))
    seen = set()
    for name, cons in _prune_cases(nz).items():
        ranges, kept = R.prune(*want_maps, n, ZR, {j: (lo, hi) for j, lo, hi in cons})
        rstart, rlen, counts = K.zone_prune(maps, n, ZR, cons)
        ws, wl = R.padded(ranges, nz)
        assert rstart.cpu().numpy().tolist() == ws.tolist(), name
        assert rlen.cpu().numpy().tolist() == wl.tolist(), name
        assert counts.cpu().numpy().tolist() == [len(ranges), kept], name
        seen.add((len(ranges), kept))
        if name == "everything" or name == "unconstrained":
            assert ranges == [(0, n)]
        if name == "nothing" or name == "empty_interval":
            assert ranges == []
        if name == "alternating":
            assert len(ranges) == nz // 2                   # the most ranges a table can have
        if name == "last_zone_clipped":
            assert ranges == [((nz - 1) * ZR, ZR - 1)]
    assert len(seen) >= 6


def test_zone_prune_wrapper_refuses_mismatch(device):
    from hyperspace_amd.ops import kernels as K
    n, cols = _prune_table(5)
    maps = K.zone_minmax([_col(v, valid, device) for v, valid in cols], ZR)
    with pytest.raises(ValueError):
        K.zone_prune(maps, n + ZR, ZR, [])                  # another zone count
    with pytest.raises(ValueError):
        K.zone_prune(maps, n, ZR, [(8, 0, 1)])              # no such map column
