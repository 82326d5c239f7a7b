"""The sketch kernels (csrc/kernels/sketch.hip) through ``K.sketch_minmax`` / ``K.sketch_bloom`` /
``K.sketch_hash_entries`` against the numpy reference of tests/sketch_ref.py (checked on the CPU
in test_sketch_ref.py), bit for bit: file sizes around the wave and the slab, several files per
call so that slabs start at unaligned rows, null masks, type extremes, NaN / inf / -0.0, filter
sizes on both sides of the LDS limit."""
import functools

import numpy as np
import pyarrow as pa
import pytest

import sketch_ref as R

gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _limits():
    from hyperspace_amd.ops import kernels as K
    return K.sketch_slab_rows(), K.sketch_bloom_lds_words()


def _sizes():
    s, _ = _limits()
    return [0, 1, 63, 64, 65, s - 1, s, s + 1, 2 * s + 7]


def _mixed():
    # odd sizes first, so every later file and most slabs start at an unaligned row
    return [5] + _sizes() + [0, 3, 64]


def _col(values, valid, device, atype=None):
    import torch
    from hyperspace_amd.exec.device_table import DeviceColumn
    a = np.ascontiguousarray(values)
    v = torch.from_numpy(np.ascontiguousarray(valid).copy()).to(device) \
        if valid is not None else None
    return DeviceColumn(torch.from_numpy(a.copy()).to(device), v,
                        atype or pa.from_numpy_dtype(a.dtype))


def _values(dtype, n, seed):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "i":
        info = np.iinfo(dtype)
        v = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        special = [info.min, info.max, 0, -1]
    else:
        v = (rng.standard_normal(n) * 1e3).astype(dtype)
        special = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, np.finfo(dtype).max,
                   np.finfo(dtype).tiny]
    if n:
        at = rng.integers(0, n, 4 * len(special))
        v[at] = np.array(special * 4, dtype=dtype)
    return v


def _valid(n, files, seed, all_null_file):
    rng = np.random.default_rng(seed)
    valid = (rng.random(n) < 0.7).astype(np.uint8)
    starts = np.concatenate([[0], np.cumsum(files)])
    valid[starts[all_null_file]:starts[all_null_file + 1]] = 0
    return valid


def _ref_minmax(values, valid, files):
    """(min image bits, max image bits, counts): expected results as raw bits, NaN canonical."""
    dtype = values.dtype
    starts = np.concatenate([[0], np.cumsum(files)]).astype(np.int64)
    mins, maxs, cnts = [], [], []
    for a, b in zip(starts[:-1], starts[1:]):
        v = values[a:b]
        if valid is not None:
            v = v[valid[a:b] != 0]
        cnts.append(len(v))
        if not len(v):
            mins.append(None)
            maxs.append(None)
            continue
        if dtype.kind == "f":
            nan = np.isnan(v)
            rest = v[~nan] + dtype.type(0)
            mx = dtype.type(np.nan) if nan.any() else rest.max()
            mn = rest.min() if len(rest) else dtype.type(np.nan)
        else:
            mn, mx = v.min(), v.max()
        mins.append(mn)
        maxs.append(mx)
    return mins, maxs, cnts


def _bits(x, dtype):
    dtype = np.dtype(dtype)
    a = np.array([x], dtype=dtype)
    if dtype.kind == "f" and np.isnan(a[0]):
        return {4: 0x7FC00000, 8: 0x7FF8000000000000}[dtype.itemsize]
    return int(a.view(f"u{dtype.itemsize}")[0])


def _check_minmax(K, values, valid, files, device):
    mn, mx, cnt = K.sketch_minmax(_col(values, valid, device), files)
    wmn, wmx, wcnt = _ref_minmax(values, valid, files)
    assert cnt.tolist() == wcnt
    assert mn.dtype == values.dtype and mx.dtype == values.dtype
    for f in range(len(files)):
        if wcnt[f]:
            assert _bits(mn[f], values.dtype) == _bits(wmn[f], values.dtype), (f, mn[f], wmn[f])
            assert _bits(mx[f], values.dtype) == _bits(wmx[f], values.dtype), (f, mx[f], wmx[f])
    return mn, mx, cnt


@gpu
def test_limits_are_what_the_sizes_assume(device):
    slab, lds_words = _limits()
    assert slab >= 1024 and slab % 64 == 0
    # two workgroups' private filters share one CU's 160 KiB of LDS
    assert 1 <= lds_words and 2 * 8 * lds_words <= 160 * 1024
    from hyperspace_amd.ops import kernels as K
    slabs, off = K.sketch_slabs([0, 1, slab, slab + 1], slab)
    assert off.tolist() == [0, 0, 1, 2, 4]
    assert slabs.tolist() == [[1, 0, 1], [2, 1, slab + 1], [3, slab + 1, 2 * slab + 1],
                              [3, 2 * slab + 1, 2 * slab + 2]]


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
@pytest.mark.parametrize("dtype", ["int8", "int16", "int32", "int64", "float32", "float64"])
def test_minmax_mixed_files(device, dtype, masked):
    from hyperspace_amd.ops import kernels as K
    files = _mixed()
    n = sum(files)
    values = _values(dtype, n, 11)
    # file 6 (slab - 1 rows) holds no non-null value
    valid = _valid(n, files, 12, 6) if masked else None
    _, _, cnt = _check_minmax(K, values, valid, files, device)
    if masked:
        assert cnt[6] == 0 and cnt[9] > 0


@gpu
def test_minmax_single_files_and_specials(device):
    from hyperspace_amd.ops import kernels as K
    for n in _sizes():
        _check_minmax(K, _values("int32", n, n), None, [n], device)
    # orderings, spelled out: NaN above +inf, -0.0 stored as +0.0, a NaN-only file
    v = np.array([1.0, np.nan, -np.inf, -0.0, np.nan, np.nan, -0.0, -3.0], dtype=np.float64)
    mn, mx, cnt = K.sketch_minmax(_col(v, None, device), [3, 1, 2, 2])
    assert cnt.tolist() == [3, 1, 2, 2]
    assert mn[0] == -np.inf and np.isnan(mx[0])
    assert _bits(mn[1], "float64") == 0 and _bits(mx[1], "float64") == 0
    assert np.isnan(mn[2]) and np.isnan(mx[2])
    assert mn[3] == -3.0 and _bits(mx[3], "float64") == 0
    v32 = np.array([-0.0, np.inf, np.nan], dtype=np.float32)
    mn, mx, _ = K.sketch_minmax(_col(v32, None, device), [1, 2])
    assert _bits(mn[0], "float32") == 0 and mn[1] == np.inf and np.isnan(mx[1])
    with pytest.raises(ValueError):
        K.sketch_minmax(_col(v32, None, device), [1, 1])


@functools.lru_cache(maxsize=None)
def _bloom_keys():
    files = _mixed()
    n = sum(files)
    keys = _values("int64", n, 21)
    h1, h2 = R.item_hashes_np(keys)
    return files, keys, h1, h2


def _ref_bloom(h1, h2, valid, files, nw, k):
    starts = np.concatenate([[0], np.cumsum(files)]).astype(np.int64)
    out = np.zeros((len(files), nw), dtype=np.uint64)
    for f, (a, b) in enumerate(zip(starts[:-1], starts[1:])):
        sel = slice(a, b) if valid is None else np.arange(a, b)[valid[a:b] != 0]
        out[f] = R.bloom_words_np(h1[sel], h2[sel], nw, k)
    return out


def _word_counts():
    _, lds = _limits()
    return [1, 3, 150, lds, lds + 1]


@gpu
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("which", range(5), ids=["1w", "3w", "150w", "lds", "lds+1"])
def test_bloom_mixed_files(device, which, k):
    from hyperspace_amd.ops import kernels as K
    nw = _word_counts()[which]
    files, keys, h1, h2 = _bloom_keys()
    assert any((R.combined_np(h1, h2, i) < 0).any() for i in range(1, k + 1))
    got = K.sketch_bloom(_col(keys, None, device), files, nw, k).cpu().numpy().view(np.uint64)
    assert got.shape == (len(files), nw)
    assert np.array_equal(got, _ref_bloom(h1, h2, None, files, nw, k))
    assert not got[1].any() and not got[-3].any()        # files without rows


@gpu
@pytest.mark.parametrize("which", [2, 4], ids=["150w", "lds+1"])
def test_bloom_masked(device, which):
    from hyperspace_amd.ops import kernels as K
    nw = _word_counts()[which]
    files, keys, h1, h2 = _bloom_keys()
    valid = _valid(len(keys), files, 22, 6)
    got = K.sketch_bloom(_col(keys, valid, device), files, nw, 7).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, _ref_bloom(h1, h2, valid, files, nw, 7))
    assert not got[6].any()                               # the all-null file


@gpu
def test_bloom_single_files_and_narrow_integers(device):
    from hyperspace_amd.ops import kernels as K
    for n in _sizes():
        keys = _values("int64", n, 100 + n)
        h1, h2 = R.item_hashes_np(keys)
        got = K.sketch_bloom(_col(keys, None, device), [n], 150, 7).cpu().numpy().view(np.uint64)
        assert np.array_equal(got[0], R.bloom_words_np(h1, h2, 150, 7)), n
    # the worked positions of the definition
    got = K.sketch_bloom(_col(np.array([0, 1, -1], dtype=np.int64), None, device), [1, 1, 1],
                         150, 7).cpu().numpy().view(np.uint64)
    for row, key in zip(got, (0, 1, -1)):
        assert np.array_equal(row, R.bloom_words([key], 150, 7))
    # narrower integers hash as their int64 value
    for dtype in ("int8", "int16", "int32"):
        v = _values(dtype, 1000, 31)
        h1, h2 = R.item_hashes_np(v.astype(np.int64))
        got = K.sketch_bloom(_col(v, None, device), [1000], 15, 7).cpu().numpy().view(np.uint64)
        assert np.array_equal(got[0], R.bloom_words_np(h1, h2, 15, 7)), dtype


# UTF-8 lengths 0, 1, 3, 4, 5, 17 (and 6): tails of 1 - 3 bytes at or above 0x80, a high byte
# inside an aligned word
ENTRIES = ["", "a", "€", "abé", "abcé", "abcdefghijklmnoé", "zzzzÿ"]


@gpu
def test_hash_entries_and_dictionary_codes(device):
    from hyperspace_amd.exec.like import device_dictionary
    from hyperspace_amd.ops import kernels as K
    from hyperspace_amd.utils import murmur3
    raw = [e.encode("utf-8") for e in ENTRIES]
    assert sorted(len(b) for b in raw) == [0, 1, 3, 4, 5, 6, 17]
    assert all(any(c >= 0x80 for c in b) for b in raw if len(b) > 1)
    dictionary = pa.array(sorted(ENTRIES, key=lambda e: e.encode("utf-8")), pa.string())
    ents = K.sketch_hash_entries(device_dictionary(dictionary, device, cache=False))
    got = ents.cpu().numpy().view(np.uint32)
    for row, e in zip(got, dictionary.to_pylist()):
        b = e.encode("utf-8")
        h1 = murmur3.hash_bytes(b, 0)
        assert (int(row[0]), int(row[1])) == (h1, murmur3.hash_bytes(b, h1)), e
        assert (int(row[0]), int(row[1])) == R.item_hashes(b), e
    # rows gather their pair by dictionary code
    rng = np.random.default_rng(41)
    files = [7, 0, 300, 65]
    codes = rng.integers(0, len(dictionary), sum(files)).astype(np.int32)
    valid = (rng.random(len(codes)) < 0.8).astype(np.uint8)
    col = _col(codes, valid, device, pa.string())
    got = K.sketch_bloom(col, files, 3, 7, ents).cpu().numpy().view(np.uint64)
    words = dictionary.to_pylist()
    starts = np.concatenate([[0], np.cumsum(files)])
    for f, (a, b) in enumerate(zip(starts[:-1], starts[1:])):
        items = [words[c] for c, ok in zip(codes[a:b], valid[a:b]) if ok]
        assert np.array_equal(got[f], R.bloom_words(items, 3, 7)), f
