"""The fixed-shape kernels of csrc/kernels/hash_agg.hip and csrc/kernels/topk_runs.hip, each
against a plain numpy reference: table merge / extract / reset, the order-preserving images, the
3-level radix select, the candidate take, the run-top-K threshold / images / gather, and the
functional-dependency lookup.  Every comparison is exact (inputs are chosen so that it can be).

The numpy references are checked on the CPU first (section 0); everything else needs the GPU.
"""
import ctypes as C
import functools
import time

import numpy as np
import pyarrow as pa
import pytest

from hyperspace_amd.exec import hash_agg as H
from hyperspace_amd.ops import _lib as NL
from hyperspace_amd.utils import murmur3

gpu = pytest.mark.gpu

_U = np.uint64
_TOP = _U(1 << 63)
_FULL = _U(0xFFFFFFFFFFFFFFFF)
_NAN_IMG = _U(0xFFFFFFFFFFFFFFFE)
_I64_MIN = -(1 << 63)
_I64_MAX = (1 << 63) - 1
_DBL_MAX = np.finfo(np.float64).max
_DBL_MIN = np.finfo(np.float64).tiny          # smallest normal
_DENORM = 5e-324
_NEG_NAN = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
SPECIALS = np.array([np.nan, _NEG_NAN, np.inf, -np.inf, -0.0, 0.0, _DENORM, -_DENORM,
                     _DBL_MIN, -_DBL_MIN, _DBL_MAX, -_DBL_MAX, 1.5, -1.5], dtype=np.float64)


# ------------------------------------------------------------------------------------------------
# 0. numpy references
# ------------------------------------------------------------------------------------------------
def ref_dimg(x) -> np.ndarray:
    """Ascending order-preserving u64 image of doubles: -0.0 as 0.0, every NaN last."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = np.where(x == 0.0, 0.0, x).view(np.uint64)
    img = np.where((b >> _U(63)) != 0, ~b, b | _TOP)
    return np.where(np.isnan(x), _NAN_IMG, img).astype(np.uint64)


def ref_simg(x) -> np.ndarray:
    """The "larger is better" signed image of doubles (wth, dmx, ctl)."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return np.where(b >= 0, b, b ^ np.int64(_I64_MAX))


def ref_unsimg(s) -> np.ndarray:
    s = np.ascontiguousarray(s, dtype=np.int64)
    return np.ascontiguousarray(np.where(s >= 0, s, s ^ np.int64(_I64_MAX))).view(np.float64)


def ref_slot_image(v) -> np.ndarray:
    """Unsigned smallest-first slot image (vimg) of larger-is-better values."""
    return ~(ref_simg(v).view(np.uint64) ^ _TOP)


REF_EMPTY = int(ref_slot_image(np.array([-np.inf]))[0])


def ref_select(img: np.ndarray, k: int) -> np.ndarray:
    """Rows whose image's top 36 bits are <= those of the k-th smallest image."""
    kth = np.partition(img, k - 1)[k - 1]
    return np.flatnonzero((img >> _U(28)) <= (kth >> _U(28)))


def test_ref_dimg_orders_like_spark():
    rng = np.random.default_rng(11)
    v = np.concatenate([SPECIALS, rng.normal(size=50) * 1e3, rng.normal(size=20) * 1e-310])
    v = v[rng.permutation(len(v))]
    img = ref_dimg(v)
    by_img = v[np.argsort(img, kind="stable")]
    assert np.array_equal(by_img, np.sort(v), equal_nan=True)     # numpy sorts NaN last too
    # the ladder: -inf < finite < +inf < NaN, signed zeros equal, every NaN the same
    ladder = np.array([-np.inf, -_DBL_MAX, -1.5, -_DBL_MIN, -_DENORM, 0.0, _DENORM, _DBL_MIN,
                       1.5, _DBL_MAX, np.inf, np.nan])
    li = ref_dimg(ladder)
    assert np.all(li[1:] > li[:-1])
    assert ref_dimg([-0.0])[0] == ref_dimg([0.0])[0] == _TOP
    assert ref_dimg([np.nan])[0] == ref_dimg([_NEG_NAN])[0] == _NAN_IMG
    # 0 and ~0 are the NULL images: no value may take them (ascending or complemented)
    assert not np.any((img == _U(0)) | (img == _FULL))


def test_ref_signed_image_roundtrip_and_empty_pattern():
    rng = np.random.default_rng(12)
    v = np.concatenate([SPECIALS[2:], rng.normal(size=64) * 1e6])
    s = ref_simg(v)
    assert np.array_equal(ref_unsimg(s).view(np.uint64), v.view(np.uint64))
    o = np.argsort(s, kind="stable")
    assert np.all(np.diff(v[o]) >= 0)
    assert ref_simg([-0.0])[0] < ref_simg([0.0])[0]
    # the slot image is smallest-first, and -inf is the empty pattern of the executor
    u = ref_slot_image(v)
    assert np.all(np.diff(v[np.argsort(u, kind="stable")]) <= 0)
    assert REF_EMPTY == H.TopKPlan(0, False, True, 1).empty_image()
    assert H.TopKPlan._unimg(int(ref_simg([-2.5])[0])) == -2.5


def test_ref_select_against_a_sort():
    rng = np.random.default_rng(13)
    img = rng.integers(0, 1 << 40, 500, dtype=np.uint64) << _U(20)
    img[:40] = img[40]                                            # ties
    for k in (1, 7, 41, 499):
        kth = sorted(int(x) for x in img)[k - 1]
        want = [i for i, x in enumerate(img) if (int(x) >> 28) <= (kth >> 28)]
        got = ref_select(img, k)
        assert got.tolist() == want
        assert len(want) >= k


# ------------------------------------------------------------------------------------------------
# device helpers
# ------------------------------------------------------------------------------------------------
def _dev(a: np.ndarray, device):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(device)


def _soa(a: np.ndarray, cap: int, fill, device):
    """[n, NA] host array -> flat SoA device array of row stride cap, the tail rows `fill`."""
    n, na = a.shape
    h = np.full((na, cap), fill, dtype=a.dtype)
    h[:, :n] = a.T
    return _dev(h.reshape(-1), device)


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------
# 1. merge -> extract against a numpy group-by
# ------------------------------------------------------------------------------------------------
def _merge_input(seed: int, n: int, nkeys: int, NA: int, special: bool = True) -> dict:
    """Rows (partial groups) whose sums are j / 1024 with |j| < 2^20 and at most 2^16 rows per
    group: every partial sum is a multiple of 2^-10 below 2^26, exact in any order."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 63, 2 * nkeys, dtype=np.uint64) << _U(1) |
                     rng.integers(0, 2, 2 * nkeys, dtype=np.uint64))
    pool = rng.permutation(pool[pool != _FULL])[:nkeys]
    assert len(pool) == nkeys
    idx = rng.integers(0, nkeys, n)
    keys = pool[idx]
    nulls = np.zeros(n, dtype=np.uint8)
    if special:
        per = max(2, n // (nkeys + 2))
        rows = rng.permutation(n)[:2 * per]
        keys[rows[:per]] = _FULL                  # the EMPTY pattern as a key: direct slot M
        nulls[rows[per:]] = 1                     # NULL key: direct slot M + 1 (key word unused)
    sums = rng.integers(-(1 << 20) + 1, 1 << 20, (n, NA)) / 1024.0
    cnts = rng.integers(0, 4, (n, NA)).astype(np.int64)
    cnts[:, NA - 1] = rng.integers(1, 4, n)       # the star aggregate counts every row
    if NA > 1:
        cnts[idx < 5, 0] = 0                      # groups whose aggregate 0 never sees a value
    mins = rng.integers(-(1 << 20) + 1, 1 << 20, (n, NA)) / 1024.0
    mins[rng.random((n, NA)) < 0.05] = 0.0
    flip = (mins == 0.0) & (rng.random((n, NA)) < 0.5)
    mins[flip] = -0.0                             # 0.0 and -0.0 both occur as incoming extrema
    maxs = mins + rng.integers(0, 1 << 10, (n, NA)) / 1024.0
    maxs[flip] = -0.0
    zero = cnts == 0
    sums[zero], mins[zero], maxs[zero] = 0.0, np.inf, -np.inf
    assert np.bincount(idx).max() <= 1 << 16
    return {"keys": keys, "nulls": nulls, "sums": sums, "cnts": cnts, "mins": mins, "maxs": maxs}


def ref_groupby(inp: dict, minmax: bool) -> dict:
    """Groups of the rows sorted by (null, key); the NULL group's key reads 0."""
    k = np.where(inp["nulls"] != 0, _U(0), inp["keys"])
    order = np.lexsort((k, inp["nulls"]))
    ks, ns = k[order], inp["nulls"][order]
    st = np.flatnonzero(np.r_[True, (ks[1:] != ks[:-1]) | (ns[1:] != ns[:-1])])
    out = {"keys": ks[st], "nulls": ns[st],
           "sums": np.add.reduceat(inp["sums"][order], st, axis=0),
           "cnts": np.add.reduceat(inp["cnts"][order], st, axis=0)}
    if minmax:
        out["mins"] = np.minimum.reduceat(inp["mins"][order], st, axis=0)
        out["maxs"] = np.maximum.reduceat(inp["maxs"][order], st, axis=0)
    return out


def _merge(t: "H.HashTable", inp: dict, in_cap: int, device) -> None:
    n = len(inp["keys"])
    assert in_cap > n
    pad = np.full(in_cap - n, 0x1234, dtype=np.uint64)
    keys = _dev(np.concatenate([inp["keys"], pad]), device)
    nulls = _dev(np.concatenate([inp["nulls"], np.ones(in_cap - n, np.uint8)]), device)
    sums = _soa(inp["sums"], in_cap, 7.0, device)
    cnts = _soa(inp["cnts"], in_cap, 9, device)
    mins = _soa(inp["mins"], in_cap, -1e300, device) if t.minmax else None
    maxs = _soa(inp["maxs"], in_cap, 1e300, device) if t.minmax else None
    NL.check(NL.lib().hs_hagg_merge(NL.ptr(keys), NL.ptr(nulls), NL.ptr(sums), NL.ptr(cnts),
                                    NL.ptr(mins), NL.ptr(maxs), n, in_cap, NL.ptr(t.keys),
                                    NL.ptr(t.sums), NL.ptr(t.cnts), NL.ptr(t.mins),
                                    NL.ptr(t.maxs), t.M, t.NA, NL.ptr(t.flag), NL.stream_ptr()),
             "hs_hagg_merge")
    import torch
    torch.cuda.synchronize(device)


def _assert_like_fresh(t: "H.HashTable", device) -> None:
    import torch
    fresh = H.HashTable(t.M, t.NA, t.minmax, device)
    for name in ("keys", "sums", "cnts", "mins", "maxs"):
        a, b = getattr(t, name), getattr(fresh, name)
        if b is None:
            assert a is None
            continue
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), name
    assert int(t.flag[0].item()) == 0


def _sorted_groups(h: dict, minmax: bool) -> dict:
    k = np.where(h["nulls"] != 0, _U(0), h["keys"])
    o = np.lexsort((k, h["nulls"]))
    out = {"keys": k[o], "nulls": h["nulls"][o], "sums": h["sums"][o], "cnts": h["cnts"][o]}
    if minmax:
        out["mins"], out["maxs"] = h["mins"][o], h["maxs"][o]
    return out


def _assert_groups(g: "H.Groups", ref: dict, minmax: bool, special: bool) -> None:
    G, over = g.count()
    assert not over
    assert G == len(ref["keys"])
    h = g.to_host()
    if special:
        # extract emits in slot order: the two direct slots come last, EMPTY key then NULL
        assert h["keys"][G - 2] == _FULL and h["nulls"][G - 2] == 0
        assert h["nulls"][G - 1] == 1
        assert not h["nulls"][:G - 1].any()
    got = _sorted_groups(h, minmax)
    for name, want in ref.items():
        assert got[name].dtype == want.dtype, name
        assert np.array_equal(got[name], want), name
    if minmax and g.NA > 1:
        never = ref["cnts"][:, 0] == 0
        assert never.any()
        assert np.all(got["mins"][never, 0] == np.inf) and np.all(got["maxs"][never, 0] == -np.inf)
        assert np.all(got["sums"][never, 0] == 0.0)


@gpu
@pytest.mark.parametrize("M,nkeys,n,NA,minmax", [
    (4096, 1500, 200_000, 3, True),
    (4096, 1500, 200_000, 1, False),
    (64, 58, 6_000, 3, True),            # 58 + EMPTY + NULL = 60 groups: load 0.9, wrap-around
    (64, 58, 6_000, 1, False),
    (1024, 400, 30_000, 3, True),        # M + 2 slots: the direct slots alone in a second block
    (4096, 1000, 2_097_152 + 513, 3, True),   # past the merge grid (8192 x 256 threads)
])
def test_merge_extract_matches_numpy_groupby_and_resets(device, M, nkeys, n, NA, minmax):
    inp = _merge_input(M + NA, n, nkeys, NA)
    ref = ref_groupby(inp, minmax)
    assert len(ref["keys"]) == nkeys + 2
    t = H.HashTable(M, NA, minmax, device)
    for _ in range(2):                   # the second round runs on the table the first one left
        _merge(t, inp, n + 129, device)
        g = t.extract(NA - 1)
        _assert_groups(g, ref, minmax, True)
        _assert_like_fresh(t, device)
        again = t.extract(NA - 1)
        assert again.count() == (0, False)
        _assert_like_fresh(t, device)


@gpu
def test_merge_overflow_sets_flag_and_extract_cleans_up(device, capsys):
    """70 distinct keys into 64 slots: six rows walk the whole bounded probe loop and give up."""
    import torch
    M, NA = 64, 2
    inp = _merge_input(99, 70, 70, NA, special=False)
    inp["keys"] = np.unique(inp["keys"])
    rng = np.random.default_rng(5)
    while len(inp["keys"]) < 70:         # every key once: one probe walk per overflowing key
        inp["keys"] = np.unique(np.r_[inp["keys"], rng.integers(1, 1 << 62, 1, dtype=np.uint64)])
    t = H.HashTable(M, NA, True, device)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    _merge(t, inp, 100, device)
    dt = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\n[hash_agg overflow merge: {dt:.3f} s]")
    assert int(t.flag[0].item()) == 1
    g = t.extract(NA - 1)
    G, over = g.count()
    assert over is True
    assert G == M
    assert int(t.flag[0].item()) == 0
    _assert_like_fresh(t, device)
    # the keys that found a slot carry exactly their row
    h = g.to_host()
    row = {int(k): i for i, k in enumerate(inp["keys"])}
    assert len(set(h["keys"].tolist())) == M
    src = np.array([row[int(k)] for k in h["keys"]])
    for name in ("sums", "cnts", "mins", "maxs"):
        assert np.array_equal(h[name], inp[name][src]), name
    # and the table works again
    small = _merge_input(7, 500, 20, NA)
    _merge(t, small, 600, device)
    _assert_groups(t.extract(NA - 1), ref_groupby(small, True), True, True)
    _assert_like_fresh(t, device)


# ------------------------------------------------------------------------------------------------
# 2. images
# ------------------------------------------------------------------------------------------------
IMG_G, IMG_NA, IMG_SHIFT, IMG_MASK = 2003, 2, 7, 0x3FF


@functools.lru_cache(maxsize=None)
def _image_groups() -> dict:
    """Host groups with every special double in the aggregates and every edge key; unique keys.
    Read-only: shared by the image, select and take tests."""
    rng = np.random.default_rng(21)
    G, NA = IMG_G, IMG_NA

    def vals():
        a = rng.normal(size=(G, NA)) * 1e3
        s = rng.random((G, NA)) < 0.25
        a[s] = SPECIALS[rng.integers(0, len(SPECIALS), int(s.sum()))]
        a[:len(SPECIALS), 0] = SPECIALS
        return a
    keys = rng.integers(0, 1 << 63, G, dtype=np.uint64) << _U(1) | \
        rng.integers(0, 2, G, dtype=np.uint64)
    # 0 and INT64_MIN are also the bits of 0.0 and -0.0; -1 is a NaN pattern
    edge = np.unique(np.concatenate([np.array([0, _I64_MIN, _I64_MAX, -1],
                                              dtype=np.int64).view(np.uint64), _bits(SPECIALS)]))
    keys[:len(edge)] = edge
    keys[len(edge):len(edge) + 8] &= ~(_U(IMG_MASK) << _U(IMG_SHIFT))     # key fields of code 0
    assert len(np.unique(keys)) == G
    nulls = (rng.random(G) < 0.1).astype(np.uint8)
    nulls[:len(edge)] = 0
    nulls[len(edge)] = 1
    cnts = rng.integers(0, 6, (G, NA)).astype(np.int64)
    cnts[:len(SPECIALS)] = 3
    cnts[len(SPECIALS):2 * len(SPECIALS), 0] = 0
    host = {"keys": keys, "nulls": nulls, "sums": vals(), "cnts": cnts, "mins": vals(),
            "maxs": vals()}
    for a in host.values():
        a.setflags(write=False)
    return host


def _strided_groups(host: dict, cap: int, device) -> "H.Groups":
    """`host` uploaded with Groups.from_host, then copied into an allocation of row stride cap
    whose rows past G hold other values."""
    G, NA = len(host["keys"]), host["sums"].shape[1]
    src = H.Groups.from_host(host, NA, True, device)
    g = H.Groups.alloc(NA, cap, True, device)
    g.keys.fill_(0x5555)
    g.nulls.fill_(1)
    g.keys[:G], g.nulls[:G] = src.keys, src.nulls
    for name, junk in (("sums", 123.0), ("cnts", 0), ("mins", -7.0), ("maxs", 7.0)):
        getattr(g, name).fill_(junk)
        getattr(g, name).view(NA, cap)[:, :G] = getattr(src, name).view(NA, G)
    g.set_count(G)
    return g


def ref_images(host: dict, src: int, agg: int, cnt_slot: int, shift: int, mask: int,
               nullable: int, desc: int) -> np.ndarray:
    G = len(host["keys"])
    c = host["cnts"][:, cnt_slot] if cnt_slot >= 0 else np.ones(G, dtype=np.int64)
    null = np.zeros(G, dtype=bool)
    if src == H.SRC_SUM:
        null, v = c == 0, ref_dimg(host["sums"][:, agg])
    elif src == H.SRC_COUNT:
        v = c.view(np.uint64) ^ _TOP
    elif src == H.SRC_MIN:
        null, v = c == 0, ref_dimg(host["mins"][:, agg])
    elif src == H.SRC_MAX:
        null, v = c == 0, ref_dimg(host["maxs"][:, agg])
    elif src == H.SRC_AVG:
        with np.errstate(all="ignore"):
            avg = host["sums"][:, agg] / np.where(c == 0, 1, c).astype(np.float64)
        null, v = c == 0, ref_dimg(np.where(c == 0, 0.0, avg))
    elif src == H.SRC_KEYFIELD:
        v = (host["keys"] >> _U(shift)) & _U(mask)
        null = (v == 0) if nullable else null
    elif src == H.SRC_RAWINT:
        null, v = host["nulls"] != 0, host["keys"] ^ _TOP
    else:
        null, v = host["nulls"] != 0, ref_dimg(host["keys"].view(np.float64))
    o = ~v if desc else v
    return np.where(null, _FULL if desc else _U(0), o).astype(np.uint64)


def _device_images(g: "H.Groups", G: int, src, agg, cnt_slot, shift, mask, nullable, desc):
    import torch
    img = torch.full((G + 3,), 0x7777, dtype=torch.int64, device=g.device)
    NL.check(NL.lib().hs_topk_images(NL.ptr(g.keys), NL.ptr(g.nulls), NL.ptr(g.sums),
                                     NL.ptr(g.cnts), NL.ptr(g.mins), NL.ptr(g.maxs), G, g.cap,
                                     src, agg, cnt_slot, shift, C.c_uint64(mask), nullable, desc,
                                     NL.ptr(img), NL.stream_ptr()), "hs_topk_images")
    h = img.cpu().numpy()
    assert np.all(h[G:] == 0x7777)
    return h[:G].view(np.uint64)


@gpu
@pytest.mark.parametrize("src", list(range(8)))
def test_topk_images_equal_numpy_elementwise(device, src):
    host = _image_groups()
    G = IMG_G
    g = _strided_groups(host, G + 37, device)
    if src == H.SRC_KEYFIELD:
        variants = [(0, 0, IMG_SHIFT, IMG_MASK, nb) for nb in (0, 1)] + [(0, 0, 0, 0xFFFFF, 1)]
    elif src in (H.SRC_RAWINT, H.SRC_RAWFLT):
        variants = [(0, 0, 0, 0, 0)]
    else:
        variants = [(agg, cs, 0, 0, 0) for agg in (0, 1) for cs in (0, 1, -1)]
    seen_null = False
    for agg, cs, shift, mask, nullable in variants:
        for desc in (0, 1):
            want = ref_images(host, src, agg, cs, shift, mask, nullable, desc)
            got = _device_images(g, G, src, agg, cs, shift, mask, nullable, desc)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (src, agg, cs, nullable, desc, bad[:5], got[bad[:5]],
                                   want[bad[:5]])
            seen_null |= bool(np.any(want == (_FULL if desc else _U(0))))
    assert seen_null == (src != H.SRC_COUNT)


# ------------------------------------------------------------------------------------------------
# 3. radix select
# ------------------------------------------------------------------------------------------------
def _device_select(img: np.ndarray, k: int, device):
    import torch
    G = len(img)
    ws = H._topk_ws(device)
    d_img = _dev(img, device)
    out = torch.full((G + 1,), -1, dtype=torch.int32, device=device)
    NL.check(NL.lib().hs_topk_select(NL.ptr(d_img), G, k, NL.ptr(ws["st"]), NL.ptr(ws["hist"]),
                                     NL.ptr(out), NL.ptr(ws["count"]), NL.stream_ptr()),
             "hs_topk_select")
    n = int(ws["count"].item())
    assert int(ws["hist"].count_nonzero().item()) == 0, "hist left dirty"
    assert 0 <= n <= G
    h = out.cpu().numpy()
    assert np.all(h[n:] == -1)
    return h[:n].astype(np.int64), n


def _assert_select(img: np.ndarray, k: int, device, all_rows: bool = False):
    want = ref_select(img, k)
    rows, n = _device_select(img, k, device)
    rows = np.sort(rows)
    assert n == len(want), (len(img), k, n, len(want))
    assert np.all(rows[1:] != rows[:-1]), "duplicate rows"
    assert np.array_equal(rows, want), (len(img), k)
    assert n >= k
    if all_rows:
        assert n == len(img)


def _select_images(kind: str, G: int, k: int) -> np.ndarray:
    rng = np.random.default_rng(G + 31 * k)
    low28 = rng.integers(0, 1 << 28, G, dtype=np.uint64)
    if kind == "random":
        return rng.integers(0, 1 << 63, G, dtype=np.uint64) << _U(1) | (low28 & _U(1))
    if kind == "equal":
        return np.full(G, 0xC0FFEE0000000123, dtype=np.uint64)
    if kind == "count":             # COUNT images: 2^63 ^ a small count, one 36-bit prefix
        return _TOP | low28
    if kind == "last_bins":
        # every top field 0xFFF; fewer than k images below the all-ones 36-bit prefix, so the
        # k-th image is in bin 4095 of every level
        img = (_U(0xFFFFFFFFF) << _U(28)) | low28
        img[:4] = [_FULL, _FULL - _U(1), _FULL, _U(0xFFFFFFFFF) << _U(28)]
        nlow = (k - 1) // 2
        img[4:4 + nlow] = (_U(0xFFF) << _U(52)) | rng.integers(0, (1 << 52) - (1 << 28), nlow,
                                                             dtype=np.uint64)
        return img[rng.permutation(G)]
    if kind == "zero_top":
        # top field 0 everywhere: the prefix after level 0 is 0 and the k-th is in a later bin
        mid = rng.integers(100, 4096, G, dtype=np.uint64)
        return (mid << _U(40)) | rng.integers(0, 1 << 40, G, dtype=np.uint64)
    raise AssertionError(kind)


@gpu
@pytest.mark.parametrize("G", [257, 5_000, 524_288 + 300, 1_048_576 + 77])
@pytest.mark.parametrize("kind", ["random", "equal", "count", "last_bins", "zero_top"])
def test_topk_select_equals_36_bit_oracle(device, kind, G):
    for k in (1, 10, 1024, G - 1):
        if k >= G:
            continue
        img = _select_images(kind, G, k)
        _assert_select(img, k, device, all_rows=kind in ("equal", "count"))


@gpu
def test_topk_select_on_sum_desc_images_with_nulls_and_nans(device):
    host = _image_groups()
    img = ref_images(host, H.SRC_SUM, 0, 0, 0, 0, 0, 1)
    assert np.any(img == _FULL) and np.any(img == ~_NAN_IMG)
    for k in (1, 10, 1024, IMG_G - 1):
        _assert_select(img, k, device)


@gpu
@pytest.mark.parametrize("order", [H.OrderSource(H.SRC_SUM, agg=0, cnt_slot=0, desc=True),
                                   H.OrderSource(H.SRC_MAX, agg=1, cnt_slot=1, desc=False)])
def test_topk_candidates_take_returns_the_oracle_rows(device, order):
    host = _image_groups()
    G, NA, k = IMG_G, IMG_NA, 25
    g = _strided_groups(host, G + 37, device)
    img = ref_images(host, order.src, order.agg, order.cnt_slot, 0, 0, 0, int(order.desc))
    want = ref_select(img, k)
    cand, n = H.topk_candidates(g, G, order, k)
    assert int(H._topk_ws(device)["hist"].count_nonzero().item()) == 0
    assert n == len(want) and cand.count() == (n, False)
    got = cand.to_host()

    def rows(h, idx):
        return {(int(h["nulls"][i]), int(h["keys"][i])):
                tuple(_bits(h[a][i]).tolist() for a in ("sums", "mins", "maxs")) +
                (tuple(h["cnts"][i].tolist()),) for i in idx}
    got_rows = rows(got, range(n))
    assert len(got_rows) == n
    assert got_rows == rows(host, want)


# ------------------------------------------------------------------------------------------------
# 4. run top-K
# ------------------------------------------------------------------------------------------------
def _table_groups(NA: int, G: int, cap: int, rng, zero_counts: bool, over: int, device):
    """Dense table groups (count on the device, as extract leaves it) of row stride cap > G;
    the rows past G hold plausible values that must never be read as groups."""
    import torch
    keys = (np.arange(cap, dtype=np.uint64) + _U(1)) * _U(1_000_003)
    nulls = np.zeros(cap, dtype=np.uint8)
    nulls[3] = 1
    sums = np.round(rng.normal(size=(cap, NA)) * 1e4) / 8.0
    sp = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, _DENORM, -_DBL_MAX])[:max(0, cap - 5)]
    sums[5:5 + len(sp)] = sp[:, None]
    cnts = rng.integers(1, 1 << 20, (cap, NA)).astype(np.int64)
    if zero_counts:
        cnts[rng.random((cap, NA)) < 0.2] = 0
    g = H.Groups.alloc(NA, cap, False, device)
    g.keys, g.nulls = _dev(keys, device), _dev(nulls, device)
    g.sums, g.cnts = _soa(sums, cap, 0.0, device), _soa(cnts, cap, 0, device)
    g.total = torch.tensor([G, over], dtype=torch.int64, device=device)
    return g, {"keys": keys, "nulls": nulls, "sums": sums, "cnts": cnts}


def _fill_slots(plan: "H.TopKPlan", rng, live_frac: float, ties: bool, device):
    cap, NA = plan.cap, plan.NA
    keys = (np.arange(cap, dtype=np.uint64) + _U(1)) * _U(7_000_003) + _U(1 << 40)
    sums = np.round(rng.normal(size=(cap, NA)) * 1e4) / 8.0
    cnts = rng.integers(1, 1 << 20, (cap, NA)).astype(np.int64)
    if ties:
        sums[:], cnts[:] = 5.0, 5
    else:
        # the worst value (-inf descending, +inf ascending) is the empty pattern: not a live slot
        sums[2:8] = np.array([-0.0, 0.0, np.nan, _DENORM, -_DBL_MAX,
                              np.inf if plan.desc else -np.inf])[:, None]
    live = rng.random(cap) < live_frac
    if not ties and not plan.src_count:
        # a slot written with the worst value carries the empty pattern: the kernels (and this
        # oracle) treat it as empty, and the executor's guards re-run such queries exactly
        sums[8], live[8] = (-np.inf if plan.desc else np.inf), False
    value = cnts[:, plan.agg].astype(np.float64) if plan.src_count else sums[:, plan.agg]
    vimg = ref_slot_image(value if plan.desc else -value)
    assert ties or plan.src_count or vimg[8] == _U(REF_EMPTY)
    vimg[~live] = _U(REF_EMPTY)
    assert np.all(vimg[live] != _U(REF_EMPTY))
    plan.keys.copy_(_dev(keys, device))
    plan.vimg.copy_(_dev(vimg, device))
    plan.sums.copy_(_soa(sums, cap, 0.0, device))
    plan.cnts.copy_(_soa(cnts, cap, 0, device))
    return {"keys": keys, "sums": sums, "cnts": cnts, "live": live}


def ref_runs_images(plan, slots, table, G, cnt_slot):
    def image(x):
        return ~ref_dimg(x) if plan.desc else ref_dimg(x)
    sx = slots["cnts"][:, plan.agg].astype(np.float64) if plan.src_count else \
        slots["sums"][:, plan.agg]
    simg = np.where(slots["live"], image(sx), _FULL)
    c = table["cnts"][:, cnt_slot] if cnt_slot >= 0 else np.ones(len(table["keys"]), np.int64)
    tx = c.astype(np.float64) if plan.src_count else table["sums"][:, plan.agg]
    timg = image(tx)
    if not plan.src_count:
        timg = np.where(c == 0, _FULL if plan.desc else _U(0), timg)
    timg[G:] = _FULL
    return np.concatenate([simg, timg]).astype(np.uint64)


def _set_bounds(plan, rng, device):
    w = np.round(rng.normal(size=plan.nwv) * 1e3) / 4.0
    d = np.round(rng.normal(size=plan.nwv) * 1e3) / 4.0
    plan.wth.copy_(_dev(ref_simg(w), device))
    plan.dmx.copy_(_dev(ref_simg(d), device))
    return float(max(w.max(), d.max()))


def _run_plan(plan, g, cnt_slot, k):
    import torch
    plan.finish(NL.stream_ptr())
    blk = plan.gather(g, cnt_slot, k)
    assert int(H._topk_ws(plan.keys.device)["hist"].count_nonzero().item()) == 0
    torch.cuda.synchronize(plan.keys.device)
    return plan.unpack(blk.copy())


def _candidate_rows(keys, nulls, sums, cnts):
    return {(int(n), int(k)): (tuple(_bits(s).tolist()), tuple(int(x) for x in c))
            for k, n, s, c in zip(keys, nulls, sums, cnts)}


def _check_run_topk(plan, slots, table, g, G, cnt_slot, k, bound, over):
    img = ref_runs_images(plan, slots, table, G, cnt_slot)
    want = ref_select(img, k)
    r = _run_plan(plan, g, cnt_slot, k)
    dev_img = plan._img[:plan.cap + g.cap].cpu().numpy().view(np.uint64)
    assert np.array_equal(dev_img, img), np.flatnonzero(dev_img != img)[:5]
    assert r["n"] == len(want)
    assert r["G"] == G and r["over"] is bool(over)
    assert _bits([r["bound"]])[0] == _bits([bound])[0]
    if len(want) > plan.OUT:
        assert r["host"] is None and r["empty"] == 0
        return r
    sl = want[want < plan.cap]
    tb = want[want >= plan.cap] - plan.cap
    live = sl[slots["live"][sl]]
    assert r["empty"] == len(sl) - len(live)
    exp = _candidate_rows(slots["keys"][live], np.zeros(len(live), np.uint8),
                          slots["sums"][live], slots["cnts"][live])
    exp.update(_candidate_rows(table["keys"][tb], table["nulls"][tb], table["sums"][tb],
                               table["cnts"][tb]))
    assert len(exp) == len(live) + len(tb)
    h = r["host"]
    got = _candidate_rows(h["keys"], h["nulls"], h["sums"], h["cnts"])
    assert len(got) == len(h["keys"]) == len(exp)
    assert got == exp
    return r


@gpu
@pytest.mark.parametrize("K", [16, 32])
@pytest.mark.parametrize("NA", [1, 2])
def test_run_topk_candidates_equal_oracle(device, K, NA):
    rng = np.random.default_rng(100 * K + NA)
    nwv, G, cap, k = 5, 300, 350, 10
    for src_count in (False, True):
        for desc in (False, True):
            plan = H.TopKPlan(NA - 1, src_count, desc, NA, K)
            plan.bind(nwv, device)
            for zero_counts, cnt_slot, over in ((False, NA - 1, 0), (True, NA - 1, 1),
                                                (True, -1, 0)):
                g, table = _table_groups(NA, G, cap, rng, zero_counts, over, device)
                slots = _fill_slots(plan, rng, 0.7, False, device)
                bound = _set_bounds(plan, rng, device)
                r = _check_run_topk(plan, slots, table, g, G, cnt_slot, k, bound, over)
                # without a count every table group counts 1: ascending, all G of them tie
                all_tie = src_count and cnt_slot < 0 and not desc
                assert (r["host"] is None) == all_tie and r["empty"] == 0


@gpu
def test_run_topk_selects_empty_slots_when_k_exceeds_live_entries(device):
    rng = np.random.default_rng(41)
    NA, K, nwv, G, cap = 2, 16, 3, 20, 24
    plan = H.TopKPlan(1, False, True, NA, K)
    plan.bind(nwv, device)
    g, table = _table_groups(NA, G, cap, rng, False, 0, device)
    slots = _fill_slots(plan, rng, 0.5, False, device)
    bound = _set_bounds(plan, rng, device)
    nlive = int(slots["live"].sum())
    r = _check_run_topk(plan, slots, table, g, G, 1, nlive + G + 1, bound, 0)
    # everything is selected: the empty slots, and the table rows past G (image ~0 too)
    assert r["n"] == plan.cap + cap and r["empty"] == plan.cap - nlive


@gpu
def test_run_topk_more_ties_than_the_copy_holds(device):
    rng = np.random.default_rng(42)
    NA, K, nwv, G, cap = 1, 32, 20, 50, 60
    for src_count in (False, True):
        plan = H.TopKPlan(0, src_count, True, NA, K)
        plan.bind(nwv, device)
        g, table = _table_groups(NA, G, cap, rng, False, 0, device)
        table["sums"][:] = -1e9          # the table stays out of the top
        table["cnts"][:] = 1
        g.sums, g.cnts = _soa(table["sums"], cap, 0.0, device), _soa(table["cnts"], cap, 0, device)
        slots = _fill_slots(plan, rng, 0.8, True, device)
        bound = _set_bounds(plan, rng, device)
        r = _check_run_topk(plan, slots, table, g, G, 0, 10, bound, 0)
        assert r["host"] is None and r["n"] == int(slots["live"].sum()) > plan.OUT


@gpu
@pytest.mark.parametrize("nwv", [1, 63, 64, 65, 524_288 + 17])
def test_run_topk_threshold_is_the_exact_maximum(device, nwv):
    import torch
    rng = np.random.default_rng(nwv)
    plan = H.TopKPlan(0, False, True, 1, 16)
    plan.bind(nwv, device)
    plan.keys.zero_()
    plan.sums.zero_()
    plan.cnts.zero_()
    plan.vimg.fill_(REF_EMPTY - (1 << 64))
    g, _ = _table_groups(1, 4, 8, rng, False, 0, device)
    neg_inf = ref_simg([-np.inf])[0]
    cases = [(a, p) for a in ("wth", "dmx") for p in sorted({0, nwv // 2, nwv - 1})]
    for which, pos in cases + [("none", 0)]:
        # every other value is far below zero; the maximum is -0.0 or a positive value
        w = np.round(rng.normal(size=nwv) * 1e3) / 4.0 - 1e4
        d = np.round(rng.normal(size=nwv) * 1e3) / 4.0 - 1e4
        assert max(w.max(), d.max()) < -1e3
        if which == "none":
            w[:], d[:] = -np.inf, -np.inf
        else:
            (w if which == "wth" else d)[pos] = 12345.678 if pos % 2 else -0.0
        want = float(max(w.max(), d.max()))
        plan.wth.copy_(_dev(ref_simg(w), device))
        plan.dmx.copy_(_dev(ref_simg(d), device))
        r = _run_plan(plan, g, 0, 1)
        assert _bits([r["bound"]])[0] == _bits([want])[0], (which, pos, r["bound"], want)
        ctl = plan.ctl.cpu().numpy()
        assert ctl[0] == ref_simg(w).max() and ctl[2] == ref_simg(d).max() and ctl[1] == 0
        assert ref_unsimg([max(ctl[0], ctl[2])])[0].view(np.uint64) == _bits([want])[0]
        if which == "none":
            assert ctl[0] == neg_inf and r["bound"] == -np.inf
        assert r["G"] == 4 and r["n"] == 1 and r["empty"] == 0


# ------------------------------------------------------------------------------------------------
# 5. functional-dependency lookup
# ------------------------------------------------------------------------------------------------
FD_OUT = 256
FD_SENTINEL = -0x0123456789ABCDEF


def _right_table(key_type: int, nb: int, lo: int, span: int, device) -> dict:
    """~5,000 unique right keys in [lo, lo + span), rows sorted by (bucket, key), with four
    value columns (int32, int64, float64, nullable int64)."""
    rng = np.random.default_rng(nb + key_type)
    np_t, pa_t = (np.int64, pa.int64()) if key_type == NL.I64 else (np.int32, pa.int32())
    keys = np.unique(rng.integers(lo, lo + span, 5_200)).astype(np_t)
    assert len(keys) > 4_500 and (keys < 0).any()
    bucket = murmur3.bucket_ids([pa.array(keys, pa_t)], nb)
    order = np.lexsort((keys, bucket))
    keys, bucket = keys[order], bucket[order]
    n = len(keys)
    off = np.searchsorted(bucket, np.arange(nb + 1)).astype(np.int64)
    f = rng.normal(size=n)
    f[:len(SPECIALS)] = SPECIALS
    cols = [(NL.I32, rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32), None),
            (NL.I64, rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64), None),
            (NL.F64, f[rng.permutation(n)], None),
            (NL.I64, rng.integers(-99, 99, n).astype(np.int64),
             (rng.random(n) < 0.7).astype(np.uint8))]
    t = {"keys": keys, "off": off, "nb": nb, "cols": cols, "type": key_type,
         "d_keys": _dev(keys, device), "d_off": _dev(off, device),
         "d_cols": [(_dev(v, device), None if m is None else _dev(m, device))
                    for _, v, m in cols]}
    t["row"] = {int(k): i for i, k in enumerate(keys)}
    return t


def _fd_lookup(t: dict, packed_keys: np.ndarray, nsel: int, ncols: int, raw: int, lo: int,
               shift: int, mask: int, device) -> np.ndarray:
    import torch
    out = np.zeros(8 + FD_OUT, dtype=np.int64)
    out[0] = nsel
    m = min(len(packed_keys), FD_OUT)
    out[8:8 + m] = packed_keys[:m].view(np.int64)
    d_out = _dev(out, device)
    tail = 64
    fdo = torch.full((FD_OUT * (1 + 2 * ncols) + tail,), FD_SENTINEL, dtype=torch.int64,
                     device=device)
    kd = NL.ColDesc(t["d_keys"].data_ptr(), None, t["type"], 0)
    descs = (NL.ColDesc * 4)(*[NL.ColDesc(v.data_ptr(), None if m is None else m.data_ptr(),
                                          t["cols"][a][0], 0)
                               for a, (v, m) in enumerate(t["d_cols"][:ncols])])
    NL.check(NL.lib().hs_topk_runs_fd(NL.ptr(d_out), FD_OUT, raw, lo, shift, C.c_uint64(mask),
                                      C.byref(kd), NL.ptr(t["d_off"]), t["nb"], descs, ncols,
                                      NL.ptr(fdo), NL.stream_ptr()), "hs_topk_runs_fd")
    h = fdo.cpu().numpy()
    assert np.all(h[FD_OUT * (1 + 2 * ncols):] == FD_SENTINEL)
    return h[:FD_OUT * (1 + 2 * ncols)].reshape(1 + 2 * ncols, FD_OUT)


def ref_fd(t: dict, values: np.ndarray, m: int, ncols: int) -> np.ndarray:
    want = np.full((1 + 2 * ncols, FD_OUT), FD_SENTINEL, dtype=np.int64)
    for j in range(m):
        row = t["row"].get(int(values[j]), -1)
        want[0, j] = row
        for a in range(ncols):
            typ, v, valid = t["cols"][a]
            x = ok = 0
            if row >= 0:
                x = int(_bits([v[row]]).view(np.int64)[0]) if typ == NL.F64 else int(v[row])
                ok = 1 if valid is None or valid[row] else 0
            want[1 + a, j], want[1 + ncols + a, j] = x, ok
    return want


@gpu
@pytest.mark.parametrize("nb", [1, 7, 200])
@pytest.mark.parametrize("key_type", [NL.I64, NL.I32])
def test_topk_runs_fd_lookup_equals_dict(device, key_type, nb):
    rng = np.random.default_rng(17 * nb + key_type)
    bits, shift, lo = 20, 5, -300_000
    mask = (1 << bits) - 1
    wide = _right_table(key_type, nb, -(1 << 62) if key_type == NL.I64 else -(1 << 31),
                        1 << 63 if key_type == NL.I64 else 1 << 32, device)
    dense = _right_table(key_type, nb, lo, 1 << bits, device)
    for t, raw in ((wide, 1), (dense, 1), (dense, 0)):
        present = rng.permutation(t["keys"])[:300].astype(np.int64)
        absent = rng.integers(lo, lo + (1 << bits), 120) if t is dense else \
            rng.integers(-(1 << 31), 1 << 31, 120)
        absent = np.array([v for v in absent if int(v) not in t["row"]], dtype=np.int64)
        assert len(absent) > 10
        values = rng.permutation(np.concatenate([present, absent]))
        if raw:
            packed = values.view(np.uint64).copy()
        else:
            junk_lo = rng.integers(0, 1 << shift, len(values), dtype=np.uint64)
            junk_hi = rng.integers(0, 1 << 30, len(values), dtype=np.uint64) << _U(shift + bits)
            packed = ((values - lo).astype(np.uint64) << _U(shift)) | junk_lo | junk_hi
        for nsel, ncols in ((200, 4), (FD_OUT, 3), (len(values), 4), (37, 0), (1, 1)):
            assert nsel <= len(values)
            got = _fd_lookup(t, packed, nsel, ncols, raw, 0 if raw else lo, 0 if raw else shift,
                             0 if raw else mask, device)
            m = min(nsel, FD_OUT)
            want = ref_fd(t, values, m, ncols)
            assert (want[0, :m] == -1).any() or m < 5
            assert np.array_equal(got, want), (key_type, nb, raw, nsel, ncols,
                                               np.argwhere(got != want)[:5])
