"""A numpy model of the order in which ``hs_agg_final_kernel`` / ``hs_agg_fold_kernel``
(csrc/kernels/scan_filter.hip) fold a query's partials, used bit for bit by
``tests/test_agg_fold_gpu.py``: lane ``t`` of the FIN_BLOCK threads sums partials
``t, t + FIN_BLOCK, ...`` in order, each 64-lane wave reduces with an xor butterfly
(``hs_wave_sum``: offsets 32, 16, ..., 1, every lane adds its partner's value), and thread 0 adds
the waves in order.
"""
import re
import os

import numpy as np

FIN_BLOCK = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _butterfly(v: np.ndarray, op) -> np.ndarray:
    """``v``: [waves, 64]; after the five xor steps every lane of a wave holds its total."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lanes ^ off])
    return v


def fold_model(psum, pcnt, pmin, pmax, nblk: int, GA: int):
    """(sum, count, min, max) [GA] of partials laid out [nblk, GA], in the kernels' order.
    (fmin / fmax: ``make_partials`` gives no NaN and no +0.0, so np.minimum / np.maximum agree
    with them bit for bit.)"""
    outs = (np.empty(GA), np.empty(GA, np.int64), np.empty(GA), np.empty(GA))
    for i in range(GA):
        s = np.zeros(FIN_BLOCK)
        c = np.zeros(FIN_BLOCK, np.int64)
        mn = np.full(FIN_BLOCK, np.inf)
        mx = np.full(FIN_BLOCK, -np.inf)
        for b0 in range(0, nblk, FIN_BLOCK):            # lane t: b0 + t, in order of b0
            n = min(FIN_BLOCK, nblk - b0)
            o = (b0 + np.arange(n)) * GA + i
            s[:n] = s[:n] + psum[o]
            c[:n] = c[:n] + pcnt[o]
            mn[:n] = np.minimum(mn[:n], pmin[o])
            mx[:n] = np.maximum(mx[:n], pmax[o])
        ws = _butterfly(s.reshape(-1, 64), np.add)[:, 0]
        wc = _butterfly(c.reshape(-1, 64), np.add)[:, 0]
        wmn = _butterfly(mn.reshape(-1, 64), np.minimum)[:, 0]
        wmx = _butterfly(mx.reshape(-1, 64), np.maximum)[:, 0]
        ts, tc, tmn, tmx = 0.0, np.int64(0), np.inf, -np.inf
        for k in range(FIN_BLOCK // 64):                # thread 0: the waves in order
            ts = ts + ws[k]
            tc = tc + wc[k]
            tmn = min(tmn, wmn[k])
            tmx = max(tmx, wmx[k])
        outs[0][i], outs[1][i], outs[2][i], outs[3][i] = ts, tc, tmn, tmx
    return outs


def make_partials(nblk: int, GA: int, seed: int):
    """Partials of mixed sign and magnitude, counts above 2^40, mins and maxes with +-inf and
    -0.0."""
    rng = np.random.default_rng(seed)
    n = nblk * GA
    psum = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 12, n)
    pcnt = rng.integers(0, 1 << 20, n).astype(np.int64)
    pcnt[rng.random(n) < 0.3] += (1 << 41)
    pmin = rng.standard_normal(n) * 1e3
    pmax = rng.standard_normal(n) * 1e3
    for a, fill in ((pmin, np.inf), (pmax, -np.inf)):
        a[rng.random(n) < 0.3] = fill              # a block that saw no row
        a[rng.random(n) < 0.1] = -0.0
    return psum, pcnt, pmin, pmax


def test_model_constant_matches_the_kernel_source():
    src = open(os.path.join(ROOT, "csrc", "kernels", "scan_filter.hip")).read()
    assert int(re.search(r"#define FIN_BLOCK (\d+)", src).group(1)) == FIN_BLOCK
    common = open(os.path.join(ROOT, "csrc", "kernels", "hs_common.h")).read()
    body = common[common.index("T hs_wave_sum(T v)"):]
    assert "for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);" in \
        body[:body.index("}")]


def test_model_equals_a_plain_sum_to_fp64_tolerance():
    for nblk in (1, 63, 64, 255, 256, 257, 1000):
        for GA in (1, 3, 5):
            p = make_partials(nblk, GA, 100 * nblk + GA)
            got = fold_model(*p, nblk, GA)
            s2 = p[0].reshape(nblk, GA)
            # |error| <= (n - 1) * eps * sum |x| for any summation order of n terms
            bound = nblk * np.finfo(np.float64).eps * np.abs(s2).sum(axis=0)
            exact = np.array([float(np.sum(s2[:, i].astype(np.longdouble))) for i in range(GA)])
            assert (np.abs(got[0] - exact) <= bound).all(), (nblk, GA)
            assert np.array_equal(got[1], p[1].reshape(nblk, GA).sum(axis=0))
            assert (got[1] > (1 << 40)).any() or nblk < 8
            assert np.array_equal(got[2], p[2].reshape(nblk, GA).min(axis=0))
            assert np.array_equal(got[3], p[3].reshape(nblk, GA).max(axis=0))


def test_model_is_sensitive_to_the_order_of_its_inputs():
    """Permuting the partials of a slot changes the sum's bits for such inputs, so a bitwise
    match of kernel and model says the kernel adds in the model's order."""
    for nblk in (63, 257, 1000):
        p = make_partials(nblk, 1, 7)
        base = fold_model(*p, nblk, 1)
        rng = np.random.default_rng(8)
        differs = 0
        for _ in range(16):
            perm = rng.permutation(nblk)
            got = fold_model(p[0][perm], p[1][perm], p[2][perm], p[3][perm], nblk, 1)
            differs += got[0][0] != base[0][0]
            # (the integer sum and the extremes do not depend on the order)
            assert got[1][0] == base[1][0] and got[2][0] == base[2][0] and got[3][0] == base[3][0]
        assert differs >= 1, nblk
