"""Phase 1 of the two-phase run-keyed merge join, four runs per lane (exec/jit_runs.py,
``rt2_wide = 4``): 256-run blocks with 16-byte loads and the next stage's loads issued ahead.

GPU tier: the wide form, the one-run form and numpy agree on aggregates (and on the recorded
per-run match) for an exact foreign key, for keys missing on both sides, for ranges that start
and end inside a block, an empty bucket, a bucket below one block, run counts of 1, 3 and 255
modulo 256 and tag widths 1, 2, 4 and 8 - with one block per wavefront (the default grid) and
with long per-wavefront chunks (a 2-workgroup grid), where the pipeline runs.  CPU tier: which
joins the lowering gives the wide form.
"""
import functools

import numpy as np
import pyarrow as pa
import pytest

from hyperspace_amd.ops import _lib as NL
from test_jit import _agg, _col, _fake, _q3_compacts, _q3_params

GROUPS = {10: 3, 11: 9, 12: 200}     # right group-key slot -> its number of groups


@functools.lru_cache(maxsize=None)
def _data(kind: str, tail: int):
    """Bucket-sorted join inputs (host): unique sorted right keys per bucket, 0-7 left rows per
    key ("exact": 1-7, every right key before the cut has left rows, no orphans; "mixed": ~5 % of the right
    keys without left rows and ~3000 left keys without a right row), a bucket below one
    256-run block, a bucket with left rows and no right rows, an empty bucket; the left table
    is cut at its end so that the run count is ``tail`` modulo 256."""
    rng = np.random.default_rng(7 + tail)
    sizes = [9000, 0, 60, 12000, 0, 10000, 9000]
    orphan_only = 1                                   # bucket 1: left rows, no right rows
    lks, rks, key0 = [], [], 1 << 20
    for b, n in enumerate(sizes):
        rk = key0 + 4 * np.arange(1, n + 1, dtype=np.int64)
        key0 += 4 * (n + 1000)
        per = rng.integers(1, 8, n)
        if kind == "mixed":
            per[rng.random(n) < 0.05] = 0
        lk = np.repeat(rk, per)
        if kind == "mixed" and n > 1000:
            orphan = rk[rng.integers(0, n, 750)] + 1
            lk = np.sort(np.concatenate([lk, orphan]))
        if kind == "mixed" and b == orphan_only:
            lk = np.repeat(key0 + 4 * np.arange(1, 101, dtype=np.int64), 3)
            key0 += 4000
        lks.append(lk)
        rks.append(rk)
    # cut the last bucket's tail: run count == tail (mod 256)
    nruns = sum(len(np.unique(x)) for x in lks)
    drop = (nruns - tail) % 256
    last = lks[-1]
    lks[-1] = last[last < np.unique(last)[len(np.unique(last)) - drop]] if drop else last
    lk, rk = np.concatenate(lks), np.concatenate(rks)
    loff = np.concatenate([[0], np.cumsum([len(x) for x in lks])]).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum([len(x) for x in rks])]).astype(np.int64)
    d = {"lk": lk, "rk": rk, "loff": loff, "roff": roff,
         "ldate": rng.integers(0, 1000, len(lk)).astype(np.int32),
         "lprice": np.round(rng.random(len(lk)) * 1000, 2),
         "rdate": rng.integers(0, 1000, len(rk)).astype(np.int32)}
    g = rng.integers(0, 200, len(rk)).astype(np.int32)
    for slot, n in GROUPS.items():
        d[f"g{slot}"] = g % n
    st = np.concatenate([[True], lk[1:] != lk[:-1]])
    d["run_of_row"] = np.cumsum(st) - 1
    d["runkeys"] = lk[st]
    assert len(d["runkeys"]) % 256 == tail
    return d


def _ranges(d, sub: bool):
    starts, lens = d["loff"][:-1].copy(), d["loff"][1:] - d["loff"][:-1]
    if sub:     # ranges that start and end inside a 256-run block (where the bucket allows)
        big = lens > 9
        starts[big] += 5
        lens = np.where(big, lens - 9, lens)
    return starts, lens


def _expect(d, starts, lens, gslot: int):
    """numpy: (sums, counts) per group of the join's passing rows, and the matched runs."""
    G = GROUPS[gslot] if gslot >= 0 else 1
    rows = np.concatenate([np.arange(s, s + n) for s, n in zip(starts, lens)])
    order = np.argsort(d["rk"], kind="stable")
    srt = d["rk"][order]
    idx = np.minimum(np.searchsorted(srt, d["lk"][rows]), len(srt) - 1)
    match = srt[idx] == d["lk"][rows]
    rrow = order[idx]
    ok = match & (d["rdate"][rrow] < 500) & (d["ldate"][rows] > 300)
    grp = d[f"g{gslot}"][rrow][ok] if gslot >= 0 else np.zeros(int(ok.sum()), np.int64)
    val = d["lprice"][rows] * (1.0 + 0.001 * d["ldate"][rows])
    sums = np.bincount(grp, weights=val[ok], minlength=G)
    cnts = np.bincount(grp, minlength=G)
    runs = np.unique(d["run_of_row"][rows])
    matched = len(np.unique(d["run_of_row"][rows][match]))
    return sums, cnts, len(runs), matched


def _expect_match(d, starts, lens):
    """numpy: each run's matched right row under the ranges, else -1."""
    out = np.full(len(d["runkeys"]), -1, np.int64)
    for b, (s, n) in enumerate(zip(starts, lens)):
        if n <= 0:
            continue
        r0, r1 = d["run_of_row"][s], d["run_of_row"][s + n - 1] + 1
        seg = d["rk"][d["roff"][b]:d["roff"][b + 1]]
        if len(seg) == 0:
            continue
        keys = d["runkeys"][r0:r1]
        i = np.minimum(np.searchsorted(seg, keys), len(seg) - 1)
        out[r0:r1] = np.where(seg[i] == keys, d["roff"][b] + i, -1)
    return out


@functools.lru_cache(maxsize=None)
def _device_inputs(kind: str, tail: int):
    import torch
    from hyperspace_amd.exec.encoding import encode
    dev = torch.device("cuda:0")
    d = _data(kind, tail)
    cols = {0: d["lk"], 1: d["ldate"], 2: d["lprice"], 8: d["rk"], 9: d["rdate"]}
    cols.update({slot: d[f"g{slot}"] for slot in GROUPS})
    dc = {s: _col(pa.array(a), dev) for s, a in cols.items()}
    p = NL.JoinParams()
    for s, c in dc.items():
        p.cols[s] = c.desc()
    p.preds[0] = NL.Pred(NL.PK_INT_LIT, NL.OP_GT, 1, 0, 0, 0, 300, 0.0, None)
    p.preds[1] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 9, 0, 1, 0, 500, 0.0, None)
    p.nlp, p.npreds = 1, 2
    p.aggs[0] = _agg(NL.AK_SUM, [(2, 0.0, 1.0), (1, 1.0, 0.001)])
    p.aggs[1] = _agg(NL.AK_COUNT_STAR)
    p.naggs, p.lkey, p.rkey, p.key_is_float = 2, 0, 8, 0
    comp = {s: e for s, e in ((s, encode(c)) for s, c in dc.items()) if e is not None}
    rng_t = {}
    B = len(d["loff"]) - 1
    for sub in (False, True):
        starts, lens = _ranges(d, sub)
        rng_t[sub] = (torch.from_numpy(starts.astype(np.int64)).to(dev),
                      torch.from_numpy(lens.astype(np.int64)).to(dev),
                      torch.arange(B, dtype=torch.int32, device=dev),
                      torch.from_numpy(d["roff"]).to(dev))
    return p, dc, comp, rng_t


def _run(p, comp, rt, nrows, G, **cfg):
    from hyperspace_amd.exec import jit, jit_runs, kernel_config
    with kernel_config.use(rt2_match=False, rt2_copy=False, mj_2p=True, **cfg):
        got = [t.cpu().numpy() for t in
               jit.merge_join_agg(p, *rt, comp, nrows=nrows, rdup=False)]
        launcher = jit.LAST_MJ_LAUNCHER[0]
        assert isinstance(launcher, jit_runs.TwoPhaseLauncher)
        assert ("IMGV(" in launcher.kt.src) == (cfg.get("rt2_wide") == 4), cfg
    return got[0].reshape(G, 2)[:, 0], got[1].reshape(G, 2)[:, 1]


# (data, run count modulo 256, sub-ranges, group slots: -1 = ungrouped W 1, 10 = W 2, 11 = W 4,
# 12 = W 8)
CASES = [("exact", 1, False, (-1, 10)), ("exact", 1, True, (-1, 10)),
         ("mixed", 3, False, (-1, 10)), ("mixed", 3, True, (-1, 10, 11)),
         ("mixed", 255, False, (-1, 10, 12)), ("mixed", 255, True, (-1, 10))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,tail,sub,gslots", CASES)
def test_wide_tags_match_one_run_form_and_numpy(device, kind, tail, sub, gslots):
    from hyperspace_amd.exec import jit_runs
    d = _data(kind, tail)
    p, _, comp, rng_t = _device_inputs(kind, tail)
    starts, lens = _ranges(d, sub)
    try:
        for gslot in gslots:
            G = GROUPS[gslot] if gslot >= 0 else 1
            p.group_col, p.num_groups, p.group_base = (gslot, G, 0) if gslot >= 0 else (-1, 1, 0)
            assert jit_runs.tag_width(p) == {-1: 1, 10: 2, 11: 4, 12: 8}[gslot]
            es, ec, nr, matched = _expect(d, starts, lens, gslot)
            if kind == "exact":
                assert matched == nr
            else:
                assert 0 < matched < nr        # guesses drift: hits and gallops both occur
            ref = _run(p, comp, rng_t[sub], len(d["lk"]), G, rt2_wide=1)
            # one block per wavefront, then ~20 blocks (two and one per pipeline stage)
            for cfg in ({}, {"rt2_wide_grid": 2}, {"rt2_wide_grid": 2, "rt2_unroll": 1}):
                s_, c_ = _run(p, comp, rng_t[sub], len(d["lk"]), G, rt2_wide=4, **cfg)
                print(kind, tail, sub, gslot, cfg, c_.sum(), ec.sum())
                assert (c_ == ec).all(), (gslot, cfg, c_, ec)
                assert np.allclose(s_, es, rtol=1e-12), (gslot, cfg)
                assert (c_ == ref[1]).all() and np.allclose(s_, ref[0], rtol=1e-12), (gslot, cfg)
    finally:
        p.group_col, p.num_groups = -1, 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind,tail,sub", [("exact", 1, False), ("mixed", 3, True)])
def test_wide_record_mode_stores_each_runs_match(device, kind, tail, sub):
    """Mode "rec": MOUT is the row where the key matches, else -1; a reused lowering that
    switches to the recorded match returns the same aggregates."""
    from hyperspace_amd.exec import jit, jit_join, jit_runs, kernel_config
    d = _data(kind, tail)
    p, _, comp, rng_t = _device_inputs(kind, tail)
    starts, lens = _ranges(d, sub)
    p.group_col, p.num_groups, p.group_base = -1, 1, 0
    nruns = len(d["runkeys"])
    exp_m = _expect_match(d, starts, lens)
    es, ec, _, _ = _expect(d, starts, lens, -1)
    for cfg in ({}, {"rt2_wide_grid": 2}):
        with kernel_config.use(rt2_wide=4, rt2_match=False, rt2_copy=False, mj_2p=True, **cfg):
            comp2, runs = jit_join._with_runs(p, comp)
            assert runs is not None and int(runs.runkeys.numel()) == nruns
            lz = jit_runs.lower(p, *rng_t[sub], comp2, runs, len(d["lk"]), False)
            m = jit_runs.record_matches(p, lz.compacts, 1, lz.vt, nruns, lz.grid_t, device)
            kr = jit_runs.gen_run_tags2(p, lz.compacts, 1, True, "rec")
            assert "IMGV(" in kr.src and "hs_i4*)(a.MOUT" in kr.src
            m = m.cpu().numpy()
            assert len(m) == (nruns + 63) // 64 * 64 and (m[nruns:] == -1).all()
            assert np.array_equal(m[:nruns], exp_m), cfg
        with kernel_config.use(rt2_wide=4, rt2_match=True, rt2_copy=False, mj_2p=True, **cfg):
            first = jit.merge_join_agg(p, *rng_t[sub], comp, nrows=len(d["lk"]), rdup=False,
                                       record=True, cache_spans=True)
            launcher = jit.LAST_MJ_LAUNCHER[0]
            assert "IMGV(" in launcher.kt.src
            again = launcher.launch(p)          # records the match, then reads it
            assert "a.MATCH[" in launcher.kt.src
            for got in (first, again):
                got = [t.cpu().numpy() for t in got]
                assert got[1].reshape(1, 2)[0, 1] == ec[0], cfg
                assert np.allclose(got[0].reshape(1, 2)[0, 0], es[0], rtol=1e-12), cfg


def test_lowering_selects_the_wide_form():
    """``tags2_shape`` separates the two forms; the wide form is chosen only for the verifying
    kernel with 32-bit indices over plainly stored, non-null right columns."""
    import torch
    from hyperspace_amd.exec import jit_runs, kernel_config
    from hyperspace_amd.exec.encoding import Compact, GroupedCompact, RunCompact
    c = dict(_q3_compacts())
    c[0] = Compact(None, 4, 1 + (1 << 31), None, NL.I64, 1, 600_000_000)
    c[8] = Compact(None, 4, 1 + (1 << 31), None, NL.I64, 1, 600_000_000)
    c[0] = RunCompact(c[0], torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64),
                      torch.zeros(1, dtype=torch.int32))
    p = _q3_params()
    with kernel_config.use(rt2_wide=1):
        one = jit_runs.tags2_shape(p, c, 1, True)
        assert jit_runs.tags2_wide(p, c, True) == 1
        assert "IMGV(" not in jit_runs.gen_run_tags2(p, c, 1, True).src
    with kernel_config.use(rt2_wide=4):
        assert jit_runs.tags2_shape(p, c, 1, True) != one
        assert jit_runs.tags2_wide(p, c, True) == 4 and jit_runs.tags2_wide(p, c, True, "rec") == 4
        k = jit_runs.gen_run_tags2(p, c, 1, True)
        assert "IMGV(" in k.src and "const hs_c9x4*)(a.c9" in k.src
        # 64-bit indices, the recorded-match and 16-bit-half modes: the one-run form
        assert jit_runs.tags2_wide(p, c, False) == 1
        assert jit_runs.tags2_shape(p, c, 1, False)[-1] == 1
        assert "IMGV(" not in jit_runs.gen_run_tags2(p, c, 1, False).src
        for mode in ("match", "copy", "lo16", "lo16prep"):
            assert jit_runs.tags2_wide(p, c, True, mode) == 1
            assert "IMGV(" not in jit_runs.gen_run_tags2(p, c, 1, True, mode).src
        # grouped 16-bit right keys and a nullable staged column: the one-run form
        c16 = dict(c)
        c16[8] = GroupedCompact(None, None, None, 1 + (1 << 31), NL.I64, 1, 600_000_000)
        assert jit_runs.tags2_wide(p, c16, True) == 1
        assert "IMGV(" not in jit_runs.gen_run_tags2(p, c16, 1, True).src
        pn = _q3_params()
        pn.cols[9] = _fake(NL.I32, True)
        assert jit_runs.tags2_wide(pn, c, True) == 1
        pk = _q3_params()
        pk.cols[8] = _fake(NL.I64, True)
        assert jit_runs.tags2_wide(pk, c, True) == 1
