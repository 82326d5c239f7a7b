"""The four-run phase 1 of the run-keyed merge join over 16-bit key offsets (exec/jit_runs.py,
``rt2_k16``): both key columns are read as uint16 offsets from the bases of 32-element groups
(``hs_group16_32``, csrc/kernels/key_runs.hip) and rebuilt as code = base + offset.

CPU tier: the host encoder against a numpy reference (exactness, wide groups, padding), which
joins the lowering gives the form, and its sources compile for gfx950.  GPU tier: the native
encoder equals the reference; the join equals numpy and, bit for bit in tags and aggregates, the
32-bit kernel - on data with keys whose low halves collide at the guessed row, offsets at or
above 32768, right keys outside the key frame, and wide groups on either side; with and without
the pruned pair; one launcher serving three literal vectors; uncovered joins keep the old
kernel.  (The key frame is the left key's own value range, ``jit_join._key32_frame``, so only
right keys can lie outside it: the data has right keys below and above it.)  A host model of the
kernel's stage walk (``_stage_walk``) pins which runs a fast stage resolves: the colliding keys
and the stages around the wide groups among them.
"""
import functools

import numpy as np
import pyarrow as pa
import pytest

from hyperspace_amd.ops import _lib as NL
from test_jit import _col, _fake, _q3_compacts, _q3_params, rt  # noqa: F401
from test_run_prune import LONG_RUN, _expect, _params, _ranges, _run

WIDE = -(1 << 31)
SIZES = (0, 1, 31, 32, 33, 255, 256, 257, 20_011)


def _ref32(x: np.ndarray):
    """numpy reference of the 32-group encoding: (offsets uint16, bases int32, wide per group),
    padded to a multiple of 256 elements."""
    n = len(x)
    npad = max(256, (n + 255) // 256 * 256)
    off = np.zeros(npad, np.uint16)
    base = np.full(npad // 32, WIDE, np.int32)
    ng = (n + 31) // 32
    wide = np.zeros(ng, bool)
    for g in range(ng):
        seg = x[32 * g:32 * g + 32].astype(np.int64)
        wide[g] = seg.max() - seg.min() >= (1 << 16) or seg.min() == WIDE
        if not wide[g]:
            base[g] = seg.min()
            off[32 * g:32 * g + len(seg)] = seg - seg.min()
    return off, base, wide


def _codes(n: int, seed: int = 5) -> np.ndarray:
    """Sorted int32 codes with gaps of 2^16 or more at a group's first and last element, at a
    bucket edge (a multiple of 32 and one that is none), one span of exactly 2^16 - 1 and one of
    exactly 2^16, and negative codes."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.integers(1, 1600, n)).astype(np.int64) - (1 << 20)
    for at in (32 * 3, 32 * 5 + 31, 32 * 20 + 1, 1000, 32 * 40 + 7):
        if at < n:
            x[at:] += 70_000        # the gap lies before element ``at``
    if n > 32 * 12 + 32:            # group 11: span 2^16 - 1 (narrow); group 12: 2^16 (wide)
        for g, span in ((11, (1 << 16) - 1), (12, 1 << 16)):
            lo = x[32 * g - 1] + 1
            x[32 * g:32 * g + 32] = lo + np.linspace(0, span, 32).astype(np.int64)
            x[32 * g + 32:] += max(0, x[32 * g + 31] + 1 - x[32 * g + 32])
    assert (np.diff(x) >= 0).all() and np.abs(x).max(initial=0) < (1 << 31)
    return x.astype(np.int32)


def _check_form(x: np.ndarray, off: np.ndarray, base: np.ndarray):
    n = len(x)
    roff, rbase, wide = _ref32(x)
    assert off.dtype == np.uint16 and base.dtype == np.int32
    assert len(off) == len(roff) and len(off) % 256 == 0 and len(base) == len(off) // 32
    assert np.array_equal(base, rbase) and np.array_equal(off, roff)
    # exact outside wide groups; wide exactly when the span reaches 2^16; zero / wide padding
    g = np.arange(n) >> 5
    ok = ~wide[g]
    assert np.array_equal(base[g][ok].astype(np.int64) + off[:n][ok], x[ok].astype(np.int64))
    assert np.array_equal(base[:len(wide)] == WIDE, wide)
    assert (off[:n][~ok] == 0).all() and (off[n:] == 0).all() and (base[len(wide):] == WIDE).all()
    return wide


def test_host_encoder_equals_numpy_reference():
    import torch
    from hyperspace_amd.exec import encoding as E
    some_wide = some_big = False
    for n in SIZES[1:]:
        x = _codes(n)
        r = E.group16_32(torch.from_numpy(x), 1.0)
        wide = _check_form(x, r[0].numpy().view(np.uint16), r[1].numpy())
        some_wide |= bool(wide.any()) and not wide.all()
        some_big |= bool((r[0].numpy().view(np.uint16) >= 32768).any())
        # refused above the share of wide groups asked for
        assert (E.group16_32(torch.from_numpy(x), 0.0) is None) == bool(wide.any())
    assert some_wide and some_big
    x = _codes(20_011)
    wide = _ref32(x)[2]
    assert wide[12] and not wide[11] and wide[5] and wide[20] and wide[31] and wide[40]
    assert not wide[2] and not wide[3]          # a gap between two groups widens neither
    assert E.group16_32(torch.from_numpy(x[:0].copy()), 1.0) is None


def _k16_compacts():
    import torch
    from hyperspace_amd.exec.encoding import Compact, RunCompact
    c = dict(_q3_compacts())
    c[2] = Compact(None, 4, 0, 100.0, NL.F64)
    z = torch.zeros(4, dtype=torch.int32)
    c[0] = RunCompact(Compact(None, 4, 0, None, NL.I64, 0, 1000), z, z.long(), z)
    c[8] = Compact(None, 4, 0, None, NL.I64, 0, 1000)
    return c


def test_lowering_selects_the_k16_form():
    from hyperspace_amd.exec import jit_runs, kernel_config
    from hyperspace_amd.exec.encoding import Compact, GroupedCompact
    p, c = _q3_params(), _k16_compacts()
    pr = jit_runs.prune_plan(p, c, 1)
    assert pr
    with kernel_config.use(rt2_k16=False):
        assert not jit_runs.tags2_k16(p, c, True)
        off = [jit_runs.gen_run_tags2(p, c, 1, True, "", q).src for q in ((), pr)]
        shp = [jit_runs.tags2_shape(p, c, 1, True, "", q) for q in ((), pr)]
    with kernel_config.use(rt2_k16=True):
        assert jit_runs.tags2_k16(p, c, True) and jit_runs.tags2_wide(p, c, True) == 4
        # the 32-bit kernel's source and shape do not change with the switch alone
        assert off == [jit_runs.gen_run_tags2(p, c, 1, True, "", q).src for q in ((), pr)]
        assert shp == [jit_runs.tags2_shape(p, c, 1, True, "", q) for q in ((), pr)]
        for i, q in enumerate(((), pr)):
            k = jit_runs.gen_run_tags2(p, c, 1, True, "", q, True)
            assert jit_runs.tags2_shape(p, c, 1, True, "", q, True) != shp[i]
            assert jit_runs.tags2_shape(p, c, 1, True, "", q, True)[-1] == 4
            assert k.src != off[i] and "const hs_us4*)(a.LO16 +" in k.src
            assert "const hs_ro4*)(a.RO16 +" in k.src and "a.LG16[" in k.src and "a.RG16[" in k.src
            assert "IMGV(" in k.src and ("a.RMX1" in k.src) == bool(q)
            # the gallop and the 64-run code keep the 32-bit arrays
            assert "a.RK0[" in k.src and "a.c8[" in k.src
        # not covered: 64-bit indices, the recording / recorded forms, one run per lane
        assert not jit_runs.tags2_k16(p, c, False)
        for mode in ("rec", "match", "copy"):
            assert not jit_runs.tags2_k16(p, c, True, mode)
            assert jit_runs.tags2_shape(p, c, 1, True, mode, (), True) == \
                jit_runs.tags2_shape(p, c, 1, True, mode)
        with kernel_config.use(rt2_wide=1):
            assert not jit_runs.tags2_k16(p, c, True)
        with kernel_config.use(rt2_lo16=True):
            assert not jit_runs.tags2_k16(p, c, True)
        # a nullable right key, a right key stored grouped, stored at full width or narrower
        pn = _q3_params()
        pn.cols[8] = _fake(NL.I64, True)
        assert not jit_runs.tags2_k16(pn, c, True)
        for rc in (GroupedCompact(None, None, None, 0, NL.I64, 0, 1), None,
                   Compact(None, 2, 0, None, NL.I64, 0, 1000)):
            cc = dict(c)
            cc[8] = rc
            if rc is None:
                del cc[8]
            assert not jit_runs.tags2_k16(p, cc, True)
        # a left key without the run form
        cc = dict(c)
        cc[0] = Compact(None, 4, 0, None, NL.I64, 0, 1000)
        assert not jit_runs.tags2_k16(p, cc, True)


def test_k16_sources_compile(rt, tmp_path):  # noqa: F811
    from hyperspace_amd.exec import jit_runs, kernel_config
    jit = rt
    p, c = _q3_params(), _k16_compacts()
    rg = _q3_params()
    rg.preds[2] = rg.preds[1]
    rg.preds[1] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 1, 0, 7, 0, 9100, 0.0, None)
    rg.nlp, rg.npreds = 2, 3
    with kernel_config.use(rt2_k16=True):
        ks = [jit_runs.gen_run_tags2(p, c, 1, True, "", (), True)]
        for q in (p, rg):
            ks.append(jit_runs.gen_run_tags2(q, c, 1, True, "", jit_runs.prune_plan(q, c, 1), True))
        with kernel_config.use(rt2_unroll=1):       # one block per stage
            ks.append(jit_runs.gen_run_tags2(p, c, 1, True, "", jit_runs.prune_plan(p, c, 1), True))
    assert len({k.src for k in ks}) == 4
    for k in ks:
        rc = jit.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                                   str(tmp_path).encode())
        assert rc == 0, jit.runtime().hs_jit_last_error().decode()


# ------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_native_encoder_equals_numpy_reference(device):
    import torch
    from hyperspace_amd.ops import kernels as K
    for n in SIZES:
        x = _codes(n)
        off, base = K.group16_32(torch.from_numpy(x).to(device))
        torch.cuda.synchronize()
        _check_form(x, off.cpu().numpy().view(np.uint16), base.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _data(kind: str = "mixed"):
    """Bucket-sorted join inputs (host) in the shape of ``test_run_prune._data``: ~20 k unique
    sorted right keys, 1-7 left rows per key (one key with LONG_RUN rows), ~5 % unmatched keys
    on each side, an empty bucket, a run count that is no multiple of 4.

    Buckets 0 and 1 hold 1300 runs each (whole 512-run stages lie inside them:
    ``test_fast_stages_see_the_cases``), one run per right row and no match: every left key is its guessed
    right row's key + 65536 (bucket 0: those right keys lie below every left key, outside the
    key frame) or - 2 * 65536 (bucket 1), so the low halves of the two codes are equal at the
    guess and group bases differ.  Bucket 3's keys lie 1500 apart: offsets reach 32768 and
    more.  Bucket 5 has, past its first 512 runs, a stretch of keys the right side lacks (a
    wide group on the left only), one the left side lacks (right only) and a gap in both.  The
    last bucket's tail of right keys lies above every left key.  ``kind`` "sparse": every key
    3000 apart, so every group is wide and the form is refused."""
    rng = np.random.default_rng(29)
    lks, rks, key0 = [], [], 1 << 20
    if kind == "sparse":
        plan = [(2500, 3000, ""), (0, 3000, ""), (2500, 3000, "")]
    else:
        plan = [(1300, 40, "adv+"), (1300, 40, "adv-"), (0, 40, ""), (2400, 1500, "long"),
                (2600, 40, ""), (5000, 40, "wide"), (2300, 40, ""), (5000, 40, "above")]
    for n, step, what in plan:
        rk = key0 + step * np.arange(1, n + 1, dtype=np.int64)
        if what == "wide":
            rk[2010:] += 100_000                # a gap on both sides
            rk[1400:] += 90_000                 # a gap the left side fills (below): right only
            rk[800:] += 360 * np.minimum(np.arange(n - 800), 200)   # rows 800 .. 1000: 400 apart
        key0 = (rk[-1] if n else key0) + 400_000
        if what.startswith("adv"):
            lk = rk + (65536 if what == "adv+" else -2 * 65536)
            lks.append(lk)
            rks.append(rk)
            continue
        per = rng.integers(1, 8, n)
        if n:
            per[rng.random(n) < 0.05] = 0
        if what == "long":
            per[1200] = LONG_RUN
        if what == "wide":
            per[798:1002] = 0                   # 80 000 codes of right keys without left rows
        if what == "above":
            per[-400:] = 0
        lk = np.repeat(rk, per)
        if n:
            at = rng.integers(0, n, 300)
            if what == "wide":
                at = at[(at < 790) | (at > 1010)]
            extra = rk[at] + 1
            if what == "wide":                  # 100 left keys in the right side's gap
                extra = np.concatenate([extra, rk[1399] + 800 * np.arange(1, 101)])
            lk = np.sort(np.concatenate([lk, extra]))
        lks.append(lk)
        rks.append(rk)
    lk, rk = np.concatenate(lks), np.concatenate(rks)
    while len(np.unique(lk)) % 4 == 0 or len(lk) % 64 == 0:
        lk = lk[:-1]
        lks[-1] = lks[-1][:-1]
    assert (np.diff(lk) >= 0).all() and (np.diff(rk) > 0).all()
    d = {"lk": lk, "rk": rk,
         "loff": np.concatenate([[0], np.cumsum([len(x) for x in lks])]).astype(np.int64),
         "roff": np.concatenate([[0], np.cumsum([len(x) for x in rks])]).astype(np.int64),
         "ldate": rng.integers(0, 1000, len(lk)).astype(np.int32),
         "lprice": np.round(rng.random(len(lk)) * 1000, 2),
         "lqty": rng.integers(0, 1 << 30, len(lk)).astype(np.int64),
         "rdate": rng.integers(0, 1000, len(rk)).astype(np.int32)}
    d["starts"] = np.flatnonzero(np.concatenate([[True], lk[1:] != lk[:-1]]))
    return d


def test_join_data_holds_the_cases():
    """The host data has what its docstring claims, in the encoding the kernel reads."""
    d = _data()
    runkeys = d["lk"][d["starts"]]
    lcode = (runkeys - d["rk"].min() - (1 << 30)).astype(np.int32)   # one bias for both sides
    rcode = (d["rk"] - d["rk"].min() - (1 << 30)).astype(np.int32)
    lo, lb, lw = _ref32(lcode)
    ro, rb, rw = _ref32(rcode)
    assert 0 < lw.mean() < 0.03 and 0 < rw.mean() < 0.03
    # colliding low halves at the guessed row, in narrow groups with different bases
    for b in (0, 1):
        assert d["loff"][b] == d["roff"][b] and d["loff"][b + 1] == d["roff"][b + 1]
        sl = slice(int(d["roff"][b]), int(d["roff"][b + 1]))
        assert ((runkeys[sl] - d["rk"][sl]) % 65536 == 0).all() and (runkeys[sl] != d["rk"][sl]).all()
        g = np.arange(sl.start, sl.stop) >> 5
        inner = (g > g.min()) & (g < g.max())
        assert inner.sum() > 200 and not lw[g][inner].any() and not rw[g][inner].any()
        assert np.array_equal(lo[sl][inner], ro[sl][inner]) and (lb[g] != rb[g])[inner].all()
    assert (lo >= 32768).any() and (ro >= 32768).any()
    assert d["rk"].min() < d["lk"].min() and d["rk"].max() > d["lk"].max()
    # wide groups on one side only and on both (by key range), past bucket 5's first 512 runs
    r0 = np.searchsorted(runkeys, d["lk"][d["loff"][5]])
    lwk = [(runkeys[32 * g], runkeys[min(32 * g + 31, len(runkeys) - 1)]) for g in np.flatnonzero(lw)
           if 32 * g >= r0 + 512 and 32 * g + 32 <= np.searchsorted(runkeys, d["lk"][d["loff"][6]])]
    rwk = [(d["rk"][32 * g], d["rk"][32 * g + 31]) for g in np.flatnonzero(rw)
           if d["roff"][5] <= 32 * g and 32 * g + 32 <= d["roff"][6]]

    def overlaps(a, others):
        return any(a[0] <= o[1] and o[0] <= a[1] for o in others)
    assert any(not overlaps(a, rwk) for a in lwk) and any(not overlaps(a, lwk) for a in rwk)
    assert any(overlaps(a, rwk) for a in lwk)
    nruns = len(runkeys)
    assert nruns % 4 and nruns % 256 and len(d["lk"]) % 64
    assert (np.diff(np.concatenate([d["starts"], [len(d["lk"])]])) == LONG_RUN).any()
    sp = _data("sparse")
    assert _ref32((sp["rk"] - sp["rk"].min()).astype(np.int32))[2].mean() > 0.9


def _stage_walk(d, sub: bool, grid: int, U: int):
    """Host model of the four-run kernel's walk over its 256-run blocks (``_Tags2.block_loop``
    with ``k16``) for the ranges of ``_ranges(d, sub)``: per wavefront the events
    ("fast", first run, guess base) - a stage of U blocks resolved from the 16-bit arrays -,
    ("wide", first run, left wide, right wide) - a loaded stage that met a wide group and left
    the pipeline - and ("slow", first run) - a block through the 64-run code."""
    runkeys, rk = d["lk"][d["starts"]], d["rk"]
    # the stored codes: value - (smallest value + 2^31), per column (exec/encoding.py)
    lw = _ref32((runkeys - d["lk"].min() - (1 << 31)).astype(np.int32))[2]
    rw = _ref32((rk - rk.min() - (1 << 31)).astype(np.int32))[2]
    starts, lens = _ranges(d, sub)
    keep = lens > 0
    b_ = np.flatnonzero(keep)
    first = np.searchsorted(d["starts"], starts[keep], "right") - 1
    last = np.searchsorted(d["starts"], starts[keep] + lens[keep] - 1, "right") - 1
    RG = sorted(zip(first, last + 1, d["roff"][b_], d["roff"][b_ + 1]))
    NR, NRG, INF = len(runkeys), len(RG), 1 << 62
    NB, G, R = (NR + 255) >> 8, (NR + 63) >> 6, 256 * U
    nwv = grid * 4
    per = ((NB + nwv - 1) // nwv + U - 1) // U * U

    def match(r, a0, a1):       # (hit, lower-bound row) of run r in right rows [a0, a1)
        m = a0 + int(np.searchsorted(rk[a0:a1], runkeys[r]))
        return m < a1 and rk[m] == runkeys[r], m

    waves = []
    for wv in range(nwv):
        bbeg = wv * per
        bend = min(NB, bbeg + per)
        if bbeg >= bend or NRG <= 0:
            continue
        gend = min(G, bend << 2)
        ev = []
        rg = max([0] + [m for m in range(NRG) if RG[m][0] <= (bbeg << 8)])
        lr0, lr1, s0, s1 = RG[rg]
        nxt0 = RG[rg + 1][0] if rg + 1 < NRG else INF
        gbase, slow, nb = -1, 0, bbeg

        def fast(blk, off):
            rb = blk << 8
            base = gbase + off if gbase >= 0 else s0 + (rb - lr0)
            return (slow == 0 and blk + U <= bend and rb >= lr0 and rb + R <= lr1 and
                    rb + R <= NR and rb + R <= nxt0 and base >= s0 and base + R <= s1), rb, base

        while nb < bend:
            while nxt0 <= (nb << 8):
                rg += 1
                lr0, lr1, s0, s1 = RG[rg]
                gbase = -1
                nxt0 = RG[rg + 1][0] if rg + 1 < NRG else INF
            f, rb, base = fast(nb, 0)
            if not f:
                ev.append(("slow", nb << 8))
                for gi in range(nb << 2, min((nb + 1) << 2, gend)):
                    while nxt0 <= (gi << 6):
                        rg += 1
                        lr0, lr1, s0, s1 = RG[rg]
                        gbase = -1
                        nxt0 = RG[rg + 1][0] if rg + 1 < NRG else INF
                    r = (gi << 6) + 63
                    own, (l0, l1, a0, a1) = r < nxt0, (lr0, lr1, s0, s1)
                    if not own:
                        l0, l1, a0, a1 = RG[max(q for q in range(NRG) if RG[q][0] <= r)]
                    hit, m = (r < NR and l0 <= r < l1 and a1 > a0) and match(r, a0, a1) or (False, 0)
                    gbase = m + 1 if hit and own else -1
                slow -= 1 if slow > 0 else 0
                nb += 1
                continue
            pb = base
            while True:
                fn, _, basen = fast(nb + U, R)
                lwd = bool(lw[(nb << 8) >> 5:((nb << 8) + R) >> 5].any())
                rwd = bool(rw[pb >> 5:((pb + R - 1) >> 5) + 1].any())
                if lwd or rwd:
                    ev.append(("wide", nb << 8, lwd, rwd))
                    slow = U
                    break
                ev.append(("fast", nb << 8, pb))
                hit, m = match((nb << 8) + R - 1, s0, s1)
                gbase = m + 1 if hit else -1
                nb += U
                if not fn:
                    break
                pb = basen
        waves.append(ev)
    return waves


def test_fast_stages_see_the_cases():
    """By the host model of the stage walk: fast stages resolve whole 512-run stretches of
    bucket 1, where the guessed right row's key is in the key frame and equals the run's key in
    its low half only; every configuration of the GPU tests takes fast stages; and with long
    per-wavefront chunks loaded stages meet the wide groups of bucket 5 - left only, right only,
    both - and at least one of them follows a fast stage."""
    d = _data()
    runkeys, rk = d["lk"][d["starts"]], d["rk"]
    for sub in (False, True):
        for grid, U in ((16384, 2), (2, 2), (1, 1)):        # CFGS below
            waves = _stage_walk(d, sub, grid, U)
            evs = [e for w in waves for e in w]
            nfast = sum(e[0] == "fast" for e in evs)
            assert nfast * 256 * U > 0.4 * len(runkeys), (sub, grid, U, nfast)
            assert any(e[0] == "wide" for e in evs) and any(e[0] == "slow" for e in evs)
            # every block is taken once: fast stages and slow blocks tile the run list
            took = sorted([(e[1], 256 * U) for e in evs if e[0] == "fast"] +
                          [(e[1], 256) for e in evs if e[0] == "slow"])
            assert took[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(took, took[1:]))
            assert took[-1][0] + took[-1][1] >= len(runkeys)
            if sub:
                continue
            # colliding low halves, in frame, at the guess of a fast stage
            lo, hi = int(d["roff"][1]), int(d["roff"][2])
            seen = 0
            for e in evs:
                if e[0] == "fast" and lo <= e[1] and e[1] + 256 * U <= hi:
                    r = np.arange(e[1], e[1] + 256 * U)
                    j = e[2] + (r - e[1])
                    dk = runkeys[r] - rk[j]
                    assert (dk % 65536 == 0).all() and (dk != 0).all()
                    assert (rk[j] >= d["lk"].min()).all() and (rk[j] <= d["lk"].max()).all()
                    seen += len(r)
            assert seen >= 512, (grid, U, seen)
            if grid > 2:
                continue
            # wide stages right after a fast one, among bucket 5's runs
            b5 = (np.searchsorted(runkeys, d["lk"][d["loff"][5]]),
                  np.searchsorted(runkeys, d["lk"][d["loff"][6] - 1]))
            wide = {(e[2], e[3]) for e in evs if e[0] == "wide" and b5[0] <= e[1] <= b5[1]}
            after = {(e[2], e[3]) for w in waves for p_, e in zip(w, w[1:])
                     if p_[0] == "fast" and e[0] == "wide" and b5[0] <= e[1] <= b5[1]}
            print(grid, U, wide, after)
            assert wide == {(True, False), (False, True), (True, True)} and after, (wide, after)


@functools.lru_cache(maxsize=None)
def _device_inputs(kind: str = "mixed", nullable_key: bool = False, grouped_key: bool = False):
    import torch
    from hyperspace_amd.exec.encoding import encode
    dev = torch.device("cuda:0")
    d = _data(kind)
    rk = pa.array(d["rk"], mask=np.zeros(len(d["rk"]), bool) | (np.arange(len(d["rk"])) == 7)) \
        if nullable_key else pa.array(d["rk"])
    cols = {0: pa.array(d["lk"]), 1: pa.array(d["ldate"]), 2: pa.array(d["lprice"]),
            3: pa.array(d["lqty"]), 8: rk, 9: pa.array(d["rdate"])}
    dc = {s: _col(a, dev) for s, a in cols.items()}
    comp = {s: e for s, e in ((s, encode(c)) for s, c in dc.items()) if e is not None}
    assert comp[0].width == 4 and comp[8].width == 4 and comp[1].width == 2
    if grouped_key:     # the right key stored as 16-bit codes over 64-row groups
        from hyperspace_amd.exec.encoding import grouped16
        comp[8] = grouped16(comp[8], 1.0)
        assert comp[8] is not None and comp[8].signature() == (2, False, 64)
    B = len(d["loff"]) - 1
    rng_t = {}
    for sub in (False, True):
        starts, lens = _ranges(d, sub)
        rng_t[sub] = (torch.from_numpy(starts.astype(np.int64)).to(dev),
                      torch.from_numpy(lens.astype(np.int64)).to(dev),
                      torch.arange(B, dtype=torch.int32, device=dev),
                      torch.from_numpy(d["roff"]).to(dev))
    return dc, comp, rng_t


def _tags(lz, d) -> np.ndarray:
    import torch
    torch.cuda.synchronize()
    return lz.tags[:(len(d["starts"]) + 31) // 32].cpu().numpy().copy()


def _is_k16(lz) -> bool:
    return "a.LO16 +" in lz.kt.src and "a.RG16[" in lz.kt.src


# (grids: one stage per wavefront; long chunks, so a wide stage follows fast ones; one block
# per stage)
CFGS = ({}, {"rt2_wide_grid": 2}, {"rt2_wide_grid": 1, "rt2_unroll": 1})


@pytest.mark.gpu
@pytest.mark.parametrize("prune", [True, False])
def test_k16_join_equals_numpy_and_the_32_bit_kernel(device, prune):
    d = _data()
    dc, comp, rng_t = _device_inputs()
    n = len(d["lk"])
    for lit, rlit in ((300, 500), (-5, 1500)):
        p = _params(dc, [(">", lit, 0)], rlit)
        lmask = d["ldate"] > lit
        for sub in (False, True):
            es, ec = _expect(d, *_ranges(d, sub), lmask, rlit)
            for cfg in CFGS:
                rs, rc, l32 = _run(p, comp, rng_t[sub], n, pruned=prune, rs_prune=prune,
                                   rt2_k16=False, **cfg)
                t32 = _tags(l32, d)
                s_, c_, l16 = _run(p, comp, rng_t[sub], n, pruned=prune, rs_prune=prune,
                                   rt2_k16=True, **cfg)
                t16 = _tags(l16, d)
                print(prune, lit, sub, cfg, c_, ec, s_, es)
                assert _is_k16(l16) and not _is_k16(l32), cfg
                assert l16.kt.src != l32.kt.src and "a.LO16" not in l32.kt.src
                assert c_ == ec == rc, (lit, sub, cfg)
                assert np.allclose(s_, es, rtol=1e-12), (lit, sub, cfg)
                assert s_ == rs, (lit, sub, cfg)                  # bit-identical sums
                assert np.array_equal(t16, t32), (lit, sub, cfg)  # bit-identical tags
    assert ec > 0


@pytest.mark.gpu
def test_colliding_low_halves_do_not_match(device):
    """Buckets 0 and 1 alone: every run's guessed right row has a key with the run's low half
    and another high half; no run may be tagged."""
    d = _data()
    dc, comp, rng_t = _device_inputs()
    n = len(d["lk"])
    p = _params(dc, [(">", -5, 0)], 1500)           # every row passes both predicates
    rt_ = tuple(t[:2].contiguous() if i < 3 else t for i, t in enumerate(rng_t[False]))
    s_, c_, lz = _run(p, comp, rt_, n, pruned=True, rt2_k16=True)
    assert _is_k16(lz) and c_ == 0
    assert not _tags(lz, d)[:int(d["roff"][2]) // 32].any()
    # ... and the matching buckets beside them still match
    es, ec = _expect(d, *_ranges(d, False), np.ones(n, bool), 1500)
    s_, c_, lz = _run(p, comp, rng_t[False], n, pruned=True, rt2_k16=True)
    assert c_ == ec > 0 and np.allclose(s_, es, rtol=1e-12)
    assert not _tags(lz, d)[:int(d["roff"][2]) // 32].any()


@pytest.mark.gpu
def test_one_k16_launcher_rebinds_literals(device):
    d = _data()
    dc, comp, rng_t = _device_inputs()
    n = len(d["lk"])
    p = _params(dc, [(">", 300, 0)])
    _, _, lz = _run(p, comp, rng_t[False], n, pruned=True, rt2_k16=True)
    assert _is_k16(lz) and lz.graphable()
    for graph in (False, True):
        for lit, rlit in ((900, 500), (120, 700), (640, 250)):
            p = _params(dc, [(">", lit, 0)], rlit)
            es, ec = _expect(d, *_ranges(d, False), d["ldate"] > lit, rlit)
            out = lz.launch(p, key=(lit, rlit), graph=graph)
            got = out.result() if graph else [t.cpu().numpy() for t in out]
            assert int(np.asarray(got[1]).reshape(-1)[1]) == ec, (graph, lit, rlit)
            assert np.allclose(np.asarray(got[0]).reshape(-1)[0], es, rtol=1e-12), (graph, lit)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sparse_keys", "nullable_key", "grouped_key", "record",
                                  "one_run", "i64"])
def test_uncovered_joins_keep_the_32_bit_kernel(device, case):
    from hyperspace_amd.exec import kernel_config
    kind = "sparse" if case == "sparse_keys" else "mixed"
    d = _data(kind)
    dc, comp, rng_t = _device_inputs(kind, case == "nullable_key", case == "grouped_key")
    n = len(d["lk"])
    p = _params(dc, [(">", 300, 0)])
    cfg = {"record": True, "rt2_match": True} if case == "record" else \
        {"rt2_wide": 1} if case == "one_run" else {"rt2_i32": False} if case == "i64" else {}
    rs, rc, l32 = _run(p, comp, rng_t[False], n, rt2_k16=False, **cfg)
    s_, c_, l16 = _run(p, comp, rng_t[False], n, rt2_k16=True, **cfg)
    assert not _is_k16(l16) and l16.kt.src == l32.kt.src and "a.LO16" not in l16.kt.src, case
    assert c_ == rc and s_ == rs, case
    if case != "nullable_key":
        es, ec = _expect(d, *_ranges(d, False), d["ldate"] > 300)
        assert c_ == ec and np.allclose(s_, es, rtol=1e-12), case
    if case == "record":
        # the launcher's second launch records the match and switches phase 1 to the "copy" /
        # "match" form: still without the 16-bit key arguments, same result
        with kernel_config.use(rt2_k16=True, rt2_match=True, rt2_copy=False, mj_2p=True):
            got = [t.cpu().numpy() for t in l16.launch(p)]
        assert l16.kt.src != l32.kt.src and "a.LO16" not in l16.kt.src
        assert ("a.HIT[" in l16.kt.src) or ("a.MATCH[" in l16.kt.src)
        assert int(got[1].reshape(-1)[1]) == ec and got[0].reshape(-1)[0] == s_
