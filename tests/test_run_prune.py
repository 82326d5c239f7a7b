"""The pruned pair of the two-phase run-keyed merge join (exec/jit_runs.py, ``rs_prune``):
phase 1 also tests per-run bounds of the left predicate columns (``hs_run_minmax16``), phase 2
(``hs_jit_run_bits_cand``) tests only the tagged runs' rows, on predicate fields of the
row-packed tail word.

GPU tier: the bounds kernel equals numpy's reduceat; the join equals numpy and, bit for bit,
the streaming pair (``rs_prune=False``) for every comparison, a range on one column, literals
below / above every value and equal to a run's bound, full and unaligned ranges, one and four
runs per lane and long per-wavefront chunks; a tile whose every row is a candidate takes
rounds; one launcher serves three literal vectors (plain and captured launches); joins the
pruned pair does not cover keep the streaming kernels.  CPU tier: which joins the lowering
gives the pruned pair, and its sources compile.
"""
import functools

import numpy as np
import pyarrow as pa
import pytest

from hyperspace_amd.ops import _lib as NL
from test_jit import _agg, _col, _fake, _q3_compacts, _q3_params, rt  # noqa: F401

OPS = {">": NL.OP_GT, ">=": NL.OP_GE, "<": NL.OP_LT, "<=": NL.OP_LE}
NPOP = {">": np.greater, ">=": np.greater_equal, "<": np.less, "<=": np.less_equal}
LONG_RUN = 200          # rows of one left key: the run crosses three 64-row group boundaries


@functools.lru_cache(maxsize=None)
def _data(dense: bool = False):
    """Bucket-sorted join inputs (host): 8 buckets, ~20 k unique sorted right keys, 1-7 left
    rows per key (one key with LONG_RUN rows), ~5 % of the right keys without left rows and
    left keys without a right row.  ``dense``: one bucket, every left key matched and every
    right row passing (the dense-tile case)."""
    rng = np.random.default_rng(23)
    sizes = [10_000] if dense else [2500, 2600, 0, 2400, 2700, 2500, 2300, 5000]
    lks, rks, key0 = [], [], 1 << 20
    for b, n in enumerate(sizes):
        rk = key0 + 40 * np.arange(1, n + 1, dtype=np.int64)     # a key span of 32-bit codes
        key0 += 40 * (n + 1000)
        per = rng.integers(1, 8, n)
        if not dense and n:
            per[rng.random(n) < 0.05] = 0
            if b == 3:
                per[1200] = LONG_RUN
        lk = np.repeat(rk, per)
        if not dense and n:
            lk = np.sort(np.concatenate([lk, rk[rng.integers(0, n, 300)] + 1]))
        lks.append(lk)
        rks.append(rk)
    lk, rk = np.concatenate(lks), np.concatenate(rks)
    # cut the table's tail: a run count that is no multiple of 4, a row count none of 64
    while len(np.unique(lk)) % 4 == 0 or len(lk) % 64 == 0:
        lk = lk[:-1]
        lks[-1] = lks[-1][:-1]
    d = {"lk": lk, "rk": rk,
         "loff": np.concatenate([[0], np.cumsum([len(x) for x in lks])]).astype(np.int64),
         "roff": np.concatenate([[0], np.cumsum([len(x) for x in rks])]).astype(np.int64),
         "ldate": rng.integers(0, 1000, len(lk)).astype(np.int32),
         "lprice": np.round(rng.random(len(lk)) * 1000, 2),
         "lqty": rng.integers(0, 1 << 30, len(lk)).astype(np.int64),
         "rdate": (np.zeros(len(rk)) if dense else rng.integers(0, 1000, len(rk))).astype(np.int32)}
    st = np.concatenate([[True], lk[1:] != lk[:-1]])
    d["starts"] = np.flatnonzero(st)
    return d


def _ranges(d, sub: bool):
    starts, lens = d["loff"][:-1].copy(), d["loff"][1:] - d["loff"][:-1]
    if sub:     # a run straddles each range edge (where the bucket has rows)
        big = lens > 9
        starts[big] += 5
        lens = np.where(big, lens - 9, lens)
    return starts, lens


def _expect(d, starts, lens, lmask, rlit: int = 500):
    """numpy: (sum, count) of the rows of the ranges with a right row of ``rdate < rlit`` and
    ``lmask`` set."""
    rows = np.concatenate([np.arange(s, s + n) for s, n in zip(starts, lens)])
    idx = np.minimum(np.searchsorted(d["rk"], d["lk"][rows]), len(d["rk"]) - 1)
    ok = (d["rk"][idx] == d["lk"][rows]) & (d["rdate"][idx] < rlit) & lmask[rows]
    val = d["lprice"][rows] * (1.0 + 0.001 * d["ldate"][rows])
    return float(val[ok].sum()), int(ok.sum())


@functools.lru_cache(maxsize=None)
def _device_inputs(dense: bool = False, nullable: bool = False):
    import torch
    from hyperspace_amd.exec.encoding import encode
    dev = torch.device("cuda:0")
    d = _data(dense)
    ldate = pa.array(d["ldate"], mask=(np.arange(len(d["lk"])) % 7 == 3)) if nullable else \
        pa.array(d["ldate"])
    cols = {0: pa.array(d["lk"]), 1: ldate, 2: pa.array(d["lprice"]), 3: pa.array(d["lqty"]),
            8: pa.array(d["rk"]), 9: pa.array(d["rdate"])}
    dc = {s: _col(a, dev) for s, a in cols.items()}
    comp = {s: e for s, e in ((s, encode(c)) for s, c in dc.items()) if e is not None}
    assert comp[1].width == 2 and comp[2].width == 4 and comp[3].width == 4
    B = len(d["loff"]) - 1
    rng_t = {}
    for sub in (False, True):
        starts, lens = _ranges(d, sub)
        rng_t[sub] = (torch.from_numpy(starts.astype(np.int64)).to(dev),
                      torch.from_numpy(lens.astype(np.int64)).to(dev),
                      torch.arange(B, dtype=torch.int32, device=dev),
                      torch.from_numpy(d["roff"]).to(dev))
    return dc, comp, rng_t


def _params(dc, lpreds, rlit: int = 500, wide_tail: bool = False):
    """Join parameters: left conjuncts ``lpreds`` ((op, literal, group) on the date column;
    op "notnull": IS NOT NULL, as the optimizer adds beside a comparison),
    the right predicate ``rdate < rlit``, SUM(price * (1 + 0.001 date)) and COUNT(*)."""
    p = NL.JoinParams()
    for s, c in dc.items():
        p.cols[s] = c.desc()
    for k, (op, lit, grp) in enumerate(lpreds):
        p.preds[k] = NL.Pred(NL.PK_NOT_NULL, 0, 1, 0, grp, 0, 0, 0.0, None) if op == "notnull" \
            else NL.Pred(NL.PK_INT_LIT, OPS[op], 1, 0, grp, 0, int(lit), 0.0, None)
    n = len(lpreds)
    p.preds[n] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 9, 0, 100, 0, rlit, 0.0, None)
    p.nlp, p.npreds = n, n + 1
    p.aggs[0] = _agg(NL.AK_SUM, [(2, 0.0, 1.0), (1, 1.0, 0.001)])
    p.aggs[1] = _agg(NL.AK_COUNT_STAR)
    p.naggs = 2
    if wide_tail:       # a third aggregate input: 32 + 16 + 32 bits do not fit the tail word
        p.aggs[2] = _agg(NL.AK_SUM, [(3, 0.0, 1.0)])
        p.naggs = 3
    p.lkey, p.rkey, p.key_is_float = 0, 8, 0
    p.group_col, p.num_groups, p.group_base = -1, 1, 0
    return p


def _run(p, comp, rt_, nrows, pruned=None, **cfg):
    """(sum, count, launcher) of one lowering + launch under ``cfg``; ``pruned``: which pair of
    kernels the launcher must hold (None: not checked)."""
    from hyperspace_amd.exec import jit, jit_runs, kernel_config
    kw = dict(rt2_match=False, rt2_copy=False, mj_2p=True)
    kw.update(cfg)
    record = kw.pop("record", False)
    with kernel_config.use(**kw):
        got = [t.cpu().numpy() for t in
               jit.merge_join_agg(p, *rt_, comp, nrows=nrows, rdup=False, record=record,
                                  cache_spans=record)]
        launcher = jit.LAST_MJ_LAUNCHER[0]
        assert isinstance(launcher, jit_runs.TwoPhaseLauncher)
    if pruned is not None:
        assert (launcher.ks.name == "hs_jit_run_bits_cand") == pruned, cfg
        assert ("clst_" in launcher.ks.src) == pruned and ("a.RM" in launcher.kt.src) == pruned
    # one group: aggregate 0 is the SUM, aggregate 1 the COUNT(*)
    return got[0].reshape(-1)[0], int(got[1].reshape(-1)[1]), launcher


@pytest.mark.gpu
def test_run_minmax16_equals_reduceat(device):
    import torch
    from hyperspace_amd.exec.encoding import key_runs
    from hyperspace_amd.ops import kernels as K
    d = _data()
    _, comp, _ = _device_inputs()
    runs = key_runs(comp[0])
    st = d["starts"]
    nruns, n = len(st), len(d["lk"])
    lens = np.diff(np.concatenate([st, [n]]))
    assert runs is not None and runs.nruns == nruns
    assert (lens == 1).any() and (lens == LONG_RUN).any()
    assert n % 64 and nruns % 4 and nruns % 256
    long0 = st[np.argmax(lens == LONG_RUN)]
    assert (long0 + LONG_RUN - 1) // 64 - long0 // 64 >= 3      # crosses three group edges
    codes = comp[1].codes
    assert codes.dtype == torch.int16
    mn, mx = K.run_minmax16(runs.gmask, runs.gruns, nruns, codes)
    torch.cuda.synchronize()
    img = codes.cpu().numpy().astype(np.int32) + 32768       # order-preserving uint16 image
    mn = mn.cpu().numpy().view(np.uint16)
    mx = mx.cpu().numpy().view(np.uint16)
    assert len(mn) == len(mx) == (nruns + 255) // 256 * 256
    assert np.array_equal(mn[:nruns], np.minimum.reduceat(img, st))
    assert np.array_equal(mx[:nruns], np.maximum.reduceat(img, st))
    assert (mn[nruns:] == 0xFFFF).all() and (mx[nruns:] == 0).all()


def _bound_literal(d, op: str) -> int:
    """A literal equal to one run's bound in the direction ``op`` prunes by: the run passes
    under >= / <= and fails under > / <."""
    st = d["starts"]
    r = 777
    seg = d["ldate"][st[r]:st[r + 1]]
    return int(seg.max() if op in (">", ">=") else seg.min())


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(OPS))
def test_pruned_join_matches_streaming_form_and_numpy(device, op):
    d = _data()
    dc, comp, rng_t = _device_inputs()
    n = len(d["lk"])
    for lit in (300, -5, 1500, _bound_literal(d, op)):
        # (under ">" with the IS NOT NULL conjunct a planned query carries: the literal slot is 1)
        p = _params(dc, [("notnull", 0, 3), (op, lit, 0)] if op == ">" else [(op, lit, 0)])
        lmask = NPOP[op](d["ldate"], lit)
        for sub in (False, True):
            es, ec = _expect(d, *_ranges(d, sub), lmask)
            rs, rc, _ = _run(p, comp, rng_t[sub], n, pruned=False, rs_prune=False)
            for cfg in ({"rt2_wide": 1}, {"rt2_wide": 4}, {"rt2_wide": 4, "rt2_wide_grid": 2},
                        {"rt2_wide": 1, "rt2_grid": 2}):
                s_, c_, _ = _run(p, comp, rng_t[sub], n, pruned=True, **cfg)
                print(op, lit, sub, cfg, c_, ec, s_, es)
                assert c_ == ec == rc, (op, lit, sub, cfg)
                assert np.allclose(s_, es, rtol=1e-12), (op, lit, sub, cfg)
                assert s_ == rs, (op, lit, sub, cfg)        # bit-identical sums


@pytest.mark.gpu
def test_pruned_join_range_on_one_column(device):
    """Two conjuncts on the date column: phase 1 reads the runs' minimum and maximum."""
    d = _data()
    dc, comp, rng_t = _device_inputs()
    n = len(d["lk"])
    for lo, hi in ((300, 420), (_bound_literal(d, ">"), _bound_literal(d, ">") + 3), (600, 500)):
        p = _params(dc, [(">=", lo, 0), ("<", hi, 1)])
        lmask = (d["ldate"] >= lo) & (d["ldate"] < hi)
        for sub in (False, True):
            es, ec = _expect(d, *_ranges(d, sub), lmask)
            rs, rc, _ = _run(p, comp, rng_t[sub], n, pruned=False, rs_prune=False)
            for cfg in ({"rt2_wide": 1}, {"rt2_wide": 4}, {"rt2_wide": 4, "rt2_wide_grid": 2}):
                s_, c_, lz = _run(p, comp, rng_t[sub], n, pruned=True, **cfg)
                assert "a.RMX1[" in lz.kt.src or "a.RMX1 +" in lz.kt.src
                assert "a.RMN1[" in lz.kt.src or "a.RMN1 +" in lz.kt.src
                assert c_ == ec == rc, (lo, hi, sub, cfg)
                assert np.allclose(s_, es, rtol=1e-12) and s_ == rs, (lo, hi, sub, cfg)


@pytest.mark.gpu
def test_dense_tile_takes_rounds(device):
    """Every run tagged and every row passing: a 4096-row tile has more candidates than one
    filter pass and more passing rows than the walk's list holds."""
    d = _data(True)
    dc, comp, rng_t = _device_inputs(True)
    n = len(d["lk"])
    assert n > 2 * 4096
    p = _params(dc, [(">", -5, 0)])
    es, ec = _expect(d, *_ranges(d, False), np.ones(n, bool))
    assert ec == n
    for cfg in ({"rt2_wide": 4}, {"rt2_wide": 4, "rs_bits_grid": 1}):
        s_, c_, _ = _run(p, comp, rng_t[False], n, pruned=True, **cfg)
        assert c_ == ec and np.allclose(s_, es, rtol=1e-12), cfg


@pytest.mark.gpu
def test_one_launcher_rebinds_literals(device):
    """Three literal vectors through one launcher, plain and as replays of the captured
    pipeline: the phase-1 bound literals are patched with phase 2's."""
    d = _data()
    dc, comp, rng_t = _device_inputs()
    n = len(d["lk"])
    p = _params(dc, [(">", 300, 0)])
    _, _, lz = _run(p, comp, rng_t[False], n, pruned=True, rt2_wide=4)
    assert lz.graphable()
    for graph in (False, True):
        for lit, rlit in ((900, 500), (120, 700), (640, 250)):
            p = _params(dc, [(">", lit, 0)], rlit)
            es, ec = _expect(d, *_ranges(d, False), d["ldate"] > lit, rlit)
            out = lz.launch(p, key=(lit, rlit), graph=graph)
            if graph:
                got = out.result()
            else:
                got = [t.cpu().numpy() for t in out]
            assert int(np.asarray(got[1]).reshape(-1)[1]) == ec, (graph, lit, rlit)
            assert np.allclose(np.asarray(got[0]).reshape(-1)[0], es, rtol=1e-12), (graph, lit)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nullable", "or_group", "wide_layout", "record"])
def test_uncovered_joins_keep_the_streaming_kernels(device, case):
    d = _data()
    dc, comp, rng_t = _device_inputs(False, case == "nullable")
    n = len(d["lk"])
    lmask = d["ldate"] > 300
    cfg = {}
    if case == "nullable":
        p = _params(dc, [(">", 300, 0)])
        lmask = lmask & (np.arange(n) % 7 != 3)
    elif case == "or_group":
        p = _params(dc, [(">", 800, 0), ("<", 100, 0)])
        lmask = (d["ldate"] > 800) | (d["ldate"] < 100)
    elif case == "wide_layout":
        p = _params(dc, [(">", 300, 0)], wide_tail=True)
    else:
        p = _params(dc, [(">", 300, 0)])
        cfg = {"record": True, "rt2_match": True}
    es, ec = _expect(d, *_ranges(d, False), lmask)
    rs, rc, _ = _run(p, comp, rng_t[False], n, pruned=False, rs_prune=False, **cfg)
    s_, c_, _ = _run(p, comp, rng_t[False], n, pruned=False, **cfg)
    assert c_ == ec == rc and s_ == rs and np.allclose(s_, es, rtol=1e-12), case


def test_lowering_selects_the_pruned_pair():
    """``prune_plan``: single-leaf <, <=, >, >= conjuncts on non-nullable 16-bit compact
    columns whose codes fit the tail word, 1-bit tags, plain aggregates, no recorded match."""
    from hyperspace_amd.exec import jit_runs, kernel_config
    from hyperspace_amd.exec.encoding import Compact
    c = dict(_q3_compacts())
    c[2] = Compact(None, 4, 0, 100.0, NL.F64)
    p = _q3_params()
    assert jit_runs.prune_plan(p, c, 1) == ((0, 1, True),)
    assert jit_runs.pack_layout(p, c, (1,)) == ((2, 0, 4), (3, 32, 1), (1, 40, 2))
    assert jit_runs.pack_layout(p, c) == ((2, 0, 4), (3, 32, 1))
    with kernel_config.use(rs_prune=False):
        assert jit_runs.prune_plan(p, c, 1) == ()
    assert jit_runs.prune_plan(p, c, 2) == () and jit_runs.prune_plan(p, c, 1, record=True) == ()
    assert jit_runs.prune_plan(p, c, 1, hk=object()) == ()
    lt = _q3_params()
    lt.preds[0] = NL.Pred(NL.PK_INT_LIT, NL.OP_LE, 1, 0, 0, 0, 9000, 0.0, None)
    assert jit_runs.prune_plan(lt, c, 1) == ((0, 1, False),)
    # an IS NOT NULL conjunct on the non-nullable column is passed over (its own group only)
    nn = _q3_params()
    nn.preds[2], nn.preds[1] = nn.preds[1], nn.preds[0]
    nn.preds[0] = NL.Pred(NL.PK_NOT_NULL, 0, 1, 0, 5, 0, 0, 0.0, None)
    nn.nlp, nn.npreds = 2, 3
    assert jit_runs.prune_plan(nn, c, 1) == ((1, 1, True),)
    nn.preds[0] = NL.Pred(NL.PK_NOT_NULL, 0, 1, 0, 0, 0, 0, 0.0, None)      # OR-ed with the compare
    assert jit_runs.prune_plan(nn, c, 1) == ()
    for bad in ("nullable", "eq", "or", "wide_code", "wide_layout", "grouped"):
        q, cc = _q3_params(), dict(c)
        if bad == "nullable":
            q.cols[1] = _fake(NL.I32, True)
        elif bad == "eq":
            q.preds[0] = NL.Pred(NL.PK_INT_LIT, NL.OP_EQ, 1, 0, 0, 0, 9000, 0.0, None)
        elif bad == "or":
            q.preds[2] = q.preds[1]
            q.preds[1] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 1, 0, 0, 0, 8100, 0.0, None)
            q.nlp, q.npreds = 2, 3
        elif bad == "wide_code":
            cc[1] = Compact(None, 4, 8000, None, NL.I32)
        elif bad == "wide_layout":
            cc[3] = Compact(None, 4, 0, 100.0, NL.F64)
        else:
            q.cols[4] = _fake(NL.I32)
            q.group_col, q.num_groups = 4, 3
        assert jit_runs.prune_plan(q, cc, 1) == (), bad
    # the shapes separate the pairs; the streaming sources do not change with the switch
    pr = jit_runs.prune_plan(p, c, 1)
    assert jit_runs.tags2_shape(p, c, 1, True, "", pr) != jit_runs.tags2_shape(p, c, 1, True)
    assert jit_runs.sparse_shape(p, c, cand=(1,)) != jit_runs.sparse_shape(p, c)
    with kernel_config.use(rs_prune=False):
        off = (jit_runs.gen_run_tags2(p, c, 1, True).src, jit_runs.gen_run_sparse_scan(p, c).src)
    assert off == (jit_runs.gen_run_tags2(p, c, 1, True).src,
                   jit_runs.gen_run_sparse_scan(p, c).src)


def test_pruned_sources_compile(rt, tmp_path):  # noqa: F811
    """Both kernels of the pruned pair (one bound, and a range's two) compile for gfx950; the
    four-run phase 1 loads a lane's four bounds at once and phase 2 reads no row stream."""
    from hyperspace_amd.exec import jit_runs
    from hyperspace_amd.exec.encoding import Compact
    jit = rt
    c = dict(_q3_compacts())
    c[2] = Compact(None, 4, 0, 100.0, NL.F64)
    p = _q3_params()
    rg = _q3_params()
    rg.preds[2] = rg.preds[1]
    rg.preds[1] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 1, 0, 7, 0, 9100, 0.0, None)
    rg.nlp, rg.npreds = 2, 3
    nn = _q3_params()
    nn.preds[2], nn.preds[1] = nn.preds[1], nn.preds[0]
    nn.preds[0] = NL.Pred(NL.PK_NOT_NULL, 0, 1, 0, 5, 0, 0, 0.0, None)
    nn.nlp, nn.npreds = 2, 3
    ks = []
    for q in (p, rg, nn):
        pr = jit_runs.prune_plan(q, c, 1)
        assert len(pr) == (1 if q is nn else q.nlp)
        wide = jit_runs.gen_run_tags2(q, c, 1, True, "", pr)
        one = jit_runs.gen_run_tags2(q, c, 1, False, "", pr)
        cand = jit_runs.gen_run_sparse_scan(q, c, None, None, (1,))
        assert "IMGV(" in wide.src and "const hs_us4*)(a.RMX1 +" in wide.src
        assert "a.RMX1[" in one.src and "IMGV(" not in one.src
        assert ("a.RMN1" in wide.src) == (q is rg)
        assert cand.name == "hs_jit_run_bits_cand" and "clst_" in cand.src
        assert "P12_" not in cand.src and "bload<" not in cand.src.split("void hs_jit")[1]
        lit = "a.CL1" if q is nn else "a.CL0"
        assert lit in wide.src and lit in cand.src
        ks += [wide, one, cand]
    for k in ks:
        rc = jit.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                                   str(tmp_path).encode())
        assert rc == 0, jit.runtime().hs_jit_last_error().decode()
