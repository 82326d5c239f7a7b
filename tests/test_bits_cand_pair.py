"""The pair form of the candidate phase 2 (exec/jit_runs.py ``rs_pair``, kernel
``hs_jit_run_bits_cand2``): one pass over the tiles gathers the tail words of two paired queries'
candidates once; each query keeps its own predicate test, list, walk and partials.

CPU tier: which lowerings get the form, what its source holds, and that it compiles for gfx950.
GPU tier, kernel level: one ``launch_pair`` equals two ``launch`` calls exactly (results and both
bitmaps), over tables and literal sets that take the union path, the dense path and both in one
launch - which path a set takes is computed on the host from the single launches' bitmaps and
asserted.  GPU tier, end to end: interleaved asynchronous join and filter queries equal
one-by-one ``collect()`` exactly with ``rs_pair`` on and off.
"""
import functools
import os

import numpy as np
import pyarrow as pa
import pytest

from hyperspace_amd.ops import _lib as NL
from test_jit import _agg, _col, _fake, _q3_params, rt  # noqa: F401
from test_tags2_keys16 import _k16_compacts
from test_tags2_pair import (LITERALS, _behind_busy_device, _check_pair, _counts, _join_data,
                             _lower, _q3, _q6, _query, _rows, _still_busy)

CAP = 1024      # list entries per wavefront and round (gen_run_sparse_scan)
TILE = 4096     # rows per wavefront tile


# ------------------------------------------------------------------------------------------------
# CPU tier: the form and its source
# ------------------------------------------------------------------------------------------------
def _cand(p, c):
    from hyperspace_amd.exec import jit_runs
    pr = jit_runs.prune_plan(p, c, 1)
    return tuple(dict.fromkeys(sl for _, sl, _ in pr))


def test_lowering_selects_the_pair_form():
    from hyperspace_amd.exec import jit_runs, kernel_config
    assert (CAP, TILE) == (jit_runs.BITS_CAP, jit_runs.BITS_TILE)
    p, c = _q3_params(), _k16_compacts()
    with kernel_config.use(rs_pair=True):
        cand = _cand(p, c)
        assert cand and jit_runs.cand_pair(p, c, cand)
        assert jit_runs.sparse_shape(p, c, None, None, cand, True) != \
            jit_runs.sparse_shape(p, c, None, None, cand)
        # refused: no prune plan, the hash and top-K walks, a grouped tail
        assert not jit_runs.cand_pair(p, c, ())
        assert not jit_runs.cand_pair(p, c, cand, hk=object())
        assert not jit_runs.cand_pair(p, c, cand, hk=object(), tk=object())
        g = _q3_params()
        g.cols[4] = _fake(NL.I32)
        g.group_col, g.num_groups, g.group_base = 4, 3, 0
        assert jit_runs._scan_grouped(g) and not jit_runs.prune_plan(g, c, 1)
        assert not jit_runs.cand_pair(g, c, cand)
        # the streaming form has no pair form: its shape key ignores the request
        assert jit_runs.sparse_shape(p, c, None, None, (), True) == jit_runs.sparse_shape(p, c)
    with kernel_config.use(rs_pair=False):
        assert not jit_runs.cand_pair(p, c, cand)
        assert jit_runs.sparse_shape(p, c, None, None, cand, True) == \
            jit_runs.sparse_shape(p, c, None, None, cand)
    with kernel_config.use(rs_pair=True, rs_lut=False):
        assert not jit_runs.cand_pair(p, c, cand)


def test_pair_source_holds_both_queries():
    from hyperspace_amd.exec import jit_runs, kernel_config
    p, c = _q3_params(), _k16_compacts()
    with kernel_config.use(rs_pair=True):
        cand = _cand(p, c)
        one = jit_runs.gen_run_sparse_scan(p, c, None, None, cand)
        two = jit_runs.gen_run_sparse_scan(p, c, None, None, cand, True)
    assert one.name == "hs_jit_run_bits_cand" and two.name == "hs_jit_run_bits_cand2"
    assert "tags_b" not in one.src and "_b;" not in one.src
    n1, n2 = [n for _, n, _ in one.args.slots], [n for _, n, _ in two.args.slots]
    # the single form's arguments, in order, among the pair's; the rest are the second set
    assert [n for n in n2 if not n.endswith("_b")] == n1
    lits = [n for n in n1 if jit_runs._LIT_SLOT2.match("a." + n)]
    assert {"CL0", "CH0", "A0_0", "B0_0", "A0_1", "B0_1"} <= set(lits)
    assert sorted(n for n in n2 if n.endswith("_b")) == \
        sorted([n + "_b" for n in lits + ["tags", "psum", "pcnt", "pmin", "pmax"]])
    for n in ("tags_b", "psum_b", "pcnt_b", "pmin_b", "pmax_b", "CL0_b", "A0_0_b"):
        assert "a." + n in two.src, n
    # a candidate's tail word is loaded in the filter pass as often as in the single source: once
    # per entry in the union path, and the dense path is the single loop once per query
    loads = one.src.count("PKc_[")
    assert loads == jit_runs.RS_WALK > 0
    union, dense = two.src.split("// union path")[1].split("// dense path")
    assert union.count("PKc_[") == loads and dense.count("PKc_[") == 2 * loads
    assert two.src.count("PKc_[") == 3 * loads
    # the union path walks each list once, the dense path is the single loop twice
    assert union.count("for (int cb = 0;") == 2 and dense.count("for (int cb = 0;") == 2
    assert union.count("for (;;)") == 0 and dense.count("for (;;)") == 2
    # both partial sets are flushed
    assert two.src.count("a.psum[o] =") == two.src.count("a.psum_b[o] =") == p.naggs
    # the tile split is the single form's
    for line in ("const i64 per = (ntiles + nwv - 1) / nwv;", "const i64 t0 = wid * per;"):
        assert line in one.src and line in two.src


def test_pair_sources_compile(rt, tmp_path):  # noqa: F811
    from hyperspace_amd.exec import jit_runs, kernel_config
    p, c = _q3_params(), _k16_compacts()
    ks = []
    for walk in (4, 2):
        with kernel_config.use(rs_pair=True, rs_walk=walk):
            ks.append(jit_runs.gen_run_sparse_scan(p, c, None, None, _cand(p, c), True))
    assert ks[0].src != ks[1].src
    for k in ks:
        rc = rt.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                                  str(tmp_path).encode())
        assert rc == 0, rt.runtime().hs_jit_last_error().decode()


# ------------------------------------------------------------------------------------------------
# GPU tier, kernel level
# ------------------------------------------------------------------------------------------------
# Sparse: both queries under CAP candidates in every tile, partly overlapping.  Mixed: sparse for
# one query, every run for the other - a wavefront with several tiles takes both paths.
SPARSE = ((480, 520, 300), (500, 540, 350))
EVERY = (-5, 2000, 1500)
SETS = dict(LITERALS, sparse=SPARSE, mixed=(SPARSE[0], EVERY), mixed_mirror=(EVERY, SPARSE[0]))
DENSE = ("nested", "none_all", "mixed", "mixed_mirror")


def _clustered(nkeys: int):
    """``_join_data`` with the left dates clustered per run (a run's rows lie within 80 days of
    each other, as a line item's ship dates lie near its order's date), so that the per-run
    bounds prune: a 40-day range keeps about a ninth of the runs, a third of those pass the
    right literal - 3-4 % of the rows are candidates."""
    d = dict(_join_data(nkeys))
    rng = np.random.default_rng(11)
    st, n = d["starts"], len(d["lk"])
    base = np.repeat(rng.integers(0, 920, len(st)), np.diff(np.append(st, n)))
    d["ldate"] = (base + rng.integers(0, 80, n)).astype(np.int32)
    return d


@functools.lru_cache(maxsize=None)
def _inputs(nkeys: int):
    """As ``test_tags2_pair._inputs``, over ``_clustered`` data."""
    import torch
    from hyperspace_amd.exec.encoding import Compact, encode
    dev = torch.device("cuda:0")
    d = _clustered(nkeys)
    cols = {0: pa.array(d["lk"]), 1: pa.array(d["ldate"]), 2: pa.array(d["lprice"]),
            3: pa.array(d["lqty"]), 8: pa.array(d["rk"]), 9: pa.array(d["rdate"])}
    dc = {s: _col(a, dev) for s, a in cols.items()}
    comp = {s: e for s, e in ((s, encode(c)) for s, c in dc.items()) if e is not None}
    for s in (0, 8):
        if comp[s].width != 4:      # (the one-key table: ``test_tags2_pair._inputs``)
            v = dc[s].data.long()
            lo, hi = int(v.min()), int(v.max())
            comp[s] = Compact((v - lo - (1 << 31)).to(torch.int32), 4, lo + (1 << 31), None,
                              dc[s].hs_type, lo, hi)
    B = len(d["loff"]) - 1
    rt_ = (torch.from_numpy(d["loff"][:-1].copy()).to(dev),
           torch.from_numpy(np.diff(d["loff"])).to(dev),
           torch.arange(B, dtype=torch.int32, device=dev), torch.from_numpy(d["roff"]).to(dev))
    return d, dc, comp, rt_


def _tile_counts(d, bitmap) -> list:
    """Per 4096-row tile of phase 2 (64-aligned from each range's start), the number of
    candidate rows: rows of the range whose run is tagged in ``bitmap`` (a single launch's)."""
    words = np.asarray(bitmap.cpu()).view(np.uint32)
    st, n = d["starts"], len(d["lk"])
    runs = np.arange(len(st))
    bits = ((words[runs >> 5] >> (runs & 31).astype(np.uint32)) & 1).astype(np.int64)
    rows = np.repeat(bits, np.diff(np.append(st, n)))
    out = []
    for b in range(len(d["loff"]) - 1):
        rs, re = int(d["loff"][b]), int(d["loff"][b + 1])
        tb = rs & ~63
        while tb < re:
            out.append((b, int(rows[max(tb, rs):min(tb + TILE, re)].sum())))
            tb += TILE
    return out


def test_clustered_tables_hold_the_cases():
    """Host side of what the GPU cases rely on: more than one tile in the first range of the
    large table, bucket starts off the 64-row grid, and sparse sets that prune."""
    d = _clustered(6000)
    assert d["loff"][1] - d["loff"][0] > TILE
    assert any(int(x) % 64 for x in d["loff"][1:-1])
    for lo, hi, _ in SPARSE:
        st, n = d["starts"], len(d["lk"])
        mx = np.maximum.reduceat(d["ldate"], st)
        mn = np.minimum.reduceat(d["ldate"], st)
        keep = (mx >= lo) & (mn < hi)
        assert 0.05 < keep.mean() < 0.2
        inside = (d["ldate"] >= lo) & (d["ldate"] < hi)
        assert 0 < inside.sum() < np.repeat(keep, np.diff(np.append(st, n))).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [None, 1])
@pytest.mark.parametrize("nkeys", [1, 255, 256, 257, 3000, 6000, 9600])
def test_pair_launch_equals_two_single_launches(device, monkeypatch, nkeys, grid):
    """``grid`` 1: four wavefronts walk every tile in turn (lists and counts reset between tiles,
    the accumulators carry); the default grid gives one tile per wavefront, the rest idle.
    6000 keys: the first range has two tiles and the bucket starts are off the 64-row grid;
    9600 keys: with grid 1 a wavefront gets a short tile (584 rows), an empty one and a full
    one, so the mixed sets take the union path and the dense path in one wavefront."""
    d, dc, comp, rt_ = _inputs(nkeys)
    assert len(d["starts"]) == nkeys
    cfg = {} if grid is None else {"rs_bits_grid": grid}
    lz = _lower(dc, comp, rt_, len(d["lk"]), True, monkeypatch, rs_pair=True, **cfg)
    # (the one-key table has no 16-bit date codes, so no pruned form: the three-kernel chain)
    assert (lz.ksp is not None) == (nkeys > 1)
    if lz.ksp is not None:
        assert lz.ksp.name == "hs_jit_run_bits_cand2" and lz.ks.name == "hs_jit_run_bits_cand"
        assert "a.tags_b[" in lz.ksp.src
    for name, lits in SETS.items():
        # three pairs of one launcher: the eager one, the capture and a replay
        reps = 3 if name in ("sparse", "mixed") and nkeys == 3000 else 1
        for rep in range(reps):
            want_t, want_r = _check_pair(lz, d, dc, lits, (nkeys, grid, name, rep))
        if reps > 1:
            # ... and a single-query replay afterwards equals the first result
            got = lz.launch(_query(dc, *lits[0]), key=((nkeys, grid, name, 0), "a") + lits[0],
                            graph=True).result()
            for x, y in zip(got, want_r[0]):
                assert np.array_equal(np.asarray(x), np.asarray(y))
            assert lz.graph.pairs and lz.graph.pair_replays >= 2
        # which path the tiles took
        tiles = [_tile_counts(d, t) for t in want_t]
        top = [max(c for _, c in t) for t in tiles]
        if name == "sparse":
            assert max(top) <= CAP, (nkeys, top)
            if nkeys >= 255:
                assert min(top) > 0 and not np.array_equal(*[np.asarray(t.cpu()) for t in want_t])
                assert all(int(np.asarray(r[1]).reshape(-1)[1]) > 0 for r in want_r)
        elif name in DENSE and nkeys >= 3000:
            assert max(top) > CAP, (nkeys, name, top)
        if name.startswith("mixed") and nkeys >= 3000:
            assert min(top) <= CAP < max(top)
            if nkeys == 9600 and grid == 1:
                # one wavefront takes both paths: grid 1 is four wavefronts over ``per``
                # consecutive tiles each; one of them gets a tile where both queries have
                # candidates but neither more than CAP, and a tile above CAP
                both = [(min(a[1], b[1]), max(a[1], b[1])) for a, b in zip(*tiles)]
                per = -(-len(both) // 4)
                assert any(any(0 < lo and hi <= CAP for lo, hi in both[i:i + per]) and
                           any(hi > CAP for _, hi in both[i:i + per])
                           for i in range(0, len(both), per)), both
    if nkeys == 6000:
        first = [b for b, _ in _tile_counts(d, want_t[0])]
        assert first.count(0) >= 2 and any(int(x) % 64 for x in d["loff"][1:-1])


@pytest.mark.gpu
def test_unpruned_launcher_pairs_through_the_old_chain(device, monkeypatch):
    d, dc, comp, rt_ = _inputs(3000)
    lz = _lower(dc, comp, rt_, len(d["lk"]), False, monkeypatch, rs_pair=True)
    assert lz.ksp is None and lz.ks.name == "hs_jit_run_bits_scan"
    for name in ("nested", "sparse"):
        for rep in range(3):
            _check_pair(lz, d, dc, SETS[name], ("old", name, rep))
    assert lz.graph.pairs


@pytest.mark.gpu
def test_pair_off_keeps_the_three_kernel_chain(device, monkeypatch):
    d, dc, comp, rt_ = _inputs(3000)
    lz = _lower(dc, comp, rt_, len(d["lk"]), True, monkeypatch, rs_pair=False)
    assert lz.ksp is None and lz.ks.name == "hs_jit_run_bits_cand"
    _check_pair(lz, d, dc, SETS["sparse"], ("off", 0))


# ------------------------------------------------------------------------------------------------
# GPU tier, end to end
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[True, False], ids=["rs_pair_on", "rs_pair_off"])
def env(request, tmp_path_factory):
    """The tables and indexes of ``test_tags2_pair.env`` under a session that sets ``rs_pair``."""
    from conftest import gpu_available
    if not gpu_available():
        pytest.skip("no GPU")
    import pyarrow.parquet as pq
    from hyperspace_amd import Hyperspace, IndexConfig, Session
    from hyperspace_amd.exec import kernel_config
    prev = kernel_config.active()
    tmp_path = tmp_path_factory.mktemp("candpair")
    rng = np.random.default_rng(5)
    n_ord = 20_000
    okeys = rng.permutation(np.arange(1, n_ord + 1, dtype=np.int64) * 4)
    od = pa.table({"o_orderkey": okeys,
                   "o_orderdate": pa.array(rng.integers(8000, 10500, n_ord).astype(np.int32))
                   .view(pa.date32()),
                   "o_shippriority": np.zeros(n_ord, np.int32)})
    lk = np.repeat(okeys, rng.integers(1, 8, n_ord))
    n = len(lk)
    li = pa.table({"l_orderkey": lk,
                   "l_quantity": rng.integers(1, 51, n).astype(np.float64),
                   "l_extendedprice": np.round(rng.random(n) * 1e5, 2),
                   "l_discount": rng.integers(0, 11, n) / 100.0,
                   "l_shipdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32))
                   .view(pa.date32())})
    for name, t in (("lineitem", li), ("orders", od)):
        os.makedirs(tmp_path / name)
        pq.write_table(t, tmp_path / name / "part-0.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.numBuckets": "8",
                      "spark.sql.autoBroadcastJoinThreshold": "-1",
                      "spark.hyperspace.mi.execution.device": "gpu",
                      "spark.hyperspace.mi.kernel.rs_pair": "true" if request.param else "false"},
                warehouse_dir=str(tmp_path / "wh"))
    hs = Hyperspace(s)
    lidf = s.read.parquet(str(tmp_path / "lineitem"))
    oddf = s.read.parquet(str(tmp_path / "orders"))
    hs.createIndex(lidf, IndexConfig("li_ship", ["l_shipdate"],
                                     ["l_discount", "l_quantity", "l_extendedprice"]))
    hs.createIndex(lidf, IndexConfig("li_ok", ["l_orderkey"],
                                     ["l_extendedprice", "l_discount", "l_shipdate"]))
    hs.createIndex(oddf, IndexConfig("od_ok", ["o_orderkey"], ["o_orderdate", "o_shippriority"]))
    Hyperspace.enable(s)
    for i in (100, 101, 102):
        _q3(lidf, oddf, i).collect()
        _q6(lidf, i).collect()
    yield s, lidf, oddf, request.param
    kernel_config.bind(prev)


@pytest.mark.gpu
def test_interleaved_async_queries_pair_up(env):
    from hyperspace_amd.exec import jit, jit_runs, kernel_config
    s, li, od, on = env
    assert kernel_config.active().rs_pair == on
    ids = [50 + k for k in range(5)]
    want = [(_rows(_q3(li, od, i).collect()), _rows(_q6(li, i).collect())) for i in ids]
    lz = jit.LAST_MJ_LAUNCHER[0]
    assert isinstance(lz, jit_runs.TwoPhaseLauncher) and lz.ktp is not None
    assert (lz.ksp is not None) == on and lz.ks.name == "hs_jit_run_bits_cand"
    p0, _ = _counts(s)
    primer = _behind_busy_device(s, li, od, 100)
    futs = []
    for i in ids:
        futs.append((_q3(li, od, i).collect_async(), _q6(li, i).collect_async()))
        if len(futs) == 3:
            _still_busy(primer)
    got = [(_rows(a.result()), _rows(b.result())) for a, b in futs]
    primer.result()
    assert _counts(s)[0] - p0 >= 1
    assert all(a.path == "native" and b.path == "native" for a, b in futs)
    assert got == want              # exactly: the same sums in the same order
    assert not s.backend().pair_gate.held
