"""The captured pipelines of ``exec/graphs.py`` end in the fold kernel (``hs_agg_fold``): kernel
nodes only, results written into the slots' pinned host blocks, one capture per shape."""
import functools

import numpy as np
import pyarrow as pa
import pytest

from hyperspace_amd.ops import _lib as NL
from test_bits_cand_pair import SETS
from test_bits_cand_pair import _inputs as _clustered_inputs
from test_jit import _agg, _col, _scan_params
from test_tags2_pair import _lower, _query

NB = 5          # buckets of the scanned table
NROWS = 6000


def _same(got, want, what=""):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w.cpu() if hasattr(w, "cpu") else w)
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint64),
                              np.ascontiguousarray(w).view(np.uint64)), (what, g, w)


@pytest.fixture
def captures(monkeypatch):
    """Counts the stream captures begun through the runtime."""
    from hyperspace_amd.exec import jit
    R = jit.runtime()
    begin, calls = R.hs_graph_capture_begin, []
    monkeypatch.setattr(R, "hs_graph_capture_begin", lambda st: calls.append(st) or begin(st))
    return calls


# ------------------------------------------------------------------------------------------------
# Q6 shape: range search (bounds by value) -> tile prefix -> scan -> fold
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan_table():
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    sizes = rng.multinomial(NROWS, [0.3, 0.1, 0.0, 0.35, 0.25])      # (an empty bucket)
    key = np.concatenate([np.sort(rng.integers(0, 2000, n)) for n in sizes]).astype(np.int32)
    cols = {0: _col(pa.array(key), dev),
            1: _col(pa.array(rng.integers(0, 11, NROWS) / 100.0), dev),
            2: _col(pa.array(np.round(rng.random(NROWS) * 1000, 2)), dev)}
    boff = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
    return cols, boff


def _scan_query(cols, lo: int, hi: int, disc: float):
    preds = [NL.Pred(NL.PK_INT_LIT, NL.OP_GE, 0, 0, 0, 0, lo, 0.0, None),
             NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 0, 0, 1, 0, hi, 0.0, None),
             NL.Pred(NL.PK_FLT_LIT, NL.OP_GE, 1, 0, 2, 0, 0, disc, None)]
    aggs = [_agg(NL.AK_SUM, [(2, 0.0, 1.0), (1, 0.0, 1.0)]), _agg(NL.AK_MIN, [(2, 0.0, 1.0)]),
            _agg(NL.AK_MAX, [(2, 0.0, 1.0)]), _agg(NL.AK_COUNT_STAR)]
    return _scan_params({s: c.desc() for s, c in cols.items()}, preds, aggs)


def _scan_graph(cols, boff):
    from hyperspace_amd.exec import jit
    from hyperspace_amd.exec.graphs import ScanAggGraph
    p = _scan_query(cols, 0, 1, 0.0)
    k = jit.kernel_for(jit.scan_agg_shape(p, None, 0), lambda: jit.gen_scan_agg(p, None, 0))
    grid = jit.SCAN_GRID or NL.lib().hs_scan_grid()
    return ScanAggGraph(k, cols[0].desc(), boff, NB, grid, p.naggs, 0, boff.device, 0), k


def _scan_launch(g, k, cols, lo, hi, disc):
    from hyperspace_amd.exec import jit
    from hyperspace_amd.exec.graphs import _cbuf, range_bounds
    from hyperspace_amd.ops import kernels as K
    p = _scan_query(cols, lo, hi, disc)
    v = g.values_template()
    v.update({"num_groups": p.num_groups, "group_base": p.group_base, "nrows": 0})
    jit._fill_cols(v, p.cols, None)
    jit.fill_preds_aggs(v, [(i, p.preds[i]) for i in range(p.npreds)],
                        [p.aggs[i] for i in range(p.naggs)], None)
    bounds = range_bounds(K.sortable_image(lo, NL.I32), True, K.sortable_image(hi, NL.I32), False)
    return g.launch(bounds, _cbuf(k.args.pack(v, default=0)))


def _scan_eager(cols, boff, lo, hi, disc):
    from hyperspace_amd.exec import jit
    from hyperspace_amd.ops import kernels as K
    rs, rl, _ = K.range_search(cols[0], boff, None, K.sortable_image(lo, NL.I32), True,
                               K.sortable_image(hi, NL.I32), False)
    return [t.cpu().numpy() for t in jit.scan_agg(_scan_query(cols, lo, hi, disc), rs, rl)]


def _scan_lits(n: int):
    return [(50 * i, 2000 - 130 * i, 0.01 * (i % 7)) for i in range(n)]


@pytest.mark.gpu
def test_scan_graph_launches_queued_over_the_ring_equal_the_eager_path(device, captures):
    from hyperspace_amd.exec import graphs
    cols, boff = _scan_table()
    g, k = _scan_graph(cols, boff)
    lits = _scan_lits(2 * g.RING + 1)
    want = [_scan_eager(cols, boff, *x) for x in lits]
    assert len({w[0].tobytes() for w in want}) == len(want) and all(w[1][3] > 0 for w in want)
    hs = [_scan_launch(g, k, cols, *x) for x in lits]       # all queued before any is read
    for h, w, x in zip(hs, want, lits):
        _same(g.result(h), w, x)
    # one capture served every slot; the chain is four kernel nodes and no copy
    assert len(captures) == 1 and all(sl.graph is not None for sl in g.slots)
    assert [graphs.node_counts(sl.graph) for sl in g.slots] == [(4, 0, 0)] * g.RING
    assert g.replays == len(lits) - 1
    # a second round, read in reverse: no further capture in any slot
    hs = [_scan_launch(g, k, cols, *x) for x in lits[:g.RING]]
    for h, w in reversed(list(zip(hs, want))):
        _same(g.result(h), w)
    assert len(captures) == 1


# ------------------------------------------------------------------------------------------------
# Q3 shape: phase 1 -> phase 2 -> fold; a pair: pair phase 1 -> pair phase 2 -> ONE fold
# ------------------------------------------------------------------------------------------------
def _join_lits(n: int):
    return [(40 * i, 1000 - 35 * i, 300 + 60 * i) for i in range(n)]


@pytest.mark.gpu
def test_join_graph_launches_queued_over_the_ring_equal_the_eager_path(device, monkeypatch,
                                                                       captures):
    from hyperspace_amd.exec import graphs
    d, dc, comp, rt_ = _clustered_inputs(3000)
    lz = _lower(dc, comp, rt_, len(d["lk"]), True, monkeypatch, rs_pair=True)
    ring = graphs.TwoPhaseGraph.RING
    lits = _join_lits(2 * ring + 1)
    ps = [_query(dc, *x) for x in lits]
    want = [[t.cpu().numpy() for t in lz.launch(p)] for p in ps]          # eager, hs_agg_final
    assert len({w[0].tobytes() for w in want}) == len(want)
    pend = [lz.launch(p, key=("ring", i), graph=True) for i, p in enumerate(ps)]
    for h, w, x in zip(pend, want, lits):
        _same(h.result(), w, x)
    g = lz.graph
    assert len(captures) == 1 and g.replays == len(lits) - 1
    assert [graphs.node_counts(sl.graph) for sl in g.slots] == [(3, 0, 0)] * ring


@pytest.mark.gpu
@pytest.mark.parametrize("ksp", [True, False])
def test_pair_launch_equals_two_single_launches_in_every_position(device, monkeypatch, captures,
                                                                  ksp):
    """With the pair phase 2 (``ksp``) the pair's chain is three kernels with one fold of both
    partial sets; without it each query keeps its own fold (five kernels).  One capture of the
    pair and one of the single query serve every slot and every position of a pair in the ring
    (a single launch in between moves the pairs to the odd positions)."""
    from hyperspace_amd.exec import graphs
    d, dc, comp, rt_ = _clustered_inputs(3000)
    lz = _lower(dc, comp, rt_, len(d["lk"]), ksp, monkeypatch, rs_pair=True)
    assert (lz.ksp is not None) == ksp
    la, lb = SETS["sparse"]
    pa_, pb_ = _query(dc, *la), _query(dc, *lb)
    ka, kb = ("pos", "a") + tuple(la), ("pos", "b") + tuple(lb)
    wa = lz.launch(pa_, key=ka, graph=True).result()        # the eager single query
    wb = lz.launch(pb_, key=kb, graph=True).result()        # the single query's capture
    assert not np.array_equal(np.asarray(wa[0]), np.asarray(wb[0]))
    g = lz.graph
    assert len(captures) == 1
    seen = set()
    for rep in range(2 * g.RING + 2):
        if rep == g.RING:
            _same(lz.launch(pa_, key=ka, graph=True).result(), wa, "single between pairs")
        seen.add(g._next)
        a, b = lz.launch_pair(pa_, ka, pb_, kb)
        if rep % 2:
            _same(b.result(), wb, ("pair B", rep))
            _same(a.result(), wa, ("pair A", rep))
        else:
            _same(a.result(), wa, ("pair A", rep))
            _same(b.result(), wb, ("pair B", rep))
    assert len(seen) == g.RING                  # a pair started in every slot
    # the eager pair, then ONE capture of the pair; everything else replays a clone
    assert len(captures) == 2 and g.pair_replays == 2 * g.RING + 1
    assert set(g.pairs) == set(range(g.RING))
    assert {graphs.node_counts(h) for h in g.pairs.values()} == {(3, 0, 0) if ksp else (5, 0, 0)}
    assert [graphs.node_counts(sl.graph) for sl in g.slots] == [(3, 0, 0)] * g.RING
    # the device result block holds the last query's result, as after two single launches
    import torch
    torch.cuda.synchronize()
    _same([t.cpu().numpy() for t in g.out], wb, "device result block")
