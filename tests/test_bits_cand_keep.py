"""The candidate phase 2 keeps passing tail words in LDS (exec/jit_runs.py ``rs_keep``; kernels
``hs_jit_run_bits_cand`` and ``hs_jit_run_bits_cand2``): the filter pass writes a passing row's
64-bit tail word into a small per-wavefront ring, and the sums are taken from there in whole
groups of 64 entries after each pass, instead of listing row offsets and loading the words again
after the tile's last pass.

CPU tier: what the two sources hold with the switch on, that they are the previous recorded
sources byte for byte with it off (``tests/golden/bits_cand_listing``), that no other phase-2 form
changes, that the new form compiles for gfx950, and its LDS per workgroup.
GPU tier, kernel level: block partials and results with the switch on equal those with it off
exactly - single launches and ``launch_pair`` - over a table built so that tiles hold 0, 1, 63, 64,
65, 128 and more than CAP passing rows (counted on the host and asserted), and over the tables and
literal sets of ``test_bits_cand_pair``.  GPU tier, end to end: interleaved asynchronous queries
equal one-by-one ``collect()`` with the switch on and off, and both equal each other.
"""
import functools
import os
import re
import sys

import numpy as np
import pyarrow as pa
import pytest

from hyperspace_amd.ops import _lib as NL
from test_bits_cand_pair import CAP, DENSE, SETS, TILE, _tile_counts
from test_bits_cand_pair import _inputs as _clustered_inputs
from test_jit import _col, rt  # noqa: F401
from test_tags2_pair import (_behind_busy_device, _check_pair, _lower, _q3, _q6, _query, _rows,
                             _still_busy)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bits_cand_listing")
LDS_PER_CU = 160 * 1024


# ------------------------------------------------------------------------------------------------
# CPU tier: the sources
# ------------------------------------------------------------------------------------------------
def _headline_params():
    """Join parameters and compact columns (host tensors) that generate the headline Q3's phase-2
    sources as they were recorded on the device: IS NOT NULL on the key beside the left range
    test, SUM(price * (1 - discount)) and two COUNT(*)."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts", "dev"))
    try:
        import gen_join_src as G
    finally:
        sys.path.pop(0)
    p, comp, keep = G.q3_params(1)
    p.preds[0] = NL.Pred(NL.PK_NOT_NULL, NL.OP_GT, 0, 0, 0, 0, 0, 0.0, None)
    p.preds[1] = NL.Pred(NL.PK_INT_LIT, NL.OP_GT, 1, 0, 1, 0, 9000, 0.0, None)
    p.preds[2] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 9, 0, 2, 0, 9000, 0.0, None)
    p.nlp, p.npreds = 2, 3
    p.aggs[2] = G.agg(NL.AK_COUNT_STAR)
    p.naggs = 3
    return p, comp, keep


def _sources(**cfg):
    """(single, pair) candidate kernels of the headline's shape under ``cfg``."""
    from hyperspace_amd.exec import jit_runs, kernel_config
    with kernel_config.use(**cfg):
        p, comp, keep = _headline_params()
        pr = jit_runs.prune_plan(p, comp, 1)
        cand = tuple(dict.fromkeys(sl for _, sl, _ in pr))
        assert cand and jit_runs.cand_pair(p, comp, cand)
        return (jit_runs.gen_run_sparse_scan(p, comp, None, None, cand),
                jit_runs.gen_run_sparse_scan(p, comp, None, None, cand, True))


_SIZES = {"unsigned char": 1, "unsigned short": 2, "unsigned": 4, "int": 4, "u64": 8, "i64": 8,
          "double": 8, "hs_v4u": 16}


def _lds_bytes(src: str) -> int:
    """Static LDS of a generated kernel: the sum of its ``__shared__`` array declarations."""
    na = int(re.search(r"constexpr int NA = (\d+);", src).group(1))
    total = 0
    decls = re.findall(r"__shared__\s+([\w ]+?)\s+\w+((?:\[[^\]]+\])+)\s*;", src)
    assert decls
    for ct, dims in decls:
        n = _SIZES[ct]
        for d in re.findall(r"\[([^\]]+)\]", dims):
            n *= na if d == "NA" else int(d)
        total += n
    return total


def test_on_sources_keep_the_word_and_load_nothing_in_the_walk():
    from hyperspace_amd.exec import jit_runs, kernel_config
    assert kernel_config.KernelConfig().rs_keep is True
    one, two = _sources(rs_keep=True)
    off1, off2 = _sources(rs_keep=False)
    for k, off in ((one, off1), (two, off2)):
        assert "PKt_[" not in k.src and "PKt_[" in off.src
        assert not re.search(r"\blst_", k.src) and "unsigned short lst_[" in off.src
        assert "clst_" in k.src and "__shared__ u64 kw_[" in k.src
        # the walk reads the ring and nothing else; the filter pass still loads each word once
        assert k.src.count("PKc_[") == off.src.count("PKc_[")
        assert k.src.count("for (int cb = 0;") == off.src.count("for (int cb = 0;")
        assert [n for _, n, _ in k.args.slots] == [n for _, n, _ in off.args.slots]
    # the ring: the leftover of a 64-entry group plus one pass's appends, per query
    cc = 64 * jit_runs.RS_WALK
    assert f"kw_[4][{63 + cc}];" in one.src and f"kw_[4][{2 * (63 + cc)}];" in two.src
    # the switch is part of the shape key
    p, comp, _ = _headline_params()
    cand = (1,)
    for pair in (False, True):
        with kernel_config.use(rs_keep=True):
            a = jit_runs.sparse_shape(p, comp, None, None, cand, pair)
        with kernel_config.use(rs_keep=False):
            b = jit_runs.sparse_shape(p, comp, None, None, cand, pair)
        assert a != b


def test_off_sources_are_the_recorded_listing_sources():
    got = {k.name: k.src for k in _sources(rs_keep=False)}
    files = sorted(os.listdir(GOLDEN))
    assert [f.split(".")[0] for f in files] == ["hs_jit_run_bits_cand", "hs_jit_run_bits_cand2"]
    for f in files:
        with open(os.path.join(GOLDEN, f)) as fh:
            assert got[f.split(".")[0]] == fh.read(), f


def test_recorded_aot_sources_are_the_on_form():
    """The ahead-of-time set holds the default (on) sources of both kernels under the names
    ``hs_jit_get`` looks them up by, and not the listing form's."""
    import hashlib
    from hyperspace_amd.exec import jit
    have = set(os.listdir(jit.AOT_DIR))
    for k in _sources(rs_keep=True):
        h = hashlib.sha1(k.src.encode()).hexdigest()[:16]
        assert f"{k.name}.{h}.hip" in have
        with open(os.path.join(jit.AOT_DIR, f"{k.name}.{h}.hip")) as fh:
            assert fh.read() == k.src
        assert len([f for f in have if f.split(".")[0] == k.name]) == 1


def test_other_phase2_forms_do_not_change():
    """The streaming, hash and top-K sources (``test_jit.test_run_topk_sources_compile``'s
    recipe) and their shape keys are the same under both settings."""
    import types
    from hyperspace_amd.exec import hash_agg as H
    from hyperspace_amd.exec import jit_runs, kernel_config
    from test_jit import _q3_compacts, _q3_params

    def forms():
        p, comp, _ = _headline_params()
        j, jc = _q3_params(), _q3_compacts()
        c = types.SimpleNamespace(hs_type=NL.I64, valid=None, dictionary=None, offsets=None,
                                  atype=pa.int64())
        hk = H.plan_keys([(0, None, c, (1, 600_000_000, None))], (False, False), False)
        tk = H.TopKPlan(0, False, True, 2, 16)
        ks = [jit_runs.gen_run_sparse_scan(p, comp), jit_runs.gen_run_sparse_scan(j, jc),
              jit_runs.gen_run_sparse_scan(j, jc, hk), jit_runs.gen_run_sparse_scan(j, jc, hk, tk)]
        shapes = [jit_runs.sparse_shape(p, comp), jit_runs.sparse_shape(j, jc),
                  jit_runs.sparse_shape(j, jc, hk), jit_runs.sparse_shape(j, jc, hk, tk)]
        return [k.name for k in ks], [k.src for k in ks], shapes
    with kernel_config.use(rs_keep=True):
        on = forms()
    with kernel_config.use(rs_keep=False):
        off = forms()
    assert on == off        # (equal shape keys: the cache entries are shared)
    assert on[0] == ["hs_jit_run_bits_scan", "hs_jit_run_bits_scan", "hs_jit_run_bits_hash",
                     "hs_jit_run_bits_topk"]
    assert all("kw_[" not in x and re.search(r"\blst_", x) for x in on[1])


def test_on_sources_compile(rt, tmp_path):  # noqa: F811
    ks = []
    for walk in (4, 2):
        ks += list(_sources(rs_keep=True, rs_walk=walk))
    assert len({k.src for k in ks}) == 4
    for k in ks:
        assert "PKt_[" not in k.src
        rc = rt.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                                  str(tmp_path).encode())
        assert rc == 0, rt.runtime().hs_jit_last_error().decode()


def test_lds_per_workgroup_leaves_the_occupancy_to_the_registers():
    """The single form takes 62 VGPRs (eight waves per SIMD = eight 256-thread workgroups per
    CU), so its LDS must fit eight times into a CU's 160 KB.  The pair form is bounded to five
    waves by its registers (six spill); its two rings must leave six workgroups per CU possible,
    so that LDS is not what holds it at five."""
    one, two = _sources(rs_keep=True)
    off1, off2 = _sources(rs_keep=False)
    assert _lds_bytes(off1.src) == 12992 and _lds_bytes(off2.src) == 21376    # as recorded
    # 512 (nibble table) + 4 x 256 x 2 (clst_) + 4 x 319 x 8 (ring) + 4 x 3 x 16 (flush)
    assert _lds_bytes(one.src) == 512 + 2048 + 4 * 319 * 8 + 192 == 12960
    assert _lds_bytes(two.src) == 512 + 2048 + 2 * 4 * 319 * 8 + 2 * 192 == 23360
    assert _lds_bytes(one.src) <= LDS_PER_CU // 8
    assert _lds_bytes(two.src) <= LDS_PER_CU // 6
    assert "amdgpu_waves_per_eu(5, 5)" in two.src and "amdgpu_waves_per_eu" not in one.src


# ------------------------------------------------------------------------------------------------
# GPU tier, kernel level
# ------------------------------------------------------------------------------------------------
ROWS_PER_KEY = 4
# Left date values: 120 passes the wide range only, 150 passes both ranges, 900 neither; 50 beside
# 900 makes a run a candidate (its bounds straddle the ranges) without a passing row.
NESTED = ((100, 200, 500), (140, 160, 500))        # B's passing rows are a strict subset of A's
DISJOINT = ((100, 130, 500), (140, 160, 500))      # A: the 120 rows, B: the 150 rows
KEEP_SETS = {"nested": NESTED, "disjoint": DISJOINT, "mirror": (NESTED[1], NESTED[0])}
# per tile (rows with 120, rows with 150, placed as whole runs?): bucket 0 starts at row 0, so its
# tiles are rows [4096 i, 4096 i + 4096); its last tile is cut short by the bucket's end
BUCKET0 = [(0, 0, False), (1, 0, False), (0, 63, False), (1, 63, False), (1, 64, False),
           (63, 65, False), (64, 64, True), (1200, 300, False), (5, 128, False), (10, 1, False)]
BUCKET0_ROWS = 9 * TILE + 1500          # ends mid-tile, and 38364 % 64 = 28: bucket 1 starts
BUCKET1 = [(64, 0, True), (3, 64, False), (0, 2, False)]     # mid-group
BUCKET1_ROWS = 2 * TILE + 36 + 700      # its tiles are 64-aligned from row 38336


def _keep_data():
    """Bucket-sorted join inputs in the layout of ``test_tags2_pair._join_data``: two buckets,
    four left rows per key, every left key with one right row; a tenth of the right rows fail
    the right literal (their runs hold decoy rows that would pass on the left)."""
    rng = np.random.default_rng(23)
    assert BUCKET0_ROWS % ROWS_PER_KEY == 0 and BUCKET1_ROWS % ROWS_PER_KEY == 0
    assert BUCKET0_ROWS % 64 and BUCKET0_ROWS % TILE
    lks, rks, key0 = [], [], 1 << 20
    for rows in (BUCKET0_ROWS, BUCKET1_ROWS):
        keys = key0 + 40 * np.arange(1, rows // ROWS_PER_KEY + 1, dtype=np.int64)
        key0 = int(keys[-1]) + 400_000
        lks.append(np.repeat(keys, ROWS_PER_KEY))
        rks.append(keys)
    lk, rk = np.concatenate(lks), np.concatenate(rks)
    n = len(lk)
    loff = np.array([0, BUCKET0_ROWS, n], np.int64)
    rdate = np.zeros(len(rk), np.int32)
    bad = rng.random(len(rk)) < 0.1
    rdate[bad] = 999
    run_of = np.arange(n) // ROWS_PER_KEY
    ldate = np.full(n, 900, np.int32)
    ldate[0], ldate[1] = 0, 999          # the code range of a 16-bit column (run 0 stays pruned
    rdate[0] = 999                       # on the right)
    bad[0] = True
    for b, specs in enumerate((BUCKET0, BUCKET1)):
        rs, re = int(loff[b]), int(loff[b + 1])
        tb = rs & ~63
        for n120, n150, whole in specs:
            lo, hi = max(tb, rs), min(tb + TILE, re)
            assert lo < hi
            runs = np.unique(run_of[lo:hi])
            runs = runs[(runs * ROWS_PER_KEY >= lo) & ((runs + 1) * ROWS_PER_KEY <= hi)]
            good = runs[~bad[runs]]
            rng.shuffle(good)
            if whole:       # whole runs pass: the filter pass's first entries all pass
                assert n120 % ROWS_PER_KEY == 0 and n150 % ROWS_PER_KEY == 0
                k1, k2 = n120 // ROWS_PER_KEY, n150 // ROWS_PER_KEY
                for v, rr in ((120, good[:k1]), (150, good[k1:k1 + k2])):
                    for j in range(ROWS_PER_KEY):
                        ldate[rr * ROWS_PER_KEY + j] = v
                used = k1 + k2
            else:
                rows = (good[:, None] * ROWS_PER_KEY + np.arange(ROWS_PER_KEY)).reshape(-1)
                pick = rng.choice(rows, n120 + n150, replace=False)
                ldate[pick[:n120]] = 120
                ldate[pick[n120:]] = 150
                used = len(good)        # (any run may hold a picked row)
            # candidate runs without a passing row, and decoys in runs the right side drops
            for r_ in good[used:used + 40]:
                ldate[r_ * ROWS_PER_KEY] = 50
            for r_ in runs[bad[runs]][:20]:
                ldate[r_ * ROWS_PER_KEY + 1] = 150
                ldate[r_ * ROWS_PER_KEY + 2] = 120
            tb += TILE
        assert tb >= re
    d = {"lk": lk, "rk": rk, "loff": loff,
         "roff": np.array([0, len(rks[0]), len(rk)], np.int64),
         "ldate": ldate, "lprice": np.round(rng.random(n) * 1000, 2),
         "lqty": rng.integers(0, 1 << 30, n).astype(np.int64), "rdate": rdate}
    d["starts"] = np.flatnonzero(np.concatenate([[True], lk[1:] != lk[:-1]]))
    return d


def _tile_passing(d, lo: int, hi: int, rlit: int) -> list:
    """Per phase-2 tile (as ``_tile_counts``), the join's passing rows: left range test on the
    row, right literal on its run's right row."""
    ok = (d["ldate"] >= lo) & (d["ldate"] < hi) & \
        np.repeat(d["rdate"] < rlit, ROWS_PER_KEY)
    out = []
    for b in range(len(d["loff"]) - 1):
        rs, re = int(d["loff"][b]), int(d["loff"][b + 1])
        tb = rs & ~63
        while tb < re:
            out.append(int(ok[max(tb, rs):min(tb + TILE, re)].sum()))
            tb += TILE
    return out


def test_keep_table_holds_the_cases():
    """Host side of what the GPU cases rely on: the passing rows per tile are the designed
    counts - a tile meant to hold 64 holds 64 - and the ranges end mid-tile / start mid-group."""
    d = _keep_data()
    spec = BUCKET0 + BUCKET1
    assert int(d["loff"][1]) % 64 == 28 and int(d["loff"][1]) % TILE
    assert len(_tile_passing(d, *NESTED[0])) == len(spec) == 13
    assert _tile_passing(d, *NESTED[0]) == [a + b for a, b, _ in spec]
    assert _tile_passing(d, *NESTED[1]) == [b for _, b, _ in spec]
    assert _tile_passing(d, *DISJOINT[0]) == [a for a, _, _ in spec]
    a, b = _tile_passing(d, *NESTED[0]), _tile_passing(d, *NESTED[1])
    assert {0, 1, 63, 64, 65, 128} <= set(a) and {0, 1, 63, 64, 65, 128} <= set(b)
    assert max(a) > CAP and all(y <= x for x, y in zip(a, b)) and a != b
    # a wavefront of grid 1 (four wavefronts, four tiles each) and of grid 2 (two each) gets the
    # tile above CAP beside sparse ones
    assert a.index(max(a)) == 7 and 0 < a[6] <= CAP and 0 < a[4] <= CAP


@functools.lru_cache(maxsize=None)
def _keep_inputs():
    """``test_bits_cand_pair._inputs`` over ``_keep_data``."""
    import torch
    from hyperspace_amd.exec.encoding import encode
    dev = torch.device("cuda:0")
    d = _keep_data()
    cols = {0: pa.array(d["lk"]), 1: pa.array(d["ldate"]), 2: pa.array(d["lprice"]),
            3: pa.array(d["lqty"]), 8: pa.array(d["rk"]), 9: pa.array(d["rdate"])}
    dc = {s: _col(a, dev) for s, a in cols.items()}
    comp = {s: e for s, e in ((s, encode(c)) for s, c in dc.items()) if e is not None}
    assert comp[0].width == 4 and comp[8].width == 4 and comp[1].width == 2
    B = len(d["loff"]) - 1
    rt_ = (torch.from_numpy(d["loff"][:-1].copy()).to(dev),
           torch.from_numpy(np.diff(d["loff"])).to(dev),
           torch.arange(B, dtype=torch.int32, device=dev), torch.from_numpy(d["roff"]).to(dev))
    return d, dc, comp, rt_


def _bits(t) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(t.cpu() if hasattr(t, "cpu") else t)) \
        .reshape(-1).view(np.uint8)


def _run(inputs, sets, keep: bool, grid, monkeypatch, tag) -> dict:
    """Every set through one launcher lowered with ``rs_keep`` = keep: the single launches'
    partials and results, then ``launch_pair``'s (checked against the singles by
    ``_check_pair``), as raw bytes."""
    import torch
    d, dc, comp, rt_ = inputs
    cfg = {} if grid is None else {"rs_bits_grid": grid}
    lz = _lower(dc, comp, rt_, len(d["lk"]), True, monkeypatch, rs_pair=True, rs_keep=keep, **cfg)
    assert lz.ks.name == "hs_jit_run_bits_cand" and lz.ksp.name == "hs_jit_run_bits_cand2"
    for k in (lz.ks, lz.ksp):
        assert ("PKt_[" not in k.src) == keep and ("kw_[" in k.src) == keep
    out = {}
    for name, lits in sets.items():
        for q, lit in zip("ab", lits):
            r = lz.launch(_query(dc, *lit), key=(tag, name, q) + lit, graph=True).result()
            torch.cuda.synchronize()
            out[name, q, "parts"] = [_bits(t).copy() for t in lz.graph.parts]
            out[name, q, "result"] = [_bits(x).copy() for x in r]
        want_t, want_r = _check_pair(lz, d, dc, lits, (tag, name, keep))
        torch.cuda.synchronize()
        out[name, "pair", "parts"] = [_bits(t).copy() for t in
                                      (*lz.graph.parts, *lz.graph.parts_b)]
        out[name, "pair", "result"] = [_bits(x).copy() for r in want_r for x in r]
        out[name, "tags"] = want_t
        out[name, "counts"] = [int(np.asarray(r[1]).reshape(-1)[1]) for r in want_r]
    return out


def _same(on: dict, off: dict) -> None:
    assert on.keys() == off.keys()
    for k in on:
        if k[-1] in ("tags", "counts"):
            continue
        assert len(on[k]) == len(off[k]), k
        for i, (x, y) in enumerate(zip(on[k], off[k])):
            assert np.array_equal(x, y), (k, i)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [1, 2])
def test_keep_equals_listing_on_group_boundaries(device, monkeypatch, grid):
    """Grid 1: four wavefronts with four tiles each, grid 2: eight with two; per tile and query
    0 / 1 / 63 / 64 / 65 / 128 / more than CAP passing rows (``test_keep_table_holds_the_cases``),
    so a leftover is carried to a tile's end and dropped there, groups complete inside a pass,
    and the wavefront that owns tile 7 takes the dense path between union-path tiles."""
    inputs = _keep_inputs()
    d = inputs[0]
    off = _run(inputs, KEEP_SETS, False, grid, monkeypatch, ("off", grid))
    on = _run(inputs, KEEP_SETS, True, grid, monkeypatch, ("on", grid))
    _same(on, off)
    for name, lits in KEEP_SETS.items():
        # the results count exactly the host's passing rows ...
        assert on[name, "counts"] == [sum(_tile_passing(d, *lit)) for lit in lits], name
        # ... and which path the tiles took: the candidates per tile from the singles' bitmaps
        cands = [[c for _, c in _tile_counts(d, t)] for t in on[name, "tags"]]
        dense = [i for i, (x, y) in enumerate(zip(*cands)) if max(x, y) > CAP]
        assert dense == [7], (name, cands)
        # candidates that fail the left test in every union-path tile with passing rows
        for c, lit in zip(cands, lits):
            assert all(x > y for x, y in zip(c, _tile_passing(d, *lit)) if y), (name, c)
        # more than one filter pass in a union-path tile: 64 * rs_walk candidates per pass
        assert any(256 < max(x, y) <= CAP for x, y in zip(*cands))


@pytest.mark.gpu
@pytest.mark.parametrize("nkeys,grid", [(9600, 1), (6000, None)])
def test_keep_equals_listing_on_the_pair_tests_tables(device, monkeypatch, nkeys, grid):
    """The clustered tables of ``test_bits_cand_pair``: 9600 keys with grid 1 - the mixed sets
    take the union path and the dense path in one wavefront - and 6000 keys on the default grid
    (two tiles in the first range, bucket starts off the 64-row grid)."""
    inputs = _clustered_inputs(nkeys)
    d = inputs[0]
    sets = {k: SETS[k] for k in ("sparse", "mixed", "mixed_mirror", "nested", "none_all")}
    off = _run(inputs, sets, False, grid, monkeypatch, ("off", nkeys))
    on = _run(inputs, sets, True, grid, monkeypatch, ("on", nkeys))
    _same(on, off)
    for name in sets:
        top = [max(c for _, c in _tile_counts(d, t)) for t in on[name, "tags"]]
        if name == "sparse":
            assert 0 < min(top) and max(top) <= CAP
        elif name in DENSE:
            assert max(top) > CAP
        if name.startswith("mixed"):
            assert min(top) <= CAP < max(top)


# ------------------------------------------------------------------------------------------------
# GPU tier, end to end
# ------------------------------------------------------------------------------------------------
_E2E: dict = {}     # rs_keep -> the interleaved run's rows, compared across the two sessions


@pytest.fixture(scope="module", params=[True, False], ids=["rs_keep_on", "rs_keep_off"])
def env(request, tmp_path_factory):
    """The tables and indexes of ``test_bits_cand_pair.env`` under a session that sets
    ``rs_keep``."""
    from conftest import gpu_available
    if not gpu_available():
        pytest.skip("no GPU")
    import pyarrow.parquet as pq
    from hyperspace_amd import Hyperspace, IndexConfig, Session
    from hyperspace_amd.exec import kernel_config
    prev = kernel_config.active()
    tmp_path = tmp_path_factory.mktemp("candkeep")
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
                      "spark.hyperspace.mi.kernel.rs_keep": "true" if request.param else "false"},
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
def test_interleaved_async_queries_equal_collect(env):
    from hyperspace_amd.exec import jit, jit_runs, kernel_config
    s, li, od, on = env
    assert kernel_config.active().rs_keep == on
    ids = [50 + k for k in range(5)]
    want = [(_rows(_q3(li, od, i).collect()), _rows(_q6(li, i).collect())) for i in ids]
    lz = jit.LAST_MJ_LAUNCHER[0]
    assert isinstance(lz, jit_runs.TwoPhaseLauncher) and lz.ksp is not None
    for k in (lz.ks, lz.ksp):
        assert ("kw_[" in k.src) == on and ("PKt_[" in k.src) == (not on)
    # the pair kernels load (the listing form: compile) now, not while the device is kept busy
    lz.ktp.function(), lz.ksp.function()
    primer =_behind_busy_device(s, li, od, 100)
    futs = []
    for i in ids:
        futs.append((_q3(li, od, i).collect_async(), _q6(li, i).collect_async()))
        if len(futs) == 3:
            _still_busy(primer)
    got = [(_rows(a.result()), _rows(b.result())) for a, b in futs]
    primer.result()
    assert all(a.path == "native" and b.path == "native" for a, b in futs)
    assert got == want              # exactly: the same sums in the same order
    assert s.backend().pair_gate.pairs >= 1 and not s.backend().pair_gate.held
    _E2E[on] = got
    if len(_E2E) == 2:
        assert _E2E[True] == _E2E[False]
