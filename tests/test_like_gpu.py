"""SQL LIKE on the device: the dictionary-match kernel (csrc/kernels/dict_like.hip) against
``pyarrow.compute.match_like`` bit for bit, LIKE queries through covering indexes (kernel, code
interval and host-bitmap routes, all scanned natively), Hybrid Scan with a dictionary per part,
the kernel's caps, and a warm resubmission without host synchronization."""
import os
import warnings

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import Hyperspace, IndexConfig, Session, col, count, max_, sum_
from hyperspace_amd.exec import like as LK

from test_gpu_e2e import _both, _close
from test_like import ENTRIES, PATTERNS

pytestmark = pytest.mark.gpu

# exactly the kernel's token cap; matches the 300-byte entry
CAP_PATTERN = "a" * (LK.MAX_TOKENS - 1) + "%"


# -- 7. the kernel against pyarrow ----------------------------------------------------------------
def _draw(n):
    """``n`` corpus entries: the special ones first (so every size holds some), then keys."""
    return ENTRIES[:n]


@pytest.fixture(scope="module")
def expected():
    """(pattern, n) -> match_like bits, computed once."""
    out = {}
    for n in (1, 63, 64, 65, 130, 5013):
        arr = pa.array(_draw(n), pa.string())
        for p in PATTERNS + [CAP_PATTERN]:
            out[p, n] = np.asarray(pc.match_like(arr, p).to_numpy(zero_copy_only=False), bool)
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 5013])
def test_kernel_bits_equal_match_like(device, expected, n):
    from hyperspace_amd.ops import kernels as K
    assert len(ENTRIES) == 5013
    d = pa.array(_draw(n), pa.string())
    dd = LK.device_dictionary(d, device)
    assert dd.n == n and dd.max_len == max(len(s.encode()) for s in _draw(n))
    for p in PATTERNS + [CAP_PATTERN]:
        prog = LK.compile_like(p)
        if p == PATTERNS[-1]:
            # the pattern longer than every entry (301 tokens) is over the kernel's token cap:
            # the engine's bitmap for it comes from the host route, held to the same bits
            assert not LK.kernel_eligible(prog, dd.max_len)
            host = LK.LIKE_STATS["host"]
            words = LK.like_bitmap(d, prog, device).cpu().numpy().view(np.uint64)
            assert LK.LIKE_STATS["host"] == host + 1
        else:
            assert LK.kernel_eligible(prog, dd.max_len)
            words = K.dict_like(dd, prog).cpu().numpy().view(np.uint64)
        assert len(words) == (n + 63) // 64
        bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
        want = expected[p, n]
        assert np.array_equal(bits[:n], want), (p, n, np.flatnonzero(bits[:n] != want)[:5])
        assert not bits[n:].any(), (p, n)


def test_kernel_empty_dictionary_launches_nothing(device, monkeypatch):
    from hyperspace_amd.ops import _lib as NL
    from hyperspace_amd.ops import kernels as K
    d = pa.array([], pa.string())
    dd = LK.device_dictionary(d, device)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called for an empty dictionary")
    monkeypatch.setattr(NL, "lib", lambda: NoLaunch())
    words = K.dict_like(dd, LK.compile_like("%a%"))
    assert words.numel() == 0


# -- 8. end to end, through an index --------------------------------------------------------------
@pytest.fixture
def strs(tmp_path, device):
    rng = np.random.default_rng(11)
    n_dim = 5000
    keys = np.array([f"key-{i:05d}-{'x' * (i % 7)}" for i in range(n_dim)])
    fk = keys[rng.integers(0, n_dim, 60_000)]
    nulls = rng.random(len(fk)) < 0.1
    fact = pa.table({"c3": pa.array(fk), "c3n": pa.array(fk, mask=nulls), "v": rng.random(len(fk)),
                     "q": rng.integers(1, 10, len(fk)).astype(np.int64),
                     "w": rng.integers(0, 100, len(fk)).astype(np.int64)})
    os.makedirs(tmp_path / "fact")
    step = (fact.num_rows + 2) // 3
    for i in range(3):
        pq.write_table(fact.slice(i * step, step), tmp_path / "fact" / f"part-{i}.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.numBuckets": "16",
                      "spark.sql.autoBroadcastJoinThreshold": "-1",
                      "spark.sql.shuffle.partitions": "8",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    LK.clear_caches()
    return s, str(tmp_path / "fact"), keys, rng


def _delta(before):
    return {k: LK.LIKE_STATS[k] - before[k] for k in before}


def _check(s, q, index, **routes):
    """``q`` natively through ``index`` equals the host engine; LIKE_STATS moved by ``routes``
    (``interval`` binds are not cached, so that one counts at least once)."""
    plan = q.queryExecution.executed_plan.tree_string()
    assert any(f"Name: {i}" in plan for i in index.split("|")), plan
    before = dict(LK.LIKE_STATS)
    g, c, path = _both(s, q)
    assert path == "native", s.backend().fallback_reason
    _close(g, c)
    d = _delta(before)
    for k in ("kernel", "host", "exact"):
        assert d[k] == routes.get(k, 0), (k, d)
    assert (d["interval"] >= 1) == bool(routes.get("interval")), d
    return g, d


def _agg(df):
    return df.agg(sum_("v").alias("sv"), count("*").alias("n"))


@pytest.mark.parametrize("column", ["c3", "c3n"])
def test_like_queries_through_indexes_native(strs, column):
    s, fpath, keys, _ = strs
    hs = Hyperspace(s)
    fact = s.read.parquet(fpath)
    hs.createIndex(fact, IndexConfig("f_str", [column], ["v", "q"]))     # string column indexed
    hs.createIndex(fact, IndexConfig("f_q", ["q"], [column, "w"]))       # ... and included
    Hyperspace.enable(s)
    fact = s.read.parquet(fpath)
    c = col(column)
    g, _ = _check(s, _agg(fact.filter(c.like("%-0012%"))), "f_str", kernel=1)
    assert g.column("n")[0].as_py() > 0
    g, _ = _check(s, _agg(fact.filter(c.like("key-0001%"))), "f_str", interval=1)
    assert g.column("n")[0].as_py() > 0
    _check(s, _agg(fact.filter(~c.like("key-0001%"))), "f_str", kernel=1)   # negated prefix
    _check(s, _agg(fact.filter(c.like("key-0002%") | (col("q") > 8))), "f_str", kernel=1)
    _check(s, _agg(fact.filter(f"{column} LIKE '%-0012_-x%' AND q < 7")), "f_str", kernel=1)
    _check(s, _agg(fact.filter(c.like("key-00012-xxxxx"))), "f_str", exact=1)
    _check(s, _agg(fact.filter(c.like("nothing%"))), "f_str", interval=1)   # empty interval
    # rows, not an aggregate
    g, _ = _check(s, fact.filter(c.like("%-00_23-%")).select(column, "v"), "f_str", kernel=1)
    assert g.num_rows > 0
    # the included copy (only f_q covers w) has its own table and dictionary: its own bitmap
    def wagg(df):
        return df.agg(sum_("w").alias("sw"), count("*").alias("n"))
    _check(s, wagg(fact.filter((col("q") >= 2) & c.like("%-0012%"))), "f_q", kernel=1)
    _check(s, wagg(fact.filter((col("q") >= 2) & c.startswith("key-0001"))), "f_q", interval=1)
    _check(s, wagg(fact.filter((col("q") >= 2) & ~c.contains("-001"))), "f_q", kernel=1)
    # repeats launch nothing: the same query again (its prepared lowering may not even bind),
    # and the same pattern under another aggregate of the same columns (the same resident
    # table, so the same dictionary object), which binds and must hit the bitmap cache
    before = dict(LK.LIKE_STATS)
    _check(s, _agg(fact.filter(c.like("%-0012%"))), "f_str")
    _check(s, fact.filter(c.like("%-0012%")).agg(max_("v").alias("mv"), count("*").alias("n")),
           "f_str")
    assert _delta(before)["cache_hits"] >= 1


# -- 9. Hybrid Scan -------------------------------------------------------------------------------
def test_like_over_hybrid_scan_native(strs):
    s, fpath, keys, rng = strs
    for k, v in (("hybridscan.enabled", "true"), ("hybridscan.maxAppendedRatio", "0.5")):
        s.conf.set(f"spark.hyperspace.index.{k}", v)
    hs = Hyperspace(s)
    hs.createIndex(s.read.parquet(fpath), IndexConfig("f_str", ["c3"], ["v", "q"]))
    newk = np.array([f"new-{i}-0012" for i in range(300)])
    k2 = np.concatenate([newk[rng.integers(0, 300, 3000)], keys[rng.integers(0, len(keys), 3000)]])
    app = pa.table({"c3": pa.array(k2), "c3n": pa.array(k2), "v": rng.random(6000),
                    "q": rng.integers(1, 10, 6000).astype(np.int64),
                    "w": rng.integers(0, 100, 6000).astype(np.int64)})
    pq.write_table(app, os.path.join(fpath, "part-app.parquet"))
    Hyperspace.enable(s)
    fact = s.read.parquet(fpath)
    for cond in (col("c3").like("%-0012%"), col("c3").like("new-1%"), ~col("c3").like("%-001%")):
        q = _agg(fact.filter(cond))
        assert "Name: f_str" in q.queryExecution.executed_plan.tree_string()
        g, c, path = _both(s, q)
        assert path == "native", s.backend().fallback_reason
        _close(g, c)
        assert g.column("n")[0].as_py() > 0
    # appended rows with the new strings were seen
    n_new = _both(s, _agg(fact.filter(col("c3").like("new-%"))))[0].column("n")[0].as_py()
    assert n_new == int(np.char.startswith(k2, "new-").sum())


# -- 10. caps -------------------------------------------------------------------------------------
def test_caps_take_the_host_bitmap_route(tmp_path, device):
    rng = np.random.default_rng(3)
    long_entry = "L" + "ab" * 2500                      # 5001 bytes
    vals = np.array([f"w{i:03d}" for i in range(200)] + [long_entry])
    t = pa.table({"c3": pa.array(vals[rng.integers(0, len(vals), 20_000)]),
                  "v": rng.random(20_000)})
    os.makedirs(tmp_path / "t")
    pq.write_table(t, tmp_path / "t" / "p0.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.numBuckets": "4",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    LK.clear_caches()
    hs = Hyperspace(s)
    hs.createIndex(s.read.parquet(str(tmp_path / "t")), IndexConfig("t_c3", ["c3"], ["v"]))
    Hyperspace.enable(s)
    df = s.read.parquet(str(tmp_path / "t"))
    # an entry over the kernel's length cap
    g, _ = _check(s, _agg(df.filter(col("c3").like("%ab%"))), "t_c3", host=1)
    assert g.column("n")[0].as_py() > 0
    _check(s, _agg(df.filter(col("c3").like("%1_"))), "t_c3", host=1)
    # a program over the token cap (on a dictionary the kernel would take)
    short = pa.table({"c3": pa.array([f"w{i:03d}" for i in rng.integers(0, 200, 20_000)]),
                      "v": rng.random(20_000)})
    os.makedirs(tmp_path / "u")
    pq.write_table(short, tmp_path / "u" / "p0.parquet")
    hs.createIndex(s.read.parquet(str(tmp_path / "u")), IndexConfig("u_c3", ["c3"], ["v"]))
    du = s.read.parquet(str(tmp_path / "u"))
    pattern = "w" + "%_" * 149 + "%"                    # 1 + 298 + 1 = 300 tokens
    assert len(LK.compile_like(pattern)) == 300
    _check(s, _agg(du.filter(col("c3").like(pattern))), "u_c3", host=1)
    g, _ = _check(s, _agg(du.filter(col("c3").like("w%_1"))), "u_c3", kernel=1)
    assert g.column("n")[0].as_py() > 0


# -- 11. sync discipline --------------------------------------------------------------------------
def _submit_syncs(df):
    """Host synchronizations of one asynchronous submission of ``df``: torch's sync debug mode
    reports plus explicit device / stream / event waits (the warm-submit counting of the
    sharded-query tests)."""
    import torch
    counts = {"wait": 0}
    saved = []
    for obj, name in ((torch.cuda, "synchronize"), (torch.cuda.Stream, "synchronize"),
                      (torch.cuda.Event, "synchronize")):
        orig = getattr(obj, name)

        def wrapped(*a, _orig=orig, **k):
            counts["wait"] += 1
            return _orig(*a, **k)
        saved.append((obj, name, orig))
        setattr(obj, name, wrapped)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            fut = df.queryExecution.to_arrow_async()
            torch.cuda.set_sync_debug_mode("default")
        msgs = [str(x.message)[:200] for x in w if "called a synchronizing" in str(x.message)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
        for obj, name, orig in saved:
            setattr(obj, name, orig)
    return counts["wait"] + len(msgs), msgs, fut


@pytest.mark.parametrize("pattern", ["%-0012%", "key-0001%"])
def test_warm_like_query_submits_without_host_sync(strs, pattern):
    import torch
    s, fpath, _, _ = strs
    hs = Hyperspace(s)
    hs.createIndex(s.read.parquet(fpath), IndexConfig("f_str", ["c3"], ["v", "q"]))
    Hyperspace.enable(s)
    fact = s.read.parquet(fpath)

    def q():
        return _agg(fact.filter(col("c3").like(pattern)))
    want = None
    for _ in range(3):
        want = q().collect()
        assert s.backend().last_path == "native", s.backend().fallback_reason
    torch.cuda.synchronize()
    before = dict(LK.LIKE_STATS)
    n, msgs, fut = _submit_syncs(q())
    res = fut.result()
    assert n == 0, msgs
    assert fut.path == "native"
    (sv, n_rows), = [tuple(r.values()) for r in res.to_pylist()]
    assert n_rows == want[0][1] and n_rows > 0
    assert abs(sv - want[0][0]) <= 1e-9 * abs(want[0][0])    # fp64 sums, order may differ
    d = _delta(before)
    assert d["kernel"] == 0 and d["host"] == 0, d
