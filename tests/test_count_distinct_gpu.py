"""count(DISTINCT x) end to end on the device: level 1 through the hash-mode aggregate on
(g..., x), level 2 through the dense or the hash regroup (csrc/kernels/distinct_agg.hip).  Every
query is checked against the host oracle and must run native unless it says otherwise."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import (Hyperspace, IndexConfig, Session, avg, col, count, countDistinct,
                            sum_)

from conftest import gpu_available
from test_gpu_e2e import _both, _close

pytestmark = pytest.mark.gpu

N = 4000


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    if not gpu_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("cd")
    rng = np.random.default_rng(17)
    k = rng.integers(0, 400, N).astype(np.int64)
    g2 = rng.integers(0, 60, N).astype(np.int32)
    x = rng.integers(0, 50, N).astype(np.int64)
    xmask = rng.random(N) < 0.15
    xmask |= (g2 == 7) & (k == k[g2 == 7][0])     # one (g2, k) group whose x is all NULL
    t = pa.table({"k": k, "g2": g2, "x": pa.array(x, mask=xmask),
                  "gs": pa.array(rng.choice(["ash", "birch", "cedar", "fir"], N)),
                  "sx": pa.array([f"w{v}" for v in rng.integers(0, 30, N)]),
                  "f": rng.choice(np.array([0.0, -0.0, 1.5, -1.5, 2.25, 1e9]), N),
                  "v": np.round(rng.random(N) * 100, 2)})
    o = pa.table({"ok": np.arange(400, dtype=np.int64),
                  "od": rng.integers(0, 12, 400).astype(np.int32)})
    for name, tb in (("t", t), ("o", o)):
        os.makedirs(tmp / name)
        half = tb.num_rows // 2
        pq.write_table(tb.slice(0, half), tmp / name / "part-0.parquet")
        pq.write_table(tb.slice(half), tmp / name / "part-1.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp / "idx"),
                      "spark.hyperspace.index.numBuckets": "8",
                      "spark.sql.autoBroadcastJoinThreshold": "-1",
                      "spark.sql.shuffle.partitions": "8",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp / "wh"))
    hs = Hyperspace(s)
    df, od = s.read.parquet(str(tmp / "t")), s.read.parquet(str(tmp / "o"))
    hs.createIndex(df, IndexConfig("t_k", ["k"], ["g2", "x", "gs", "sx", "f", "v"]))
    hs.createIndex(od, IndexConfig("o_ok", ["ok"], ["od"]))
    Hyperspace.enable(s)
    return s, df, od, t


def _check(s, q, sort=True, level2=None):
    g, c, path = _both(s, q, sort=sort)
    assert path == "native", s.backend().fallback_reason
    _close(g, c)
    if level2 is not None:
        assert s.backend().metrics.get("distinct_level2") == level2
    return g


def test_ungrouped_integer_under_a_range_filter(data):
    s, df, _, t = data
    g = _check(s, df.filter((col("k") >= 50) & (col("k") < 300)).agg(countDistinct("x").alias("c")),
               level2="dense")
    want = len({r["x"] for r in t.to_pylist() if 50 <= r["k"] < 300 and r["x"] is not None})
    assert g.column("c").to_pylist() == [want]


def test_ungrouped_dictionary_string_and_float_with_both_zeros(data):
    s, df, _, t = data
    g = _check(s, df.filter(col("k") >= 20).agg(countDistinct("sx").alias("c")), level2="dense")
    assert g.column("c").to_pylist() == [len({r["sx"] for r in t.to_pylist() if r["k"] >= 20})]
    g = _check(s, df.filter(col("k") >= 20).agg(countDistinct("f").alias("c")), level2="dense")
    assert g.column("c").to_pylist() == [5]          # 0.0 and -0.0 are one value


def test_one_dictionary_group_column_dense_level2(data):
    s, df, _, _ = data
    q = df.filter(col("k") < 350).groupBy("gs").agg(
        countDistinct("x").alias("c"), sum_("v").alias("sv"), avg("v").alias("av"),
        count("*").alias("n"))
    g = _check(s, q, level2="dense")
    assert g.num_rows == 4


def test_two_group_columns_hash_level2_and_overflow_retry(data):
    s, df, _, t = data
    q = df.filter(col("k") >= 0).groupBy("g2", "k").agg(
        countDistinct("x").alias("c"), sum_("v").alias("sv"), count("x").alias("nx"))
    g = _check(s, q, level2="hash")
    assert g.num_rows > 2000
    rows = {(r["g2"], r["k"]): r["c"] for r in g.to_pylist()}
    null_groups = [gk for gk, c in rows.items() if c == 0]
    assert null_groups                                # a group whose x is all NULL counts 0
    # a stale, tiny level-2 table overflows its probe budget: 4x re-runs, same result
    be = s.backend()
    keys = [key for key in be.htables.sizes if key and key[0] == "distinct"]
    assert keys
    for key in keys:
        be.htables.sizes[key] = 16
    g2 = _check(s, q, level2="hash")
    for name in ("g2", "k", "c", "nx"):
        assert g2.column(name).equals(g.column(name))
    assert all(be.htables.sizes[key] >= 4096 for key in keys)


def test_distinct_count_over_a_join_of_co_bucketed_indexes(data):
    s, df, od, _ = data
    q = df.join(od, df["k"] == od["ok"]).groupBy("od").agg(
        countDistinct("x").alias("c"), sum_("v").alias("sv"))
    g = _check(s, q)
    assert g.num_rows == 12


def test_order_by_count_desc_limit(data):
    s, df, _, _ = data
    q = df.filter(col("k") >= 10).groupBy("g2").agg(countDistinct("x").alias("cnt")) \
        .orderBy(col("cnt").desc(), col("g2")).limit(5)
    g = _check(s, q, sort=False)
    assert g.num_rows == 5
    assert g.column("cnt").to_pylist() == sorted(g.column("cnt").to_pylist(), reverse=True)


def test_filter_that_passes_nothing(data):
    s, df, _, _ = data
    q = df.filter(col("k") > 10_000).agg(countDistinct("x").alias("c"), sum_("v").alias("sv"),
                                         count("*").alias("n"))
    g = _check(s, q)
    assert [tuple(r.values()) for r in g.to_pylist()] == [(0, None, 0)]
    q = df.filter(col("k") > 10_000).groupBy("gs").agg(countDistinct("x").alias("c"))
    assert _check(s, q).num_rows == 0


def test_two_distinct_columns_fall_back_to_the_host(data):
    s, df, _, t = data
    q = df.filter(col("k") >= 100).agg(countDistinct("x").alias("cx"),
                                       countDistinct("sx").alias("cs"))
    g, c, path = _both(s, q)
    assert path == "fallback"
    assert "more than one distinct column" in s.backend().fallback_reason
    _close(g, c)
    rows = [r for r in t.to_pylist() if r["k"] >= 100]
    assert g.to_pylist() == [{"cx": len({r["x"] for r in rows if r["x"] is not None}),
                              "cs": len({r["sx"] for r in rows})}]


def test_same_query_twice_with_different_literals(data):
    s, df, _, t = data
    q = lambda lo: df.filter(col("k") >= lo).groupBy("gs").agg(   # noqa: E731
        countDistinct("x").alias("c"), count("*").alias("n"))
    got = []
    for lo in (120, 330):
        g = _check(s, q(lo), level2="dense")
        got.append({r["gs"]: (r["c"], r["n"]) for r in g.to_pylist()})
        want = {}
        for r in t.to_pylist():
            if r["k"] >= lo:
                e = want.setdefault(r["gs"], [set(), 0])
                e[1] += 1
                if r["x"] is not None:
                    e[0].add(r["x"])
        assert got[-1] == {gs: (len(e[0]), e[1]) for gs, e in want.items()}
    assert got[0] != got[1]
