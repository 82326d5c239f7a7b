"""Window functions end to end on the device (exec/window.py over csrc/kernels/window.hip): every
query is checked against the host engine and must run native unless it says otherwise; the
fallback cases must run on the host with the same answer."""
import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import (Hyperspace, IndexConfig, Session, Window, avg, col, count, dense_rank,
                            max_, min_, rank, row_number, sum_)

from conftest import gpu_available
from test_gpu_e2e import _both, _close

pytestmark = pytest.mark.gpu

N = 6000        # a few tiles of the window kernels after a filter, and more than one block


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    if not gpu_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("win")
    rng = np.random.default_rng(23)
    k = rng.integers(0, 500, N).astype(np.int64)
    x = np.round(rng.random(N) * 100, 2)
    xmask = (rng.random(N) < 0.2) | (k == 7)                 # partition 7: x all NULL
    t = pa.table({
        "id": np.arange(N, dtype=np.int64), "k": k,
        "g": rng.integers(0, 9, N).astype(np.int32),
        "d": pa.array(rng.integers(0, 12, N).astype(np.int32), mask=rng.random(N) < 0.1),
        "f": pa.array(rng.choice(np.array([0.0, -0.0, 1.5, -2.5, 7.25, 1e9, np.nan, -np.nan]), N),
                      mask=rng.random(N) < 0.1),
        "s": pa.array(rng.choice(["ash", "birch", "cedar", "fir", "oak"], N),
                      mask=rng.random(N) < 0.1),
        "x": pa.array(x, mask=xmask),
        "i": pa.array(rng.integers(-50, 50, N).astype(np.int32), mask=rng.random(N) < 0.2),
        "m": pa.array([decimal.Decimal(int(v)) / 100 for v in rng.integers(0, 10_000, N)],
                      pa.decimal128(9, 2))})
    os.makedirs(tmp / "t")
    half = N // 2
    pq.write_table(t.slice(0, half), tmp / "t" / "part-0.parquet")
    pq.write_table(t.slice(half), tmp / "t" / "part-1.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp / "idx"),
                      "spark.hyperspace.index.numBuckets": "8",
                      "spark.sql.autoBroadcastJoinThreshold": "-1",
                      "spark.sql.shuffle.partitions": "8",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp / "wh"))
    hs = Hyperspace(s)
    df = s.read.parquet(str(tmp / "t"))
    hs.createIndex(df, IndexConfig("t_k", ["k"], ["id", "g", "d", "f", "s", "x", "i"]))
    Hyperspace.enable(s)
    return s, df, t, tmp


def _check(s, q, skipped=None, sort=True):
    g, c, path = _both(s, q, sort=sort)
    assert path == "native", s.backend().fallback_reason
    _close(g, c)
    if skipped is not None:
        assert s.backend().metrics.get("window_sort_skipped") is skipped
    return g


def _fallback(s, q, reason):
    g, c, path = _both(s, q)
    assert path == "fallback" and reason in s.backend().fallback_reason, \
        (path, s.backend().fallback_reason)
    _close(g, c)
    return g


def _all_functions(w, tie):
    """Every window function over ``w``; ``tie`` breaks order ties so row_number is defined."""
    wt = w.orderBy(*tie) if tie else w
    cols = [sum_("x").over(w).alias("sx"), sum_("i").over(w).alias("si"),
            count("x").over(w).alias("cx"), count("*").over(w).alias("n"),
            min_("x").over(w).alias("mnx"), max_("x").over(w).alias("mxx"),
            min_("i").over(w).alias("mni"), max_("i").over(w).alias("mxi"),
            avg("x").over(w).alias("ax"), avg("i").over(w).alias("ai"),
            max_("s").over(w).alias("mxs"), min_("d").over(w).alias("mnd")]
    if tie:
        cols += [rank().over(w).alias("r"), dense_rank().over(w).alias("dr"),
                 row_number().over(wt).alias("rn")]
    return cols


def test_every_function_over_the_index_and_over_plain_files(data):
    s, df, t, _ = data
    w = Window.partitionBy("k").orderBy("d")
    tie = [col("d"), col("id")]
    q = df.filter(col("k") >= 0).select("id", "k", *_all_functions(w, tie))
    g = _check(s, q, skipped=False)       # ordered by d: one device sort
    assert g.num_rows == N
    whole = df.filter(col("k") >= 0).select("id", "k", *_all_functions(Window.partitionBy("k"),
                                                                      None))
    g = _check(s, whole, skipped=True)    # the index order is the window's
    by_k = {}
    for r in t.to_pylist():
        by_k.setdefault(r["k"], []).append(r)
    rows = {r["id"]: r for r in g.to_pylist()}
    for r in t.to_pylist()[:200]:
        xs = [q["x"] for q in by_k[r["k"]] if q["x"] is not None]
        got = rows[r["id"]]
        assert got["n"] == len(by_k[r["k"]]) and got["cx"] == len(xs)
        assert got["sx"] == (pytest.approx(sum(xs)) if xs else None)
    assert all(r["sx"] is None and r["cx"] == 0 for r in rows.values() if r["k"] == 7)
    # the plain relation (no index): exchange and sort belong to the plan, one device sort runs
    s.disableHyperspace()
    try:
        _check(s, df.select("id", "k", *_all_functions(w, tie)), skipped=False)
        _check(s, df.select("id", *_all_functions(Window.partitionBy("g"), None)), skipped=False)
    finally:
        s.enableHyperspace()


@pytest.mark.parametrize("key", ["d", "f", "s", "i", "id"])
@pytest.mark.parametrize("asc", [True, False], ids=["asc", "desc"])
def test_order_keys_ascending_and_descending(data, key, asc):
    s, df, _, _ = data
    o = col(key) if asc else col(key).desc()
    w = Window.partitionBy("k").orderBy(o)
    q = df.filter(col("k") >= 0).select(
        "id", rank().over(w).alias("r"), dense_rank().over(w).alias("dr"),
        row_number().over(Window.partitionBy("k").orderBy(o, col("id"))).alias("rn"),
        sum_("i").over(w).alias("si"), count("x").over(w).alias("cx"),
        max_("x").over(w).alias("mx"))
    _check(s, q, skipped=False)


def test_sort_skipped_only_for_an_index_on_the_partition_column(data):
    s, df, _, _ = data
    base = df.filter(col("k") >= 0)
    _check(s, base.select("id", count("*").over(Window.partitionBy("k")).alias("n")), skipped=True)
    _check(s, base.select("id", max_("x").over(Window.partitionBy("k")).alias("m"))
           .groupBy("m").agg(count("*").alias("c")), skipped=True)
    _check(s, base.select("id", count("*").over(Window.partitionBy("g")).alias("n")),
           skipped=False)
    _check(s, base.select("id", count("*").over(Window.partitionBy("k", "g")).alias("n")),
           skipped=False)
    _check(s, base.select("id", sum_("i").over(Window.orderBy("id")).alias("run")), skipped=False)
    _check(s, base.select("id", rank().over(Window.partitionBy("k").orderBy(col("k").desc()))
                          .alias("r")), skipped=False)


def test_filter_below_and_above_the_window(data):
    s, df, t, _ = data
    w = Window.partitionBy("k").orderBy(col("x").desc(), col("id"))
    ranked = df.filter((col("k") >= 100) & (col("k") < 400) & (col("g") != 3)).select(
        "id", "k", "x", row_number().over(w).alias("rn"), sum_("x").over(w).alias("run"))
    g = _check(s, ranked)
    assert g.num_rows == sum(1 for r in t.to_pylist() if 100 <= r["k"] < 400 and r["g"] != 3)
    _check(s, ranked.filter((col("rn") <= 3) & (col("run") > 50.0)))
    # filtered rows of the index in table order: still no sort
    q = df.filter((col("k") >= 100) & (col("g") != 3)).select(
        "id", sum_("i").over(Window.partitionBy("k")).alias("si"))
    _check(s, q, skipped=True)


def test_top_three_per_key_and_an_aggregate_over_the_result(data):
    s, df, t, _ = data
    w = Window.partitionBy("k").orderBy(col("x").desc(), col("id"))
    top = df.filter(col("k") >= 0).select("id", "k", "g", "x", row_number().over(w).alias("rn")) \
        .filter(col("rn") <= 3)
    g = _check(s, top)
    by_k = {}
    for r in t.to_pylist():
        by_k.setdefault(r["k"], []).append(r)
    want = set()
    for rs in by_k.values():
        rs.sort(key=lambda r: (r["x"] is None, -(r["x"] or 0.0), r["id"]))
        want |= {r["id"] for r in rs[:3]}
    assert set(g.column("id").to_pylist()) == want
    _check(s, top.agg(sum_("x").alias("sx"), count("*").alias("n")))
    _check(s, top.groupBy("g").agg(sum_("x").alias("sx"), count("*").alias("n"),
                                   max_("rn").alias("mr")))
    df.createOrReplaceTempView("t")
    q = s.sql("SELECT k, id, rn FROM (SELECT k, id, row_number() OVER (PARTITION BY k ORDER BY "
              "x DESC, id) AS rn FROM t WHERE k >= 0) r WHERE rn <= 3 ORDER BY k, rn LIMIT 40")
    g = _check(s, q, sort=False)
    assert g.num_rows == 40 and g.column("rn").to_pylist()[:3] == [1, 2, 3]


def test_two_specs_in_one_select(data):
    s, df, _, _ = data
    w1 = Window.partitionBy("k").orderBy("d")
    w2 = Window.partitionBy("g").orderBy(col("id").desc())
    q = df.filter(col("k") >= 0).select(
        "id", rank().over(w1).alias("r"), sum_("x").over(w1).alias("sx"),
        (sum_("i").over(w2) + 1).alias("si1"), count("*").over(Window.partitionBy("k")).alias("n"))
    _check(s, q)


def test_over_an_empty_specification(data):
    s, df, t, _ = data
    w = Window.partitionBy()
    q = df.filter(col("k") >= 0).select("id", count("*").over(w).alias("n"),
                                        sum_("i").over(w).alias("si"), max_("x").over(w).alias("mx"))
    g = _check(s, q, skipped=False)
    assert set(g.column("n").to_pylist()) == {N}
    df.createOrReplaceTempView("t")
    g = _check(s, s.sql("SELECT id, count(*) OVER () AS n, min(d) OVER () AS md FROM t "
                        "WHERE k >= 250"))
    assert set(g.column("n").to_pylist()) == {sum(1 for v in t.column("k").to_pylist()
                                                  if v >= 250)}


def test_nan_order_keys_rank_as_the_greatest_value_on_both_engines(data):
    s, df, t, _ = data
    base = df.filter(col("k") >= 0)
    for asc in (True, False):
        w = Window.partitionBy("g").orderBy(col("f") if asc else col("f").desc())
        g = _check(s, base.select("id", "g", rank().over(w).alias("r"),
                                  dense_rank().over(w).alias("dr"),
                                  count("i").over(w).alias("ci")))
        rows = t.to_pylist()
        nan_ids = {r["id"] for r in rows if r["f"] is not None and r["f"] != r["f"]}
        assert nan_ids
        got = {r["id"]: r for r in g.to_pylist()}
        per_g = {}
        for r in rows:
            per_g.setdefault(r["g"], []).append(r)
        for i in list(nan_ids)[:50]:
            rs = per_g[got[i]["g"]]
            nans = sum(1 for r in rs if r["f"] is not None and r["f"] != r["f"])
            # after every number and NULL ascending, before all of them descending
            assert got[i]["r"] == (len(rs) - nans + 1 if asc else 1)


def test_same_shape_with_new_literals(data):
    s, df, t, _ = data
    w = Window.partitionBy("k").orderBy("id")
    q = lambda lo: df.filter(col("k") >= lo).select(        # noqa: E731
        "id", row_number().over(w).alias("rn")).agg(max_("rn").alias("m"), count("*").alias("n"))
    got = [_check(s, q(lo)).to_pylist()[0] for lo in (100, 450)]
    assert [r["n"] for r in got] == [sum(1 for v in t.column("k").to_pylist() if v >= lo)
                                     for lo in (100, 450)]


# ------------------------------------------------------------------------------------------------
# fallbacks: the host engine answers, with the same result
# ------------------------------------------------------------------------------------------------
def test_expression_key_float_partition_key_and_decimal_argument_fall_back(data):
    s, df, _, _ = data
    base = df.filter(col("k") >= 0)
    _fallback(s, base.select("id", count("*").over(Window.partitionBy(col("k") % 3)).alias("n")),
              "key that is an expression")
    _fallback(s, base.select("id", rank().over(Window.partitionBy("k").orderBy(col("i") * 2))
                             .alias("r")), "key that is an expression")
    _fallback(s, base.select("id", count("*").over(Window.partitionBy("f")).alias("n")),
              "float column")
    s.disableHyperspace()           # the decimal column is not in the index
    try:
        _fallback(s, df.select("id", sum_("m").over(Window.partitionBy("k")).alias("sm")),
                  "decimal")
    finally:
        s.enableHyperspace()


def test_streamed_index_falls_back(data):
    s, df, _, _ = data
    q = df.filter(col("k") >= 0).select("id", sum_("i").over(Window.partitionBy("k")).alias("si"))
    _check(s, q)
    budget = "spark.hyperspace.mi.deviceCacheBytes"
    s.conf.set(budget, str(64 * 1024))
    try:
        _fallback(s, q, "streamed")
    finally:
        s.conf.unset(budget)
    _check(s, q)


def test_more_than_one_rank_falls_back(data, monkeypatch):
    s, df, _, _ = data
    q = df.filter(col("k") >= 0).select("id", sum_("i").over(Window.partitionBy("k")).alias("si"))

    class TwoRanks:
        rank, world = 0, 2
    from hyperspace_amd.exec import window as W
    real = W.window_rel

    def two_ranks(be, p):
        monkeypatch.setattr(be, "_dist", lambda: TwoRanks(), raising=False)
        try:
            return real(be, p)
        finally:
            monkeypatch.undo()
    monkeypatch.setattr(W, "window_rel", two_ranks)
    _fallback(s, q, "more than one rank")


def test_string_key_without_a_device_dictionary_falls_back(data, monkeypatch):
    """No load path leaves a string column without its dictionary today, so the scan's relation
    is given one: the same codes with ``dictionary=None``."""
    s, df, _, _ = data
    from hyperspace_amd.exec.device_table import DeviceColumn
    from hyperspace_amd.exec.gpu import GpuBackend
    real = GpuBackend._scan_memo

    def undictionaried(self, p):
        r = real(self, p)
        for a in p.output:
            if a.name == "s":
                c = r.col(a)
                r.extra[r.colmap[a.expr_id]] = DeviceColumn(c.data, c.valid, c.atype, None)
        return r
    base = df.filter(col("k") >= 0)
    queries = [
        (base.select("id", rank().over(Window.partitionBy("k").orderBy("s")).alias("r")), "key s"),
        (base.select("id", count("*").over(Window.partitionBy("s")).alias("n")), "key s"),
        (base.select("id", max_("s").over(Window.partitionBy("k")).alias("m")), "max over")]
    for q, _ in queries:
        _check(s, q)
    monkeypatch.setattr(GpuBackend, "_scan_memo", undictionaried)
    for q, reason in queries:
        g = _fallback(s, q, reason)
        assert "without a device dictionary" in s.backend().fallback_reason
        assert g.num_rows == N


def test_bucket_union_input_falls_back(data):
    s, df, t, tmp = data
    for k, v in (("lineage.enabled", "true"), ("hybridscan.enabled", "true"),
                 ("hybridscan.maxAppendedRatio", "0.9")):
        s.conf.set(f"spark.hyperspace.index.{k}", v)
    src = tmp / "h"
    os.makedirs(src)
    small = t.select(["id", "k", "i"]).slice(0, 2000)
    pq.write_table(small, src / "part-0.parquet")
    hs = Hyperspace(s)
    hs.createIndex(s.read.parquet(str(src)), IndexConfig("h_k", ["k"], ["id", "i"]))
    pq.write_table(small.slice(0, 300), src / "part-1.parquet")
    hdf = s.read.parquet(str(src))
    q = hdf.filter(col("k") >= 0).select("id", sum_("i").over(Window.partitionBy("k")).alias("si"))
    try:
        assert "BucketUnion" in q.queryExecution.executed_plan.tree_string()
        s.conf.set("spark.hyperspace.mi.hybridMerge.enabled", "false")
        _fallback(s, q, "bucket union")
        s.conf.set("spark.hyperspace.mi.hybridMerge.enabled", "true")
        _check(s, q)                  # merged into one table: native
    finally:
        s.conf.set("spark.hyperspace.mi.hybridMerge.enabled", "true")
        for k in ("lineage.enabled", "hybridscan.enabled", "hybridscan.maxAppendedRatio"):
            s.conf.unset(f"spark.hyperspace.index.{k}")
