"""count(DISTINCT x), countDistinct and DataFrame.distinct(): parser, API, plan shape, the host
oracle against plain Python sets, the plan cache and the index rules.  No GPU needed."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import (Hyperspace, HyperspaceException, IndexConfig, avg, col, count,
                            countDistinct, count_distinct, max_, min_, sum_)
from hyperspace_amd.plan import expressions as E, physical as X
from hyperspace_amd.plan.parser import parse_expression
from hyperspace_amd.plan.plan_cache import plan_cache

from helpers import index_names_used

_NAN2 = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]


def _table() -> pa.Table:
    """Groups: "a" (x and f with duplicates, both zeros), "b" (x all NULL, two NaN payloads),
    "c", and the NULL group."""
    g = ["a"] * 6 + ["b"] * 4 + ["c"] * 3 + [None] * 3
    x = [1, 1, 2, None, 3, 3, None, None, None, None, 7, 7, 7, 5, None, 6]
    f = [0.0, -0.0, 1.5, 1.5, None, -0.0, float("nan"), _NAN2, float("nan"), 2.0,
         -1.0, -1.0, None, 0.0, 4.0, float("nan")]
    s = ["p", "q", "p", None, "r", "r", "z", "z", None, "z", "u", "v", "w", None, "m", "m"]
    y = [1.0, None, 3.0, 4.0, 5.0, 6.0, None, None, 9.0, 10.0, 11.0, 12.0, 13.0, 14.0, None,
         16.0]
    return pa.table({"g": pa.array(g), "x": pa.array(x, pa.int64()), "f": pa.array(f),
                     "s": pa.array(s), "y": pa.array(y),
                     "k": pa.array(np.arange(16, dtype=np.int64))})


@pytest.fixture
def frame(session, tmp_path):
    (tmp_path / "t").mkdir()
    pq.write_table(_table(), tmp_path / "t" / "p0.parquet")
    return session, session.read.parquet(str(tmp_path / "t"))


def _fkey(v):
    """Spark's equality of doubles for a distinct count: one zero, one NaN."""
    if v != v:
        return "nan"
    return 0.0 if v == 0.0 else v


def _expected(rows, groups=True):
    """{group: (distinct x, distinct f, distinct s, sum y, count(*), count y, min y, max y,
    avg y)} from plain Python sets."""
    out = {}
    for r in rows:
        out.setdefault(r["g"] if groups else None, []).append(r)
    res = {}
    for gk, rs in out.items():
        ys = [r["y"] for r in rs if r["y"] is not None]
        res[gk] = (len({r["x"] for r in rs if r["x"] is not None}),
                   len({_fkey(r["f"]) for r in rs if r["f"] is not None}),
                   len({r["s"] for r in rs if r["s"] is not None}),
                   sum(ys) if ys else None, len(rs), len(ys), min(ys) if ys else None,
                   max(ys) if ys else None, sum(ys) / len(ys) if ys else None)
    return res


# ------------------------------------------------------------------------------------------------
# parser
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", ["count(DISTINCT x)", "COUNT( distinct x )", "Count(Distinct x)"])
def test_parser_accepts_count_distinct(text):
    e = parse_expression(text)
    assert isinstance(e, E.CountDistinct) and not isinstance(e, E.Count)
    assert isinstance(e.child, E.UnresolvedAttribute) and e.child.name == "x"
    assert e.sql().startswith("count(DISTINCT ")
    assert e.data_type == pa.int64() and not e.nullable


def test_parser_distinct_over_an_expression_and_plain_count_unchanged():
    e = parse_expression("count(distinct x + 1) > 2")
    assert isinstance(e.left, E.CountDistinct) and isinstance(e.left.child, E.Add)
    assert type(parse_expression("count(x)")) is E.Count
    assert type(parse_expression("count(*)")) is E.Count


@pytest.mark.parametrize("text", ["count(DISTINCT a, b)", "sum(DISTINCT x)", "avg(distinct x)"])
def test_parser_rejects_unsupported_distinct_spellings(text):
    with pytest.raises(SyntaxError, match="not supported"):
        parse_expression(text)


def test_sql_select_having_and_order_by_alias(frame):
    s, df = frame
    df.createOrReplaceTempView("t")
    q = s.sql("SELECT g, COUNT(DISTINCT x) AS c FROM t GROUP BY g "
              "HAVING count( distinct x ) >= 1 ORDER BY c DESC, g")
    want = _expected(_table().to_pylist())
    rows = [(r[0], r[1]) for r in q.collect()]
    assert sorted(rows, key=str) == sorted(((g, v[0]) for g, v in want.items() if v[0] >= 1),
                                           key=str)
    assert [r[1] for r in rows] == sorted((r[1] for r in rows), reverse=True)
    with pytest.raises(SyntaxError, match="not supported"):
        s.sql("SELECT count(DISTINCT x, y) FROM t")
    with pytest.raises(SyntaxError, match="not supported"):
        s.sql("SELECT sum(DISTINCT x) FROM t")


# ------------------------------------------------------------------------------------------------
# API
# ------------------------------------------------------------------------------------------------
def test_api_spellings_agree(frame):
    _, df = frame
    a = df.groupBy("g").agg(countDistinct("x").alias("c")).collect()
    b = df.groupBy("g").agg(count_distinct(col("x")).alias("c")).collect()
    c = df.groupBy("g").agg("count(DISTINCT x)").collect()
    d = df.groupBy("g").agg({"x": "count_distinct"}).collect()
    key = lambda rows: sorted(((r[0], r[1]) for r in rows), key=str)   # noqa: E731
    assert key(a) == key(b) == key(c) == key(d)
    assert dict(key(a)) == {g: v[0] for g, v in _expected(_table().to_pylist()).items()}
    with pytest.raises(HyperspaceException, match="not supported"):
        countDistinct("x", "y")


def test_distinct_rows_and_count_distinct(frame):
    _, df = frame
    for name in ("x", "s", "g"):
        n = df.agg(countDistinct(name)).collect()[0][0]
        has_null = _table().column(name).null_count > 0
        assert df.select(name).distinct().count() == n + (1 if has_null else 0)
    pairs = {(r["g"], r["x"]) for r in _table().to_pylist()}
    assert df.select("g", "x").distinct().count() == len(pairs)


def test_explain_shows_count_distinct(frame):
    _, df = frame
    q = df.groupBy("g").agg(countDistinct("x").alias("c"))
    text = q.queryExecution.explain_string(True)
    assert text.count("count(DISTINCT x#") >= 3      # analyzed, optimized and physical plan


# ------------------------------------------------------------------------------------------------
# plan shape
# ------------------------------------------------------------------------------------------------
def test_distinct_aggregate_plans_one_complete_aggregate_over_an_exchange(frame):
    _, df = frame
    for q, part in ((df.groupBy("g").agg(countDistinct("x"), sum_("y")), X.HashPartitioning),
                    (df.agg(countDistinct("x")), X.SinglePartition)):
        plan = q.queryExecution.executed_plan
        aggs = plan.collect(lambda p: isinstance(p, X.HashAggregateExec))
        assert [a.mode for a in aggs] == ["complete"]
        assert isinstance(aggs[0].child, X.ShuffleExchangeExec)
        assert isinstance(aggs[0].child.partitioning, part)
        assert not isinstance(aggs[0].child.child, X.HashAggregateExec)


def test_non_distinct_aggregate_plan_is_unchanged(frame):
    _, df = frame
    q = df.groupBy("g").agg(sum_("y").alias("sy"), count("*").alias("n"))
    plan = q.queryExecution.executed_plan
    assert [a.mode for a in plan.collect(lambda p: isinstance(p, X.HashAggregateExec))] == \
        ["final", "partial"]
    import re
    text = re.sub(r"#\d+", "#", plan.tree_string())
    lines = [ln.strip() for ln in text.splitlines()]
    assert lines[0] == "HashAggregate(keys=[g#], functions=[sum(y#), count(1)])"
    assert lines[1].startswith("+- Exchange hashpartitioning(g#, ")
    assert lines[2] == "+- HashAggregate(keys=[g#], functions=[partial_sum(y#), partial_count(1)])"
    assert lines[3].startswith("+- FileScan parquet [g#,y#]")


def test_optimizer_keeps_x_and_infers_no_not_null(frame):
    _, df = frame
    q = df.filter(col("k") >= 0).groupBy("g").agg(countDistinct("x").alias("c"))
    opt = q.queryExecution.optimized_plan.tree_string()
    assert "isnotnull(x#" not in opt
    scan = q.queryExecution.executed_plan.collect(
        lambda p: isinstance(p, X.FileSourceScanExec))[0]
    assert {a.name for a in scan.output} == {"g", "x", "k"}


# ------------------------------------------------------------------------------------------------
# host results against Python sets
# ------------------------------------------------------------------------------------------------
def test_grouped_results_match_python_sets(frame):
    _, df = frame
    q = df.groupBy("g").agg(countDistinct("x").alias("dx"), countDistinct("f").alias("df"),
                            countDistinct("s").alias("ds"), sum_("y").alias("sy"),
                            count("*").alias("n"), count("y").alias("ny"),
                            min_("y").alias("mn"), max_("y").alias("mx"), avg("y").alias("av"))
    got = {r[0]: tuple(r[1:]) for r in q.collect()}
    want = _expected(_table().to_pylist())
    assert set(got) == set(want) == {"a", "b", "c", None}
    for gk in want:
        assert got[gk] == pytest.approx(want[gk]), gk
    assert want["b"][0] == 0 and got["b"][0] == 0           # x all NULL in "b"
    assert got["a"][1] == 2                                 # 0.0, -0.0 once; 1.5
    assert got["b"][1] == 2                                 # two NaN payloads once; 2.0
    t = q.to_arrow()
    assert t.schema.field("dx").type == pa.int64() and t.column("dx").null_count == 0


def test_ungrouped_and_empty_input(frame):
    _, df = frame
    q = df.agg(countDistinct("x"), countDistinct("f"), countDistinct("s"), sum_("y"), count("*"),
               count("y"), min_("y"), max_("y"), avg("y"))
    want = _expected(_table().to_pylist(), groups=False)[None]
    assert tuple(q.collect()[0]) == pytest.approx(want)
    empty = df.filter(col("k") > 1000).agg(countDistinct("x"), sum_("y"), count("*"))
    assert [tuple(r) for r in empty.collect()] == [(0, None, 0)]
    # grouped over an empty input: no rows
    assert df.filter(col("k") > 1000).groupBy("g").agg(countDistinct("x")).count() == 0


def test_distinct_of_an_expression_and_a_grouping_expression(frame):
    _, df = frame
    q = df.groupBy((col("k") % 2).alias("m")).agg(countDistinct(col("x") % 2).alias("c"))
    want = {}
    for r in _table().to_pylist():
        if r["x"] is not None:
            want.setdefault(r["k"] % 2, set()).add(r["x"] % 2)
        else:
            want.setdefault(r["k"] % 2, set())
    assert {r[0]: r[1] for r in q.collect()} == {m: len(v) for m, v in want.items()}


# ------------------------------------------------------------------------------------------------
# plan cache and index rules
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def indexed(session, tmp_path):
    rng = np.random.default_rng(5)
    n = 3000
    x = rng.integers(0, 40, n).astype(np.int64)
    t = pa.table({"k": rng.integers(0, 300, n).astype(np.int64),
                  "x": pa.array(x, mask=rng.random(n) < 0.1),
                  "v": rng.random(n)})
    (tmp_path / "big").mkdir()
    pq.write_table(t, tmp_path / "big" / "p0.parquet")
    hs = Hyperspace(session)
    df = session.read.parquet(str(tmp_path / "big"))
    hs.createIndex(df, IndexConfig("by_k", ["k"], ["x", "v"]))
    Hyperspace.enable(session)
    return session, df, t


def _py_distinct(t, lo):
    return len({r["x"] for r in t.to_pylist() if r["k"] >= lo and r["x"] is not None})


def test_plan_cache_keeps_count_and_count_distinct_apart(indexed):
    s, df, t = indexed
    a = df.filter(col("k") >= 10).agg(count("x").alias("c")).collect()[0][0]
    b = df.filter(col("k") >= 10).agg(countDistinct("x").alias("c")).collect()[0][0]
    assert b == _py_distinct(t, 10)
    assert a == sum(1 for r in t.to_pylist() if r["k"] >= 10 and r["x"] is not None)
    assert a > b


def test_plan_cache_hit_takes_the_new_literal(indexed):
    s, df, t = indexed
    pc = plan_cache(s)
    q = lambda lo: df.filter(col("k") >= lo).agg(countDistinct("x").alias("c"))   # noqa: E731
    first = q(250).collect()[0][0]
    hits = pc.hits
    second = q(295).collect()[0][0]
    assert pc.hits > hits
    assert first == _py_distinct(t, 250) and second == _py_distinct(t, 295)
    assert first != second


def test_filter_index_rule_still_swaps_the_scan(indexed):
    s, df, t = indexed
    q = lambda: df.filter(col("k") >= 100).groupBy("k").agg(   # noqa: E731
        countDistinct("x").alias("c"), sum_("v").alias("sv"))
    assert index_names_used(q()) == {"by_k"}
    on = sorted(tuple(r) for r in q().collect())
    s.disableHyperspace()
    assert index_names_used(q()) == set()
    off = sorted(tuple(r) for r in q().collect())
    assert [r[:2] for r in on] == [r[:2] for r in off]
    assert [r[2] for r in on] == pytest.approx([r[2] for r in off])
    want = {}
    for r in t.to_pylist():
        if r["k"] >= 100:
            want.setdefault(r["k"], set())
            if r["x"] is not None:
                want[r["k"]].add(r["x"])
    assert {r[0]: r[1] for r in on} == {k: len(v) for k, v in want.items()}
