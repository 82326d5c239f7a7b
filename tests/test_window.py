"""Window functions (``fn(...) OVER (PARTITION BY ... ORDER BY ...)``): parser, API, errors, result
types, plan shape, optimizer rules, the plan cache and the host engine against a plain Python
loop.  No GPU needed."""
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import (Hyperspace, HyperspaceException, IndexConfig, Window, avg, col, count,
                            dense_rank, max_, min_, rank, row_number, sum_)
from hyperspace_amd.plan import expressions as E, logical as L, physical as X
from hyperspace_amd.plan import plan_cache as PC
from hyperspace_amd.plan.parser import parse_expression

from helpers import index_names_used


def _table() -> pa.Table:
    """Partitions by k: 1 (ties and a NULL in d), 2 (x all NULL), 3 (one row), NULL (two rows)."""
    k = [1, 1, 1, 1, 1, 2, 2, 2, 3, None, None, 1]
    d = [5, 3, 3, None, 9, 4, 4, 1, 7, 2, None, 3]
    x = [1.5, 2.0, None, 4.0, -1.0, None, None, None, 8.0, 0.25, 3.0, 6.5]
    i = [10, None, 30, 40, 50, 1, None, 3, None, 7, 8, 9]
    s = ["b", "a", None, "d", "c", "z", "y", None, "q", "m", "n", "a"]
    return pa.table({"id": pa.array(range(len(k)), pa.int64()), "k": pa.array(k, pa.int64()),
                     "d": pa.array(d, pa.int32()), "x": pa.array(x, pa.float64()),
                     "i": pa.array(i, pa.int32()), "s": pa.array(s)})


@pytest.fixture
def frame(session, tmp_path):
    (tmp_path / "t").mkdir()
    t = _table()
    pq.write_table(t.slice(0, 7), tmp_path / "t" / "p0.parquet")
    pq.write_table(t.slice(7), tmp_path / "t" / "p1.parquet")
    return session, session.read.parquet(str(tmp_path / "t"))


# ------------------------------------------------------------------------------------------------
# the reference: a plain Python loop
# ------------------------------------------------------------------------------------------------
def py_window(rows, part, order, fn, arg=None):
    """{id: value} of ``fn`` (row_number / rank / dense_rank / sum / count / min / max / avg of
    column ``arg``) over PARTITION BY ``part`` ORDER BY ``order`` [(column, ascending)], Spark's
    default frame; ASC sorts NULLS FIRST, DESC NULLS LAST.  ``row_number`` of tied rows follows
    the input order (a stable sort), which a caller must not rely on."""
    parts = {}
    for r in rows:
        parts.setdefault(tuple(r[c] for c in part), []).append(r)
    out = {}
    for rs in parts.values():
        for c, asc in reversed(order):
            some = next((r[c] for r in rs if r[c] is not None), 0)
            rs.sort(key=lambda r: (r[c] is not None, r[c] if r[c] is not None else type(some)()),
                    reverse=not asc)
        peer = [tuple(r[c] for c, _ in order) for r in rs]
        for j, r in enumerate(rs):
            if order:
                first = peer.index(peer[j])
                last = len(rs) - 1 - peer[::-1].index(peer[j])
            else:
                first, last = 0, len(rs) - 1
            if fn == "row_number":
                out[r["id"]] = j + 1
            elif fn == "rank":
                out[r["id"]] = first + 1
            elif fn == "dense_rank":
                out[r["id"]] = len(dict.fromkeys(peer[:first + 1]))
            else:
                vals = [1 if arg is None else q[arg] for q in rs[:last + 1]
                        if arg is None or q[arg] is not None]
                if fn == "count":
                    out[r["id"]] = len(vals)
                elif not vals:
                    out[r["id"]] = None
                elif fn == "sum":
                    out[r["id"]] = sum(vals)
                elif fn == "avg":
                    out[r["id"]] = sum(vals) / len(vals)
                else:
                    out[r["id"]] = min(vals) if fn == "min" else max(vals)
    return out


def _by_id(q, name):
    return {r["id"]: r[name] for r in q.to_arrow().to_pylist()}


def _same(got: dict, want: dict):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, float) and g is not None:
            assert g == pytest.approx(w, rel=1e-12), k
        else:
            assert g == w, (k, g, w)


# ------------------------------------------------------------------------------------------------
# parser, SQL text and the API
# ------------------------------------------------------------------------------------------------
def test_parser_builds_the_window_expression():
    e = parse_expression("sum(x) OVER (PARTITION BY k, g ORDER BY d DESC, e)")
    assert isinstance(e, E.WindowExpression) and isinstance(e.function, E.Sum)
    assert [c.name for c in e.spec.partition_by] == ["k", "g"]
    assert [(c.name, a) for c, a in e.spec.order_by] == [("d", False), ("e", True)]
    assert e.sql() == ("sum('x) OVER (PARTITION BY 'k, 'g ORDER BY 'd DESC NULLS LAST, "
                       "'e ASC NULLS FIRST)")
    e = parse_expression("row_number() over (order by d asc nulls first) <= 3")
    assert isinstance(e, E.LessThanOrEqual) and isinstance(e.left.function, E.RowNumber)
    e = parse_expression("count(*) over ()")
    assert isinstance(e.function, E.Count) and e.spec.partition_by == [] and not e.spec.order_by
    for name, cls in (("rank", E.Rank), ("dense_rank", E.DenseRank), ("ROW_NUMBER", E.RowNumber)):
        assert type(parse_expression(f"{name}() over (order by d)").function) is cls
    # plain calls and a column called "over" parse as before
    assert type(parse_expression("sum(x)")) is E.Sum
    assert parse_expression("over > 1").left.name == "over"


def test_sql_round_trip_resolves_to_the_same_plan(frame):
    s, df = frame
    df.createOrReplaceTempView("t")
    a = s.sql("SELECT id, rank() OVER (PARTITION BY k ORDER BY d DESC) AS r, "
              "sum(x) OVER (PARTITION BY k ORDER BY d DESC) sx FROM t")
    w = Window.partitionBy("k").orderBy(col("d").desc())
    b = df.select("id", rank().over(w).alias("r"), sum_("x").over(w).alias("sx"))
    strip = lambda p: re.sub(r"#\d+", "#", p.tree_string())    # noqa: E731
    assert strip(a.plan) == strip(b.plan)
    assert "rank() OVER (PARTITION BY k# ORDER BY d# DESC NULLS LAST) AS r#" in strip(a.plan)
    _same(_by_id(a, "r"), _by_id(b, "r"))
    text = a.queryExecution.explain_string(True)
    assert text.count("OVER (PARTITION BY k#") >= 6         # two functions in three plans


def test_error_cases(frame):
    s, df = frame
    df.createOrReplaceTempView("t")
    with pytest.raises(HyperspaceException, match="frames .* not supported"):
        parse_expression("sum(x) over (order by d rows between 1 preceding and current row)")
    with pytest.raises(HyperspaceException, match="frames .* not supported"):
        s.sql("SELECT sum(x) OVER (ORDER BY d RANGE BETWEEN UNBOUNDED PRECEDING AND "
              "CURRENT ROW) FROM t")
    with pytest.raises(HyperspaceException, match="frames .* not supported"):
        Window.partitionBy("k").orderBy("d").rowsBetween(Window.unboundedPreceding, 0)
    with pytest.raises(HyperspaceException, match="frames .* not supported"):
        Window.orderBy("d").rangeBetween(-1, 1)
    with pytest.raises(HyperspaceException, match="frames .* not supported"):
        E.WindowSpecDefinition([], [], frame="ROWS BETWEEN 1 PRECEDING AND CURRENT ROW")
    for fn in (row_number, rank, dense_rank):
        with pytest.raises(HyperspaceException, match="requires the window to be ordered"):
            fn().over(Window.partitionBy("k"))
    with pytest.raises(HyperspaceException, match="requires the window to be ordered"):
        s.sql("SELECT dense_rank() OVER (PARTITION BY k) FROM t")
    with pytest.raises(HyperspaceException, match="requires an OVER clause"):
        df.select("id", rank())
    with pytest.raises(HyperspaceException, match="not a window function"):
        (col("x") + 1).over(Window.partitionBy("k"))
    with pytest.raises(HyperspaceException, match="not allowed in WHERE"):
        s.sql("SELECT id FROM t WHERE row_number() OVER (ORDER BY d) <= 3")
    with pytest.raises(HyperspaceException, match="not allowed in a filter"):
        df.filter("row_number() over (order by d) <= 3")
    with pytest.raises(HyperspaceException, match="default null ordering"):
        parse_expression("rank() over (order by d desc nulls first)")
    with pytest.raises(SyntaxError, match="no arguments"):
        parse_expression("rank(x) over (order by d)")


def test_keys_and_sql_text_carry_function_keys_and_directions():
    def w(fn, part, order):
        return E.WindowExpression(fn, E.WindowSpecDefinition(
            [E.UnresolvedAttribute(c) for c in part],
            [(E.UnresolvedAttribute(c), a) for c, a in order]))
    base = w(E.Rank(), ["k"], [("d", True)])
    others = [w(E.DenseRank(), ["k"], [("d", True)]), w(E.RowNumber(), ["k"], [("d", True)]),
              w(E.Rank(), ["k"], [("d", False)]), w(E.Rank(), ["g"], [("d", True)]),
              w(E.Rank(), ["k"], [("e", True)]), w(E.Rank(), [], [("d", True)]),
              w(E.Rank(), ["k"], [("d", True), ("e", True)]),
              w(E.Rank(), ["k", "d"], [("d", True)])]
    assert base.semantic_equals(w(E.Rank(), ["k"], [("d", True)]))
    for o in others:
        assert not base.semantic_equals(o), o.sql()
        assert base.sql() != o.sql()
    # a key moved between the two lists is another window
    assert not w(E.Sum(E.UnresolvedAttribute("x")), ["k", "d"], []).semantic_equals(
        w(E.Sum(E.UnresolvedAttribute("x")), ["k"], [("d", True)]))


def test_contains_aggregate_looks_past_window_expressions(frame):
    _, df = frame
    w = Window.partitionBy("k")
    e = sum_("x").over(w).expr
    assert not E.contains_aggregate(e) and E.contains_window(e)
    assert not E.contains_aggregate(E.Add(e, E.Literal(1)))
    assert E.contains_aggregate(E.Sum(E.UnresolvedAttribute("x")))
    q = df.select("id", sum_("x").over(w).alias("sx"))
    assert isinstance(q.plan, L.Project) and isinstance(q.plan.child, L.Window)
    assert q.count() == _table().num_rows         # a projection: one row per input row


def test_result_types(frame):
    _, df = frame
    w = Window.partitionBy("k").orderBy("d")
    q = df.select(row_number().over(w).alias("rn"), rank().over(w).alias("r"),
                  dense_rank().over(w).alias("dr"), count("x").over(w).alias("c"),
                  count("*").over(w).alias("cs"), sum_("i").over(w).alias("si"),
                  sum_("x").over(w).alias("sx"), avg("i").over(w).alias("ai"),
                  min_("i").over(w).alias("mi"), max_("x").over(w).alias("mx"),
                  min_("s").over(w).alias("ms"))
    want = {"rn": pa.int32(), "r": pa.int32(), "dr": pa.int32(), "c": pa.int64(),
            "cs": pa.int64(), "si": pa.int64(), "sx": pa.float64(), "ai": pa.float64(),
            "mi": pa.int32(), "mx": pa.float64(), "ms": pa.string()}
    assert {f.name: f.type for f in q.schema} == want
    t = q.to_arrow()
    assert {f.name: f.type for f in t.schema} == want
    for name in ("rn", "r", "dr", "c", "cs"):
        assert not q.schema.field(name).nullable and t.column(name).null_count == 0


# ------------------------------------------------------------------------------------------------
# plan shape and optimizer rules
# ------------------------------------------------------------------------------------------------
def _ops(plan):
    return [type(p).__name__ for p in plan.iter_pre()]


def test_plan_is_window_over_sort_over_exchange(frame):
    s, df = frame
    w = Window.partitionBy("k").orderBy(col("d").desc())
    q = df.select("id", rank().over(w).alias("r"))
    plan = q.queryExecution.executed_plan
    win = plan.collect(lambda p: isinstance(p, X.WindowExec))
    assert len(win) == 1
    sort = win[0].child
    assert isinstance(sort, X.SortExec) and not sort.global_sort
    assert [(o.child.name, o.ascending) for o in sort.order] == [("k", True), ("d", False)]
    exch = sort.child
    assert isinstance(exch, X.ShuffleExchangeExec)
    assert isinstance(exch.partitioning, X.HashPartitioning)
    assert [e.name for e in exch.partitioning.expressions] == ["k"]
    text = re.sub(r"#\d+", "#", win[0].simple_string())
    assert text == ("Window [rank() OVER (PARTITION BY k# ORDER BY d# DESC NULLS LAST) AS r#], "
                    "[k#], [d# DESC NULLS LAST]")
    # no partition keys: one partition
    q = df.select("id", row_number().over(Window.orderBy("d")).alias("rn"))
    win = q.queryExecution.executed_plan.collect(lambda p: isinstance(p, X.WindowExec))[0]
    assert isinstance(win.child.child.partitioning, X.SinglePartition)
    # the operator is counted by explain
    from hyperspace_amd.plananalysis.analyzer import physical_operator_stats
    assert physical_operator_stats(plan)["Window"] == 1


def test_two_specs_chain_two_windows_and_share_the_exchange(frame):
    _, df = frame
    w1 = Window.partitionBy("k").orderBy("d")
    w2 = Window.partitionBy("k")
    q = df.select("id", rank().over(w1).alias("r"), sum_("x").over(w1).alias("sx"),
                  (sum_("x").over(w2) + 1).alias("t"), count("*").over(w2).alias("n"))
    wins = q.plan.collect(lambda p: isinstance(p, L.Window))
    assert [len(x.window_exprs) for x in wins] == [2, 2]
    plan = q.queryExecution.executed_plan
    assert _ops(plan).count("WindowExec") == 2
    # the second window is partitioned and sorted by the first one's input already
    assert _ops(plan).count("ShuffleExchangeExec") == 1 and _ops(plan).count("SortExec") == 1


@pytest.fixture
def indexed(session, tmp_path):
    rng = np.random.default_rng(11)
    n = 2000
    t = pa.table({"id": np.arange(n, dtype=np.int64),
                  "k": rng.integers(0, 150, n).astype(np.int64),
                  "d": pa.array(rng.integers(0, 20, n).astype(np.int32), mask=rng.random(n) < 0.1),
                  "x": pa.array(rng.integers(-50, 50, n).astype(np.float64),
                                mask=rng.random(n) < 0.2),
                  "unused": rng.random(n)})
    (tmp_path / "big").mkdir()
    pq.write_table(t, tmp_path / "big" / "p0.parquet")
    hs = Hyperspace(session)
    df = session.read.parquet(str(tmp_path / "big"))
    hs.createIndex(df, IndexConfig("by_k", ["k"], ["id", "d", "x"]))
    Hyperspace.enable(session)
    return session, df, t


def test_matching_index_needs_neither_sort_nor_exchange(indexed):
    s, df, t = indexed
    q = df.filter(col("k") >= 0).select("id", "k", sum_("x").over(Window.partitionBy("k"))
                                        .alias("sx"))
    assert index_names_used(q) == {"by_k"}
    ops = _ops(q.queryExecution.executed_plan)
    assert "WindowExec" in ops and "SortExec" not in ops and "ShuffleExchangeExec" not in ops
    rows = [r for r in t.to_pylist() if r["k"] >= 0]
    _same(_by_id(q, "sx"), py_window(rows, ["k"], [], "sum", "x"))
    # an ORDER BY the index does not give: the sort stays, the exchange still goes
    q = df.filter(col("k") >= 0).select(
        "id", rank().over(Window.partitionBy("k").orderBy("d")).alias("r"))
    ops = _ops(q.queryExecution.executed_plan)
    assert ops.count("SortExec") == 1 and "ShuffleExchangeExec" not in ops
    _same(_by_id(q, "r"), py_window(rows, ["k"], [("d", True)], "rank"))
    # without the index both are planned
    s.disableHyperspace()
    ops = _ops(q.queryExecution.executed_plan)
    assert ops.count("SortExec") == 1 and ops.count("ShuffleExchangeExec") == 1


def test_filter_index_rule_applies_below_a_window(indexed):
    s, df, t = indexed
    q = lambda: df.filter(col("k") >= 100).select(    # noqa: E731
        "id", dense_rank().over(Window.partitionBy("k").orderBy(col("d").desc())).alias("dr"))
    opt = q().queryExecution.optimized_plan
    win = opt.find(lambda p: isinstance(p, L.Window))
    assert win is not None
    below = win.child.collect(lambda p: isinstance(p, (L.Filter, L.LogicalRelation)))
    assert isinstance(below[0], L.Filter) and below[1].relation.is_index()
    assert index_names_used(q()) == {"by_k"}
    on = _by_id(q(), "dr")
    s.disableHyperspace()
    assert index_names_used(q()) == set()
    _same(on, _by_id(q(), "dr"))
    rows = [r for r in t.to_pylist() if r["k"] >= 100]
    _same(on, py_window(rows, ["k"], [("d", False)], "dense_rank"))


def test_column_pruning_narrows_the_scan_below_a_window(indexed):
    _, df, _ = indexed
    q = df.select("id", sum_("x").over(Window.partitionBy("k").orderBy("d")).alias("sx"))
    scan = q.queryExecution.executed_plan.collect(
        lambda p: isinstance(p, X.FileSourceScanExec))[0]
    assert {a.name for a in scan.output} == {"id", "k", "d", "x"}
    # a window column nobody reads does not keep its inputs alive above the window
    q2 = q.select("id")
    assert [a.name for a in q2.queryExecution.optimized_plan.output] == ["id"]


def test_filter_stays_above_the_window(indexed):
    _, df, t = indexed
    w = Window.partitionBy("k").orderBy("id")
    ranked = df.select("id", "k", row_number().over(w).alias("rn"))
    q = ranked.filter((col("rn") <= 2) & (col("k") < 40))
    opt = q.queryExecution.optimized_plan
    f = opt.find(lambda p: isinstance(p, L.Filter))
    assert f.find(lambda p: isinstance(p, L.Window)) is not None      # Window below the filter
    win = opt.find(lambda p: isinstance(p, L.Window))
    assert win.find(lambda p: isinstance(p, L.Filter)) is None        # and none pushed below
    want = {i: v for i, v in py_window(t.to_pylist(), ["k"], [("id", True)], "row_number").items()
            if v <= 2 and t.column("k")[i].as_py() < 40}
    _same(_by_id(q, "rn"), want)


# ------------------------------------------------------------------------------------------------
# plan cache
# ------------------------------------------------------------------------------------------------
def test_plan_cache_fingerprints_keep_windows_apart(frame):
    _, df = frame

    def fp(q, native):
        ctx = PC._Ctx()
        return PC.fingerprint(q.plan, ctx, native=native)

    def queries():
        k, d = Window.partitionBy("k"), col("d")
        return [df.select("id", rank().over(k.orderBy(d)).alias("v")),
                df.select("id", dense_rank().over(k.orderBy(d)).alias("v")),
                df.select("id", row_number().over(k.orderBy(d)).alias("v")),
                df.select("id", rank().over(k.orderBy(d.desc())).alias("v")),
                df.select("id", rank().over(k.orderBy(d.asc())).alias("v")),
                df.select("id", rank().over(Window.partitionBy("i").orderBy(d)).alias("v")),
                df.select("id", rank().over(Window.orderBy(d)).alias("v")),
                df.select("id", rank().over(Window.partitionBy("k", "d").orderBy(d)).alias("v")),
                df.select("id", sum_("x").over(k.orderBy(d)).alias("v")),
                df.select("id", sum_("x").over(k).alias("v")),
                df.select("id", max_("x").over(k).alias("v"))]
    walks = [False] + ([True] if PC._NATIVE_FP is not None else [])
    for native in walks:
        fps = [fp(q, native) for q in queries()]
        # ASC spelled out is the default: entries 0 and 4 are one shape, all others differ
        assert fps[0] == fps[4]
        rest = fps[:4] + fps[5:]
        assert len(set(rest)) == len(rest)
        assert fps == [fp(q, native) for q in queries()]       # and stable across builds
    if PC._NATIVE_FP is not None:
        for q in queries():
            assert fp(q, True) == fp(q, False)


def test_plan_cache_serves_each_function_its_own_plan(indexed):
    s, df, t = indexed
    pc = PC.plan_cache(s)
    w = Window.partitionBy("k").orderBy("d")
    rows = lambda lo: [r for r in t.to_pylist() if r["k"] >= lo]      # noqa: E731
    q = lambda fn, lo, ww=w: df.filter(col("k") >= lo).select(       # noqa: E731
        "id", fn().over(ww).alias("v"))
    _same(_by_id(q(rank, 20), "v"), py_window(rows(20), ["k"], [("d", True)], "rank"))
    _same(_by_id(q(dense_rank, 20), "v"), py_window(rows(20), ["k"], [("d", True)], "dense_rank"))
    wd = Window.partitionBy("k").orderBy(col("d").desc())
    _same(_by_id(q(rank, 20, wd), "v"), py_window(rows(20), ["k"], [("d", False)], "rank"))
    hits = pc.hits
    _same(_by_id(q(rank, 90), "v"), py_window(rows(90), ["k"], [("d", True)], "rank"))
    assert pc.hits > hits                                      # same shape, new literal


# ------------------------------------------------------------------------------------------------
# host results against the Python loop
# ------------------------------------------------------------------------------------------------
ORDERS = [[("d", True)], [("d", False)], [("d", True), ("i", False)], [("s", False)],
          [("x", True)]]


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "-".join(
    f"{c}{'' if a else '_desc'}" for c, a in o))
def test_ranking_and_running_aggregates_with_ties_and_null_keys(frame, order):
    _, df = frame
    rows = _table().to_pylist()
    w = Window.partitionBy("k").orderBy(*[col(c) if a else col(c).desc() for c, a in order])
    q = df.select("id", rank().over(w).alias("rank"), dense_rank().over(w).alias("dense_rank"),
                  row_number().over(w).alias("row_number"),
                  sum_("x").over(w).alias("sum_x"), sum_("i").over(w).alias("sum_i"),
                  count("x").over(w).alias("count_x"), count("*").over(w).alias("count_None"),
                  min_("x").over(w).alias("min_x"), max_("i").over(w).alias("max_i"),
                  avg("x").over(w).alias("avg_x"), max_("s").over(w).alias("max_s"),
                  min_("s").over(w).alias("min_s"))
    t = q.to_arrow()
    got = {n: dict(zip(t.column("id").to_pylist(), t.column(n).to_pylist()))
           for n in t.column_names if n != "id"}
    for name in got:
        if name == "row_number":
            continue
        fn, _, arg = name.partition("_") if not name.endswith("rank") else (name, "", None)
        arg = None if arg in ("None", "") else arg
        _same(got[name], py_window(rows, ["k"], order, fn, arg))
    # row_number: a permutation of the peer group's positions (ties in any order)
    rk = py_window(rows, ["k"], order, "rank")
    peers = {}
    for r in rows:
        peers.setdefault((r["k"], rk[r["id"]]), []).append(got["row_number"][r["id"]])
    for (_, first), nums in peers.items():
        assert sorted(nums) == list(range(first, first + len(nums)))
    # the partition whose x is all NULL: NULL sums, zero counts
    for r in rows:
        if r["k"] == 2:
            assert got["sum_x"][r["id"]] is None and got["count_x"][r["id"]] == 0
            assert got["min_x"][r["id"]] is None and got["avg_x"][r["id"]] is None


def test_whole_partition_frame_and_null_partition_keys(frame):
    _, df = frame
    rows = _table().to_pylist()
    w = Window.partitionBy("k")
    q = df.select("id", sum_("x").over(w).alias("sx"), count("*").over(w).alias("n"),
                  max_("i").over(w).alias("mi"), avg("i").over(w).alias("ai"))
    _same(_by_id(q, "sx"), py_window(rows, ["k"], [], "sum", "x"))
    _same(_by_id(q, "n"), py_window(rows, ["k"], [], "count"))
    _same(_by_id(q, "mi"), py_window(rows, ["k"], [], "max", "i"))
    _same(_by_id(q, "ai"), py_window(rows, ["k"], [], "avg", "i"))
    n = _by_id(q, "n")
    assert n[9] == n[10] == 2                      # the two NULL keys form one partition
    # two partition keys, one of them a nullable string; and no partition key at all
    q = df.select("id", count("*").over(Window.partitionBy("s", "k")).alias("n"),
                  sum_("i").over(Window.orderBy("d", "id")).alias("run"))
    _same(_by_id(q, "n"), py_window(rows, ["s", "k"], [], "count"))
    _same(_by_id(q, "run"), py_window(rows, [], [("d", True), ("id", True)], "sum", "i"))


@pytest.mark.parametrize("partitions", ["5", "8", "200"])
def test_float_keys_compare_like_spark(session, tmp_path, partitions):
    """Both zeros, both NaN payloads and both NULLs are one partition each whatever the shuffle
    width: the exchange hashes normalised floats (at 8 and 200 partitions the raw bits of 0.0
    and -0.0 hash to different partitions).  As order keys NaN is the greatest value."""
    from hyperspace_amd.utils import murmur3
    zeros = pa.array([0.0, -0.0])
    assert len(set(murmur3.bucket_ids([zeros], 8))) == 2
    assert len(set(murmur3.bucket_ids([zeros], 200))) == 2
    session.conf.set("spark.sql.shuffle.partitions", partitions)
    nan2 = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
    t = pa.table({"id": pa.array(range(8), pa.int64()),
                  "f": pa.array([0.0, -0.0, float("nan"), nan2, 1.5, 1.5, None, None]),
                  "g": pa.array([-0.0, 0.0, 1.5, nan2, float("nan"), 0.0, None, 1.5],
                                pa.float32())})
    (tmp_path / "f").mkdir()
    pq.write_table(t, tmp_path / "f" / "p0.parquet")
    df = session.read.parquet(str(tmp_path / "f"))
    q = df.select("id", count("*").over(Window.partitionBy("f")).alias("n"),
                  count("*").over(Window.partitionBy("g")).alias("ng"),
                  count("*").over(Window.partitionBy("f", "id")).alias("n1"),
                  dense_rank().over(Window.orderBy("f")).alias("dr"),
                  rank().over(Window.orderBy(col("f").desc())).alias("rd"))
    plan = q.queryExecution.executed_plan.tree_string()
    assert "hashpartitioning(knownfloatingpointnormalized(normalizenanandzero(f#" in plan
    assert _by_id(q, "n") == {i: 2 for i in range(8)}
    assert _by_id(q, "ng") == {0: 3, 1: 3, 5: 3, 2: 2, 7: 2, 3: 2, 4: 2, 6: 1}
    assert _by_id(q, "n1") == {i: 1 for i in range(8)}
    # ASC: NULL, 0.0 = -0.0, 1.5, NaN; DESC: NaN, 1.5, zeros, NULL
    assert _by_id(q, "dr") == {6: 1, 7: 1, 0: 2, 1: 2, 4: 3, 5: 3, 2: 4, 3: 4}
    assert _by_id(q, "rd") == {2: 1, 3: 1, 4: 3, 5: 3, 0: 5, 1: 5, 6: 7, 7: 7}


def test_over_an_empty_specification(frame):
    """``fn(...) OVER ()``: one partition, the whole input as the frame, no sort planned."""
    s, df = frame
    df.createOrReplaceTempView("t")
    rows = _table().to_pylist()
    xs = [r["x"] for r in rows if r["x"] is not None]
    for q in (s.sql("SELECT id, count(*) OVER () AS n, sum(x) OVER () AS sx, max(i) OVER () mi "
                    "FROM t"),
              df.select("id", count("*").over(Window.partitionBy()).alias("n"),
                        sum_("x").over(Window.partitionBy()).alias("sx"),
                        max_("i").over(Window).alias("mi"))):
        plan = q.queryExecution.executed_plan
        ops = _ops(plan)
        assert ops.count("WindowExec") == 1 and "SortExec" not in ops
        win = plan.collect(lambda p: isinstance(p, X.WindowExec))[0]
        assert isinstance(win.child, X.ShuffleExchangeExec)
        assert isinstance(win.child.partitioning, X.SinglePartition)
        got = q.to_arrow().to_pylist()
        assert sorted(r["id"] for r in got) == list(range(len(rows)))
        assert {r["n"] for r in got} == {len(rows)}
        assert {r["mi"] for r in got} == {50}
        assert all(r["sx"] == pytest.approx(sum(xs)) for r in got)
    # over no rows, and an aggregate of the result
    assert df.filter(col("id") > 1000).select(count("*").over(Window.partitionBy())).count() == 0
    q = df.select(count("*").over(Window.partitionBy()).alias("n")).agg(sum_("n").alias("t"))
    assert q.collect()[0][0] == len(rows) ** 2


def test_empty_input(frame):
    _, df = frame
    w = Window.partitionBy("k").orderBy("d")
    q = df.filter(col("id") > 1000).select("id", rank().over(w).alias("r"),
                                           sum_("x").over(w).alias("sx"))
    t = q.to_arrow()
    assert t.num_rows == 0 and t.column_names == ["id", "r", "sx"]
    assert t.schema.field("r").type == pa.int32() and t.schema.field("sx").type == pa.float64()


def test_top_n_per_key_through_a_subquery(frame):
    s, df = frame
    df.createOrReplaceTempView("t")
    q = s.sql("SELECT id, k, rn FROM (SELECT id, k, row_number() OVER "
              "(PARTITION BY k ORDER BY x DESC, id) AS rn FROM t) r WHERE rn <= 2 ORDER BY k, rn")
    rows = _table().to_pylist()
    rn = py_window(rows, ["k"], [("x", False), ("id", True)], "row_number")
    want = sorted(((r["k"], rn[r["id"]], r["id"]) for r in rows if rn[r["id"]] <= 2),
                  key=lambda v: (v[0] is not None, v[0] or 0, v[1]))
    assert [(r["k"], r["rn"], r["id"]) for r in q.collect()] == want
    # the same through the DataFrame API, then aggregated
    w = Window.partitionBy("k").orderBy(col("x").desc(), col("id"))
    top = df.withColumn("rn", row_number().over(w)).filter(col("rn") <= 2)
    agg = top.groupBy("k").agg(count("*").alias("n"), sum_("x").alias("sx"))
    got = {r["k"]: (r["n"], r["sx"]) for r in agg.collect()}
    exp = {}
    for r in rows:
        if rn[r["id"]] <= 2:
            e = exp.setdefault(r["k"], [0, None])
            e[0] += 1
            if r["x"] is not None:
                e[1] = (e[1] or 0.0) + r["x"]
    assert got == {k: tuple(v) for k, v in exp.items()}
