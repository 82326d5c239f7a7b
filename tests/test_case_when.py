"""CASE WHEN without a GPU: the expression, the ``when`` / ``otherwise`` API, the SQL and
expression grammar (searched and simple CASE, IF, coalesce, nullif), type resolution, the plan
cache fingerprint, the optimizer, the host engine against the row-by-row reference of
tests/case_ref.py, the lowering of conditional aggregates onto guards, and the generated guarded
kernels compiled for gfx950."""
import datetime
import hashlib
import math
import os
import types

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import case_ref as CR
from hyperspace_amd import HyperspaceException, Session, avg, col, count, sum_, when
from hyperspace_amd.exec import compile as CP
from hyperspace_amd.ops import _lib as NL
from hyperspace_amd.plan import expressions as E
from hyperspace_amd.plan.parser import parse_expression as P

from test_jit import _agg, _fake, _scan_params, rt  # noqa: F401  (rt: the runtime fixture)

GG = CP.GUARD_GROUP


# -- parser and API ---------------------------------------------------------------------------------
def test_searched_simple_if_coalesce_nullif_desugar():
    e = P("CASE WHEN a > 1 THEN 1 WHEN b THEN 2 ELSE 0 END")
    assert isinstance(e, E.CaseWhen) and len(e.branches) == 2 and e.else_value.value == 0
    assert e.sql() == "CASE WHEN ('a > 1) THEN 1 WHEN ('b) THEN 2 ELSE 0 END"
    s = P("case x when 1 then 'one' when 2 then 'two' end")
    assert [c.sql() for c, _ in s.branches] == ["('x = 1)", "('x = 2)"] and s.else_value is None
    i = P("if(a > 1, b, 2.5)")
    assert i.semantic_equals(P("CASE WHEN a > 1 THEN b ELSE 2.5 END"))
    c = P("coalesce(a, b, 0)")
    assert c.semantic_equals(P("CASE WHEN a IS NOT NULL THEN a WHEN b IS NOT NULL THEN b ELSE 0 END"))
    assert P("coalesce(a)").sql() == "'a"
    n = P("nullif(a, 0)")
    assert n.semantic_equals(P("CASE WHEN a = 0 THEN NULL ELSE a END"))
    # nested, inside arithmetic and a function
    assert isinstance(P("sum(2 * CASE WHEN a THEN CASE WHEN b THEN 1 END ELSE 0 END)"), E.Sum)
    # every literal is an ordinary Literal child
    assert sum(isinstance(x, E.Literal) for x in e.iter_tree()) == 4
    for bad in ("CASE WHEN a THEN 1", "CASE WHEN a 1 END", "if(a, 1)", "nullif(a)"):
        with pytest.raises(SyntaxError):
            P(bad)


def test_case_words_are_not_reserved():
    e = P("end > 1 AND when < 2 AND then = 3 AND else = 4")
    assert {a.name for a in e.iter_tree() if isinstance(a, E.UnresolvedAttribute)} == \
        {"end", "when", "then", "else"}
    assert P("case > 1").sql() == "('case > 1)"
    x = P("CASE WHEN end > 1 THEN when ELSE else END")
    assert isinstance(x, E.CaseWhen) and x.else_value.name == "else" and \
        x.branches[0][1].name == "when"


def test_when_otherwise_api_round_trips_with_sql(tmp_path):
    s, df = _session(tmp_path)
    a = df.select(when(col("i") > 1, col("d")).when(col("i").isNull(), 0).otherwise(-1).alias("v"))
    df.createOrReplaceTempView("t")
    b = s.sql("SELECT CASE WHEN i > 1 THEN d WHEN i IS NULL THEN 0 ELSE -1 END v FROM t")
    ea, eb = a.plan.project_list[0].child, b.plan.project_list[0].child
    assert isinstance(ea, E.CaseWhen) and ea.semantic_equals(eb)
    assert a.collect() == b.collect()
    with pytest.raises(HyperspaceException, match="otherwise"):
        col("i").otherwise(1)
    with pytest.raises(HyperspaceException, match="once"):
        when(col("i") > 1, 1).otherwise(2).otherwise(3)
    with pytest.raises(HyperspaceException, match="when"):
        when(col("i") > 1, 1).otherwise(2).when(col("i") > 2, 3)
    assert "CASE WHEN" in a.queryExecution.executed_plan.tree_string()


# -- types ----------------------------------------------------------------------------------------------
def _attrs():
    return {n: E.Attribute(n, t) for n, t in (
        ("i8", pa.int8()), ("i32", pa.int32()), ("i64", pa.int64()), ("f", pa.float64()),
        ("dec", pa.decimal128(12, 2)), ("s", pa.string()), ("d", pa.date32()),
        ("b", pa.bool_()), ("ds", pa.dictionary(pa.int32(), pa.string())))}


def test_result_type_nullable_and_errors():
    A = _attrs()
    c = E.IsNotNull(A["i32"])

    def case(*vals, else_=None):
        return E.CaseWhen([(c, v) for v in vals], else_)
    assert case(A["i8"], A["i64"]).data_type == pa.int64()
    assert case(A["i8"], else_=E.Literal(1)).data_type == pa.int32()
    assert case(A["i32"], else_=E.Literal(0.5)).data_type == pa.float64()
    assert case(A["dec"], else_=E.Literal(0)).data_type == pa.float64()
    assert case(A["s"], A["ds"]).data_type == pa.string()
    assert case(A["d"], else_=E.Literal(datetime.date(2000, 1, 1))).data_type == pa.date32()
    assert case(A["b"], else_=E.Literal(False)).data_type == pa.bool_()
    assert case(E.Literal(None), else_=A["f"]).data_type == pa.float64()
    for x, y in (("s", "i32"), ("d", "i32"), ("b", "f"), ("d", "s")):
        with pytest.raises(HyperspaceException) as ei:
            case(A[x], else_=A[y])
        assert str(_plain(A[x])) in str(ei.value) and str(_plain(A[y])) in str(ei.value)
    with pytest.raises(HyperspaceException, match="boolean"):
        E.CaseWhen([(A["i32"], E.Literal(1))])
    nn = E.Attribute("nn", pa.int32(), nullable=False)
    assert case(nn).nullable                                   # no ELSE
    assert not case(nn, else_=E.Literal(0)).nullable
    assert case(nn, else_=A["i32"]).nullable and case(A["i32"], else_=E.Literal(0)).nullable
    assert case(nn, else_=E.Literal(None)).nullable
    e = case(nn, else_=E.Literal(0))
    assert e.sql() == f"CASE WHEN (isnotnull({A['i32'].sql()})) THEN {nn.sql()} ELSE 0 END"
    assert [a.name for a in e.references()] == ["i32", "nn"]
    assert e.with_children(e.children).semantic_equals(e)
    assert not e.semantic_equals(case(nn))


def _plain(a):
    return a.dtype


def test_plan_cache_fingerprint_parameterises_case_literals(tmp_path):
    from hyperspace_amd.plan.plan_cache import _Ctx, fingerprint
    s, df = _session(tmp_path)

    def fp(q):
        ctx = _Ctx()
        return fingerprint(q.plan, ctx, native=False), [x.value for x in ctx.lits]
    q1 = df.agg(sum_(when(col("i") > 1, col("d")).otherwise(0.0)).alias("x"))
    q2 = df.agg(sum_(when(col("i") > 7, col("d")).otherwise(2.5)).alias("x"))
    q3 = df.agg(sum_(when(col("i") > 1, col("d"))).alias("x"))
    q4 = df.agg(sum_(when(col("i") > 1, col("d")).when(col("i") > 0, 1.0).otherwise(0.0)).alias("x"))
    (f1, l1), (f2, l2), (f3, _), (f4, _) = fp(q1), fp(q2), fp(q3), fp(q4)
    assert f1 == f2 and l1 == [1, 0.0] and l2 == [7, 2.5]
    assert len({f1, f3, f4}) == 3


def test_optimizer_infers_no_isnotnull_through_a_case(tmp_path):
    s, df = _session(tmp_path)
    q = df.filter(P("coalesce(i, 0) < 3 AND d > 1.0"))
    conds = E.split_conjuncts(q.queryExecution.optimized_plan.condition)
    inferred = [c.child.name for c in conds if isinstance(c, E.IsNotNull)]
    assert inferred == ["d"]          # not i: coalesce(i, 0) < 3 is true for a NULL i
    assert sorted(r[0] is None for r in q.select("i").collect()).count(True) >= 1
    with pytest.raises(HyperspaceException):
        df.filter("CASE WHEN row_number() OVER (ORDER BY i) > 1 THEN true ELSE false END")


# -- host engine ----------------------------------------------------------------------------------------
NAN = float("nan")
ROWS = {
    "i": [1, 2, None, 4, 5, None, 7, 8],
    "d": [1.5, None, NAN, -0.0, 2.25, 3.0, None, 100.0],
    "k": [10, 20, 30, None, 50, 60, 70, 80],
    "s": ["x", "y", None, "x", "z", "y", "x", None],
    "dt": [datetime.date(1995, 1, d) if d else None for d in (1, 2, 3, None, 5, 6, 7, 8)],
    "b": [True, False, None, True, False, True, None, False],
}


def _session(tmp_path):
    t = pa.table({"i": pa.array(ROWS["i"], pa.int32()), "d": pa.array(ROWS["d"], pa.float64()),
                  "k": pa.array(ROWS["k"], pa.int64()), "s": pa.array(ROWS["s"]),
                  "dt": pa.array(ROWS["dt"], pa.date32()), "b": pa.array(ROWS["b"])})
    os.makedirs(tmp_path / "t", exist_ok=True)
    pq.write_table(t, tmp_path / "t" / "p.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.mi.execution.device": "cpu"},
                warehouse_dir=str(tmp_path / "wh"))
    return s, s.read.parquet(str(tmp_path / "t"))


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return (a != a and b != b) or (a == b and math.copysign(1, a) == math.copysign(1, b)) or \
            abs(a - b) <= 1e-12 * abs(b)
    return a == b and type(a) is type(b)


def _gt(x, y):
    return None if x is None or y is None else x > y


def _rows():
    n = len(ROWS["i"])
    return [{k: v[r] for k, v in ROWS.items()} for r in range(n)]


# (SQL text of a CASE, its value for one row as a Python function)
CASES = [
    ("CASE WHEN i > 2 THEN d ELSE 0 END",
     lambda r: CR.case_value([(_gt(r["i"], 2), r["d"])], 0.0)),
    ("CASE WHEN i > 2 THEN d END", lambda r: CR.case_value([(_gt(r["i"], 2), r["d"])])),
    ("CASE WHEN i > 4 THEN k WHEN i > 1 THEN i ELSE -1 END",
     lambda r: CR.case_value([(_gt(r["i"], 4), r["k"]), (_gt(r["i"], 1), r["i"])], -1)),
    ("CASE WHEN b THEN i ELSE d END",
     lambda r: CR.case_value([(r["b"], None if r["i"] is None else float(r["i"]))], r["d"])),
    ("CASE s WHEN 'x' THEN 'ex' WHEN 'y' THEN s ELSE 'other' END",
     lambda r: CR.case_value([(None if r["s"] is None else r["s"] == "x", "ex"),
                              (None if r["s"] is None else r["s"] == "y", r["s"])], "other")),
    ("CASE WHEN i > 2 THEN dt END", lambda r: CR.case_value([(_gt(r["i"], 2), r["dt"])])),
    ("CASE WHEN d > 2 THEN b ELSE false END",
     lambda r: CR.case_value([(_gt(r["d"], 2), r["b"])], False)),
    ("if(i > 100, 1, 0)", lambda r: CR.case_value([(_gt(r["i"], 100), 1)], 0)),       # all false
    ("coalesce(i, k, 0)", lambda r: r["i"] if r["i"] is not None else
     (r["k"] if r["k"] is not None else 0)),
    ("nullif(i, 4)", lambda r: None if r["i"] == 4 else r["i"]),
]


@pytest.mark.parametrize("text,fn", CASES, ids=[c[0][:28] for c in CASES])
def test_host_engine_matches_row_by_row_reference(tmp_path, text, fn):
    s, df = _session(tmp_path)
    df.createOrReplaceTempView("t")
    got = [r[0] for r in s.sql(f"SELECT {text} v FROM t").collect()]
    want = [fn(r) for r in _rows()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, int) and not isinstance(w, bool) and isinstance(g, int):
            assert g == w
        else:
            assert (g is None and w is None) or _same(g, w), (text, got, want)
    # an empty input gives no rows; a filter that keeps nothing gives empty aggregates
    assert s.sql(f"SELECT {text} v FROM t WHERE k > 1000").collect() == []


AGG_CASES = [CASES[i] for i in (0, 1, 2, 7, 8, 9)]        # the numeric ones


@pytest.mark.parametrize("text,fn", AGG_CASES, ids=[c[0][:28] for c in AGG_CASES])
def test_host_aggregates_over_case(tmp_path, text, fn):
    """sum / count / min / max / avg over a CASE, with and without ELSE, an all-false guard and an
    empty input; NaN in the values stays out of min / max (their order of NaN is the engine's)."""
    s, df = _session(tmp_path)
    df.createOrReplaceTempView("t")
    for where, keep in (("", lambda r: True), (" WHERE k > 1000", lambda r: False),
                        (" WHERE k < 45", lambda r: r["k"] is not None and r["k"] < 45)):
        vals = [fn(r) for r in _rows() if keep(r)]
        row = s.sql(f"SELECT sum({text}) a, count({text}) c, avg({text}) g, min({text}) mn, "
                    f"max({text}) mx FROM t{where}").collect()[0]
        assert row[1] == CR.aggregate("count", vals)
        for got, name in ((row[0], "sum"), (row[2], "avg")):
            want = CR.aggregate(name, vals)
            assert (got is None and want is None) or _same(float(got), float(want)), (text, where, name)
        clean = [v for v in vals if not (isinstance(v, float) and v != v)]
        if len(clean) == len(vals):
            for got, name in ((row[3], "min"), (row[4], "max")):
                want = CR.aggregate(name, vals)
                assert (got is None and want is None) or float(got) == float(want), (text, name)


def test_count_of_a_column_counts_its_non_null_rows(tmp_path):
    """``count(Column)`` is ``count(x)``, not ``count(*)``: a Column's ``== "*"`` builds an
    expression and must not be read as a truth value."""
    s, df = _session(tmp_path)
    nn = sum(v is not None for v in ROWS["i"])
    assert 0 < nn < len(ROWS["i"])
    row = df.agg(count(col("i")).alias("c"), count("i").alias("n"), count("*").alias("all"),
                 count().alias("dflt")).collect()[0]
    assert tuple(row) == (nn, nn, len(ROWS["i"]), len(ROWS["i"]))
    per = {r[0]: r[1] for r in df.groupBy("s").agg(count(col("d")).alias("c")).collect()}
    want = {}
    for r in _rows():
        want[r["s"]] = want.get(r["s"], 0) + (r["d"] is not None)
    assert per == want


def test_grouped_conditional_aggregates_on_the_host(tmp_path):
    s, df = _session(tmp_path)
    q = df.groupBy("s").agg(sum_(when(col("i") > 2, 1).otherwise(0)).alias("n"),
                            count(when(col("d") > 2, 1)).alias("c"),
                            avg(when(col("i") > 2, col("k")).otherwise(0)).alias("a"))
    got = {r[0]: tuple(r[1:]) for r in q.collect()}
    want = {}
    for key in {r["s"] for r in _rows()}:
        rs = [r for r in _rows() if r["s"] == key]
        want[key] = (CR.aggregate("sum", [CR.case_value([(_gt(r["i"], 2), 1)], 0) for r in rs]),
                     CR.aggregate("count", [CR.case_value([(_gt(r["d"], 2), 1)]) for r in rs]),
                     CR.aggregate("avg", [CR.case_value([(_gt(r["i"], 2), r["k"])], 0) for r in rs]))
    assert got.keys() == want.keys()
    for k in got:
        assert got[k][:2] == want[k][:2] and _same(float(got[k][2]), float(want[k][2])), k


# -- lowering -------------------------------------------------------------------------------------------
def test_which_aggregates_reach_the_guard_normal_form():
    A = _attrs()
    p = E.GreaterThan(A["i32"], E.Literal(3))
    one, zero, null = E.Literal(1), E.Literal(0), E.Literal(None)
    prod = E.Multiply(A["f"], E.Subtract(E.Literal(1), A["dec"]))

    def case(v, else_=None, cond=p):
        return E.CaseWhen([(cond, v)], else_)
    fused = [E.Sum(case(one, zero)), E.Count(case(one)), E.Avg(case(A["f"], zero)),
             E.Min(case(A["d"])), E.Max(case(prod, E.Literal(-1.5))), E.Sum(case(A["i64"], null)),
             E.Sum(case(prod, zero, E.Or(p, E.Like(A["ds"], "PROMO%")))),
             E.Sum(case(one, zero, E.In(A["ds"], [E.Literal("a"), E.Literal("b")]))),
             E.Count(case(A["i32"], zero))]
    for fn in fused:
        g = CP.guard_of(fn)
        assert g is not None, fn.sql()
    assert CP.guard_of(fused[5]).else_lit is None and CP.guard_of(fused[0]).else_lit.value == 0
    three = E.Multiply(E.Multiply(A["f"], A["f"]), A["f"])
    column = [E.Sum(E.CaseWhen([(p, one), (E.IsNull(A["f"]), zero)])),       # two branches
              E.Sum(case(one, A["i32"])),                                    # a non-literal ELSE
              E.Sum(E.Multiply(E.Literal(2), case(one, zero))),              # arithmetic around it
              E.Sum(case(three, zero)),                                      # too many terms
              E.Max(case(A["s"], E.Literal("z"))),                           # a string value
              E.Sum(case(one, zero, E.GreaterThan(E.Add(A["i32"], one), one))),   # computed guard
              E.Min(case(E.Multiply(E.Literal(-1), A["f"]))),
              E.Sum(case(case(one, zero), zero)), E.CountDistinct(case(one))]
    for fn in column:
        assert CP.guard_of(fn) is None, fn.sql()


def _infos():
    A = _attrs()
    infos = {A["i32"].expr_id: CP.ColumnInfo(0, NL.I32, pa.int32()),
             A["f"].expr_id: CP.ColumnInfo(1, NL.F64, pa.float64()),
             A["d"].expr_id: CP.ColumnInfo(2, NL.I32, pa.date32()),
             A["ds"].expr_id: CP.ColumnInfo(3, NL.I32, pa.string(), pa.array(["a", "b", "c"]))}
    return A, (lambda a: infos[a.expr_id])


def test_guard_preds_bind_behind_the_filter_and_rebind_like_a_fresh_bind():
    A, info = _infos()
    lf, lg, lh, lt, le = (E.Literal(v) for v in (5, 3, 0.25, 7.0, 1.5))
    conds = [E.GreaterThan(A["i32"], lf)]
    fns = [E.Sum(E.CaseWhen([(E.Or(E.LessThan(A["i32"], lg), E.GreaterThan(A["f"], lh)), lt)], le)),
           E.Count(None),
           E.Min(E.CaseWhen([(E.GreaterThanOrEqual(A["d"], E.Literal(datetime.date(1995, 1, 1))),
                              A["f"])]))]
    guards = [CP.guard_of(fn) if fn.child is not None else None for fn in fns]

    def fresh():
        b = CP.bind(CP.to_cnf(conds), info, None)
        return CP.bind_guards(b, guards, info, None)

    def key(b):
        return [(p.kind, p.op, p.col, p.group, p.ilit, p.flit) for p in b.preds]
    b0 = fresh()
    assert b0.nfilter == 1 and len(b0.filter_preds) == 1 and len(b0.preds) == 4
    assert b0.guards == [(1, 2, False), None, (3, 1, False)]
    assert [p.group for p in b0.preds] == [0, GG, GG, 3 * GG]
    assert b0.rebindable and len(b0.lits) == 4
    specs = [CP.guarded_agg_spec(fn, g, lambda a: info(a).slot, w) if g is not None else None
             for fn, g, w in zip(fns, guards, b0.guards)]
    assert CP.guard_fields(specs[0].pad) == (1, 2, True, False)
    assert specs[0].nterms == 0 and specs[0].alpha[0] == 7.0 and specs[0].alpha[2] == 1.5
    assert CP.guard_fields(specs[2].pad) == (3, 1, False, False) and specs[2].kind == NL.AK_MIN
    assert CP.guard_fields(NL.AggSpec().pad) is None
    # in a join the right side's list follows the left one's: the guard's place shifts
    assert CP.guard_fields(CP.guarded_agg_spec(fns[0], guards[0], lambda a: info(a).slot,
                                               b0.guards[0], 2).pad)[0] == 3
    lf.value, lg.value, lh.value = 9, 4, 0.5
    rb = CP.rebind(b0)
    assert rb is not None and key(rb) == key(fresh()) != key(b0)
    assert rb.nfilter == 1 and rb.guards == b0.guards
    # a guard that can never be true is flagged; the query is not empty
    never = CP.guard_of(E.Sum(E.CaseWhen([(E.EqualTo(A["ds"], E.Literal("nope")), lt)], le)))
    bn = CP.bind_guards(CP.bind(CP.to_cnf(conds), info, None), [never], info, None)
    assert bn.guards == [(1, 0, True)] and not bn.always_false and not bn.rebindable
    # too many predicates: the caller takes the column route
    many = [CP.guard_of(E.Sum(E.CaseWhen([(E.Or(E.Or(E.LessThan(A["i32"], E.Literal(i)),
                                                     E.GreaterThan(A["f"], E.Literal(0.5))),
                                                E.IsNull(A["f"])), lt)]))) for i in range(6)]
    with pytest.raises(CP.Unsupported):
        CP.bind_guards(CP.bind(CP.to_cnf(conds), info, None), many, info, None)


# -- generated sources ----------------------------------------------------------------------------------
def _pad(first, count, has_else=False, never=False):
    return CP.G_ON | (CP.G_ELSE if has_else else 0) | (CP.G_NEVER if never else 0) | \
        (first << 8) | (count << 16)


def _guarded(a, first, count, has_else=False, never=False):
    a.pad = _pad(first, count, has_else, never)
    return a


def _compile(jit, k, tmp_path):
    rc = jit.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                               str(tmp_path).encode())
    assert rc == 0, jit.runtime().hs_jit_last_error().decode()


def _scan_case(group_col=-1, ng=1):
    descs = {0: _fake(NL.I32), 1: _fake(NL.F64), 2: _fake(NL.F64, True), 3: _fake(NL.F64),
             4: _fake(NL.I32, True)}
    preds = [NL.Pred(NL.PK_FLT_LIT, NL.OP_GE, 1, 0, 0, 0, 0, 0.05, None),
             NL.Pred(NL.PK_INT_LIT, NL.OP_EQ, 4, 0, GG, 0, 7, 0.0, None),
             NL.Pred(NL.PK_IN_SET, NL.OP_EQ, 0, 0, GG, 3, 0, 0.0, 0x5000),
             NL.Pred(NL.PK_FLT_LIT, NL.OP_LT, 1, 0, 2 * GG, 0, 0, 0.07, None),
             NL.Pred(NL.PK_BITMAP, NL.OP_EQ, 0, 0, 3 * GG, 4, 0, 0.0, 0x6000)]
    p = _scan_params(descs, preds,
                     [_guarded(_agg(NL.AK_SUM, [(3, 0.0, 1.0), (1, 1.0, -1.0)]), 1, 2, True),
                      _guarded(_agg(NL.AK_COUNT, []), 3, 1),
                      _guarded(_agg(NL.AK_MIN, [(2, 0.0, 1.0)]), 3, 1),
                      _guarded(_agg(NL.AK_MAX, [(2, 0.0, 1.0)]), 4, 1, True),
                      _guarded(_agg(NL.AK_SUM, []), 0, 0, True, never=True),
                      _agg(NL.AK_SUM, [(3, 0.0, 1.0)]), _agg(NL.AK_COUNT_STAR)], group_col, ng)
    p.npreds = 1
    return p


def test_guarded_scan_sources_compile(rt, tmp_path):
    from hyperspace_amd.exec import hash_agg as H
    from hyperspace_amd.exec.encoding import Compact
    jit = rt
    comp = {0: Compact(None, 2, 0, None, NL.I32), 1: Compact(None, 1, 0, 100.0, NL.F64),
            3: Compact(None, 4, 0, 100.0, NL.F64), 4: Compact(None, 2, 5, None, NL.I32)}
    p = _scan_case()
    k = jit.gen_scan_agg(p)
    # the guard is a select on decoded values, its literals are arguments of their own
    assert "a.L1" in k.src and "a.F3" in k.src and "a.E0" in k.src and "a.A1_0" in k.src
    assert "a.L0" not in k.src and "pass0 = act0 && ((true && ((double)x1_0 >= a.F0)));" in k.src
    assert jit._agg_slots(jit.aggs_of(p)) == [3, 1, 4, 0, 2]
    # slot 1 is a SUM term and a guard column: it decodes exactly (no reciprocal)
    kc = jit.gen_scan_agg(p, comp)
    assert "a.R3" in kc.src and "a.R1" not in kc.src and "a.Q1" in kc.src
    for vec in (0, 8, 16):
        _compile(jit, jit.gen_scan_agg(p, None, vec), tmp_path)
    for vec in (0, 8):
        _compile(jit, jit.gen_scan_agg(p, comp, vec), tmp_path)
        assert jit.scan_pack_layout(p, comp, vec) is None        # the row-packed form declines
    g = _scan_case(0, 3)
    for vec in (0, 8):
        _compile(jit, jit.gen_scan_agg(g, None, vec), tmp_path)
        _compile(jit, jit.gen_scan_agg(g, comp, vec), tmp_path)

    def kcol(t):
        return types.SimpleNamespace(hs_type=t, valid=None, dictionary=None, offsets=None,
                                     atype=pa.int64())
    hk = H.plan_keys([(0, None, kcol(NL.I32), (-5, 100, None))],
                     (True, True, True, True, True, False, False), True)
    for vec in (0, 8):
        _compile(jit, jit.gen_scan_agg(p, None, vec, hk), tmp_path)
        _compile(jit, jit.gen_scan_agg(p, comp, vec, hk), tmp_path)
    # literals are arguments: the shape ignores them, the guards are part of it
    q = _scan_case()
    q.preds[1].ilit, q.aggs[0].alpha[2] = 99, 4.0
    assert jit.scan_agg_shape(q) == jit.scan_agg_shape(p)
    q.aggs[1].pad = 0
    assert jit.scan_agg_shape(q) != jit.scan_agg_shape(p)
    v = {}
    jit.fill_preds_aggs(v, [(0, p.preds[0])], jit.aggs_of(p))
    assert v["L1"] == 7 and v["F3"] == 0.07 and v["N2"] == 3 and "E0" in v and "A1_0" in v


def test_guarded_join_sources_compile_and_specialised_forms_decline(rt, tmp_path):
    from hyperspace_amd.exec import hash_agg as H, jit_runs
    from hyperspace_amd.exec.encoding import Compact
    jit = rt
    j = NL.JoinParams()
    j.cols[0], j.cols[1], j.cols[2] = _fake(NL.I64), _fake(NL.I32), _fake(NL.F64, True)
    j.cols[8], j.cols[9], j.cols[10] = _fake(NL.I64), _fake(NL.I32), _fake(NL.I32, True)
    j.preds[0] = NL.Pred(NL.PK_INT_LIT, NL.OP_GT, 1, 0, 0, 0, 9000, 0.0, None)
    j.preds[1] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 9, 0, 1000, 0, 9000, 0.0, None)
    j.preds[2] = NL.Pred(NL.PK_INT_LIT, NL.OP_EQ, 10, 0, GG, 0, 3, 0.0, None)       # right column
    j.preds[3] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 1, 0, 2 * GG, 0, 5, 0.0, None)    # left column
    j.nlp, j.npreds = 1, 2
    j.aggs[0] = _guarded(_agg(NL.AK_SUM, [(2, 0.0, 1.0), (2, 1.0, -1.0)]), 2, 1, True)
    j.aggs[1] = _guarded(_agg(NL.AK_SUM, []), 3, 1, True)
    j.aggs[2] = _agg(NL.AK_COUNT_STAR)
    j.naggs, j.lkey, j.rkey = 3, 0, 8
    for g, fl in ((-1, 0), (10, 0), (9, 0), (-1, 1)):
        j.group_col, j.num_groups, j.key_is_float = g, 3, fl
        ks = [jit.gen_join_agg(j), jit.gen_merge_join_agg(j)]
        if not fl:
            ks += [jit.gen_join_index_agg(j), jit.gen_join_index_agg(j, vec=8, jw=1, jlog=7),
                   jit.gen_join_index_agg(j, jw=2, jlog=8)]
        for k in ks:
            _compile(jit, k, tmp_path)
    j.group_col, j.key_is_float = -1, 0
    comp = {0: Compact(None, 4, 1 + (1 << 31), None, NL.I64, 1, 600_000_000),
            8: Compact(None, 4, 1 + (1 << 31), None, NL.I64, 1, 600_000_000),
            9: Compact(None, 2, 8000, None, NL.I32), 2: Compact(None, 4, 0, 100.0, NL.F64),
            10: Compact(None, 1, 0, None, NL.I32)}
    for k in (jit.gen_join_agg(j, comp), jit.gen_merge_join_agg(j, comp),
              jit.gen_join_index_agg(j, comp, vec=8, jw=1, jlog=7),
              jit.gen_join_index_agg(j, comp, vec=8, stage=True)):
        _compile(jit, k, tmp_path)

    def kcol(t):
        return types.SimpleNamespace(hs_type=t, valid=None, dictionary=None, offsets=None,
                                     atype=pa.int64())
    hk = H.plan_keys([(9, None, kcol(NL.I32), (8000, 2500, None))], (True, True, False), True)
    _compile(jit, jit.gen_merge_join_agg(j, comp, hk), tmp_path)
    # the run-keyed forms (two-phase: bit-parallel phase 2, 12-bit pack) decline; without the
    # guards the same parameters take them
    assert not jit_runs.applies(j) and jit._with_runs(j, comp) == (comp, None)
    assert jit.merge_join_shape(j, comp) != jit.merge_join_shape(_unguard(j), comp)
    assert jit_runs.applies(_unguard(j))


def _unguard(j):
    u = NL.JoinParams.from_buffer_copy(j)
    for i in range(u.naggs):
        u.aggs[i].pad = 0
    u.aggs[1].nterms, u.aggs[1].kind = 0, NL.AK_COUNT_STAR
    return u


def test_projection_kernel_with_a_nested_case_compiles(rt, tmp_path):
    import torch
    from hyperspace_amd.exec import project
    from hyperspace_amd.exec.device_table import DeviceColumn
    jit = rt
    a = E.Attribute("a", pa.int64())
    x = E.Attribute("x", pa.float64())
    d = E.Attribute("d", pa.date32())
    b = E.Attribute("b", pa.bool_())
    s = E.Attribute("s", pa.string())
    cols = {a.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int64),
                                    torch.ones(4, dtype=torch.uint8), pa.int64()),
            x.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.float64), None, pa.float64()),
            d.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int32),
                                    torch.ones(4, dtype=torch.uint8), pa.date32()),
            b.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.uint8), None, pa.bool_())}
    inner = E.CaseWhen([(E.LessThan(x, E.Literal(2.5)), a)], E.Literal(7))
    exprs = [E.CaseWhen([(E.GreaterThan(a, E.Literal(1)), x), (E.IsNull(a), inner)], E.Literal(None)),
             E.CaseWhen([(b, E.Add(a, E.Literal(1)))]),
             E.CaseWhen([(E.LessThan(d, E.Literal("1995-01-01")), d)],
                        E.Literal(datetime.date(1999, 1, 1))),
             E.CaseWhen([(E.IsNotNull(a), E.GreaterThan(x, E.Literal(0.0)))], b),
             E.GreaterThan(E.CaseWhen([(E.IsNotNull(a), a)], E.Literal(0)), E.Literal(1))]
    k, values, outs = project.build(exprs, cols, 4, torch.device("cpu"))
    assert [o.atype for o in outs] == [pa.float64(), pa.int64(), pa.date32(), pa.bool_(), pa.bool_()]
    assert " ? " in k.src and "if (" not in k.src.split("hs_jit_project")[1]     # selects only
    _compile(jit, k, tmp_path)
    exprs[0] = E.CaseWhen([(E.GreaterThan(a, E.Literal(9)), x), (E.IsNull(a), inner)], E.Literal(None))
    assert project.build(exprs, cols, 4, torch.device("cpu"))[0] is k
    with pytest.raises(CP.Unsupported, match="string-valued CASE"):
        project.build([E.CaseWhen([(b, E.Literal("x"))], E.Literal("y"))], cols, 4,
                      torch.device("cpu"))
    from hyperspace_amd.exec.gpu_common import _needs_eval
    assert _needs_eval(exprs[4]) and not _needs_eval(E.GreaterThan(a, E.Literal(1)))


def test_unguarded_shape_and_source_are_the_parents(rt):
    """The headline Q6 scan (no guard): its source is the committed AOT file byte for byte and
    its shape key holds the (kind, terms, columns) triples it always held."""
    from test_scan_pack import _q6_params
    jit = rt
    p, comp = _q6_params()
    assert not jit.has_guards(p)
    lay = jit.scan_pack_layout(p, comp, 8)
    on = jit.gen_scan_agg(p, comp, 8, None, lay)
    h = hashlib.sha1(on.src.encode()).hexdigest()[:16]
    with open(os.path.join(jit.AOT_DIR, f"hs_jit_scan_agg.{h}.hip")) as fh:
        assert on.src == fh.read()
    assert jit.scan_agg_shape(p, comp, 8)[3] == ((NL.AK_SUM, 2, (2, 0)), (NL.AK_COUNT_STAR, 0, ()))
    assert all(not hasattr(a, "guard") for a in jit.aggs_of(p))
    # the same scan with a guard on its sum: another shape, and no row-packed form
    p.preds[5] = NL.Pred(NL.PK_FLT_LIT, NL.OP_LT, 1, 0, GG, 0, 0, 10.0, None)
    p.aggs[0].pad = _pad(5, 1, True)
    assert jit.scan_pack_layout(p, comp, 8) is None
    assert len(jit.scan_agg_shape(p, comp, 8)[3][0]) == 4


def test_conf_switch_is_documented():
    from hyperspace_amd.index import constants as C
    from hyperspace_amd.utils.conf import HyperspaceConf
    assert C.COND_AGG_FUSED == "spark.hyperspace.mi.condAgg.fused"
    assert HyperspaceConf.cond_agg_fused({}) is True
    assert HyperspaceConf.cond_agg_fused({C.COND_AGG_FUSED: "false"}) is False
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "docs", "configuration.md")) as fh:
        assert C.COND_AGG_FUSED in fh.read()
