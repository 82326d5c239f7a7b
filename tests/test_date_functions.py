"""Date functions and INTERVAL arithmetic without a GPU: the grammar (functions, EXTRACT,
INTERVAL), folding at construction, typing, the host engine against tests/date_ref.py, the device
calendar arithmetic compiled by the host compiler and run over every day of the contract range,
the generated projection kernel compiled for gfx950, the year -> range optimizer rule over a
covering index, and the plan cache."""
import datetime
import os
import random
import shutil
import subprocess

import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import date_ref as R
import hyperspace_amd as H
from hyperspace_amd import Hyperspace, HyperspaceException, IndexConfig, col, count, sum_
from hyperspace_amd.exec import arrow_eval as AE
from hyperspace_amd.plan import expressions as E
from hyperspace_amd.plan.parser import parse_expression as P
from hyperspace_amd.plan.plan_cache import plan_cache

from test_jit import rt  # noqa: F401  (the runtime fixture)

DATE = datetime.date


# -- parser ---------------------------------------------------------------------------------------
def test_every_function_parses_to_its_node():
    for text, cls in (("year(d)", E.Year), ("quarter(d)", E.Quarter), ("month(d)", E.Month),
                      ("dayofmonth(d)", E.DayOfMonth), ("day(d)", E.DayOfMonth),
                      ("dayofyear(d)", E.DayOfYear), ("dayofweek(d)", E.DayOfWeek),
                      ("weekday(d)", E.WeekDay), ("weekofyear(d)", E.WeekOfYear),
                      ("date_add(d, 7)", E.DateAdd), ("date_sub(d, n)", E.DateSub),
                      ("datediff(a, b)", E.DateDiff), ("add_months(d, -1)", E.AddMonths),
                      ("last_day(d)", E.LastDay), ("trunc(d, 'MM')", E.TruncDate),
                      ("YEAR(d)", E.Year), ("Date_Add(d, 1)", E.DateAdd)):
        e = P(text)
        assert type(e) is cls, text
        assert all(isinstance(c, (E.UnresolvedAttribute, E.Literal)) for c in e.children)
    assert P("date_add(d, 30)").sql() == "date_add('d, 30)"
    assert P("trunc(d, 'MM')").fmt == "MM" and P("trunc(d, 'MM')").level == "month"
    assert P("datediff(a, b) > 30").left.sql() == "datediff('a, 'b)"
    assert isinstance(P("year(d) = 1994 AND month(d) = 12"), E.And)
    # literal arguments are ordinary Literal children
    assert [c.value for c in P("date_add(d, 30)").children[1:]] == [30]


def test_extract():
    for field, cls in (("YEAR", E.Year), ("quarter", E.Quarter), ("Month", E.Month),
                       ("WEEK", E.WeekOfYear), ("DAY", E.DayOfMonth), ("DOW", E.DayOfWeek),
                       ("DAYOFWEEK", E.DayOfWeek), ("DOY", E.DayOfYear)):
        e = P(f"extract({field} FROM o_orderdate)")
        assert type(e) is cls and e.children[0].name == "o_orderdate"
    assert isinstance(P("EXTRACT(year from d) + 1"), E.Add)
    with pytest.raises(SyntaxError, match="YEAR, QUARTER, MONTH, WEEK, DAY, DOW"):
        P("extract(epoch FROM d)")


def test_interval_forms_lower_to_date_add_and_add_months():
    def parts(text):
        e = P(text)
        return type(e), e.children[0].name, e.children[1].value
    assert parts("d + INTERVAL '90' DAY") == (E.DateAdd, "d", 90)
    assert parts("d - INTERVAL '90' DAY") == (E.DateAdd, "d", -90)
    assert parts("d + interval 3 days") == (E.DateAdd, "d", 3)
    assert parts("INTERVAL '1' MONTH + d") == (E.AddMonths, "d", 1)
    assert parts("d - INTERVAL 2 MONTHS") == (E.AddMonths, "d", -2)
    assert parts("d + INTERVAL '1' YEAR") == (E.AddMonths, "d", 12)
    assert parts("d - INTERVAL '2' YEARS") == (E.AddMonths, "d", -24)
    assert parts("d + INTERVAL -3 DAY") == (E.DateAdd, "d", -3)
    assert parts("d - INTERVAL '-3' MONTH") == (E.AddMonths, "d", 3)
    c = P("l_shipdate <= d - INTERVAL '1' DAY + INTERVAL '1' YEAR")
    assert isinstance(c, E.LessThanOrEqual) and isinstance(c.right, E.AddMonths) and \
        isinstance(c.right.children[0], E.DateAdd)
    assert not any(type(x).__name__ == "_Interval" for x in c.iter_tree())


def test_syntax_errors():
    with pytest.raises(SyntaxError, match="unknown function upper"):
        P("upper(s)")
    with pytest.raises(SyntaxError, match="unknown function date_format"):
        P("date_format(d, 'yyyy')")
    for bad in ("INTERVAL '1' DAY", "d * INTERVAL '1' DAY", "INTERVAL '1' DAY - d",
                "year(INTERVAL '1' DAY)", "INTERVAL '1' DAY + INTERVAL '1' DAY",
                "-INTERVAL '1' DAY + d", "d > INTERVAL 3 DAY", "x IN (INTERVAL 3 DAY)"):
        with pytest.raises(SyntaxError, match="INTERVAL is only accepted as an operand"):
            P(bad)
    for bad, msg in (("year()", r"year\(\) takes one argument"),
                     ("year(a, b)", r"year\(\) takes one argument"),
                     ("date_add(d)", r"date_add\(\) takes two arguments"),
                     ("datediff(a)", r"datediff\(\) takes two arguments"),
                     ("add_months(a, 1, 2)", r"add_months\(\) takes two arguments"),
                     ("last_day(a, 1)", r"last_day\(\) takes one argument"),
                     ("trunc(d)", r"trunc\(\) takes two arguments"),
                     ("trunc(d, fmt)", r"trunc\(\) takes a string literal")):
        with pytest.raises(SyntaxError, match=msg):
            P(bad)


def test_interval_year_from_extract_are_not_reserved():
    e = P("interval > 1 AND year = 1994 AND from < 3 AND extract = 1 AND day + month > 2")
    assert {a.name for a in e.iter_tree() if isinstance(a, E.UnresolvedAttribute)} == \
        {"interval", "year", "from", "extract", "day", "month"}
    assert P("interval - 3").sql() == "('interval - 3)"
    assert P("interval + day").sql() == "('interval + 'day)"
    # ... also as the last token of an expression
    for text in ("interval", "x = interval", "a + interval", "sum(interval)", "extract",
                 "x < from", "a - interval", "interval + 1"):
        names = {a.name for a in P(text).iter_tree() if isinstance(a, E.UnresolvedAttribute)}
        assert names & {"interval", "extract", "from"}, text
    assert P("year(year)").children[0].name == "year"
    assert P("extract(year FROM from)").children[0].name == "from"


# -- folding --------------------------------------------------------------------------------------
def test_folding_happens_at_construction():
    e = P("DATE '1998-12-01' - INTERVAL '90' DAY")
    assert type(e) is E.Literal and e.value == DATE(1998, 9, 2) and e.data_type == pa.date32()
    y = P("year('1995-03-15')")
    assert type(y) is E.Literal and y.value == 1995 and y.data_type == pa.int32()
    c = P("l_shipdate <= DATE '1998-12-01' - INTERVAL '90' DAY")
    assert type(c.right) is E.Literal and c.right.value == DATE(1998, 9, 2)
    assert P("add_months('2001-01-31', 1)").value == DATE(2001, 2, 28)
    assert P("DATE '2000-02-29' + INTERVAL '1' YEAR").value == DATE(2001, 2, 28)
    assert P("trunc('2021-08-19', 'week')").value == DATE(2021, 8, 16)
    assert P("datediff('2000-03-01', DATE '2000-02-01')").value == 29
    assert P("dayofweek(TIMESTAMP '1970-01-01 23:59:59')").value == 5
    assert H.year(H.lit(DATE(2005, 1, 2))).expr.value == 2005
    assert H.weekofyear(H.lit(DATE(2005, 1, 2))).expr.value == 53
    # a column argument, or a NULL one, is not folded
    assert type(P("year(d)")) is E.Year and type(P("date_add(d, 1)")) is E.DateAdd
    assert type(P("date_add('2000-01-01', n)")) is E.DateAdd
    assert type(P("year(NULL)")) is E.Year
    # a string literal beside a column becomes a date literal, as in a comparison
    dd = E.date_function("datediff", E.Attribute("d", pa.date32()), E.Literal("1994-01-01"))
    assert type(dd) is E.DateDiff and dd.children[1].value == DATE(1994, 1, 1)


# -- typing ---------------------------------------------------------------------------------------
def _attrs():
    return {n: E.Attribute(n, t) for n, t in (
        ("d", pa.date32()), ("ts", pa.timestamp("us")), ("i8", pa.int8()), ("i32", pa.int32()),
        ("i64", pa.int64()), ("f", pa.float64()), ("s", pa.string()),
        ("ds", pa.dictionary(pa.int32(), pa.string())))}


def test_types_nullability_rendering_and_errors():
    A = _attrs()
    nn = E.Attribute("nn", pa.date32(), nullable=False)
    for name in ("year", "quarter", "month", "dayofmonth", "dayofyear", "dayofweek", "weekday",
                 "weekofyear"):
        e = E.date_function(name, A["d"])
        assert e.data_type == pa.int32() and e.nullable
        assert not E.date_function(name, nn).nullable
        assert e.sql() == f"{name}({A['d'].sql()})"
        assert E.date_function(name, A["ts"]).data_type == pa.int32()
    for name in ("date_add", "date_sub", "add_months"):
        e = E.date_function(name, nn, A["i8"])
        assert e.data_type == pa.date32() and e.nullable
        assert not E.date_function(name, nn, E.Literal(3)).nullable
        assert E.date_function(name, nn, E.Literal(None)).nullable
    assert E.date_function("date_add", A["d"], E.Literal(30)).sql() == \
        f"date_add({A['d'].sql()}, 30)"
    assert E.date_function("datediff", nn, A["d"]).data_type == pa.int32()
    assert E.date_function("last_day", nn).data_type == pa.date32()
    t = E.date_function("trunc", nn, "Mon")
    assert t.data_type == pa.date32() and not t.nullable and t.level == "month"
    assert E.date_function("trunc", nn, "day").nullable                 # unknown format: NULL
    assert not t.semantic_equals(E.date_function("trunc", nn, "year"))
    assert t.semantic_equals(E.date_function("trunc", nn, "MON"))
    assert t.with_children(t.children).semantic_equals(t)
    assert [a.name for a in E.date_function("datediff", nn, A["d"]).references()] == ["nn", "d"]
    # only children (and trunc's fmt): what the generic plan-cache walk relies on
    assert set(vars(E.date_function("date_add", nn, A["i8"]))) == {"children"}
    assert set(vars(t)) == {"children", "fmt"}
    for name, args, typ in (("year", (A["s"],), "string"), ("month", (A["ds"],), "dictionary"),
                            ("year", (A["f"],), "double"), ("last_day", (A["i32"],), "int32"),
                            ("date_add", (A["d"], A["f"]), "double"),
                            ("date_add", (A["d"], A["i64"]), "int64"),
                            ("add_months", (A["d"], A["s"]), "string"),
                            ("datediff", (A["d"], A["i32"]), "int32"),
                            ("trunc", (A["f"], "year"), "double")):
        with pytest.raises(HyperspaceException) as ei:
            E.date_function(name, *args)
        assert f"{name}()" in str(ei.value) and typ in str(ei.value)


def test_analysis_errors_surface_at_resolution(tmp_path):
    s, df = _session(tmp_path)
    with pytest.raises(HyperspaceException, match=r"year\(\).*string"):
        df.select(H.year("s"))
    with pytest.raises(HyperspaceException, match=r"year\(\).*double"):
        df.filter("year(v) = 1")
    assert df.select(H.year("d")).schema.field(0).type == pa.int32()


# -- host engine ----------------------------------------------------------------------------------
def _days(seed=11, n=2000, nulls=0.15):
    rng = random.Random(seed)
    days = R.EDGE + [rng.randint(R.MIN_DAY, R.MAX_DAY) for _ in range(n)]
    return [None if rng.random() < nulls else d for d in days], rng


def _eval(e, table):
    v = AE.eval_expr(e, table)
    v = v.combine_chunks() if isinstance(v, pa.ChunkedArray) else v
    assert v.type == e.data_type, (e.sql(), v.type)
    return (v.cast(pa.int32()) if pa.types.is_date32(v.type) else v).to_pylist()


def _date_col(days):
    return pa.array(days, pa.int32()).cast(pa.date32())


def test_host_engine_matches_reference_on_every_function():
    days, rng = _days()
    other = [None if rng.random() < 0.15 else rng.randint(R.MIN_DAY, R.MAX_DAY) for _ in days]
    raw = [None if rng.random() < 0.15 else rng.randint(-400, 400) for _ in days]
    nd = [None if d is None or n is None else R.clip_days(d, n) for d, n in zip(days, raw)]
    nm = [None if d is None or n is None else R.clip_months(d, n) for d, n in zip(days, raw)]
    nd = [n if d is not None else raw[i] for i, (d, n) in enumerate(zip(days, nd))]
    nm = [n if d is not None else raw[i] for i, (d, n) in enumerate(zip(days, nm))]
    d, d2 = E.Attribute("d", pa.date32()), E.Attribute("d2", pa.date32())
    kd, km = E.Attribute("kd", pa.int32()), E.Attribute("km", pa.int16())
    t = pa.table({AE.key(d): _date_col(days), AE.key(d2): _date_col(other),
                  AE.key(kd): pa.array(nd, pa.int32()), AE.key(km): pa.array(nm, pa.int16())})
    for name in ("year", "quarter", "month", "dayofmonth", "dayofyear", "dayofweek", "weekday",
                 "weekofyear", "last_day"):
        assert _eval(E.date_function(name, d), t) == R.lift(getattr(R, name))(days), name
    assert _eval(E.date_function("date_add", d, kd), t) == R.lift(R.date_add)(days, nd)
    neg = [None if n is None else -n for n in nd]
    t2 = t.set_column(2, AE.key(kd), pa.array(neg, pa.int32()))
    assert _eval(E.date_function("date_sub", d, kd), t2) == R.lift(R.date_sub)(days, neg)
    assert _eval(E.date_function("add_months", d, km), t) == R.lift(R.add_months)(days, nm)
    assert _eval(E.date_function("datediff", d, d2), t) == R.lift(R.datediff)(days, other)
    assert _eval(E.date_function("datediff", d2, d), t) == R.lift(R.datediff)(other, days)
    for fmt in ("year", "YYYY", "yy", "quarter", "Month", "MON", "mm", "week", "day", ""):
        got = _eval(E.date_function("trunc", d, fmt), t)
        assert got == R.lift(lambda x: R.trunc(x, fmt))(days), fmt
    # literal n: mid-range days so that every row stays in range
    mid = [x if x is None or R.MIN_DAY + 800 < x < R.MAX_DAY - 800 else 0 for x in days]
    t3 = t.set_column(0, AE.key(d), _date_col(mid))
    for n in (0, 1, -1, 365, -400):
        assert _eval(E.date_function("date_add", d, E.Literal(n)), t3) == \
            R.lift(lambda x: R.date_add(x, n))(mid)
        assert _eval(E.date_function("add_months", d, E.Literal(n % 25 - 12)), t3) == \
            R.lift(lambda x: R.add_months(x, n % 25 - 12))(mid)
    # a NULL literal, a string literal and a literal date beside a column
    assert _eval(E.date_function("date_add", d, E.Literal(None)), t) == [None] * len(days)
    assert _eval(E.date_function("datediff", d, E.Literal("2000-03-01")), t) == \
        R.lift(lambda x: x - R.day_of("2000-03-01"))(days)


def test_host_engine_takes_a_timestamp_as_its_utc_date():
    secs = [0, -1, 86399, 86400, -86400, -86401, None, 951782400 + 5]      # 2000-02-29 00:00:05
    for unit, mul in (("s", 1), ("ms", 10 ** 3), ("us", 10 ** 6), ("ns", 10 ** 9)):
        ts = E.Attribute("ts", pa.timestamp(unit))
        t = pa.table({AE.key(ts): pa.array([None if x is None else x * mul for x in secs],
                                           pa.timestamp(unit))})
        days = [None if x is None else x // 86400 for x in secs]
        assert _eval(E.date_function("dayofmonth", ts), t) == R.lift(R.dayofmonth)(days)
        assert _eval(E.date_function("last_day", ts), t) == R.lift(R.last_day)(days)
    tz = E.Attribute("tz", pa.timestamp("us", tz="Asia/Tokyo"))
    t = pa.table({AE.key(tz): pa.array([0, 86399 * 10 ** 6], pa.timestamp("us", tz="Asia/Tokyo"))})
    assert _eval(E.date_function("dayofmonth", tz), t) == [1, 1]            # the UTC date


# -- the device arithmetic, compiled by the host compiler -----------------------------------------
_MAIN = r"""
#include <cstdio>
int main(int argc, char** argv) {
  std::FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 2;
  for (int d = %d; d <= %d; ++d) {
    const int row[18] = {
        d, hs_year(d), hs_quarter(d), hs_month(d), hs_dayofmonth(d), hs_dayofyear(d),
        hs_dayofweek(d), (int)hs_weekday(d), hs_weekofyear(d), hs_last_day(d),
        hs_trunc_year(d), hs_trunc_quarter(d), hs_trunc_month(d), hs_trunc_week(d),
        hs_add_months(d, 1), hs_add_months(d, -1), hs_add_months(d, 13), hs_add_months(d, -13)};
    if (std::fwrite(row, sizeof(int), 18, f) != 18) return 4;
  }
  return std::fclose(f) == 0 ? 0 : 3;
}
"""


def test_device_calendar_arithmetic_on_every_day_of_the_range(tmp_path):
    """``project.DATE_PRELUDE`` is plain C++: with ``__device__`` defined away the host compiler
    builds it (with the undefined-behaviour sanitizer where it has one) into a program that
    writes every function for each of the 3 652 059 days of 0001-01-01 ... 9999-12-31; the
    file must equal ``date_ref``."""
    import numpy as np
    from hyperspace_amd.exec import project
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    src = tmp_path / "calendar.cpp"
    src.write_text("#define __device__\n" + project.DATE_PRELUDE + _MAIN % (R.MIN_DAY, R.MAX_DAY))
    exe = tmp_path / "calendar"
    base = [cxx, "-std=c++17", "-O1", "-o", str(exe), str(src)]
    san = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=all"],
                         capture_output=True, text=True)
    if san.returncode != 0:         # a compiler without the sanitizer: build plain
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
    out = tmp_path / "calendar.bin"
    run = subprocess.run([str(exe), str(out)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = np.fromfile(out, dtype=np.int32).reshape(-1, len(R.RANGE_COLUMNS))
    assert len(got) == R.MAX_DAY - R.MIN_DAY + 1 == 3652059
    want = R.range_columns()
    for j, name in enumerate(R.RANGE_COLUMNS):
        col_want = want[name]
        if name.startswith("add_months"):
            # a result outside the range is unspecified: not compared
            keep = np.array([x is not None for x in col_want])
            w = np.array([0 if x is None else x for x in col_want], dtype=np.int64)
            assert 0 < (~keep).sum() <= 13 * 31
        else:
            keep = np.ones(len(got), dtype=bool)
            w = np.array(col_want, dtype=np.int64)
        bad = np.nonzero((got[:, j] != w) & keep)[0]
        assert len(bad) == 0, (name, got[bad[0]].tolist(), int(w[bad[0]]))


# -- the generated kernel -------------------------------------------------------------------------
def _every_node(d, dn, n, ts=None):
    """One expression list that uses every new node over a nullable and a non-nullable date."""
    return [E.Year(d), E.Quarter(dn), E.Month(d), E.DayOfMonth(dn), E.DayOfYear(d),
            E.DayOfWeek(dn), E.WeekDay(d), E.WeekOfYear(dn),
            E.DateAdd(d, E.Literal(30)), E.DateSub(dn, n), E.DateDiff(d, dn),
            E.AddMonths(d, E.Literal(-13)), E.AddMonths(dn, n), E.LastDay(d),
            E.TruncDate(d, "year"), E.TruncDate(dn, "quarter"), E.TruncDate(d, "MM"),
            E.TruncDate(dn, "week"), E.TruncDate(d, "century"),
            E.LessThan(E.DateAdd(d, E.Literal(7)), E.Literal(DATE(1995, 1, 1))),
            E.GreaterThanOrEqual(E.LastDay(d), dn),
            E.And(E.EqualTo(E.Month(d), E.Literal(12)),
                  E.In(E.DayOfWeek(d), [E.Literal(1), E.Literal(7)])),
            E.CaseWhen([(E.EqualTo(E.Year(d), E.Literal(1995)), E.DateDiff(dn, d))],
                       E.Literal(0))]


def _cpu_cols(d, dn, n):
    import torch
    from hyperspace_amd.exec.device_table import DeviceColumn
    return {d.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int32),
                                    torch.ones(4, dtype=torch.uint8), pa.date32()),
            dn.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int32), None, pa.date32()),
            n.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int16), None, pa.int16())}


def test_date_kernel_compiles_for_gfx950(rt, tmp_path):
    import torch
    from hyperspace_amd.exec import project
    jit = rt
    d = E.Attribute("d", pa.date32())
    dn = E.Attribute("dn", pa.date32(), nullable=False)
    n = E.Attribute("n", pa.int16(), nullable=False)
    cols = _cpu_cols(d, dn, n)
    exprs = _every_node(d, dn, n)
    assert {type(x) for e in exprs for x in e.iter_tree() if isinstance(x, E.DateFunction)} == \
        set(E.DATE_FUNCTIONS.values())
    k, values, outs = project.build(exprs, cols, 4, torch.device("cpu"))
    assert [o.atype for o in outs] == [e.data_type for e in exprs]
    assert project.DATE_PRELUDE_MARK in k.src
    # all calendar arithmetic is 32-bit and divides by constants only
    prelude = project.DATE_PRELUDE
    assert "long" not in prelude and "threadIdx" not in prelude and "__builtin" not in prelude
    rc = jit.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                               str(tmp_path).encode())
    assert rc == 0, jit.runtime().hs_jit_last_error().decode()
    # literals (day counts, months, dates, IN entries) are arguments: other ones reuse the kernel
    other = _every_node(d, dn, n)
    other[8] = E.DateAdd(d, E.Literal(60))
    other[11] = E.AddMonths(d, E.Literal(5))
    other[19] = E.LessThan(E.DateAdd(d, E.Literal(9)), E.Literal(DATE(2001, 2, 3)))
    k2, values2, _ = project.build(other, cols, 4, torch.device("cpu"))
    assert k2 is k
    assert sorted(v for v in values2.values() if v in (60, 5, 9)) == [5, 9, 60]
    # the format and the function are part of the shape
    other[14] = E.TruncDate(d, "month")
    assert project.build(other, cols, 4, torch.device("cpu"))[0] is not k
    other = _every_node(d, dn, n)
    other[0] = E.Month(d)
    assert project.build(other, cols, 4, torch.device("cpu"))[0] is not k


def test_kernels_without_a_date_function_are_unchanged():
    """The prelude goes only into kernels that use it: a projection without a date function
    generates the source it always did (its cached code objects stay valid)."""
    import torch
    from hyperspace_amd.exec import jit as J
    from hyperspace_amd.exec import project
    from hyperspace_amd.exec.device_table import DeviceColumn
    a, b = E.Attribute("a", pa.int64()), E.Attribute("b", pa.int32())
    dt = E.Attribute("dt", pa.date32())
    cols = {a.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int64),
                                    torch.ones(4, dtype=torch.uint8), pa.int64()),
            b.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int32), None, pa.int32()),
            dt.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int32), None, pa.date32())}
    exprs = [E.Add(E.Multiply(a, E.Literal(3)), b),
             E.CaseWhen([(E.LessThan(dt, E.Literal("1995-01-01")), a)], E.Literal(0))]
    k, _, _ = project.build(exprs, cols, 4, torch.device("cpu"))
    assert project.DATE_PRELUDE_MARK not in k.src and "hs_civil" not in k.src
    assert k.src.startswith(J._PRELUDE + "struct Args")
    with_date = project.build(exprs + [E.Year(dt)], cols, 4, torch.device("cpu"))[0]
    assert with_date.src.startswith(J._PRELUDE + project.DATE_PRELUDE + "struct Args")


def test_timestamp_argument_is_unsupported_on_the_device():
    import torch
    from hyperspace_amd.exec import project
    from hyperspace_amd.exec.compile import Unsupported
    from hyperspace_amd.exec.device_table import DeviceColumn
    ts = E.Attribute("ts", pa.timestamp("us"))
    cols = {ts.expr_id: DeviceColumn(torch.zeros(4, dtype=torch.int64), None, pa.timestamp("us"))}
    with pytest.raises(Unsupported, match=r"timestamp argument of year\(\)"):
        project.build([E.Year(ts)], cols, 4, torch.device("cpu"))


def test_conjuncts_with_a_date_function_are_computed():
    from hyperspace_amd.exec.gpu_common import _needs_eval
    d = E.Attribute("d", pa.date32())
    assert _needs_eval(E.EqualTo(E.Month(d), E.Literal(12)))
    assert _needs_eval(E.In(E.DayOfWeek(d), [E.Literal(1), E.Literal(7)]))
    assert _needs_eval(E.LessThan(E.DateAdd(d, E.Literal(1)), E.Literal(DATE(1995, 1, 1))))
    assert not _needs_eval(E.LessThan(d, E.Literal(DATE(1995, 1, 1))))


# -- sessions -------------------------------------------------------------------------------------
def _table(seed=5, n=3000):
    rng = random.Random(seed)
    lo, hi = R.day_of("1992-01-01"), R.day_of("1998-12-31")
    # (the edge days that stay in range under the +-40 days / months of column n)
    days = [x for x in R.EDGE if R.MIN_DAY + 1500 < x < R.MAX_DAY - 1500] + \
        [rng.randint(lo, hi) for _ in range(n)]
    days = [None if rng.random() < 0.1 else x for x in days]
    return pa.table({"d": _date_col(days), "k": pa.array(range(len(days)), pa.int64()),
                     "v": pa.array([rng.random() for _ in days], pa.float64()),
                     "n": pa.array([rng.randint(-40, 40) for _ in days], pa.int32()),
                     "s": pa.array([f"s{x % 7}" for x in range(len(days))])})


def _session(tmp_path, session=None):
    t = _table()
    os.makedirs(tmp_path / "t", exist_ok=True)
    half = t.num_rows // 2
    pq.write_table(t.slice(0, half), tmp_path / "t" / "p0.parquet")
    pq.write_table(t.slice(half), tmp_path / "t" / "p1.parquet")
    s = session or H.Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                                   "spark.hyperspace.mi.execution.device": "cpu"},
                             warehouse_dir=str(tmp_path / "wh"))
    return s, s.read.parquet(str(tmp_path / "t"))


def _rows(df):
    return sorted((tuple(r) for r in df.collect()), key=repr)


def test_api_sql_and_expression_strings_agree(tmp_path):
    s, df = _session(tmp_path)
    df.createOrReplaceTempView("t")
    a = df.select(H.year("d").alias("y"), H.quarter(col("d")).alias("q"), H.month("d").alias("m"),
                  H.dayofmonth("d").alias("dd"), H.dayofyear("d").alias("dy"),
                  H.dayofweek("d").alias("dw"), H.weekofyear("d").alias("w"),
                  H.date_add("d", 30).alias("a"), H.date_sub("d", col("n")).alias("b"),
                  H.datediff("d", H.lit(DATE(1995, 1, 1))).alias("c"),
                  H.add_months("d", "n").alias("e"), H.last_day("d").alias("l"),
                  H.trunc("d", "week").alias("t"))
    b = s.sql("SELECT year(d) y, EXTRACT(QUARTER FROM d) q, extract(month from d) m, day(d) dd, "
              "dayofyear(d) dy, extract(dow from d) dw, extract(week from d) w, "
              "d + INTERVAL '30' DAY a, date_sub(d, n) b, datediff(d, DATE '1995-01-01') c, "
              "add_months(d, n) e, last_day(d) l, trunc(d, 'WEEK') t FROM t")
    assert _rows(a) == _rows(b)
    days = [None if x is None else R.to_day(x) for x in df.to_arrow().column("d").to_pylist()]
    got = {r.y for r in a.collect()}
    assert got == set(R.lift(R.year)(days))
    # an unaliased select item is named by its text
    assert s.sql("SELECT year(d), date_add(d, 30) FROM t").columns == \
        ["year(d)", "date_add(d, 30)"]
    # grouping and filtering through the grammar
    g = s.sql("SELECT extract(year FROM d) y, count(*) n FROM t WHERE month(d) = 12 AND "
              "dayofweek(d) IN (1, 7) GROUP BY extract(year FROM d)")
    want = {}
    for x in days:
        if x is not None and R.month(x) == 12 and R.dayofweek(x) in (1, 7):
            want[R.year(x)] = want.get(R.year(x), 0) + 1
    assert dict(_rows(g)) == want
    q1 = s.sql("SELECT count(*) n FROM t WHERE d <= DATE '1998-12-01' - INTERVAL '90' DAY")
    q2 = s.sql("SELECT count(*) n FROM t WHERE d <= DATE '1998-09-02'")
    assert q1.queryExecution.optimized_plan.tree_string() == \
        q2.queryExecution.optimized_plan.tree_string().replace(
            *[f"#{p.queryExecution.optimized_plan.output[0].expr_id}" for p in (q2, q1)])
    assert _rows(q1) == _rows(q2)


# -- the optimizer rule ---------------------------------------------------------------------------
@pytest.fixture
def indexed(session, tmp_path):
    s, df = _session(tmp_path, session)
    hs = Hyperspace(s)
    hs.createIndex(df, IndexConfig("li_ship", ["d"], ["v", "k"]))
    Hyperspace.enable(s)
    return s, df


def _filter_of(q):
    from hyperspace_amd.plan import logical as L
    f = q.queryExecution.optimized_plan.collect(lambda p: isinstance(p, L.Filter))
    assert len(f) == 1
    return f[0].condition


def test_year_equals_becomes_an_index_range(indexed):
    s, df = indexed
    q = df.filter(H.year(col("d")) == 1994).select("d", "v")
    cond = _filter_of(q)
    assert not E.contains_date_function(cond)
    conj = [c for c in E.split_conjuncts(cond) if not isinstance(c, E.IsNotNull)]
    assert [(type(c), c.left.name, c.right.value) for c in conj] == \
        [(E.GreaterThanOrEqual, "d", DATE(1994, 1, 1)), (E.LessThan, "d", DATE(1995, 1, 1))]
    assert "Name: li_ship" in q.queryExecution.executed_plan.tree_string()
    got = _rows(q)
    assert got and all(r[0].year == 1994 for r in got)
    s.disableHyperspace()
    assert _rows(df.filter(H.year(col("d")) == 1994).select("d", "v")) == got
    s.enableHyperspace()
    s.conf.set("spark.hyperspace.mi.datePartRange.enabled", "false")
    off = df.filter(H.year(col("d")) == 1994).select("d", "v")
    assert any(isinstance(x, E.Year) for x in _filter_of(off).iter_tree())
    assert _rows(off) == got
    s.conf.set("spark.hyperspace.mi.datePartRange.enabled", "true")
    # through an expression string and SQL too
    assert _rows(df.filter("year(d) = 1994").select("d", "v")) == got
    assert not E.contains_date_function(_filter_of(df.filter("1994 = year(d)")))


def test_rewritten_truth_tables_row_by_row(session):
    from hyperspace_amd.plan import logical as L
    from hyperspace_amd.plan.optimizer import date_part_range
    days = R.EDGE + [None, R.day_of("1993-12-31"), R.day_of("1994-01-01"),
                     R.day_of("1994-12-31"), R.day_of("1995-01-01"), None]
    d = E.Attribute("d", pa.date32())
    t = pa.table({AE.key(d): _date_col(days)})
    rel = L.LocalRelation(t, [d])
    ops = (E.EqualTo, E.LessThan, E.LessThanOrEqual, E.GreaterThan, E.GreaterThanOrEqual)
    cmp = {E.EqualTo: lambda a, b: a == b, E.LessThan: lambda a, b: a < b,
           E.LessThanOrEqual: lambda a, b: a <= b, E.GreaterThan: lambda a, b: a > b,
           E.GreaterThanOrEqual: lambda a, b: a >= b}

    def rewritten(cond):
        out = date_part_range(L.Filter(cond, rel)).condition
        assert not E.contains_date_function(out), cond.sql()
        return out

    def truth(e):
        return AE.eval_expr(e, t).to_pylist()
    for y in (1, 4, 1582, 1994, 2000, 2005, 9998):
        for op in ops:
            want = [None if x is None else cmp[op](R.year(x), y) for x in days]
            assert truth(rewritten(op(E.Year(d), E.Literal(y)))) == want, (op, y)
            flipped = [None if x is None else cmp[op](y, R.year(x)) for x in days]
            assert truth(rewritten(op(E.Literal(y), E.Year(d)))) == flipped, (op, y)
        neg = [None if x is None else R.year(x) != y for x in days]
        assert truth(rewritten(E.Not(E.EqualTo(E.Year(d), E.Literal(y))))) == neg
        either = [None if x is None else (R.year(x) == y or R.year(x) > 2004) for x in days]
        assert truth(rewritten(E.Or(E.EqualTo(E.Year(d), E.Literal(y)),
                                    E.GreaterThan(E.Year(d), E.Literal(2004))))) == either
    # left alone
    for cond in (E.EqualTo(E.Year(d), E.Literal(10000)), E.EqualTo(E.Year(d), E.Literal(9999)),
                 E.EqualTo(E.Year(d), E.Literal(0)), E.NotEqual(E.Year(d), E.Literal(1994)),
                 E.In(E.Year(d), [E.Literal(1994)]), E.EqualTo(E.Month(d), E.Literal(12)),
                 E.EqualTo(E.Year(E.DateAdd(d, E.Literal(1))), E.Literal(1994)),
                 E.EqualTo(E.Year(d), E.Literal(1994.0))):
        f = L.Filter(cond, rel)
        assert date_part_range(f) is f, cond.sql()


# -- the plan cache -------------------------------------------------------------------------------
def test_fingerprints_agree_and_literals_are_parameters(indexed):
    from hyperspace_amd.plan import plan_cache as PC
    s, df = indexed
    if PC._NATIVE_FP is None:
        from hyperspace_amd._native.build import build_host
        build_host()
        PC._NATIVE_FP = PC._native().fingerprint
    assert PC._NATIVE_FP is not None

    def q(k, fmt="month"):
        return df.filter(H.date_add("d", k) < DATE(1995, 1, 1)) \
            .groupBy(H.trunc("d", fmt).alias("t"), H.year("d").alias("y")) \
            .agg(sum_(H.datediff("d", H.add_months("d", k))).alias("x"), count("*").alias("n"))
    keys = []
    for query in (q(30), q(60), q(30, "year")):
        logical = query.queryExecution.logical
        a, b = PC._Ctx(), PC._Ctx()
        fa = PC.fingerprint(logical, a, native=False)
        fb = PC.fingerprint(logical, b, native=True)
        assert fa == fb and [id(x) for x in a.lits] == [id(x) for x in b.lits] and a.ids == b.ids
        keys.append((fa, [x.value for x in a.lits]))
    assert keys[0][0] == keys[1][0] and keys[0][0] != keys[2][0]
    assert sorted(keys[0][1], key=repr) == [30, 30, DATE(1995, 1, 1)]
    assert sorted(keys[1][1], key=repr) == [60, 60, DATE(1995, 1, 1)]


def test_plan_cache_hits_and_uncacheable_rewrites(indexed):
    s, df = indexed
    pc = plan_cache(s)

    def q(k):
        return df.filter(H.date_add("d", k) < DATE(1995, 1, 1)).agg(count("*").alias("n"))
    days = [None if x is None else R.to_day(x) for x in df.to_arrow().column("d").to_pylist()]
    limit = R.day_of("1995-01-01")
    first = _rows(q(30))
    h, m = pc.hits, pc.misses
    second = _rows(q(60))
    assert pc.hits == h + 1 and pc.misses == m
    for k, got in ((30, first), (60, second)):
        assert got == [(sum(1 for x in days if x is not None and x + k < limit),)]
    u = pc.uncacheable
    for y in (1994, 1995):
        got = _rows(df.filter(H.year("d") == y).agg(count("*").alias("n")))
        assert got == [(sum(1 for x in days if x is not None and R.year(x) == y),)]
    assert pc.uncacheable == u + 2


def test_a_column_named_interval_in_every_clause(tmp_path):
    t = pa.table({"k": pa.array([1, 2, 3, 2], pa.int32()),
                  "interval": pa.array([2, 2, 1, 5], pa.int32())})
    os.makedirs(tmp_path / "iv")
    pq.write_table(t, tmp_path / "iv" / "p.parquet")
    s = H.Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                        "spark.hyperspace.mi.execution.device": "cpu"},
                  warehouse_dir=str(tmp_path / "wh"))
    df = s.read.parquet(str(tmp_path / "iv"))
    df.createOrReplaceTempView("t")
    assert _rows(df.filter("k = interval")) == [(2, 2)]
    assert _rows(s.sql("SELECT k FROM t WHERE k = interval")) == [(2,)]
    assert [tuple(r) for r in s.sql("SELECT k, interval FROM t ORDER BY interval").collect()][0] \
        == (3, 1)
    assert _rows(s.sql("SELECT interval, count(*) n FROM t GROUP BY interval")) == \
        [(1, 1), (2, 2), (5, 1)]
    assert _rows(s.sql("SELECT k + interval s FROM t WHERE interval > 1 AND k < interval")) == \
        [(3,), (7,)]


def test_plain_date_comparison_beside_a_date_function_and_long_in_lists(rt, tmp_path):
    """``month(d) = 12 OR d < DATE ...``: the comparison without a date function is emitted on
    day numbers too; OptimizeIn's InSet form of a long list is emitted like the list."""
    import torch
    from hyperspace_amd.exec import project
    d = E.Attribute("d", pa.date32())
    dn = E.Attribute("dn", pa.date32(), nullable=False)
    n = E.Attribute("n", pa.int16(), nullable=False)
    cols = _cpu_cols(d, dn, n)
    exprs = [E.Or(E.EqualTo(E.Month(d), E.Literal(12)), E.LessThan(d, E.Literal(DATE(1995, 1, 1)))),
             E.And(E.GreaterThan(E.Year(d), E.Literal(1990)), E.LessThanOrEqual(dn, d)),
             E.InSet(E.DayOfYear(d), frozenset(range(1, 40, 3))),
             E.Not(E.InSet(E.Month(dn), frozenset([1, 2, None])))]
    k, _, outs = project.build(exprs, cols, 4, torch.device("cpu"))
    assert [o.atype for o in outs] == [pa.bool_()] * 4
    rc = rt.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                              str(tmp_path).encode())
    assert rc == 0, rt.runtime().hs_jit_last_error().decode()


def test_unsigned_day_counts_are_an_analysis_error():
    d = E.Attribute("d", pa.date32())
    for t in (pa.uint8(), pa.uint16(), pa.uint32()):
        with pytest.raises(HyperspaceException, match=r"date_add\(\).*uint"):
            E.date_function("date_add", d, E.Attribute("u", t))
