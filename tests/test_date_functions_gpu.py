"""Date functions on the MI355X: the generated projection kernel on hand-made device columns
against tests/date_ref.py (integer-exact: no tolerance), and queries end to end against the host
engine - select, WHERE, GROUP BY, INTERVAL literals, CASE over a join, the year -> range rewrite,
literal-only resubmission, Hybrid Scan and the timestamp fallback."""
import datetime
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import date_ref as R
import hyperspace_amd as H
from hyperspace_amd import Hyperspace, IndexConfig, Session, col, count, sum_
from hyperspace_amd.plan import expressions as E

from test_gpu_e2e import _both, _close

pytestmark = pytest.mark.gpu

BLOCK = 256
SIZES = [1, BLOCK - 1, BLOCK, BLOCK + 1]
GRID_CAP = 4096                       # project.evaluate launches at most this many blocks
MARGIN = 13000                        # days: room for +-400 days and +-400 months


def _days(n, seed):
    """EDGE tiled with seeded random days, ``n`` rows."""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(R.MIN_DAY, R.MAX_DAY + 1, max(n, 1))
    out = np.where(np.arange(n) % 2 == 0, np.resize(np.array(R.EDGE), n), rnd[:n])
    if n > len(R.EDGE):
        out[:len(R.EDGE)] = R.EDGE
    return out.astype(np.int32)


def _column(values, valid, atype, device):
    import torch
    from hyperspace_amd.exec.device_table import DeviceColumn
    data = torch.from_numpy(np.ascontiguousarray(values)).to(device)
    v = None if valid is None else torch.from_numpy(valid.astype(np.uint8)).to(device)
    return DeviceColumn(data, v, atype)


def _evaluate(exprs, cols, n, device):
    """``project.evaluate`` twice (bit-equal), as ({values}, {valid}) numpy arrays per output."""
    import torch
    from hyperspace_amd.exec import project
    runs = []
    for _ in range(2):
        outs = project.evaluate(exprs, cols, n, device)
        torch.cuda.synchronize()
        runs.append([(o.data.cpu().numpy().copy(), o.valid.cpu().numpy().copy()) for o in outs])
    for (a, av), (b, bv) in zip(*runs):
        assert np.array_equal(a, b) and np.array_equal(av, bv), "a repeated launch differs"
    return runs[0]


def _check(got, want, tag, null_zero=True):
    """``want``: a list with None for NULL; NULL rows store value 0 and valid 0 (a comparison's
    NULL rows keep an unspecified value: ``null_zero`` False)."""
    data, valid = got
    wv = np.array([x is not None for x in want], dtype=np.uint8)
    wd = np.array([0 if x is None else int(x) for x in want], dtype=np.int64)
    assert np.array_equal(valid, wv), (tag, "valid", np.nonzero(valid != wv)[0][:5])
    bad = np.nonzero((data.astype(np.int64) != wd) & ((wv != 0) | null_zero))[0]
    assert len(bad) == 0, (tag, int(bad[0]), int(data[bad[0]]), int(wd[bad[0]]))


def _masked(values, valid):
    return [int(x) if valid is None or valid[i] else None for i, x in enumerate(values)]


@pytest.mark.parametrize("nullable", [False, True], ids=["dense", "nullable"])
@pytest.mark.parametrize("n", SIZES)
def test_every_function_against_the_reference(device, n, nullable):
    rng = np.random.default_rng(100 + n)
    days = _days(n, n)
    valid = (rng.random(n) >= 0.15) if nullable else None
    d = E.Attribute("d", pa.date32(), nullable=nullable)
    cols = {d.expr_id: _column(days, valid, pa.date32(), device)}
    dl = _masked(days, valid)
    names = ("year", "quarter", "month", "dayofmonth", "dayofyear", "dayofweek", "weekday",
             "weekofyear", "last_day")
    fmts = ("year", "YYYY", "yy", "quarter", "month", "MON", "mm", "week", "day")
    exprs = [E.date_function(x, d) for x in names] + [E.date_function("trunc", d, f) for f in fmts]
    got = _evaluate(exprs, cols, n, device)
    for x, g in zip(names, got):
        _check(g, R.lift(getattr(R, x))(dl), x)
    for f, g in zip(fmts, got[len(names):]):
        _check(g, R.lift(lambda v: R.trunc(v, f))(dl), ("trunc", f))


@pytest.mark.parametrize("nullable", [False, True], ids=["dense", "nullable"])
@pytest.mark.parametrize("n", SIZES)
def test_day_and_month_arithmetic_with_literal_and_column_n(device, n, nullable):
    rng = np.random.default_rng(200 + n)
    days = _days(n, 7 * n)
    other = _days(n, 11 * n)[::-1].copy()
    raw = rng.integers(-400, 401, n).astype(np.int32)
    valid = (rng.random(n) >= 0.15) if nullable else None
    nvalid = (rng.random(n) >= 0.15) if nullable else None
    nd = np.array([R.clip_days(int(a), int(b)) for a, b in zip(days, raw)], dtype=np.int32)
    nneg = np.array([-R.clip_days(int(a), -int(b)) for a, b in zip(days, raw)], dtype=np.int32)
    nm = np.array([R.clip_months(int(a), int(b)) for a, b in zip(days, raw)], dtype=np.int16)
    d = E.Attribute("d", pa.date32(), nullable=nullable)
    o = E.Attribute("o", pa.date32(), nullable=nullable)
    kd, ks = E.Attribute("kd", pa.int32(), nullable=nullable), E.Attribute("ks", pa.int32())
    km = E.Attribute("km", pa.int16(), nullable=nullable)
    cols = {d.expr_id: _column(days, valid, pa.date32(), device),
            o.expr_id: _column(other, nvalid, pa.date32(), device),
            kd.expr_id: _column(nd, nvalid, pa.int32(), device),
            ks.expr_id: _column(nneg, None, pa.int32(), device),
            km.expr_id: _column(nm, nvalid, pa.int16(), device)}
    dl, ol = _masked(days, valid), _masked(other, nvalid)
    got = _evaluate([E.DateAdd(d, kd), E.DateSub(d, ks), E.AddMonths(d, km), E.DateDiff(d, o),
                     E.DateDiff(o, d)], cols, n, device)
    _check(got[0], R.lift(R.date_add)(dl, _masked(nd, nvalid)), "date_add column")
    _check(got[1], R.lift(R.date_sub)(dl, _masked(nneg, None)), "date_sub column")
    _check(got[2], R.lift(R.add_months)(dl, _masked(nm, nvalid)), "add_months column")
    _check(got[3], R.lift(R.datediff)(dl, ol), "datediff")
    _check(got[4], R.lift(R.datediff)(ol, dl), "datediff flipped")
    # literal n: days pulled away from the ends of the range so every result stays inside
    mid = np.clip(days, R.MIN_DAY + MARGIN, R.MAX_DAY - MARGIN).astype(np.int32)
    cols[d.expr_id] = _column(mid, valid, pa.date32(), device)
    ml = _masked(mid, valid)
    lits = (0, 1, -1, 400, -400)
    got = _evaluate([E.DateAdd(d, E.Literal(k)) for k in lits] +
                    [E.DateSub(d, E.Literal(k)) for k in lits] +
                    [E.AddMonths(d, E.Literal(k)) for k in lits] +
                    [E.DateAdd(d, E.Literal(None))], cols, n, device)
    for j, k in enumerate(lits):
        _check(got[j], R.lift(lambda v: R.date_add(v, k))(ml), ("date_add", k))
        _check(got[5 + j], R.lift(lambda v: R.date_sub(v, k))(ml), ("date_sub", k))
        _check(got[10 + j], R.lift(lambda v: R.add_months(v, k))(ml), ("add_months", k))
    _check(got[15], [None] * n, "date_add NULL")


def test_date_results_compare_select_and_nest(device):
    """A date-valued result against a date column, a date literal and a date-like string; an IN
    over a part; a date function inside a CASE and over another one's result."""
    n = BLOCK + 1
    days = _days(n, 3)
    mid = np.clip(days, R.MIN_DAY + MARGIN, R.MAX_DAY - MARGIN).astype(np.int32)
    valid = np.random.default_rng(9).random(n) >= 0.2
    d = E.Attribute("d", pa.date32())
    o = E.Attribute("o", pa.date32(), nullable=False)
    cols = {d.expr_id: _column(mid, valid, pa.date32(), device),
            o.expr_id: _column(days, None, pa.date32(), device)}
    lim = datetime.date(1995, 1, 1)
    L = R.to_day(lim)
    exprs = [E.LessThan(E.DateAdd(d, E.Literal(7)), E.Literal(lim)),
             E.GreaterThanOrEqual(E.LastDay(d), o),
             E.LessThanOrEqual(E.Literal("1995-01-01"), E.TruncDate(d, "month")),
             E.In(E.DayOfWeek(d), [E.Literal(1), E.Literal(7)]),
             E.In(E.Month(o), [E.Literal(2), E.Literal(None)]),
             E.CaseWhen([(E.EqualTo(E.Year(d), E.Literal(2000)), E.DateDiff(o, d))], E.Literal(0)),
             E.Year(E.AddMonths(E.LastDay(d), E.Literal(1))),
             E.CaseWhen([(E.LessThan(d, E.Literal(lim)), E.TruncDate(d, "year"))], o),
             E.Or(E.EqualTo(E.Month(d), E.Literal(12)), E.LessThan(d, E.Literal(lim))),
             E.InSet(E.DayOfYear(o), frozenset(range(1, 367, 3)))]
    got = _evaluate(exprs, cols, n, device)
    dl, ol = _masked(mid, valid), _masked(days, None)
    _check(got[0], R.lift(lambda v: v + 7 < L)(dl), "date_add < literal", False)
    _check(got[1], R.lift(lambda v, w: R.last_day(v) >= w)(dl, ol), "last_day >= column", False)
    _check(got[2], R.lift(lambda v: L <= R.trunc(v, "month"))(dl), "string <= trunc", False)
    _check(got[3], R.lift(lambda v: R.dayofweek(v) in (1, 7))(dl), "IN")
    _check(got[4], [True if R.month(w) == 2 else None for w in ol], "IN with a NULL entry")
    _check(got[5], [0 if v is None or R.year(v) != 2000 else w - v for v, w in zip(dl, ol)],
           "CASE over year")
    _check(got[6], R.lift(lambda v: R.year(R.add_months(R.last_day(v), 1)))(dl), "nested")
    _check(got[7], [w if v is None or not v < L else R.trunc(v, "year")
                    for v, w in zip(dl, ol)], "date-valued CASE")
    _check(got[8], R.lift(lambda v: R.month(v) == 12 or v < L)(dl), "OR with a plain comparison",
           False)
    _check(got[9], [R.dayofyear(w) % 3 == 1 for w in ol], "InSet")


def test_year_past_the_grid_cap(device):
    """One row more than a block past the grid cap of ``evaluate``: the grid-stride loop's
    second trip and its ragged tail."""
    n = GRID_CAP * BLOCK + BLOCK + 1
    rng = np.random.default_rng(5)
    days = rng.integers(R.MIN_DAY, R.MAX_DAY + 1, n).astype(np.int32)
    days[:len(R.EDGE)] = R.EDGE
    days[-len(R.EDGE):] = R.EDGE
    valid = rng.random(n) >= 0.1
    d = E.Attribute("d", pa.date32())
    (data, ok), = _evaluate([E.Year(d)], {d.expr_id: _column(days, valid, pa.date32(), device)},
                            n, device)
    want = np.array([R.year(x) if ok_ else 0 for x, ok_ in zip(days.tolist(), valid.tolist())],
                    dtype=np.int32)
    assert np.array_equal(ok, valid.astype(np.uint8))
    assert np.array_equal(data, want)


# -- end to end -----------------------------------------------------------------------------------
@pytest.fixture
def tpch(tmp_path, device):
    rng = np.random.default_rng(23)
    n_ord = 1500
    okeys = rng.permutation(np.arange(1, n_ord + 1, dtype=np.int64) * 4)
    lo, hi = R.day_of("1992-01-01"), R.day_of("1998-12-31")
    od = pa.table({"o_orderkey": okeys,
                   "o_orderdate": pa.array(rng.integers(lo, hi, n_ord).astype(np.int32),
                                           mask=rng.random(n_ord) < 0.05).cast(pa.date32()),
                   "o_year": rng.integers(1992, 1999, n_ord).astype(np.int32)})
    lk = np.repeat(okeys, rng.integers(1, 6, n_ord))
    n = len(lk)
    ship = rng.integers(lo, hi, n).astype(np.int32)
    li = pa.table({"l_orderkey": lk,
                   "l_quantity": rng.integers(1, 51, n).astype(np.int32),
                   "l_extendedprice": rng.integers(1, 100_000, n).astype(np.float64),
                   "l_shipdate": pa.array(ship, mask=rng.random(n) < 0.05).cast(pa.date32()),
                   "l_commitdate": pa.array(ship + rng.integers(-30, 31, n).astype(np.int32))
                   .cast(pa.date32()),
                   "l_ts": pa.array(ship.astype(np.int64) * 86_400_000_000 + 3_600_000_000,
                                    pa.timestamp("us"))})
    assert 3000 <= n <= 8000
    for name, t, parts in (("lineitem", li, 3), ("orders", od, 2)):
        os.makedirs(tmp_path / name)
        step = (t.num_rows + parts - 1) // parts
        for i in range(parts):
            pq.write_table(t.slice(i * step, step), tmp_path / name / f"part-{i}.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.numBuckets": "4",
                      "spark.sql.autoBroadcastJoinThreshold": "-1",
                      "spark.sql.shuffle.partitions": "4",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    hs = Hyperspace(s)
    lpath, opath = str(tmp_path / "lineitem"), str(tmp_path / "orders")
    hs.createIndex(s.read.parquet(lpath), IndexConfig(
        "li_ok", ["l_orderkey"], ["l_quantity", "l_extendedprice", "l_shipdate", "l_commitdate"]))
    hs.createIndex(s.read.parquet(lpath), IndexConfig(
        "li_ship", ["l_shipdate"], ["l_quantity", "l_extendedprice", "l_commitdate"]))
    hs.createIndex(s.read.parquet(opath), IndexConfig(
        "od_ok", ["o_orderkey"], ["o_orderdate", "o_year"]))
    Hyperspace.enable(s)
    s.read.parquet(lpath).createOrReplaceTempView("lineitem")
    s.read.parquet(opath).createOrReplaceTempView("orders")
    return s, lpath, opath


def _native(s, q, index=()):
    plan = q.queryExecution.executed_plan.tree_string()
    for name in index:
        assert f"Name: {name}" in plan, plan
    g, c, path = _both(s, q)
    assert path == "native", s.backend().fallback_reason
    _close(g, c)
    assert g.schema.types == c.schema.types
    return g


def test_select_of_date_parts(tpch):
    s, _, _ = tpch
    g = _native(s, s.sql(
        "SELECT l_orderkey, year(l_shipdate) y, quarter(l_shipdate) q, month(l_shipdate) m, "
        "day(l_shipdate) d, dayofyear(l_shipdate) dy, dayofweek(l_shipdate) dw, "
        "weekofyear(l_shipdate) w, last_day(l_shipdate) ld, trunc(l_shipdate, 'week') tw, "
        "add_months(l_shipdate, l_quantity) am, l_shipdate + INTERVAL '3' MONTH i3, "
        "datediff(l_commitdate, l_shipdate) dd, date_sub(l_commitdate, 7) ds "
        "FROM lineitem WHERE l_orderkey < 3000"), ["li_ok"])
    assert g.num_rows > 100
    days = [None if x is None else R.to_day(x) for x in g.column("ld").to_pylist()]
    assert g.column("y").to_pylist() == R.lift(R.year)(days)


def test_where_with_date_parts(tpch):
    s, _, _ = tpch
    g = _native(s, s.sql("SELECT count(*) n, sum(l_extendedprice) t FROM lineitem "
                         "WHERE month(l_shipdate) = 12 AND dayofweek(l_shipdate) IN (1, 7)"))
    assert g.column("n")[0].as_py() > 0
    g = _native(s, s.sql("SELECT count(*) n FROM lineitem "
                         "WHERE datediff(l_commitdate, l_shipdate) > 10 AND l_quantity < 30"))
    assert g.column("n")[0].as_py() > 0


def test_group_by_year_and_quarter(tpch):
    s, lpath, _ = tpch
    g = _native(s, s.sql("SELECT year(l_shipdate) y, quarter(l_shipdate) q, "
                         "sum(l_extendedprice) t, count(*) n FROM lineitem "
                         "GROUP BY year(l_shipdate), quarter(l_shipdate)"))
    assert g.num_rows == 7 * 4 + 1          # and the NULL group
    li = s.read.parquet(lpath)
    _native(s, li.groupBy(H.year("l_shipdate").alias("y")).agg(sum_("l_quantity").alias("q")))


def test_q1_filter_with_an_interval_literal(tpch):
    s, _, _ = tpch
    text = "SELECT sum(l_quantity) q, count(*) n FROM lineitem WHERE l_shipdate <= {}"
    a = s.sql(text.format("DATE '1998-12-01' - INTERVAL '90' DAY"))
    b = s.sql(text.format("DATE '1998-09-02'"))
    import re

    def shape(q):
        return re.sub(r"#\d+", "#", q.queryExecution.executed_plan.tree_string())
    assert shape(a) == shape(b)
    ga, gb = _native(s, a, ["li_ship"]), _native(s, b, ["li_ship"])
    assert ga.to_pylist() == gb.to_pylist() and ga.column("n")[0].as_py() > 0


def test_q8_case_over_year_grouped_by_extract_over_a_join(tpch):
    s, _, _ = tpch
    q = s.sql("SELECT extract(year FROM o_orderdate) o_y, "
              "sum(CASE WHEN year(o_orderdate) = 1995 THEN l_extendedprice ELSE 0 END) v95, "
              "sum(l_extendedprice) v, count(*) n "
              "FROM lineitem JOIN orders ON l_orderkey = o_orderkey "
              "GROUP BY extract(year FROM o_orderdate)")
    g = _native(s, q, ["li_ok", "od_ok"])
    rows = {r["o_y"]: r for r in g.to_pylist()}
    assert set(rows) == set(range(1992, 1999)) | {None}
    assert rows[1995]["v95"] == rows[1995]["v"] and rows[1996]["v95"] == 0


def test_year_filter_with_the_range_rewrite_on_and_off(tpch):
    from hyperspace_amd.utils.tracing import PROFILE_ENABLED, TRACER
    s, _, _ = tpch
    text = "SELECT sum(l_extendedprice) t, count(*) n FROM lineitem WHERE year(l_shipdate) = 1994"
    results = {}
    for on in ("true", "false"):
        s.conf.set("spark.hyperspace.mi.datePartRange.enabled", on)
        q = s.sql(text)
        s.conf.set(PROFILE_ENABLED, "true")
        TRACER.reset()
        try:
            g = _native(s, q, ["li_ship"] if on == "true" else ())
            stages = set(TRACER.report())
        finally:
            s.conf.set(PROFILE_ENABLED, "false")
            TRACER.set_profile(False)
        assert stages, "the stage trace recorded nothing"
        results[on] = (g.to_pylist(), stages)
    s.conf.set("spark.hyperspace.mi.datePartRange.enabled", "true")
    assert results["true"][0] == results["false"][0] and results["true"][0][0]["n"] > 0
    assert "project" not in results["true"][1], results["true"][1]
    assert "project" in results["false"][1], results["false"][1]


def test_literal_only_resubmission_compiles_nothing(tpch):
    from hyperspace_amd.exec import jit
    from hyperspace_amd.plan.plan_cache import plan_cache
    s, _, _ = tpch
    text = ("SELECT count(*) n, sum(l_quantity) q FROM lineitem "
            "WHERE date_add(l_shipdate, {k}) < DATE '{d}'")
    first = _native(s, s.sql(text.format(k=30, d="1995-01-01")))
    _native(s, s.sql(text.format(k=30, d="1995-01-01")))
    size, hits = len(jit._KERNELS), plan_cache(s).hits
    second = _native(s, s.sql(text.format(k=60, d="1996-06-01")))
    assert len(jit._KERNELS) == size
    assert plan_cache(s).hits > hits
    assert first.column("n")[0].as_py() < second.column("n")[0].as_py()


def test_hybrid_scan_with_appended_files(tpch):
    s, lpath, _ = tpch
    rng = np.random.default_rng(3)
    n = 400
    ship = rng.integers(R.day_of("1993-06-01"), R.day_of("1995-06-01"), n).astype(np.int32)
    extra = pa.table({"l_orderkey": (rng.integers(1, 1500, n) * 4).astype(np.int64),
                      "l_quantity": rng.integers(1, 51, n).astype(np.int32),
                      "l_extendedprice": rng.integers(1, 100_000, n).astype(np.float64),
                      "l_shipdate": pa.array(ship).cast(pa.date32()),
                      "l_commitdate": pa.array(ship + 5).cast(pa.date32()),
                      "l_ts": pa.array(ship.astype(np.int64) * 86_400_000_000, pa.timestamp("us"))})
    pq.write_table(extra, os.path.join(lpath, "part-appended.parquet"))
    s.conf.set("spark.hyperspace.index.hybridscan.enabled", "true")
    s.read.parquet(lpath).createOrReplaceTempView("lineitem")
    q = s.sql("SELECT quarter(l_shipdate) q, sum(l_extendedprice) t, count(*) n FROM lineitem "
              "WHERE l_orderkey < 4000 AND month(l_commitdate) <> 2 GROUP BY quarter(l_shipdate)")
    g = _native(s, q, ["li_ok"])
    assert g.num_rows >= 4


def test_timestamp_argument_falls_back_with_its_reason(tpch):
    s, _, _ = tpch
    q = s.sql("SELECT year(l_ts) y, count(*) n FROM lineitem GROUP BY year(l_ts)")
    g, c, path = _both(s, q)
    assert path == "fallback" and "timestamp argument of year()" in s.backend().fallback_reason
    _close(g, c)
    assert g.num_rows == 7
