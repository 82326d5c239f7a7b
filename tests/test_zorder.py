"""Z-order covering indexes in a CPU session: config and metadata, rule selection, the host
builder against the oracle (tests/zorder_ref.py), query results and the lifecycle."""
import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import zorder_ref as R
from helpers import index_names_used, make_session, scans, sorted_rows
from hyperspace_amd import (Hyperspace, HyperspaceException, IndexConfig,
                            ZOrderCoveringIndexConfig, col, count, get_context, sum_)
from hyperspace_amd.index.log_entry import (IndexLogEntry, LogEntry, ZOrderCoveringIndex,
                                            derived_dataset_from_json_obj)
from hyperspace_amd.io.writer import get_bucket_id

N = 4000
FILES = 4
# FilterIndexRule picks this kind only on request (off by default)
RULE_KEY = "spark.hyperspace.index.zorder.filterRule.enabled"


def source_table(n=N, seed=7, nulls=False) -> pa.Table:
    rng = np.random.default_rng(seed)
    mask = rng.random(n) < 0.1 if nulls else None
    return pa.table({
        "a": pa.array(rng.integers(0, 10 ** 6, n).astype(np.int32), mask=mask),
        "d": pa.array(rng.integers(10_000, 12_500, n).astype(np.int32), pa.int32()).view(
            pa.date32()),
        "f": pa.array(rng.standard_normal(n)),
        "g": pa.array(rng.integers(-2 ** 40, 2 ** 40, n)),
        "s": pa.array([f"s{v % 17}" for v in range(n)]),
    })


def write_source(directory: str, t: pa.Table, files=FILES, start=0) -> None:
    os.makedirs(directory, exist_ok=True)
    step = -(-t.num_rows // files)
    for i in range(files):
        pq.write_table(t.slice(i * step, step),
                       os.path.join(directory, f"part-{start + i:05d}.parquet"))


@pytest.fixture
def env(tmp_path):
    s = make_session(tmp_path)
    s.conf.set(RULE_KEY, "true")
    src = str(tmp_path / "src")
    write_source(src, source_table(nulls=True))
    hs = Hyperspace(s)
    yield s, hs, src
    s.disableHyperspace()


def entry_of(s, name) -> IndexLogEntry:
    return [e for e in get_context(s).index_collection_manager.get_indexes() if e.name == name][0]


def index_rows(entry) -> pa.Table:
    """The index data read back in file-name order."""
    files = sorted(entry.content.files, key=lambda p: os.path.basename(p))
    return pa.concat_tables([pq.read_table(f.replace("file:", "")) for f in files])


def storage(t: pa.Table, name: str):
    c = t.column(name).combine_chunks()
    valid = None if c.null_count == 0 else np.asarray(c.is_valid())
    if pa.types.is_date32(c.type):
        c = c.view(pa.int32())
    return np.asarray(c.fill_null(0)), valid


# -- config and metadata ----------------------------------------------------------------------
def test_config_validation():
    c = ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"])
    assert (c.indexName, c.indexedColumns, c.includedColumns) == ("z", ["a", "d"], ["f"])
    assert ZOrderCoveringIndexConfig("z", ["a"]).includedColumns == []
    for bad in (lambda: ZOrderCoveringIndexConfig("", ["a"]),
                lambda: ZOrderCoveringIndexConfig("z", []),
                lambda: ZOrderCoveringIndexConfig("z", ["a", "A"]),
                lambda: ZOrderCoveringIndexConfig("z", ["a"], ["f", "F"]),
                lambda: ZOrderCoveringIndexConfig("z", ["a"], ["A"]),
                lambda: ZOrderCoveringIndexConfig("z", [f"c{i}" for i in range(9)])):
        with pytest.raises(ValueError):
            bad()
    ZOrderCoveringIndexConfig("z", [f"c{i}" for i in range(8)])
    assert c == ZOrderCoveringIndexConfig("Z", ["A", "d"], ["f"])
    assert c != IndexConfig("z", ["a", "d"], ["f"]) and IndexConfig("z", ["a", "d"], ["f"]) != c


def test_log_entry_json_round_trip(env):
    s, hs, src = env
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"]))
    e = entry_of(s, "z")
    dd = e.derived_dataset
    assert isinstance(dd, ZOrderCoveringIndex)
    assert (dd.kind, dd.kind_abbr) == ("ZOrderCoveringIndex", "ZCI")
    o = dd.to_json_obj()
    assert o["kind"] == "ZOrderCoveringIndex" and o["kindAbbr"] == "ZCI"
    assert o["properties"]["columns"] == {"indexed": ["a", "d"], "included": ["f"]}
    assert o["properties"]["numBuckets"] == 1
    assert derived_dataset_from_json_obj(o) == dd
    back = LogEntry.from_json(e.to_json())
    assert isinstance(back.derived_dataset, ZOrderCoveringIndex) and back == e
    assert e.is_zorder and not e.is_covering and not e.is_data_skipping
    assert e.indexed_columns == ["a", "d"] and e.included_columns == ["f"]
    assert e.num_buckets == 1 and e.schema.names == ["a", "d", "f"]
    assert isinstance(e.config, ZOrderCoveringIndexConfig)
    assert e.config == ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"])
    row = hs.index("z").to_arrow().to_pylist()[0]
    assert row["kind"] == "ZOrderCoveringIndex" and row["numBuckets"] == 1
    assert row["indexedColumns"] == ["a", "d"] and row["includedColumns"] == ["f"]
    assert "z" in hs.indexes().to_arrow().column("name").to_pylist()


def test_unsupported_indexed_types_are_refused(tmp_path):
    s = make_session(tmp_path)
    src = str(tmp_path / "t")
    os.makedirs(src)
    t = pa.table({"s": pa.array(["x", "y"]), "b": pa.array([True, False]),
                  "w": pa.array([decimal.Decimal("1.5"), None], pa.decimal128(20, 2)),
                  "l": pa.array([[1], [2]], pa.list_(pa.int32())),
                  "ok": pa.array([decimal.Decimal("1.5"), None], pa.decimal128(10, 2)),
                  "i": pa.array([1, 2], pa.int8())})
    pq.write_table(t, os.path.join(src, "part-00000.parquet"))
    hs = Hyperspace(s)
    for c in ("s", "b", "w", "l"):
        with pytest.raises(HyperspaceException, match=f"'{c}'"):
            hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig(f"z_{c}", ["i", c]))
    # included columns are unrestricted; small decimals and int8 are indexable
    hs.createIndex(s.read.parquet(src),
                   ZOrderCoveringIndexConfig("z_ok", ["ok", "i"], ["s", "b", "w"]))
    assert index_rows(entry_of(s, "z_ok")).num_rows == 2


# -- rule --------------------------------------------------------------------------------------
def test_filter_on_second_indexed_column_picks_zorder(env):
    s, hs, src = env
    hs.createIndex(s.read.parquet(src), IndexConfig("ci", ["a", "d"], ["f"]))
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"]))
    Hyperspace.enable(s)
    lo = pa.scalar(11_000, pa.int32()).cast(pa.date32()).as_py()
    q = s.read.parquet(src).filter(col("d") >= lo).select("d", "f")
    assert index_names_used(q) == {"z"}
    assert all(not sc.use_bucketing for sc in scans(q))
    out = []
    hs.explain(q, redirectFunc=out.append)
    text = "".join(out)
    assert "z:" in text.split("Indexes used:")[1] and "Type: ZCI" in text
    # a covering index whose lead column is filtered wins
    q2 = s.read.parquet(src).filter((col("a") < 1000) & (col("d") >= lo)).select("d", "f")
    assert index_names_used(q2) == {"ci"}
    # an uncovered column leaves the plan alone
    q3 = s.read.parquet(src).filter(col("d") >= lo).select("d", "g")
    assert index_names_used(q3) == set()
    # so does a filter on an included column only
    q4 = s.read.parquet(src).filter(col("f") > 0).select("f")
    assert index_names_used(q4) == set()


def test_rule_selects_zorder_only_on_request(env):
    s, hs, src = env
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"]))
    Hyperspace.enable(s)
    q = lambda: s.read.parquet(src).filter(col("a") < 5000).select("a", "f")   # noqa: E731
    assert index_names_used(q()) == {"z"}
    s.conf.unset(RULE_KEY)                 # the default
    assert index_names_used(q()) == set()
    s.conf.set(RULE_KEY, "false")
    assert index_names_used(q()) == set()


def test_zorder_ranking_prefers_larger_filtered_share(env):
    s, hs, src = env
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z3", ["a", "d", "g"], ["f"]))
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z2", ["a", "d"], ["f", "g"]))
    Hyperspace.enable(s)
    q = s.read.parquet(src).filter((col("a") < 5000) & (col("g") > 0)).select("f")
    assert index_names_used(q) == {"z3"}       # 2/3 of z3 against 1/2 of z2
    q = s.read.parquet(src).filter(col("a") < 5000).select("f")
    assert index_names_used(q) == {"z2"}       # 1/2 against 1/3


def test_join_rule_ignores_zorder_index(env):
    s, hs, src = env
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a"], ["f"]))
    Hyperspace.enable(s)
    from hyperspace_amd.plan import physical as X
    from hyperspace_amd.rules.join_rule import JoinIndexRule

    def q():
        x, y = s.read.parquet(src), s.read.parquet(src)
        return x.join(y, x["a"] == y["a"]).select(x["a"], y["f"])
    plan = q().queryExecution.analyzed
    assert JoinIndexRule(s, plan) is plan or \
        JoinIndexRule(s, plan).tree_string() == plan.tree_string()
    # FilterIndexRule may still serve the inferred isnotnull(a) filters, but never as a
    # bucketed, shuffle-free join side
    shuffles = lambda d: len(d.queryExecution.executed_plan.collect(       # noqa: E731
        lambda p: isinstance(p, X.ShuffleExchangeExec)))
    assert all(not sc.use_bucketing for sc in scans(q()))
    n_on = shuffles(q())
    got = sorted_rows(q())
    s.disableHyperspace()
    assert shuffles(q()) == n_on
    assert got == sorted_rows(q())


def test_window_over_filter_reads_zorder_unbucketed(env):
    from hyperspace_amd import Window, row_number
    s, hs, src = env
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"]))
    Hyperspace.enable(s)
    w = Window.partitionBy("a", "d").orderBy("f")
    q = s.read.parquet(src).filter(col("a") < 5000).select("a", "d", "f") \
        .withColumn("rn", row_number().over(w))
    assert index_names_used(q) == {"z"}
    assert all(not sc.use_bucketing for sc in scans(q))
    got = sorted_rows(q)
    s.disableHyperspace()
    assert got == sorted_rows(q)


# -- host build --------------------------------------------------------------------------------
def test_host_build_equals_reference_order(env, tmp_path):
    s, hs, src = env
    s.conf.set("spark.hyperspace.index.lineage.enabled", "true")
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f", "s"]))
    e = entry_of(s, "z")
    files = sorted(os.listdir(src))
    t = pa.concat_tables([pq.read_table(os.path.join(src, f)) for f in files])
    order = R.order([storage(t, "a"), storage(t, "d")])
    want = t.take(pa.array(order))
    got = index_rows(e)
    assert got.num_rows == N
    for c in ("a", "d", "f", "s"):
        assert got.column(c).to_pylist() == want.column(c).to_pylist(), c
    keys = R.keys([storage(got, "a"), storage(got, "d")])
    assert (np.diff(keys) >= 0).all()
    assert got.column("_data_file_id").null_count == 0


def test_several_files_by_target_bytes(env):
    s, hs, src = env
    size = sum(os.path.getsize(os.path.join(src, f)) for f in os.listdir(src))
    s.conf.set("spark.hyperspace.index.zorder.targetSourceBytesPerPartition", str(size // 3 + 1))
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"]))
    e = entry_of(s, "z")
    assert e.num_buckets == 3
    names = sorted(os.path.basename(p) for p in e.content.files)
    assert [get_bucket_id(n) for n in names] == [0, 1, 2]
    per = -(-N // 3)
    rows = [pq.read_metadata(p.replace("file:", "")).num_rows
            for p in sorted(e.content.files, key=os.path.basename)]
    assert rows == [per, per, N - 2 * per]
    t = pa.concat_tables([pq.read_table(os.path.join(src, f)) for f in sorted(os.listdir(src))])
    want = t.take(pa.array(R.order([storage(t, "a"), storage(t, "d")])))
    assert index_rows(e).column("f").to_pylist() == want.column("f").to_pylist()


QUERIES = [
    lambda d: d.filter((col("a") >= 100_000) & (col("a") < 150_000)).select("a", "d", "f"),
    lambda d: d.filter(col("d") < pa.scalar(10_100, pa.int32()).cast(pa.date32()).as_py())
    .select("d", "f"),
    lambda d: d.filter((col("a") < 500_000) & col("d").isin(
        *[pa.scalar(v, pa.int32()).cast(pa.date32()).as_py() for v in (10_005, 11_111)]))
    .select("a", "f"),
    lambda d: d.filter(col("a").isNull()).select("d"),
    lambda d: d.filter(col("a") > 900_000).agg(sum_(col("f")).alias("sf"), count("*").alias("n")),
]


@pytest.mark.parametrize("qi", range(len(QUERIES)))
def test_query_results_equal_disabled_run(env, qi):
    s, hs, src = env
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"]))
    Hyperspace.enable(s)
    q = QUERIES[qi](s.read.parquet(src))
    assert index_names_used(q) == {"z"}
    got = sorted_rows(q)
    s.disableHyperspace()
    want = sorted_rows(QUERIES[qi](s.read.parquet(src)))
    assert len(want) > 0 and len(got) == len(want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            if qi == 4 and isinstance(b, float):
                # a float sum in another row order: |error| <= n * 2^-53 * sum|f|, n <= 4000 rows
                # of |f| < 6: 4000 * 1.1e-16 * 24000 < 1.1e-8
                assert abs(a - b) <= 1.1e-8
            else:
                assert a == b


# -- lifecycle ---------------------------------------------------------------------------------
def test_lifecycle(env):
    s, hs, src = env
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f"]))
    write_source(src, source_table(500, seed=9), files=1, start=50)
    Hyperspace.enable(s)
    q = lambda: s.read.parquet(src).filter(col("a") < 5000).select("a", "f")   # noqa: E731
    # the source changed: never a candidate by Hybrid Scan
    s.conf.set("spark.hyperspace.index.hybridscan.enabled", "true")
    assert index_names_used(q()) == set()
    s.conf.set("spark.hyperspace.index.hybridscan.enabled", "false")
    assert index_names_used(q()) == set()
    with pytest.raises(HyperspaceException, match="not supported by index kind"):
        hs.refreshIndex("z", "incremental")
    with pytest.raises(HyperspaceException, match="not supported by index kind"):
        hs.refreshIndex("z", "quick")
    with pytest.raises(HyperspaceException, match="not supported by index kind"):
        hs.optimizeIndex("z")
    hs.refreshIndex("z", "full")
    e = entry_of(s, "z")
    assert e.is_zorder and index_rows(e).num_rows == N + 500
    assert index_names_used(q()) == {"z"}
    got = sorted_rows(q())
    s.disableHyperspace()
    assert got == sorted_rows(q())
    s.enableHyperspace()
    hs.deleteIndex("z")
    assert index_names_used(q()) == set()
    hs.restoreIndex("z")
    assert index_names_used(q()) == {"z"}
    hs.deleteIndex("z")
    hs.vacuumIndex("z")
    assert "z" not in hs.indexes().to_arrow().column("name").to_pylist()
