"""Data-skipping indexes in a GPU session: the sketch table is built on the device
(exec/device_sketch.py + csrc/kernels/sketch.hip) and equals the host builder's, column for
column; scans prune per execution under the plan cache on the native executor; incremental
refresh sketches the appended files on the device."""
import decimal
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import (BloomFilterSketch, DataSkippingIndexConfig, Hyperspace, MinMaxSketch,
                            Session, col, count, get_context, sum_)
from hyperspace_amd.index import dataskipping as DS
from hyperspace_amd.plan.plan_cache import plan_cache

pytestmark = pytest.mark.gpu

SCHEMA = pa.schema([("i32", pa.int32()), ("i64", pa.int64()), ("d", pa.date32()),
                    ("ts", pa.timestamp("us")), ("f", pa.float64()), ("f32", pa.float32()),
                    ("dec", pa.decimal128(10, 2)), ("wide", pa.decimal128(20, 2)),
                    ("s", pa.string())])
# more than one slab, a small file, no row at all, nulls only, a small file
ROWS = [70_000, 3_000, 0, 1_000, 500]


def _table(i: int, n: int, all_null: bool) -> pa.Table:
    rng = np.random.default_rng(100 + i)
    base = np.arange(n, dtype=np.int64) + i * 100_000
    mask = np.ones(n, bool) if all_null else rng.random(n) < 0.1
    f = rng.standard_normal(n) * 100 + i
    if n > 10:
        f[[1, 2, 3]] = [np.nan, -0.0, np.inf] if i == 0 else [-0.0, 0.0, -1.0]
    words = np.array([f"w{v:05d}" for v in range(400)] + ["", "é", "日本語", "zzÿ"])
    cols = {
        "i32": pa.array(base.astype(np.int32), mask=mask),
        "i64": pa.array(rng.permutation(base * 7919 - 2 ** 40), mask=mask),
        "d": pa.array((base // 50).astype(np.int32), pa.int32(), mask=mask).view(pa.date32()),
        "ts": pa.array(base * 1_000_003, pa.int64(), mask=mask).view(pa.timestamp("us")),
        "f": pa.array(f, mask=mask),
        "f32": pa.array(f.astype(np.float32), mask=mask),
        "dec": pa.array([None if m else decimal.Decimal(int(b)) / 100 - 50
                         for b, m in zip(base, mask)], pa.decimal128(10, 2)),
        "wide": pa.array([None if m else decimal.Decimal(int(b)) * 10 ** 9 + decimal.Decimal("0.25")
                          for b, m in zip(base, mask)], pa.decimal128(20, 2)),
        "s": pa.array(words[rng.integers(0, len(words), n)], pa.string(), mask=mask),
    }
    return pa.table(cols, schema=SCHEMA)


def _write(src, i, n, all_null=False):
    os.makedirs(src, exist_ok=True)
    # file 1 stores its strings PLAIN, the others dictionary-encoded
    pq.write_table(_table(i, n, all_null), os.path.join(src, f"part-{i:05d}.parquet"),
                   use_dictionary=(i != 1))


def _config():
    cols = ["i32", "i64", "d", "ts", "f", "f32", "dec", "wide", "s"]
    return DataSkippingIndexConfig(
        "skip", *[MinMaxSketch(c) for c in cols],
        BloomFilterSketch("i32", 0.01, 1000),            # 150 words: filters built in LDS
        BloomFilterSketch("i64", 0.01, 200_000),         # past the LDS limit: global atomics
        BloomFilterSketch("d", 0.1, 5), BloomFilterSketch("ts", 0.01, 1000),
        BloomFilterSketch("s", 0.01, 500))


@pytest.fixture
def env(tmp_path, device):
    src = str(tmp_path / "src")
    for i, n in enumerate(ROWS):
        _write(src, i, n, all_null=(i == 3))
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.numBuckets": "4",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    hs = Hyperspace(s)
    hs.createIndex(s.read.parquet(src), _config())
    return s, hs, src


def _entry(s):
    return [e for e in get_context(s).index_collection_manager.get_indexes()
            if e.name == "skip"][0]


def _assert_equals_host(s, src, entry):
    got = DS.read_sketch_table(entry).sort_by("_data_file_id")
    rel = s.read.parquet(src).queryExecution.optimized_plan.relation
    ids = {f.name: f.id for f in entry.source_file_info_set}
    files = sorted(ids)
    want = DS.host_sketch_rows(rel, files, entry.derived_dataset.sketches, ids) \
        .sort_by("_data_file_id")
    assert got.schema.equals(want.schema)
    assert got.num_rows == want.num_rows == len(files)
    for name in want.column_names:
        g, w = got.column(name).to_pylist(), want.column(name).to_pylist()
        for a, b in zip(g, w):
            if isinstance(b, float) and b != b:
                assert a != a, name
            else:
                assert a == b and (not isinstance(b, float) or str(a) == str(b)), (name, a, b)
    return got


def test_create_builds_on_device_and_equals_host_build(env):
    from hyperspace_amd.exec.device_sketch import LAST_SKETCH_STATS as st
    s, hs, src = env
    assert st["path"] == "device", st
    assert st["files"] == len(ROWS) and st["rows"] == sum(ROWS)
    assert st["columns"]["wide"] == "host"            # decimal(20, 2) is not exact in float64
    assert all(p == "device" for c, p in st["columns"].items() if c != "wide"), st["columns"]
    assert st["upload_s"] > 0 and st["kernels_s"] > 0
    entry = _entry(s)
    t = _assert_equals_host(s, src, entry)
    no = {f.id: int(f.name.rsplit("part-", 1)[1][:5]) for f in entry.source_file_info_set}
    rows = {no[r["_data_file_id"]]: r for r in t.to_pylist()}
    assert rows[2]["MinMax_i32__min"] is None and rows[3]["MinMax_s__max"] is None
    assert rows[0]["MinMax_f__max"] != rows[0]["MinMax_f__max"]       # NaN is the largest
    assert rows[0]["MinMax_i32__min"] is not None and rows[1]["MinMax_s__min"] is not None


def test_plan_cache_prunes_per_execution_on_the_native_path(env):
    s, hs, src = env
    Hyperspace.enable(s)
    df = s.read.parquet(src)
    be = s.backend()
    pc = plan_cache(s)

    def q(lo):
        return df.filter((col("i32") >= lo) & (col("i32") < lo + 2_000)) \
            .agg(count("*").alias("n"), sum_(col("i64")).alias("t"))
    los = (1_000, 100_500, 400_100)
    h0 = pc.hits
    got, kept = [], []
    for lo in los:
        got.append(q(lo).collect())
        assert be.last_path == "native", be.fallback_reason
        kept.append(tuple(sorted(os.path.basename(p) for p in DS.LAST_PRUNE["kept_paths"])))
    assert pc.hits - h0 >= 2, (pc.hits, pc.misses)
    assert kept == [("part-00000.parquet",), ("part-00001.parquet",), ("part-00004.parquet",)]
    s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
    s.disableHyperspace()
    want = [q(lo).collect() for lo in los]
    assert [[tuple(r) for r in g] for g in got] == [[tuple(r) for r in w] for w in want]
    assert all(w[0][0] > 0 for w in want)


@pytest.mark.parametrize("groups", [("g1",), ("g1", "g2")], ids=["dense", "hash"])
def test_plan_cache_join_aggregate_prunes_per_execution(env, tmp_path, groups):
    """GROUP BY over a merge join whose left side is a data-skipping scan: the aggregate's kept
    setup (one small group column: the dense aggregate's; two columns: the hash aggregate's)
    must not serve the next literal vector from the tables of the files kept for this one."""
    s, hs, src = env
    k = np.arange(0, 410_000, dtype=np.int32)
    k = k[k % 3 != 0]
    os.makedirs(tmp_path / "dim")
    pq.write_table(pa.table({"k": k, "g1": (k % 7).astype(np.int32),
                             "g2": ((k // 100) % 5).astype(np.int32)}),
                   tmp_path / "dim" / "part-00000.parquet")
    s.conf.set("spark.sql.autoBroadcastJoinThreshold", "-1")
    Hyperspace.enable(s)
    df, dim = s.read.parquet(src), s.read.parquet(str(tmp_path / "dim"))
    be = s.backend()
    pc = plan_cache(s)

    def q(lo):
        return df.filter((col("i32") >= lo) & (col("i32") < lo + 2_000)) \
            .join(dim, df["i32"] == dim["k"]).groupBy(*groups) \
            .agg(count("*").alias("n"), sum_(col("i64")).alias("t"))

    def rows(d):
        return sorted(tuple(r) for r in d.collect())
    los = (1_000, 100_500, 400_100)
    h0 = pc.hits
    got, kept = [], []
    for lo in los:
        got.append(rows(q(lo)))
        assert be.last_path == "native", be.fallback_reason
        kept.append(tuple(sorted(os.path.basename(p) for p in DS.LAST_PRUNE["kept_paths"])))
    assert pc.hits - h0 >= 2, (pc.hits, pc.misses)
    assert kept == [("part-00000.parquet",), ("part-00001.parquet",), ("part-00004.parquet",)]
    s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
    s.disableHyperspace()
    want = [rows(q(lo)) for lo in los]
    assert got == want
    assert all(len(w) >= 7 for w in want) and len(set(map(tuple, want))) == 3


def test_incremental_refresh_sketches_on_device(env):
    from hyperspace_amd.exec.device_sketch import LAST_SKETCH_STATS as st
    s, hs, src = env
    _write(src, 5, 2_500)
    os.remove(os.path.join(src, "part-00001.parquet"))
    hs.refreshIndex("skip", "incremental")
    assert st["path"] == "device" and st["files"] == 1 and st["rows"] == 2_500, st
    entry = _entry(s)
    assert len(entry.content.files) == 1
    t = _assert_equals_host(s, src, entry)
    assert t.num_rows == len(ROWS)


def test_sources_the_device_does_not_sketch_take_the_host_builder(tmp_path, device):
    """A csv source is sketched on the host as a whole; an unsigned column of a Parquet source
    alone, next to device-built columns.  Either index prunes in the GPU session."""
    import pyarrow.csv as pcsv
    from hyperspace_amd.exec.device_sketch import LAST_SKETCH_STATS as st
    os.makedirs(tmp_path / "csv")
    os.makedirs(tmp_path / "u")
    for i in range(3):
        a = np.arange(100, dtype=np.int64) + 1000 * i
        pcsv.write_csv(pa.table({"a": a, "b": a * 2}), tmp_path / "csv" / f"part-{i:05d}.csv")
        pq.write_table(pa.table({"u": (a + 2 ** 31).astype(np.uint32), "a": a}),
                       tmp_path / "u" / f"part-{i:05d}.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    hs = Hyperspace(s)
    dc = s.read.csv(str(tmp_path / "csv"), header=True, inferSchema=True)
    du = s.read.parquet(str(tmp_path / "u"))
    hs.createIndex(dc, DataSkippingIndexConfig("c", MinMaxSketch("a"),
                                               BloomFilterSketch("a", 0.01, 100)))
    assert st["path"] == "host" and st["columns"] == {"a": "host"}, st
    hs.createIndex(du, DataSkippingIndexConfig("u", MinMaxSketch("u"), MinMaxSketch("a")))
    assert st["path"] == "device" and st["columns"] == {"u": "host", "a": "device"}, st
    entry = [e for e in get_context(s).index_collection_manager.get_indexes() if e.name == "u"][0]
    t = DS.read_sketch_table(entry).sort_by("_data_file_id")
    assert t.column("MinMax_u__min").to_pylist() == [2 ** 31 + 1000 * i for i in range(3)]
    assert t.column("MinMax_a__max").to_pylist() == [1000 * i + 99 for i in range(3)]
    Hyperspace.enable(s)
    assert [tuple(r) for r in dc.filter(col("a") == 1005).select("a", "b").collect()] == \
        [(1005, 2010)]
    assert [os.path.basename(p) for p in DS.LAST_PRUNE["kept_paths"]] == ["part-00001.csv"]
    assert du.filter(col("u") >= 2 ** 31 + 2000).select("u", "a").count() == 100
    assert [os.path.basename(p) for p in DS.LAST_PRUNE["kept_paths"]] == ["part-00002.parquet"]
