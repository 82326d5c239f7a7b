"""Broadcast hash joins on the device, end to end: a session that leaves
``spark.sql.autoBroadcastJoinThreshold`` at its default, a 6000-row fact table (padded past the
threshold, with a covering index) and small dimension tables.  Every query is checked against
the host engine, must show ``BroadcastHashJoin`` in its executed plan and must have run
natively - on a build without the hash-join operator the path is ``"fallback"``."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import Hyperspace, IndexConfig, Session, col, count, sum_

from test_gpu_e2e import _both, _close

pytestmark = pytest.mark.gpu

N = 6000
FACT_COLS = ("f_id", "f_dim", "f_cat", "f_k2", "f_x", "f_q", "f_fk")


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from conftest import gpu_available
    if not gpu_available():
        pytest.skip("no GPU")
    root = tmp_path_factory.mktemp("bhj")
    rng = np.random.default_rng(11)
    f_dim = rng.integers(0, 60, N).astype(np.int32)         # 50 .. 59 have no dimension row
    fact = pa.table({
        "f_id": np.arange(N, dtype=np.int64),
        "f_dim": pa.array(f_dim, mask=rng.random(N) < 0.05),
        "f_cat": pa.array(rng.choice(["a", "b", "c", "d", "zz"], N)),
        "f_k2": rng.integers(0, 4, N).astype(np.int16),
        "f_x": np.round(rng.random(N) * 1000, 3),
        "f_q": rng.integers(0, 100, N).astype(np.int64),
        "f_fk": rng.integers(0, 20, N).astype(np.float64),
        # never read: it takes the files past the 10 MiB broadcast threshold, so the fact
        # table is the stream side whichever side of the join it stands on
        "f_pad": pa.array([rng.bytes(1000).hex() for _ in range(N)]),
    })
    dim = pa.table({
        "d_id": np.arange(50, dtype=np.int64),               # int64 against the fact's int32
        "d_name": pa.array([f"dim-{i % 7}" for i in range(50)]),
        "d_grp": (np.arange(50) % 5).astype(np.int32),
        "d_ngrp": pa.array((np.arange(50) % 3).astype(np.int32), mask=np.arange(50) % 4 == 0),
        "d_lo": np.linspace(0.0, 900.0, 50),
    })
    dd_id = rng.integers(0, 30, 80).astype(np.int32)
    dup = pa.table({"dd_id": pa.array(dd_id, mask=rng.random(80) < 0.1),
                    "dd_v": np.arange(80, dtype=np.int64)})
    dstr = pa.table({"s_cat": pa.array(["b", "c", "q", "a", "b"]),
                     "s_val": np.arange(5, dtype=np.int64) * 10})
    two = pa.table({"t_dim": np.repeat(np.arange(40, dtype=np.int32), 3),
                    "t_k2": np.tile(np.arange(3, dtype=np.int16), 40),
                    "t_w": np.arange(120, dtype=np.int64)})
    dflt = pa.table({"ff_id": np.arange(10, dtype=np.float64),
                     "ff_v": np.arange(10, dtype=np.int64)})
    grp = pa.table({"g_id": np.arange(5, dtype=np.int32),
                    "g_name": pa.array([f"g{i}" for i in range(5)])})
    paths = {}
    for name, t, parts in (("fact", fact, 3), ("dim", dim, 1), ("dup", dup, 2), ("dstr", dstr, 1),
                           ("two", two, 1), ("dflt", dflt, 1), ("grp", grp, 1)):
        os.makedirs(root / name)
        step = (t.num_rows + parts - 1) // parts
        for i in range(parts):
            pq.write_table(t.slice(i * step, step), root / name / f"part-{i}.parquet",
                           compression="none")
        paths[name] = str(root / name)
    assert sum(os.path.getsize(os.path.join(paths["fact"], f))
               for f in os.listdir(paths["fact"])) > 10 * 1024 * 1024
    s = Session(conf={"spark.hyperspace.system.path": str(root / "idx"),
                      "spark.hyperspace.index.numBuckets": "8",
                      "spark.sql.shuffle.partitions": "8",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(root / "wh"))
    hs = Hyperspace(s)
    hs.createIndex(s.read.parquet(paths["fact"]),
                   IndexConfig("f_idx", ["f_id"], [c for c in FACT_COLS if c != "f_id"]))
    Hyperspace.enable(s)
    dfs = {k: s.read.parquet(p) for k, p in paths.items()}
    dfs["fact"] = dfs["fact"].select(*FACT_COLS)
    return s, dfs


def _native(s, q, sort=True):
    g, c, path = _both(s, q, sort)
    assert "BroadcastHashJoin" in q.queryExecution.executed_plan.tree_string()
    assert path == "native", s.backend().fallback_reason
    _close(g, c)
    return g


def _metrics(s):
    return s.backend().metrics["hash_join"]


def test_inner_join_on_a_unique_dimension(env):
    s, d = env
    f, dim = d["fact"], d["dim"]
    q = f.join(dim, f["f_dim"] == dim["d_id"]).select("f_id", "f_x", "d_id", "d_name", "d_ngrp")
    g = _native(s, q)
    m = _metrics(s)
    assert m["unique"] is True and m["build_side"] == "right"
    assert m["build_rows"] == 50 and m["keys"] == 50 and 0 < m["probe_rows"] <= N
    assert m["pairs"] == g.num_rows and 0 < g.num_rows < N
    assert m["slots"] >= 2 * m["keys"]


def test_filter_on_the_indexed_column_below_the_join(env):
    s, d = env
    f, dim = d["fact"], d["dim"]
    q = f.filter("f_id >= 1000 AND f_id < 1500").join(dim, f["f_dim"] == dim["d_id"]) \
        .select("f_id", "d_name")
    g = _native(s, q)
    assert 0 < g.num_rows <= 500
    assert 0 < _metrics(s)["probe_rows"] <= 500


def test_dimension_with_duplicate_and_null_keys(env):
    s, d = env
    f, dup = d["fact"], d["dup"]
    q = f.join(dup, f["f_dim"] == dup["dd_id"]).select("f_id", "f_dim", "dd_id", "dd_v")
    g = _native(s, q)
    m = _metrics(s)
    assert m["unique"] is False and m["keys"] < m["build_rows"] < 80     # NULL keys left out
    assert g.num_rows > N


@pytest.mark.parametrize("table", ["dim", "dup"])
def test_left_join_pads_unmatched_fact_rows(env, table):
    s, d = env
    f, t = d["fact"], d[table]
    k, v = ("d_id", "d_name") if table == "dim" else ("dd_id", "dd_v")
    q = f.join(t, f["f_dim"] == t[k], "left").select("f_id", "f_dim", k, v)
    g = _native(s, q)
    assert g.num_rows >= N and g.column(k).null_count > 0
    # fact rows with a NULL key are kept, padded
    nullkeys = [r for r in g.to_pylist() if r["f_dim"] is None]
    assert nullkeys and all(r[k] is None for r in nullkeys)


@pytest.mark.parametrize("how", ["leftsemi", "leftanti"])
@pytest.mark.parametrize("table", ["dim", "dup"])
def test_left_semi_and_anti(env, how, table):
    s, d = env
    f, t = d["fact"], d[table]
    k = "d_id" if table == "dim" else "dd_id"
    q = f.join(t, f["f_dim"] == t[k], how).select("f_id", "f_dim", "f_x")
    g = _native(s, q)
    assert 0 < g.num_rows < N


@pytest.mark.parametrize("how", ["inner", "right"])
def test_small_table_on_the_left(env, how):
    s, d = env
    f, dup = d["fact"], d["dup"]
    q = dup.join(f, dup["dd_id"] == f["f_dim"], how).select("dd_v", "dd_id", "f_id", "f_dim")
    g = _native(s, q)
    assert _metrics(s)["build_side"] == "left"
    assert g.num_rows > N


def test_string_key_with_different_dictionaries(env):
    s, d = env
    f, ds = d["fact"], d["dstr"]
    for how in ("inner", "left", "leftanti"):
        q = f.join(ds, f["f_cat"] == ds["s_cat"], how)
        q = q.select("f_id", "f_cat") if how == "leftanti" else \
            q.select("f_id", "f_cat", "s_cat", "s_val")
        g = _native(s, q)
        assert g.num_rows > 0
    assert _metrics(s)["build_rows"] == 4          # "q" is not among the fact's strings


def test_two_column_key(env):
    s, d = env
    f, two = d["fact"], d["two"]
    on = (f["f_dim"] == two["t_dim"]) & (f["f_k2"] == two["t_k2"])
    for how in ("inner", "left"):
        g = _native(s, f.join(two, on, how).select("f_id", "f_dim", "f_k2", "t_w"))
        assert g.num_rows > 0
    assert _metrics(s)["unique"] is True


def test_filters_on_both_sides(env):
    s, d = env
    f, dim = d["fact"], d["dim"]
    q = f.filter("f_q > 10 AND f_x < 800").join(dim.filter("d_grp < 3"),
                                                f["f_dim"] == dim["d_id"], "left") \
        .select("f_id", "f_q", "d_id", "d_grp")
    g = _native(s, q)
    assert g.num_rows > 0 and _metrics(s)["build_rows"] == 30


def test_inner_join_with_a_residual_condition(env):
    s, d = env
    f, dim = d["fact"], d["dim"]
    q = f.join(dim, (f["f_dim"] == dim["d_id"]) & (f["f_x"] > dim["d_lo"])) \
        .select("f_id", "f_x", "d_lo")
    g = _native(s, q)
    assert 0 < g.num_rows < _metrics(s)["pairs"]


def test_aggregates_above_the_join(env):
    s, d = env
    f, dim = d["fact"], d["dim"]
    j = f.filter("f_q < 90").join(dim, f["f_dim"] == dim["d_id"])
    _native(s, j.agg(sum_("f_x").alias("sx"), count("*").alias("n")), sort=False)
    g = _native(s, j.groupBy("d_grp").agg(sum_("f_x").alias("sx"), count("*").alias("n")))
    assert g.num_rows == 5
    # a nullable group column: the hash-mode aggregate, which records the table size that held
    # the groups of a query shape (keyed by the group columns) once it has run
    be = s.backend()

    def hash_shapes():
        return [k for k in be.htables.sizes if k and k[0] == ("d_ngrp",)]
    assert not hash_shapes()
    g = _native(s, j.groupBy("d_ngrp").agg(sum_("f_q").alias("sq"), count("*").alias("n")))
    assert g.num_rows == 4 and g.column("d_ngrp").null_count == 1
    assert len(hash_shapes()) == 1


def test_order_by_limit_above_the_join(env):
    s, d = env
    f, dim = d["fact"], d["dim"]
    q = f.join(dim, f["f_dim"] == dim["d_id"]).select("f_id", "f_x", "d_name") \
        .orderBy(col("f_x").desc(), "f_id").limit(10)
    g = _native(s, q, sort=False)
    assert g.num_rows == 10


def test_create_dataframe_build_side(env):
    s, d = env
    f = d["fact"]
    look = s.createDataFrame({"c_id": np.arange(0, 60, 2, dtype=np.int32),
                              "c_tag": [f"t{i}" for i in range(30)]})
    g = _native(s, f.join(look, f["f_dim"] == look["c_id"]).select("f_id", "f_dim", "c_tag"))
    assert g.num_rows > 0 and _metrics(s)["unique"] is True
    g = _native(s, f.join(look, f["f_dim"] == look["c_id"], "leftanti").select("f_id", "f_dim"))
    assert g.num_rows > 0


def _odd_frame(s):
    """A ``createDataFrame`` table with columns of types the device does not hold."""
    return s.createDataFrame(pa.table({
        "c_id": pa.array(np.arange(0, 60, 3, dtype=np.int32)),
        "c_tags": pa.array([[i, i + 1] for i in range(20)], pa.list_(pa.int64())),
        "c_raw": pa.array([bytes([i]) for i in range(20)], pa.binary()),
        "c_none": pa.nulls(20),
        "c_name": pa.array([f"n{i % 4}" for i in range(20)])}))


def test_create_dataframe_without_a_join(env):
    s, _ = env
    look = _odd_frame(s)
    q = look.filter(col("c_id") > 10).select("c_id", "c_name")
    assert "LocalTableScan" in q.queryExecution.executed_plan.tree_string()
    g, c, path = _both(s, q)
    assert path == "native", s.backend().fallback_reason
    _close(g, c)
    assert g.num_rows == 16
    g, c, path = _both(s, look.groupBy("c_name").agg(sum_("c_id").alias("t"),
                                                     count("*").alias("n")))
    assert path == "native", s.backend().fallback_reason
    _close(g, c)
    assert g.num_rows == 4


def test_create_dataframe_column_the_device_does_not_hold(env):
    s, d = env
    f, look = d["fact"], _odd_frame(s)
    # never read: the join runs on the device
    g = _native(s, f.join(look, f["f_dim"] == look["c_id"]).select("f_id", "c_name"))
    assert g.num_rows > 0
    # read: the host engine answers, with the reason naming the column
    for q in (look.filter(col("c_id") > 10).select("c_id", "c_tags"),
              f.filter("f_id < 200").join(look, f["f_dim"] == look["c_id"])
              .select("f_id", "c_raw")):
        g, c, path = _both(s, q, sort=False)
        assert path == "fallback"
        assert "createDataFrame column c_" in s.backend().fallback_reason
        rows = [sorted(t.to_pylist(), key=lambda r: r[t.column_names[0]]) for t in (g, c)]
        assert g.num_rows > 0 and rows[0] == rows[1]


def test_build_side_emptied_by_its_filter(env):
    s, d = env
    f, dim = d["fact"], d["dim"].filter("d_grp > 100")
    g = _native(s, f.join(dim, f["f_dim"] == dim["d_id"]).select("f_id", "d_name"))
    assert g.num_rows == 0
    g = _native(s, f.join(dim, f["f_dim"] == dim["d_id"], "left").select("f_id", "d_name"))
    assert g.num_rows == N and g.column("d_name").null_count == N
    g = _native(s, f.join(dim, f["f_dim"] == dim["d_id"], "leftanti").select("f_id"))
    assert g.num_rows == N
    assert _metrics(s)["build_rows"] == 0


def test_two_broadcast_joins_chained(env):
    s, d = env
    f, dim, grp = d["fact"], d["dim"], d["grp"]
    j = f.join(dim, f["f_dim"] == dim["d_id"]).join(grp, dim["d_grp"] == grp["g_id"])
    q = j.select("f_id", "d_name", "g_name")
    assert q.queryExecution.executed_plan.tree_string().count("BroadcastHashJoin") == 2
    g = _native(s, q)
    assert g.num_rows > 0
    g = _native(s, j.groupBy("g_id").agg(sum_("f_x").alias("sx")))
    assert g.num_rows == 5


def _fallback(s, q, reason):
    g, c, path = _both(s, q)
    assert "BroadcastHashJoin" in q.queryExecution.executed_plan.tree_string()
    assert path == "fallback"
    assert reason in s.backend().fallback_reason, s.backend().fallback_reason
    _close(g, c)
    assert g.num_rows > 0


def test_float_key_runs_on_the_host(env):
    s, d = env
    f, t = d["fact"], d["dflt"]
    _fallback(s, f.join(t, f["f_fk"] == t["ff_id"]).select("f_id", "f_fk", "ff_v"),
              "broadcast hash join on a float or decimal key")


def test_left_join_with_a_residual_runs_on_the_host(env):
    s, d = env
    f, dim = d["fact"], d["dim"]
    q = f.join(dim, (f["f_dim"] == dim["d_id"]) & (f["f_x"] > dim["d_lo"]), "left") \
        .select("f_id", "f_x", "d_lo")
    _fallback(s, q, "broadcast hash join: residual condition on a left join")
