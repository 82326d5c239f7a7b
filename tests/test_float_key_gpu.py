"""An index sorted on a float64 column, queried through the MI355X executor: range pruning on the
sort key follows the kernels' bit total order (sign-bit NaN < -inf < -0.0 < +0.0 < +inf <
positive NaN) while the predicates are IEEE (-0.0 = +0.0, every NaN comparison false).  For an
index built on the device and one built on the host (one pyarrow-ordered file per bucket) every
predicate returns exactly the rows of the host executor.  GPU-only."""
import glob
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import Hyperspace, IndexConfig, Session, col
from order_ref import SPECIAL_F64

pytestmark = pytest.mark.gpu

N = 20_000
INF, NAN = float("inf"), float("nan")
PREDICATES = {
    "ge_zero": lambda f: f >= 0.0,
    "gt_zero": lambda f: f > 0.0,
    "le_negzero": lambda f: f <= -0.0,
    "lt_zero": lambda f: f < 0.0,
    "eq_zero": lambda f: f == 0.0,
    "gt_one": lambda f: f > 1.0,
    "lt_one": lambda f: f < 1.0,
    "le_inf": lambda f: f <= INF,
    "ge_neginf": lambda f: f >= -INF,
    "eq_nan": lambda f: f == NAN,
    "between_zeros": lambda f: f.between(-0.0, 0.0),
}


def _source():
    """f: the special values (about 100 rows each, so each lands in every bucket of the (f, g)
    index), nulls and random values; g: the second indexed column; v: the row number."""
    rng = np.random.default_rng(11)
    f = rng.normal(size=N) * 3
    pick = rng.random(N) < 0.07
    f[pick] = rng.choice(SPECIAL_F64, int(pick.sum()))
    return pa.table({"f": pa.array(f, mask=rng.random(N) < 0.03),
                     "g": rng.integers(0, 8, N).astype(np.int32),
                     "v": np.arange(N, dtype=np.int64)})


@pytest.fixture(scope="module")
def float_index(tmp_path_factory):
    """{build: (session, dataframe, system path)}: the same table indexed on (f, g) by the device
    builder and by the host builder, each in a session of its own."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = tmp_path_factory.mktemp("float_key")
    os.makedirs(root / "src")
    pq.write_table(_source(), root / "src" / "part-0.parquet")
    out = {}
    for build, kind in (("device", "gpu"), ("host", "cpu")):
        s = Session(conf={"spark.hyperspace.system.path": str(root / f"idx_{build}"),
                          "spark.hyperspace.index.numBuckets": "4",
                          "spark.sql.autoBroadcastJoinThreshold": "-1",
                          "spark.hyperspace.mi.execution.device": kind},
                    warehouse_dir=str(root / f"wh_{build}"))
        df = s.read.parquet(str(root / "src"))
        Hyperspace(s).createIndex(df, IndexConfig("fidx", ["f", "g"], ["v"]))
        s.conf.set("spark.hyperspace.mi.execution.device", "gpu")
        Hyperspace.enable(s)
        out[build] = (s, df, str(root / f"idx_{build}"))
    yield out
    for s, _, _ in out.values():
        s.disableHyperspace()


def _index_files(path):
    return sorted(glob.glob(os.path.join(path, "fidx", "v__=0", "*.parquet")))


def test_both_builds_hold_every_special_in_several_buckets(float_index):
    """Both builds hold every special value in several buckets; the host build is one
    pyarrow-written file per bucket, the device build is written by the device encoder."""
    from hyperspace_amd.exec.pq_encode import CREATED_BY
    for build in ("device", "host"):
        files = _index_files(float_index[build][2])
        assert len(files) == 4, files
        by_dev = [pq.ParquetFile(f).metadata.created_by == CREATED_BY for f in files]
        assert all(by_dev) if build == "device" else not any(by_dev)
        seen = np.zeros(len(SPECIAL_F64), int)
        for f in files:
            bits = pq.read_table(f).column("f").drop_null().to_numpy().view(np.uint64)
            seen += np.isin(SPECIAL_F64.view(np.uint64), bits)
        assert (seen >= 2).all(), seen


@pytest.mark.parametrize("name", sorted(PREDICATES))
@pytest.mark.parametrize("build", ["device", "host"])
def test_float_key_predicate_rows_equal_host_executor(float_index, device, build, name):
    s, df, _ = float_index[build]
    q = df.filter(PREDICATES[name](col("f"))).select("v", "f")
    s.conf.set("spark.hyperspace.mi.execution.device", "gpu")
    g = q.to_arrow()
    be = s.backend()
    assert be.last_path == "native", be.fallback_reason
    assert "Name: fidx" in q.queryExecution.executed_plan.tree_string()
    s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
    c = q.to_arrow()
    s.conf.set("spark.hyperspace.mi.execution.device", "gpu")
    got = np.sort(g.column("v").to_numpy())
    want = np.sort(c.column("v").to_numpy())
    print(f"{build} {name}: device rows {len(got)}, host rows {len(want)}")
    # the host executor's answer is the IEEE one, worked out here from the source
    f = _source().column("f")
    fv, ok = f.fill_null(0.0).to_numpy(), f.is_valid().to_numpy(zero_copy_only=False)
    with np.errstate(invalid="ignore"):
        ieee = {"ge_zero": fv >= 0, "gt_zero": fv > 0, "le_negzero": fv <= 0, "lt_zero": fv < 0,
                "eq_zero": fv == 0, "gt_one": fv > 1, "lt_one": fv < 1, "le_inf": fv <= INF,
                "ge_neginf": fv >= -INF, "eq_nan": fv == NAN,
                "between_zeros": (fv >= 0) & (fv <= 0)}[name] & ok
    assert np.array_equal(want, np.nonzero(ieee)[0])
    assert (len(want) == 0) if name == "eq_nan" else (0 < len(want) < N)
    assert np.array_equal(got, want), \
        (len(got), len(want), np.setdiff1d(got, want)[:5], np.setdiff1d(want, got)[:5])
    # the values come back bit for bit (both zeros, no NaN)
    order_g, order_c = np.argsort(g.column("v").to_numpy()), np.argsort(c.column("v").to_numpy())
    assert np.array_equal(g.column("f").to_numpy()[order_g].view(np.uint64),
                          c.column("f").to_numpy()[order_c].view(np.uint64))
