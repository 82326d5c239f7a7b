"""Z-order covering indexes in a GPU session: the device build (hs_zorder_keys + radix sort)
equals the host build row for row; filters on either or both indexed columns run the native
fused scans over the zone-pruned ranges (hs_zone_minmax + hs_zone_prune) with the results of
the Hyperspace-disabled run, and keep exactly the zones the oracle (tests/zorder_ref.py) keeps.

200 000 rows over 4 source files, index on (a, d), zones of 2048 rows: 98 zones."""
import datetime
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import zorder_ref as R
from helpers import index_names_used
from hyperspace_amd import (Hyperspace, Session, ZOrderCoveringIndexConfig, col, count,
                            get_context, sum_)

pytestmark = pytest.mark.gpu

N = 200_000
ZONE = 2048
NZ = -(-N // ZONE)
DAY0 = 10_000
EPOCH = datetime.date(1970, 1, 1)


def _day(v: int) -> datetime.date:
    return EPOCH + datetime.timedelta(days=int(v))


def _source(nulls: bool) -> pa.Table:
    rng = np.random.default_rng(7)
    a = rng.integers(0, 10 ** 6, N).astype(np.int32)
    d = (DAY0 + rng.integers(0, 2500, N)).astype(np.int32)
    f = rng.standard_normal(N)
    g = rng.integers(-10 ** 6, 10 ** 6, N)
    mask = rng.random(N) < 0.1 if nulls else None
    return pa.table({"a": pa.array(a, mask=mask), "d": pa.array(d, pa.int32()).view(pa.date32()),
                     "f": pa.array(f), "g": pa.array(g)})


@pytest.fixture(scope="module", params=[False, True], ids=["dense", "nulls"])
def env(request, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = tmp_path_factory.mktemp("zorder_gpu")
    src = str(root / "src")
    os.makedirs(src)
    t = _source(request.param)
    step = N // 4
    for i in range(4):
        pq.write_table(t.slice(i * step, step), os.path.join(src, f"part-{i:05d}.parquet"))
    s = Session(conf={"spark.hyperspace.system.path": str(root / "idx"),
                      "spark.hyperspace.index.zorder.filterRule.enabled": "true",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(root / "wh"))
    hs = Hyperspace(s)
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f", "g"]))
    Hyperspace.enable(s)
    rows = _index_rows(_entry(s))
    cols = [_storage(rows, "a"), _storage(rows, "d")]
    yield s, hs, src, root, R.zone_maps(cols, ZONE), request.param
    s.disableHyperspace()


def _entry(s):
    return [e for e in get_context(s).index_collection_manager.get_indexes() if e.name == "z"][0]


def _index_rows(entry) -> pa.Table:
    files = sorted(entry.content.files, key=os.path.basename)
    return pa.concat_tables([pq.read_table(f.replace("file:", "")) for f in files])


def _storage(t: pa.Table, name: str):
    c = t.column(name).combine_chunks()
    valid = None if c.null_count == 0 else np.asarray(c.is_valid())
    if pa.types.is_date32(c.type):
        c = c.view(pa.int32())
    return np.asarray(c.fill_null(0)), valid


def _img(v: int) -> int:
    return int(R.image(np.array([v], dtype=np.int32))[0])


def _run(s, df):
    """(arrow result, executor path, zone metrics) of one GPU execution."""
    be = s.backend()
    be.metrics.pop("scan_zones", None)
    be.metrics.pop("scan_zones_kept", None)
    out = df.to_arrow()
    kept = be.metrics.get("scan_zones_kept")
    return out, be.last_path, be.metrics.get("scan_zones"), None if kept is None else int(kept)


def _disabled(s, make):
    s.disableHyperspace()
    try:
        return make().to_arrow()
    finally:
        s.enableHyperspace()


def _same(got: pa.Table, want: pa.Table, rows: int):
    """Row sets equal; a float sum of at most ``rows`` values |f| < 6 in another order may differ
    by rows * 2^-53 * (6 * rows)."""
    assert got.column_names == want.column_names and got.num_rows == want.num_rows
    keys = [(n, "ascending") for n in got.column_names]
    if got.num_rows > 1:
        got, want = got.sort_by(keys), want.sort_by(keys)
    tol = rows * 1.2e-16 * 6 * rows
    for name in got.column_names:
        for x, y in zip(got.column(name).to_pylist(), want.column(name).to_pylist()):
            if name == "sf":
                assert abs(x - y) <= tol, (name, x, y, tol)
            else:
                assert x == y, (name, x, y)


def test_device_build_equals_host_build(env, tmp_path):
    from hyperspace_amd.exec.device_build import LAST_BUILD_STATS as st
    s, hs, src, root, _, _ = env
    assert "zorder_keys_sort_s" in st, st
    cpu = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx_cpu"),
                        "spark.hyperspace.mi.execution.device": "cpu"},
                  warehouse_dir=str(tmp_path / "wh"))
    Hyperspace(cpu).createIndex(cpu.read.parquet(src),
                                ZOrderCoveringIndexConfig("z", ["a", "d"], ["f", "g"]))
    got, want = _index_rows(_entry(s)), _index_rows(_entry(cpu))
    assert got.num_rows == want.num_rows == N
    for c in ("a", "d", "f", "g"):
        assert got.column(c).combine_chunks().equals(want.column(c).combine_chunks()), c
    t = pa.concat_tables([pq.read_table(os.path.join(src, f)) for f in sorted(os.listdir(src))])
    order = R.order([_storage(t, "a"), _storage(t, "d")])
    assert got.column("g").to_pylist() == t.column("g").take(pa.array(order)).to_pylist()


# 5 % of either column's range
A_LO, A_HI = 400_000, 450_000
D_LO, D_HI = DAY0 + 1100, DAY0 + 1225
FILTERS = {
    "a": (lambda: (col("a") >= A_LO) & (col("a") < A_HI),
          {0: (_img(A_LO), _img(A_HI - 1))}),
    "d": (lambda: (col("d") >= _day(D_LO)) & (col("d") < _day(D_HI)),
          {1: (_img(D_LO), _img(D_HI - 1))}),
    "both": (lambda: (col("a") >= A_LO) & (col("a") < A_HI) & (col("d") >= _day(D_LO)) &
             (col("d") < _day(D_HI)),
             {0: (_img(A_LO), _img(A_HI - 1)), 1: (_img(D_LO), _img(D_HI - 1))}),
}
# zones the oracle keeps of the 98, computed on the CPU for THIS generator (dense / 10 % nulls).
# The figures differ from the 19 / 45 / 7 quoted where the feature was specified: that generator's
# draw order and its 5 % windows are not known here (a window of `d` that straddles a 512-day
# boundary of the interleave keeps about twice as many zones).  What is asserted is what was
# asked: the oracle's count, at most half the zones, and exact equality with the device.
KEPT_REF = {False: {"a": 13, "d": 26, "both": 3}, True: {"a": 13, "d": 25, "both": 3}}
SHAPES = {
    "agg": lambda df: df.agg(sum_(col("f")).alias("sf"), sum_(col("g")).alias("sg"),
                             count("*").alias("n")),
    "rows": lambda df: df.select("a", "d", "g"),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("which", list(FILTERS))
def test_pruned_scan_equals_disabled_run(env, which, shape):
    s, hs, src, root, maps, nulls = env
    cond, intervals = FILTERS[which]
    make = lambda: SHAPES[shape](s.read.parquet(src).filter(cond()))      # noqa: E731
    ranges, kept_ref = R.prune(*maps, N, ZONE, intervals)
    print(f"zorder {which}/{shape}: reference keeps {kept_ref} of {NZ} zones, "
          f"{len(ranges)} ranges")
    assert kept_ref == KEPT_REF[nulls][which] and 0 < kept_ref <= NZ // 2
    q = make()
    assert index_names_used(q) == {"z"}
    assert "Hyperspace(Type: ZCI, Name: z" in q.queryExecution.executed_plan.tree_string()
    out = []
    hs.explain(q, redirectFunc=out.append)
    assert "z:" in "".join(out).split("Indexes used:")[1]
    got, path, zones, kept = _run(s, q)
    assert path == "native", s.backend().fallback_reason
    assert (zones, kept) == (NZ, kept_ref)
    _same(got, _disabled(s, make), N)
    assert got.num_rows > 0


def test_two_literal_vectors_back_to_back(env):
    s, hs, src, root, maps, nulls = env

    def make(lo, hi):
        return s.read.parquet(src).filter((col("a") >= lo) & (col("a") < hi)) \
            .agg(sum_(col("g")).alias("sg"), count("*").alias("n"))
    seen = []
    for _ in range(2):          # the second round runs on plan-cache hits
        for lo, hi in ((100_000, 120_000), (500_000, 700_000)):
            got, path, zones, kept = _run(s, make(lo, hi))
            assert path == "native", s.backend().fallback_reason
            _, want_kept = R.prune(*maps, N, ZONE, {0: (_img(lo), _img(hi - 1))})
            assert kept == want_kept
            _same(got, _disabled(s, lambda: make(lo, hi)), N)
            seen.append(kept)
    assert seen[0] != seen[1] and seen[:2] == seen[2:]


def test_prune_off_gives_identical_results(env):
    s, hs, src, root, maps, nulls = env
    cond, _ = FILTERS["both"]
    make = lambda: s.read.parquet(src).filter(cond()).select("a", "d", "f", "g")   # noqa: E731
    on, path, zones, kept = _run(s, make())
    assert path == "native" and kept is not None and kept < NZ
    s.conf.set("spark.hyperspace.mi.zorder.prune", "false")
    try:
        q = make()
        assert index_names_used(q) == {"z"}
        off, path, zones, kept = _run(s, q)
        assert path == "native", s.backend().fallback_reason
        assert zones is None and kept is None
    finally:
        s.conf.set("spark.hyperspace.mi.zorder.prune", "true")
    keys = [(n, "ascending") for n in on.column_names]
    assert on.sort_by(keys).equals(off.sort_by(keys))


def test_filter_on_included_column_keeps_source_scan(env):
    s, hs, src, root, maps, nulls = env
    q = s.read.parquet(src).filter(col("g") > 0).select("g")
    assert index_names_used(q) == set()


def test_null_and_in_predicates(env):
    """IS NULL constrains nothing (full ranges); IN prunes to the [min, max] of its list."""
    s, hs, src, root, maps, nulls = env
    make = lambda: s.read.parquet(src).filter(col("a").isNull()).select("d", "g")   # noqa: E731
    got, path, zones, kept = _run(s, make())
    assert path == "native" and kept is None
    _same(got, _disabled(s, make), N)
    make = lambda: s.read.parquet(src).filter(col("d").isin(_day(D_LO), _day(D_LO + 20))) \
        .agg(count("*").alias("n"))                                               # noqa: E731
    got, path, zones, kept = _run(s, make())
    assert path == "native", s.backend().fallback_reason
    _, want_kept = R.prune(*maps, N, ZONE, {1: (_img(D_LO), _img(D_LO + 20))})
    assert kept == want_kept and kept < NZ
    _same(got, _disabled(s, make), N)


def test_index_larger_than_cache_budget_is_not_streamed(device, tmp_path):
    """An index of F >= 2 key-range files whose estimated size exceeds the device cache budget:
    bucket-range streaming must not cut it into passes (each pass would scan the whole table
    and the results would come out multiplied)."""
    src = str(tmp_path / "src")
    os.makedirs(src)
    t = _source(False).slice(0, 60_000)
    for i in range(3):
        pq.write_table(t.slice(i * 20_000, 20_000), os.path.join(src, f"part-{i:05d}.parquet"))
    size = sum(os.path.getsize(os.path.join(src, f)) for f in os.listdir(src))
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.zorder.filterRule.enabled": "true",
                      "spark.hyperspace.index.zorder.targetSourceBytesPerPartition":
                      str(size // 3 + 1),
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    hs = Hyperspace(s)
    hs.createIndex(s.read.parquet(src), ZOrderCoveringIndexConfig("z", ["a", "d"], ["f", "g"]))
    e = _entry(s)
    assert e.num_buckets == 3 and len(e.content.files) == 3
    index_bytes = sum(f.size for f in e.content.file_infos)
    # a fresh session whose cache budget is far below the streaming estimate (4 x file bytes)
    s2 = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                       "spark.hyperspace.index.zorder.filterRule.enabled": "true",
                       "spark.hyperspace.mi.deviceCacheBytes": str(index_bytes),
                       "spark.hyperspace.mi.execution.device": "gpu"},
                 warehouse_dir=str(tmp_path / "wh2"))
    Hyperspace.enable(s2)
    for shape in SHAPES.values():
        make = lambda: shape(s2.read.parquet(src).filter(col("a") < 300_000))    # noqa: E731
        q = make()
        assert index_names_used(q) == {"z"}
        got = q.to_arrow()
        _same(got, _disabled(s2, make), 60_000)
        assert got.num_rows > 0
    s2.disableHyperspace()


def test_decimal_indexed_column_device_build_equals_host_build(device, tmp_path):
    import decimal
    rng = np.random.default_rng(11)
    n = 30_000
    cents = rng.integers(-10 ** 7, 10 ** 7, n)
    mask = rng.random(n) < 0.1
    t = pa.table({"p": pa.array([None if m else decimal.Decimal(int(c)) / 100
                                 for c, m in zip(cents, mask)], pa.decimal128(10, 2)),
                  "k": pa.array(rng.integers(0, 1000, n).astype(np.int16)),
                  "v": pa.array(rng.integers(0, 10 ** 9, n))})
    src = str(tmp_path / "src")
    os.makedirs(src)
    for i in range(2):
        pq.write_table(t.slice(i * n // 2, n // 2), os.path.join(src, f"part-{i:05d}.parquet"))
    rows = {}
    for dev in ("gpu", "cpu"):
        s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / f"idx_{dev}"),
                          "spark.hyperspace.mi.execution.device": dev},
                    warehouse_dir=str(tmp_path / f"wh_{dev}"))
        Hyperspace(s).createIndex(s.read.parquet(src),
                                  ZOrderCoveringIndexConfig("z", ["p", "k"], ["v"]))
        rows[dev] = _index_rows(_entry(s))
    assert rows["gpu"].num_rows == n
    for c in ("p", "k", "v"):
        assert rows["gpu"].column(c).to_pylist() == rows["cpu"].column(c).to_pylist(), c


def test_build_beyond_hbm_budget_takes_host_builder(device, tmp_path):
    """The device build is one pass: a source that does not fit the build's HBM budget is built
    by the host builder, with the same rows in the same order."""
    from hyperspace_amd.exec.device_build import LAST_BUILD_STATS as st
    src = str(tmp_path / "src")
    os.makedirs(src)
    t = _source(True).slice(0, 20_000)
    for i in range(2):
        pq.write_table(t.slice(i * 10_000, 10_000), os.path.join(src, f"part-{i:05d}.parquet"))
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.mi.build.hbmBudgetBytes": "100000",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    st.clear()
    Hyperspace(s).createIndex(s.read.parquet(src),
                              ZOrderCoveringIndexConfig("z", ["a", "d"], ["f", "g"]))
    est, budget = st["zorder_build_estimate"]
    assert est > budget and "zorder_keys_sort_s" not in st
    got = _index_rows(_entry(s))
    order = R.order([_storage(t, "a"), _storage(t, "d")])
    assert got.column("g").to_pylist() == t.column("g").take(pa.array(order)).to_pylist()
