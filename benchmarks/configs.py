#!/usr/bin/env python
"""The BASELINE.json configurations next to the headline benchmark (``bench.py``).

    python benchmarks/configs.py --config csv10k            # CPU plumbing, no GPU
    python benchmarks/configs.py --config sf10_filter       # 1 MI355X
    python benchmarks/configs.py --config hybrid --sf 100   # SF100 index + 10% appended files
    python benchmarks/configs.py --config q3_3way --sf 100  # three-way join
    python benchmarks/configs.py --config data_skipping --sf 10   # sketch build + file pruning
    python benchmarks/configs.py --config all

One JSON line per configuration on stdout.  Every configuration checks its indexed results
against the same query with Hyperspace disabled (the reference's correctness oracle,
``E2EHyperspaceRulesTest.scala:1004-1019``) and reports which executor path ran.

* ``csv10k`` — 10k-row CSV covering index + equality lookups on the host executor.
* ``sf10_filter`` — TPC-H SF10 ``lineitem`` FilterIndexRule (``l_shipdate`` range, Q6).
* ``hybrid`` — SF-N indexes, then +10% appended Parquet files in both tables: Q6 + Q3 through
  Hybrid Scan (BucketUnion on the device), an incremental refresh, and the same queries on the
  refreshed index.
* ``q3_3way`` — the TPC-H Q3 three-way join customer ⋈ orders ⋈ lineitem (JoinIndexRule on the
  customer/orders join, device shuffle of the intermediate onto the lineitem index layout).
* ``streamed`` — the SF-N index set built and queried under small HBM budgets (default 8 GB)
  against the resident run: bucket-range build passes and streamed queries.
* ``tpcds_3way`` — BASELINE config #5: TPC-DS-shaped ``store_sales`` ⋈ ``item`` ⋈ ``date_dim``
  (``hyperspace_amd.models.tpcds``, SF300 = 864M fact rows by default, ``--tpcds-sf``) with
  covering indexes on all three tables; queries, then +10% appended fact files and an
  incremental ``refreshIndex``, then the same queries on the refreshed index.  Results are
  checked against an independent pyarrow-dataset computation (not this engine's host path).
* ``like`` — ``p_name LIKE '%green%'``-style filters plus an aggregate over a ``part``-shaped
  table (200k x SF rows, every name distinct) through an index that includes the
  dictionary-coded name column; also times the dictionary match kernel against the host route
  (``match_like`` + pack + upload) at 10^4, 10^6 and all entries.
* ``count_distinct`` — ``count(DISTINCT x)`` over a synthetic table (200k x SF rows) under a
  range filter: ungrouped, grouped by one dictionary column (few groups, the dense level 2) and
  grouped by an integer column (>= 10^5 groups at SF >= 5, the hash level 2); q/s on the device
  against the host engine, the level-1 and level-2 kernel times and the level-2 shape that ran.
* ``window`` — window functions over TPC-H SF-N ``lineitem`` through an index on
  ``l_orderkey``: top-3 lines per order by price (``row_number``, filtered and aggregated), a
  running ``sum(l_quantity)`` per supplier by ship date, and a per-order total that needs no
  sort; q/s on the device against the host engine and whether the device sort was skipped.
* ``broadcast_join`` — ``lineitem`` (index on ``l_shipdate``) joined to small tables with the
  broadcast threshold at its default: ``supplier`` summed, grouped by nation, ``nation`` chained
  on top, and a left-anti join against a 1000-key local list; ms per query, the executor path
  and the hash-join metrics of each shape.  ``--probe-sweep`` instead times the probe kernel
  alone against a 25-key and a 1M-key table for 1 / 2 / 4 / 8 stream rows per lane.
* ``data_skipping`` — a data-skipping index (MinMax + Bloom sketches) over 128 source files:
  device and host sketch build, a range filter and a point lookup with and without the index,
  and the host cost of probing the sketches (``--sf 10`` for the recorded run).
* ``zorder`` — a Z-order covering index on ``lineitem (l_shipdate, l_suppkey)``
  (``--zorder-sf``, default 10): device and host ``createIndex``, zone-map build and prune pass,
  and 5 % range filters on either or both columns with the index, with pruning off, and with
  Hyperspace disabled (one session each, alternating).
* ``date_fns`` — date functions (``--date-sf``, default 10): the ``year(l_shipdate)`` projection
  against a same-byte arithmetic one, a Q8-style query grouped by ``extract(year FROM ...)``
  against one grouped by a stored column, and ``WHERE year(l_shipdate) = 1994`` with the range
  rewrite on and off; alternating runs, medians.
* ``case_when`` — conditional aggregates over the bench's lineitem / orders index pair
  (``--case-sf``, default 10): a Q12-style grouped join, a Q14-style ratio and an ungrouped
  Q6-style query, each as fused guards, as a hidden computed column, with the guard in WHERE
  and on the host engine (alternating runs, medians).
"""
import argparse
import datetime
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _session(root, device, buckets, **extra):
    from hyperspace_amd import Session
    conf = {"spark.hyperspace.system.path": os.path.join(root, "indexes"),
            "spark.hyperspace.index.numBuckets": str(buckets),
            "spark.sql.autoBroadcastJoinThreshold": "-1",
            "spark.sql.shuffle.partitions": str(buckets),
            "spark.hyperspace.mi.execution.device": device}
    conf.update(extra)
    return Session(conf=conf, warehouse_dir=os.path.join(root, "wh"))


def _sync(device):
    if device == "gpu":
        import torch
        torch.cuda.synchronize()


def _mark(device):
    """HS_CFG_MARK=1: a short spin kernel (``torch.cuda._sleep``) that brackets each timed loop
    in a kernel trace (gpu.sh cfgprof)."""
    if device == "gpu" and os.environ.get("HS_CFG_MARK"):
        import torch
        torch.cuda._sleep(1000)


def _timed_loop(fn, n, device):
    _mark(device)
    _sync(device)
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    _sync(device)
    el = time.perf_counter() - t0
    _mark(device)
    if os.environ.get("HS_CFG_CPROFILE"):     # where the host time of the loop goes
        import cProfile
        import io
        import pstats
        pr = cProfile.Profile()
        pr.enable()
        for i in range(n):
            fn(i)
        _sync(device)
        pr.disable()
        buf = io.StringIO()
        pstats.Stats(pr, stream=buf).sort_stats("cumulative").print_stats(45)
        print(f"[cprofile] {getattr(fn, '__name__', fn)} x{n}\n{buf.getvalue()}",
              file=sys.stderr, flush=True)
    return el


def _rows(df):
    return sorted(tuple(r) for r in df.collect())


def _close(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            if isinstance(u, float) or isinstance(v, float):
                if abs(u - v) > 1e-9 * max(1.0, abs(v)):
                    return False
            elif u != v:
                return False
    return True


# ------------------------------------------------------------------------------------ csv10k
def config_csv10k(args):
    import numpy as np
    import pyarrow as pa
    import pyarrow.csv as pacsv
    from hyperspace_amd import Hyperspace, IndexConfig, col
    root = os.path.join(args.data_dir, "csv10k")
    shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.join(root, "src"))
    rng = np.random.default_rng(7)
    n = 10_000
    queries = np.array(["donde", "facebook", "ibraco", "miperro", "google", "bing", "yahoo"])
    t = pa.table({"Date": pa.array([f"2019-10-{d:02d}" for d in rng.integers(1, 29, n)]),
                  "RGUID": pa.array([f"{x:08x}" for x in rng.integers(0, 2**32, n)]),
                  "Query": pa.array(queries[rng.integers(0, len(queries), n)]),
                  "imprs": pa.array(rng.integers(1, 1000, n).astype(np.int32)),
                  "clicks": pa.array(rng.integers(0, 100, n).astype(np.int64))})
    for i in range(4):
        pacsv.write_csv(t.slice(i * n // 4, n // 4), os.path.join(root, "src", f"part-{i}.csv"))
    s = _session(root, "cpu", 8)
    hs = Hyperspace(s)
    df = s.read.option("header", "true").csv(os.path.join(root, "src"))
    tb = time.perf_counter()
    hs.createIndex(df, IndexConfig("csvIdx", ["Query"], ["clicks", "imprs"]))
    build_s = time.perf_counter() - tb

    def q(i):
        return df.filter(col("Query") == str(queries[i % len(queries)])).select("Query", "clicks")
    Hyperspace.enable(s)
    used = "csvIdx" in q(0).queryExecution.executed_plan.tree_string()
    on = [_rows(q(i)) for i in range(len(queries))]
    dt_on = _timed_loop(lambda i: q(i).collect(), 50, "cpu")
    s.disableHyperspace()
    off = [_rows(q(i)) for i in range(len(queries))]
    dt_off = _timed_loop(lambda i: q(i).collect(), 50, "cpu")
    return {"config": "csv10k", "device": "cpu", "rows": n, "index_build_s": round(build_s, 4),
            "lookups_per_s_indexed": round(50 / dt_on, 2),
            "lookups_per_s_no_index": round(50 / dt_off, 2),
            "index_used": used, "match": all(_close(a, b) for a, b in zip(on, off))}


# ------------------------------------------------------------------------------------ TPC-H
def _tpch(args, sf, with_customer=False):
    from hyperspace_amd.models import tpch
    nfiles = max(8, int(round(sf * 1.28)))
    data = os.path.join(args.data_dir, f"tpch_sf{sf:g}_f{nfiles}")
    tpch.generate(data, sf, nfiles, workers=min(16, os.cpu_count() or 8))
    if with_customer:
        tpch.write_customers(data, sf, max(4, nfiles // 8))
    return data, nfiles


def _build(hs, df, cfg, device):
    from hyperspace_amd.exec import device_build
    _sync(device)
    t0 = time.perf_counter()
    hs.createIndex(df, cfg)
    _sync(device)
    dt = time.perf_counter() - t0
    nbytes = device_build.LAST_BUILD_STATS.get("source_bytes", 0) if device == "gpu" else 0
    return dt, nbytes


def _q6(li, i):
    from hyperspace_amd import col, sum_
    year = 1993 + i % 5
    disc = 0.02 + (i % 8) * 0.01
    lo, hi = datetime.date(year, 1, 1), datetime.date(year + 1, 1, 1)
    return li.filter((col("l_shipdate") >= lo) & (col("l_shipdate") < hi) &
                     (col("l_discount") >= round(disc - 0.01, 2)) &
                     (col("l_discount") <= round(disc + 0.01, 2)) &
                     (col("l_quantity") < 24 + (i % 2))) \
        .agg(sum_(col("l_extendedprice") * col("l_discount")).alias("revenue"))


def _q3(li, od, i):
    from hyperspace_amd import col, count, sum_
    dd = datetime.date(1995, 3, 1) + datetime.timedelta(days=(i * 7) % 30)
    j = li.join(od, li["l_orderkey"] == od["o_orderkey"]) \
        .filter((col("o_orderdate") < dd) & (col("l_shipdate") > dd))
    return j.groupBy("o_shippriority").agg(
        sum_(col("l_extendedprice") * (1 - col("l_discount"))).alias("revenue"),
        count("*").alias("lines"))


def config_sf10_filter(args):
    from hyperspace_amd import Hyperspace, IndexConfig
    sf = 10.0
    data, _ = _tpch(args, sf)
    root = os.path.join(args.data_dir, "cfg_sf10")
    shutil.rmtree(root, ignore_errors=True)
    s = _session(root, args.device, args.buckets)
    hs = Hyperspace(s)
    li = s.read.parquet(os.path.join(data, "lineitem"))
    dt, nbytes = _build(hs, li, IndexConfig("li_shipdate", ["l_shipdate"],
                                            ["l_discount", "l_quantity", "l_extendedprice"]),
                        args.device)
    Hyperspace.enable(s)
    for i in range(3):
        _q6(li, 1000 + i).collect()
    k = args.steps * 5
    el = _timed_loop(lambda i: _q6(li, i).collect(), k, args.device)
    path = getattr(s.backend(), "last_path", None)
    got = _q6(li, 0).collect()[0][0]
    s.disableHyperspace()
    ref = _q6(li, 0).collect()[0][0]
    return {"config": "sf10_filter", "device": args.device, "queries_per_s": round(k / el, 2),
            "q6_ms": round(el / k * 1e3, 3), "index_build_s": round(dt, 3),
            "index_build_gbps": round(nbytes / dt / 1e9, 3) if nbytes else None,
            "path": path, "match": abs(got - ref) <= 1e-9 * abs(ref)}


def config_hybrid(args):
    import pyarrow.parquet as pq  # noqa: F401
    from hyperspace_amd import Hyperspace, IndexConfig
    from hyperspace_amd.models import tpch
    sf = args.sf
    data, nfiles = _tpch(args, sf)
    # a private copy: appending files must not disturb the shared generated data set
    work = os.path.join(args.data_dir, f"cfg_hybrid_sf{sf:g}")
    shutil.rmtree(work, ignore_errors=True)
    for t in ("lineitem", "orders"):
        os.makedirs(os.path.join(work, "data", t))
        for f in os.listdir(os.path.join(data, t)):
            os.link(os.path.join(data, t, f), os.path.join(work, "data", t, f))
    s = _session(work, args.device, args.buckets,
                 **{"spark.hyperspace.index.lineage.enabled": "true",
                    "spark.hyperspace.index.hybridscan.enabled": "true",
                    "spark.hyperspace.index.hybridscan.maxAppendedRatio": "0.3"})
    hs = Hyperspace(s)
    lpath, opath = os.path.join(work, "data", "lineitem"), os.path.join(work, "data", "orders")
    li, od = s.read.parquet(lpath), s.read.parquet(opath)
    builds = {}
    for df, cfg in ((li, IndexConfig("li_orderkey", ["l_orderkey"],
                                     ["l_extendedprice", "l_discount", "l_shipdate"])),
                    (od, IndexConfig("ord_orderkey", ["o_orderkey"],
                                     ["o_orderdate", "o_shippriority"])),
                    (li, IndexConfig("li_shipdate", ["l_shipdate"],
                                     ["l_discount", "l_quantity", "l_extendedprice"]))):
        builds[cfg.indexName] = round(_build(hs, df, cfg, args.device)[0], 3)
    # +10%: chunks nfiles.. extend the key domain (fresh orders and their lineitems)
    extra = max(1, nfiles // 10)
    for i in range(nfiles, nfiles + extra):
        tpch.write_chunk(os.path.join(work, "data"), sf, nfiles, i)
    Hyperspace.enable(s)
    li, od = s.read.parquet(lpath), s.read.parquet(opath)

    def step(i):
        _q6(li, i).collect()
        _q3(li, od, i).collect()
    plan = _q3(li, od, 0).queryExecution.executed_plan.tree_string()
    for i in range(2):
        step(1000 + i)
    from hyperspace_amd.utils.tracing import TRACER, format_report
    TRACER.reset()
    el_h = _timed_loop(step, args.steps, args.device)
    path_h = getattr(s.backend(), "last_path", None)
    merge_skip = getattr(s.backend(), "metrics", {}).get("hybrid_merge_skip")
    print(f"[hybrid] merged union skipped: {merge_skip}", file=sys.stderr, flush=True)
    if TRACER.profile:   # the filter query's plan and whether its scan pruned key ranges
        q6p = _q6(li, 0)
        q6p.collect()
        print(q6p.queryExecution.executed_plan.tree_string()[:3000], file=sys.stderr, flush=True)
        print(f"[hybrid] q6 metrics {getattr(s.backend(), 'metrics', {})}", file=sys.stderr,
              flush=True)
    if TRACER.profile:   # HS_PROFILE=1: where the Hybrid Scan steps spend their time
        print("[hybrid] hybrid-scan stage profile\n" + format_report(TRACER.report()),
              file=sys.stderr, flush=True)
        print(plan, file=sys.stderr, flush=True)
    hyb = (_q6(li, 0).collect()[0][0], _rows(_q3(li, od, 0)))
    tr = time.perf_counter()
    for name in ("li_orderkey", "ord_orderkey", "li_shipdate"):
        t1 = time.perf_counter()
        hs.refreshIndex(name, "incremental")
        _sync(args.device)
        st = {}
        if args.device == "gpu":
            from hyperspace_amd.exec import device_build
            st = {k: v for k, v in device_build.LAST_BUILD_STATS.items()
                  if isinstance(v, (int, float, str))}
        print(f"[hybrid] refresh {name}: {time.perf_counter() - t1:.3f}s {st}", file=sys.stderr,
              flush=True)
    _sync(args.device)
    refresh_s = time.perf_counter() - tr
    li, od = s.read.parquet(lpath), s.read.parquet(opath)
    for i in range(2):
        step(2000 + i)
    TRACER.reset()
    be = s.backend()
    cache0 = (be.cache.hits, be.cache.misses) if hasattr(be, "cache") else (0, 0)
    el_r = _timed_loop(step, args.steps, args.device)
    cache1 = (be.cache.hits, be.cache.misses, round(be.cache.resident_bytes / 1e9, 1)) \
        if hasattr(be, "cache") else (0, 0, 0)
    print(f"[hybrid] refreshed loop device cache hits/misses {cache0} -> {cache1}",
          file=sys.stderr, flush=True)
    if TRACER.profile:   # HS_PROFILE=1: where the refreshed-index steps spend their time
        print("[hybrid] refreshed stage profile\n" + format_report(TRACER.report()),
              file=sys.stderr, flush=True)
        for q in (_q6(li, 0), _q3(li, od, 0)):
            print(q.queryExecution.executed_plan.tree_string(), file=sys.stderr, flush=True)
    ref = (_q6(li, 0).collect()[0][0], _rows(_q3(li, od, 0)))
    match = abs(hyb[0] - ref[0]) <= 1e-9 * abs(ref[0]) and _close(hyb[1], ref[1])
    return {"config": "hybrid", "device": args.device, "sf": sf, "appended_files": extra,
            "hybrid_queries_per_s": round(2 * args.steps / el_h, 2),
            "refreshed_queries_per_s": round(2 * args.steps / el_r, 2),
            "incremental_refresh_s": round(refresh_s, 3), "index_build_s": builds,
            "bucket_union_in_plan": "BucketUnion" in plan, "path": path_h,
            "hybrid_merge_skip": merge_skip,
            "hybrid_matches_refreshed": bool(match)}


def config_q3_3way(args):
    from hyperspace_amd import Hyperspace, IndexConfig, col, count, sum_
    sf = args.sf
    data, _ = _tpch(args, sf, with_customer=True)
    root = os.path.join(args.data_dir, f"cfg_q3_sf{sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    s = _session(root, args.device, args.buckets)
    hs = Hyperspace(s)
    c = s.read.parquet(os.path.join(data, "customer"))
    o = s.read.parquet(os.path.join(data, "orders"))
    li = s.read.parquet(os.path.join(data, "lineitem"))
    builds = {}
    for df, cfg in ((c, IndexConfig("cust", ["c_custkey"], ["c_mktsegment"])),
                    (o, IndexConfig("ord_cust", ["o_custkey"],
                                    ["o_orderkey", "o_orderdate", "o_shippriority"])),
                    # the orders-key index the 2-way Q3 joins: the executor's co-partitioned
                    # semi-join reads it for the (customer x orders) x lineitem join
                    (o, IndexConfig("ord_orderkey", ["o_orderkey"],
                                    ["o_custkey", "o_orderdate", "o_shippriority"])),
                    (li, IndexConfig("li_orderkey", ["l_orderkey"],
                                     ["l_extendedprice", "l_discount", "l_shipdate"]))):
        builds[cfg.indexName] = round(_build(hs, df, cfg, args.device)[0], 3)
    segs = ["BUILDING", "AUTOMOBILE", "MACHINERY", "HOUSEHOLD", "FURNITURE"]

    def q(i):
        d = datetime.date(1995, 3, 1) + datetime.timedelta(days=(i * 7) % 30)
        co = c.join(o, c["c_custkey"] == o["o_custkey"]) \
            .filter((col("c_mktsegment") == segs[i % 5]) & (col("o_orderdate") < d))
        return co.join(li, co["o_orderkey"] == li["l_orderkey"]).filter(col("l_shipdate") > d) \
            .agg(sum_(col("l_extendedprice") * (1 - col("l_discount"))).alias("revenue"),
                 count("*").alias("lines"))
    Hyperspace.enable(s)
    plan = q(0).queryExecution.executed_plan.tree_string()
    for i in range(2):
        q(1000 + i).collect()
    k = max(3, args.steps // 2)
    from hyperspace_amd.utils.tracing import TRACER, format_report
    TRACER.reset()
    el = _timed_loop(lambda i: q(i).collect(), k, args.device)
    semi = getattr(s.backend(), "last_semi_join", None)
    if TRACER.profile:   # HS_PROFILE=1: where the 3-way join's time goes
        print("[q3_3way] stage profile\n" + format_report(TRACER.report()), file=sys.stderr,
              flush=True)
        print(plan, file=sys.stderr, flush=True)
    path = getattr(s.backend(), "last_path", None)
    reason = getattr(s.backend(), "fallback_reason", None)
    got = _rows(q(0))
    s.disableHyperspace()
    t0 = time.perf_counter()
    ref = _rows(q(0))
    noidx_s = time.perf_counter() - t0
    return {"config": "q3_3way", "device": args.device, "sf": sf,
            "queries_per_s": round(k / el, 3), "q3_3way_ms": round(el / k * 1e3, 2),
            "no_index_query_s": round(noidx_s, 3), "index_build_s": builds,
            "indexes_in_plan": [n for n in ("cust", "ord_cust", "li_orderkey") if n in plan],
            "path": path, "fallback_reason": reason, "match": _close(got, ref),
            "semi_join": semi}


def config_streamed(args):
    """SURVEY §5.7 / BASELINE config #5's "beyond one GPU's HBM": the bench's SF-N index set
    built and queried under small HBM budgets (``--hbm-budget-gb``, default 8 GB for the build
    working set, ``build.hbmBudgetBytes``, and for resident index tables, ``deviceCacheBytes``)
    against the resident run on the same files: a build in bucket-range passes (GB/s), then Q6
    and Q3 that stream their index scans bucket range by bucket range (q/s).  Every streamed
    result must equal the resident one (itself the engine's oracle-checked path)."""
    from hyperspace_amd import Hyperspace, IndexConfig
    sf = args.sf
    data, _ = _tpch(args, sf)
    budget = int(args.hbm_budget_gb * (1 << 30))
    li_cfgs = (IndexConfig("li_shipdate", ["l_shipdate"],
                           ["l_discount", "l_quantity", "l_extendedprice"]),
               IndexConfig("li_orderkey", ["l_orderkey"],
                           ["l_extendedprice", "l_discount", "l_shipdate"]))
    od_cfg = IndexConfig("ord_orderkey", ["o_orderkey"], ["o_orderdate", "o_shippriority"])
    out = {"config": "streamed", "device": args.device, "sf": sf,
           "hbm_budget_gb": args.hbm_budget_gb}
    results = {}
    for mode in ("resident", "streamed"):
        root = os.path.join(args.data_dir, f"cfg_stream_{mode}")
        shutil.rmtree(root, ignore_errors=True)
        extra = {}
        if mode == "streamed":
            extra = {"spark.hyperspace.mi.build.hbmBudgetBytes": str(budget)}
        s = _session(root, args.device, args.buckets, **extra)
        hs = Hyperspace(s)
        li = s.read.parquet(os.path.join(data, "lineitem"))
        od = s.read.parquet(os.path.join(data, "orders"))
        from hyperspace_amd.exec import device_build
        bt, bb, passes = 0.0, 0, {}
        for df, cfg in ((li, li_cfgs[0]), (li, li_cfgs[1]), (od, od_cfg)):
            dt, nb = _build(hs, df, cfg, args.device)
            bt += dt
            bb += nb
            passes[cfg.indexName] = device_build.LAST_BUILD_STATS.get("passes", 1)
        if mode == "streamed":
            s.conf.set("spark.hyperspace.mi.deviceCacheBytes", str(budget))
        Hyperspace.enable(s)

        def step(i):
            _q6(li, i).collect()
            _q3(li, od, i).collect()
        for i in range(2):
            step(1000 + i)
        be = s.backend()
        el = _timed_loop(step, args.steps, args.device)
        res = [(_q6(li, i).collect()[0][0], _rows(_q3(li, od, i))) for i in range(3)]
        results[mode] = res
        out[mode] = {"queries_per_s": round(2 * args.steps / el, 2),
                     "index_build_s": round(bt, 3),
                     "index_build_gbps": round(bb / bt / 1e9, 3) if bb else None,
                     "build_passes": passes, "path": getattr(be, "last_path", None),
                     "stream_passes": getattr(be, "last_stream_passes", None)}
        # the next mode's session starts from an empty device
        del s, hs, be
        if args.device == "gpu":
            from hyperspace_amd.exec.gpu import release_process_device_memory
            release_process_device_memory()
    a, b = results["resident"], results["streamed"]
    out["match"] = all(abs(x[0] - y[0]) <= 1e-9 * abs(x[0]) and _close(x[1], y[1])
                       for x, y in zip(a, b))
    out["streamed_vs_resident_qps"] = round(out["streamed"]["queries_per_s"] /
                                            out["resident"]["queries_per_s"], 3)
    out["streamed_vs_resident_build"] = round(out["resident"]["index_build_s"] /
                                              out["streamed"]["index_build_s"], 3)
    return out


# ------------------------------------------------------------------------------------ TPC-DS
def _tpcds_query(ss, it, dd, i):
    """TPC-DS Q3-shaped star join: one manufacturer's items sold in one month of the year."""
    from hyperspace_amd import col, count, sum_
    m, moy = 1 + (i * 37) % 1000, 1 + i % 12
    items = it.filter(col("i_manufact_id") == m)
    days = dd.filter(col("d_moy") == moy)
    j = ss.join(items, ss["ss_item_sk"] == items["i_item_sk"])
    j = j.join(days, j["ss_sold_date_sk"] == days["d_date_sk"])
    return j.agg(sum_(col("ss_ext_sales_price")).alias("sales"), count("*").alias("lines"))


def _tpcds_oracle(paths, i):
    """The query computed independently with pyarrow datasets (filter pushdown, no join)."""
    import pyarrow.compute as pc
    import pyarrow.dataset as ds
    import pyarrow.parquet as pq
    m, moy = 1 + (i * 37) % 1000, 1 + i % 12
    it = pq.read_table(paths["item"], columns=["i_item_sk", "i_manufact_id"])
    items = it.filter(pc.equal(it["i_manufact_id"], m))["i_item_sk"]
    dd = pq.read_table(paths["date_dim"], columns=["d_date_sk", "d_moy"])
    days = dd.filter(pc.equal(dd["d_moy"], moy))["d_date_sk"]
    t = ds.dataset(paths["store_sales"], format="parquet").to_table(
        columns=["ss_ext_sales_price"],
        filter=ds.field("ss_item_sk").isin(items) & ds.field("ss_sold_date_sk").isin(days))
    return [(float(pc.sum(t["ss_ext_sales_price"]).as_py() or 0.0), t.num_rows)]


def config_tpcds_3way(args):
    from hyperspace_amd import Hyperspace, IndexConfig
    from hyperspace_amd.models import tpcds
    sf = args.tpcds_sf
    nfiles = max(4, int(round(sf * 1.28)))
    data = os.path.join(args.data_dir, f"tpcds_sf{sf:g}_f{nfiles}")
    tg = time.perf_counter()
    tpcds.generate(data, sf, nfiles, workers=min(16, os.cpu_count() or 8))
    gen_s = time.perf_counter() - tg
    work = os.path.join(args.data_dir, f"cfg_tpcds_sf{sf:g}")
    shutil.rmtree(work, ignore_errors=True)
    for t in ("store_sales", "item", "date_dim"):       # private links: appends stay local
        os.makedirs(os.path.join(work, "data", t))
        for f in os.listdir(os.path.join(data, t)):
            os.link(os.path.join(data, t, f), os.path.join(work, "data", t, f))
    paths = {t: os.path.join(work, "data", t) for t in ("store_sales", "item", "date_dim")}
    s = _session(work, args.device, args.buckets)
    hs = Hyperspace(s)
    ss, it, dd = (s.read.parquet(paths[t]) for t in ("store_sales", "item", "date_dim"))
    builds = {}
    for df, cfg in ((ss, IndexConfig("ss_item", ["ss_item_sk"],
                                     ["ss_sold_date_sk", "ss_ext_sales_price"])),
                    (it, IndexConfig("item_idx", ["i_item_sk"], ["i_manufact_id"])),
                    (dd, IndexConfig("date_idx", ["d_date_sk"], ["d_moy"]))):
        builds[cfg.indexName] = round(_build(hs, df, cfg, args.device)[0], 3)
    Hyperspace.enable(s)
    k = max(3, args.steps)

    def run_queries(tag):
        ss_, it_, dd_ = (s.read.parquet(paths[t]) for t in ("store_sales", "item", "date_dim"))
        plan = _tpcds_query(ss_, it_, dd_, 0).queryExecution.executed_plan.tree_string()
        for i in range(2):
            _tpcds_query(ss_, it_, dd_, 1000 + i).collect()
        from hyperspace_amd.utils.tracing import TRACER, format_report
        TRACER.reset()
        el = _timed_loop(lambda i: _tpcds_query(ss_, it_, dd_, i).collect(), k, args.device)
        if TRACER.profile:   # HS_PROFILE=1: where the star join's time goes
            print(f"[tpcds_3way:{tag}] stage profile\n" + format_report(TRACER.report()),
                  file=sys.stderr, flush=True)
            print(plan, file=sys.stderr, flush=True)
        got = _rows(_tpcds_query(ss_, it_, dd_, 0))
        ref = _tpcds_oracle(paths, 0)
        return {f"{tag}_queries_per_s": round(k / el, 3), f"{tag}_query_ms": round(el / k * 1e3, 2),
                f"{tag}_match": _close(got, ref), f"{tag}_lines": got[0][1] if got else None,
                f"{tag}_indexes_in_plan": [n for n in ("ss_item", "item_idx", "date_idx")
                                           if n in plan],
                f"{tag}_path": getattr(s.backend(), "last_path", None)}
    out = {"config": "tpcds_3way", "device": args.device, "sf": sf,
           "store_sales_rows": tpcds.store_sales_rows(sf), "source_files": nfiles,
           "datagen_s": round(gen_s, 2), "index_build_s": builds}
    out.update(run_queries("base"))
    # +10% fact rows: new files with the same domains, then an incremental refresh
    extra = max(1, nfiles // 10)
    tpcds.write_store_sales_files(os.path.join(work, "data"), sf, nfiles, first=nfiles,
                                  count=extra, workers=min(16, os.cpu_count() or 8))
    _sync(args.device)
    tr = time.perf_counter()
    hs.refreshIndex("ss_item", "incremental")
    _sync(args.device)
    out["appended_files"] = extra
    out["incremental_refresh_s"] = round(time.perf_counter() - tr, 3)
    out.update(run_queries("refreshed"))
    return out


# -------------------------------------------------------------------------------------- LIKE
_COLORS = ("almond antique aquamarine azure beige bisque black blanched blue blush brown "
           "burlywood burnished chartreuse chiffon chocolate coral cornflower cornsilk cream "
           "cyan dark deep dim dodger drab firebrick floral forest frosted gainsboro ghost "
           "goldenrod green grey honeydew hot indian ivory khaki lace lavender lawn lemon light "
           "lime linen magenta maroon medium metallic midnight mint misty moccasin navajo navy "
           "olive orange orchid pale papaya peach peru pink plum powder puff purple red rose "
           "rosy royal saddle salmon sandy seashell sienna sky slate smoke snow spring steel "
           "tan thistle tomato turquoise violet wheat white yellow").split()


def _part_table(n, seed=17):
    """A TPC-H ``part``-shaped table: ``p_name`` is five colour words and the part key, so
    every name is distinct (the dictionary has ``n`` entries)."""
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    rng = np.random.default_rng(seed)
    colors = pa.array(_COLORS)
    words = [colors.take(pa.array(rng.integers(0, len(_COLORS), n).astype(np.int32)))
             for _ in range(5)]
    key = np.arange(n, dtype=np.int64)
    name = pc.binary_join_element_wise(*words, pc.cast(pa.array(key), pa.string()), " ")
    return pa.table({"p_partkey": key, "p_name": name,
                     "p_size": rng.integers(1, 51, n).astype(np.int32),
                     "p_retailprice": np.round(900 + rng.random(n) * 1200, 2)})


def _median_ms(fn, runs, device):
    ts = []
    for _ in range(runs):
        _sync(device)
        t0 = time.perf_counter()
        fn()
        _sync(device)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 4)


def config_like(args):
    """``p_name LIKE '%green%'`` plus an aggregate over a part-shaped table (200k x SF rows)
    whose name column is dictionary-coded and included in a ``p_size`` index: q/s on the
    device against the host engine, and the dictionary match itself - the ``hs_dict_like``
    kernel against the host route (``match_like`` + pack + upload) at 10^4, 10^6 and all
    entries, medians of ``--like-runs`` alternating runs."""
    import pyarrow.parquet as pq
    from hyperspace_amd import Hyperspace, IndexConfig, col, count, sum_
    n = int(200_000 * args.sf)
    root = os.path.join(args.data_dir, f"cfg_like_sf{args.sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.join(root, "part"))
    t = _part_table(n)
    nfiles = 8
    step = (n + nfiles - 1) // nfiles
    for i in range(nfiles):
        pq.write_table(t.slice(i * step, step), os.path.join(root, "part", f"part-{i}.parquet"))
    del t
    s = _session(root, args.device, args.buckets)
    hs = Hyperspace(s)
    part = s.read.parquet(os.path.join(root, "part"))
    dt, _ = _build(hs, part, IndexConfig("part_size", ["p_size"], ["p_name", "p_retailprice"]),
                   args.device)
    Hyperspace.enable(s)
    pats = ["%green%", "%dark%rose%", "forest%", "%_lmond %", "%99"]

    def q(i):
        return part.filter((col("p_size") >= 1 + i % 3) & col("p_name").like(pats[i % len(pats)])) \
            .agg(sum_("p_retailprice").alias("price"), count("*").alias("n"))
    used = "part_size" in q(0).queryExecution.executed_plan.tree_string()
    got = [_rows(q(i)) for i in range(len(pats))]
    path = getattr(s.backend(), "last_path", None)
    reason = getattr(s.backend(), "fallback_reason", None)
    k = args.steps * 5
    el = _timed_loop(lambda i: q(i).collect(), k, args.device)
    out = {"config": "like", "device": args.device, "sf": args.sf, "rows": n,
           "index_build_s": round(dt, 3), "index_used": used, "path": path,
           "fallback_reason": reason, "queries_per_s": round(k / el, 2)}
    if args.device == "gpu":
        from hyperspace_amd.exec import like as LK
        from hyperspace_amd.ops import kernels as K
        import torch
        out["like_stats"] = dict(LK.LIKE_STATS)
        # the dictionary the queries matched: the resident index table's p_name column
        dicts = [d.dictionary for d in LK._DEV_DICTS.values()]
        full = max(dicts, key=len)
        prog = LK.compile_like("%green%")
        dev = torch.device("cuda", torch.cuda.current_device())
        sizes = sorted({min(10_000, len(full)), min(1_000_000, len(full)), len(full)})
        out["dict_match"] = []
        for m in sizes:
            d = full.slice(0, m)
            tu0 = time.perf_counter()
            dd = LK.device_dictionary(d, dev)
            _sync("gpu")
            upload_ms = (time.perf_counter() - tu0) * 1e3
            kw = K.dict_like(dd, prog)
            hw = torch.from_numpy(LK.host_bitmap_words(d, prog.pattern)).to(dev)
            same = bool(torch.equal(kw, hw))
            kt, ht = [], []
            for _ in range(args.like_runs):          # alternating, one run each
                kt.append(_median_ms(lambda: K.dict_like(dd, prog), 1, "gpu"))
                ht.append(_median_ms(lambda: torch.from_numpy(
                    LK.host_bitmap_words(d, prog.pattern)).to(dev), 1, "gpu"))
            kt.sort()
            ht.sort()
            out["dict_match"].append({
                "entries": m, "mean_entry_bytes": round(int(dd.chars.numel()) / max(m, 1), 2),
                "max_entry_bytes": dd.max_len, "runs": args.like_runs,
                "hs_dict_like_ms": kt[len(kt) // 2], "host_route_ms": ht[len(ht) // 2],
                "hs_dict_like_ms_min_max": [kt[0], kt[-1]], "host_route_ms_min_max": [ht[0], ht[-1]],
                "dictionary_upload_once_ms": round(upload_ms, 3), "bitmaps_equal": same})
    # the host engine on the same queries (and the cross-check)
    s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
    ref = [_rows(q(i)) for i in range(len(pats))]
    kh = max(3, args.steps)
    el_h = _timed_loop(lambda i: q(i).collect(), kh, "cpu")
    out["host_engine_queries_per_s"] = round(kh / el_h, 3)
    out["match"] = all(_close(a, b) for a, b in zip(got, ref))
    out["matching_rows"] = [g[0][1] for g in got]
    return out


def config_case_when(args):
    """Conditional aggregates over the lineitem / orders index pair of the bench (TPC-H SF
    ``--case-sf``): a Q12-style grouped join query, a Q14-style ratio over the join and an
    ungrouped Q6-style single-table query.  Each is cross-checked against the host engine and
    timed four ways: fused guards (``condAgg.fused`` on), the CASE as a hidden computed column
    (off) - alternating pairs in one process, medians of ``--case-runs`` - the same query with
    the guard moved into WHERE (it reads the same columns without the feature: a floor), and the
    host engine."""
    from hyperspace_amd import Hyperspace, IndexConfig
    sf = args.case_sf
    data, _ = _tpch(args, sf)
    root = os.path.join(args.data_dir, f"cfg_case_when_sf{sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    s = _session(root, args.device, args.buckets)
    hs = Hyperspace(s)
    li = s.read.parquet(os.path.join(data, "lineitem"))
    od = s.read.parquet(os.path.join(data, "orders"))
    for df, cfg in ((li, IndexConfig("li_shipdate", ["l_shipdate"],
                                     ["l_discount", "l_quantity", "l_extendedprice"])),
                    (li, IndexConfig("li_orderkey", ["l_orderkey"],
                                     ["l_extendedprice", "l_discount", "l_shipdate",
                                      "l_returnflag"])),
                    (od, IndexConfig("ord_orderkey", ["o_orderkey"],
                                     ["o_orderdate", "o_shippriority", "o_orderpriority"]))):
        _build(hs, df, cfg, args.device)
    Hyperspace.enable(s)
    li.createOrReplaceTempView("lineitem")
    od.createOrReplaceTempView("orders")
    join = "FROM lineitem JOIN orders ON l_orderkey = o_orderkey"
    rev = "l_extendedprice * (1 - l_discount)"
    queries = {
        # (the query, the same query with its guard as a WHERE conjunct)
        "q12_grouped": (
            f"SELECT l_returnflag, sum(CASE WHEN o_orderpriority IN ('1-URGENT', '2-HIGH') "
            f"THEN 1 ELSE 0 END) high, count(*) n {join} "
            f"WHERE l_shipdate >= DATE '1994-01-01' AND l_shipdate < DATE '1995-01-01' "
            f"GROUP BY l_returnflag",
            f"SELECT l_returnflag, count(*) high {join} "
            f"WHERE l_shipdate >= DATE '1994-01-01' AND l_shipdate < DATE '1995-01-01' "
            f"AND o_orderpriority IN ('1-URGENT', '2-HIGH') GROUP BY l_returnflag"),
        "q14_ratio": (
            f"SELECT 100.0 * sum(CASE WHEN o_orderdate < DATE '1995-09-16' THEN {rev} ELSE 0 END)"
            f" / sum({rev}) early {join} "
            f"WHERE l_shipdate >= DATE '1995-09-01' AND l_shipdate < DATE '1995-10-01'",
            f"SELECT sum({rev}) early {join} "
            f"WHERE l_shipdate >= DATE '1995-09-01' AND l_shipdate < DATE '1995-10-01' "
            f"AND o_orderdate < DATE '1995-09-16'"),
        "q6_ungrouped": (
            "SELECT sum(CASE WHEN l_discount >= 0.05 AND l_discount <= 0.07 "
            "THEN l_extendedprice * l_discount ELSE 0 END) revenue, "
            "count(CASE WHEN l_quantity < 24 THEN 1 END) small, count(*) n FROM lineitem "
            "WHERE l_shipdate >= DATE '1994-01-01' AND l_shipdate < DATE '1995-01-01'",
            "SELECT sum(l_extendedprice * l_discount) revenue, count(*) n FROM lineitem "
            "WHERE l_shipdate >= DATE '1994-01-01' AND l_shipdate < DATE '1995-01-01' "
            "AND l_discount >= 0.05 AND l_discount <= 0.07"),
    }
    key = "spark.hyperspace.mi.condAgg.fused"
    be = s.backend()
    out = {"config": "case_when", "device": args.device, "sf": sf, "runs": args.case_runs,
           "queries": {}}

    def route(text, fused):
        s.conf.set(key, "true" if fused else "false")
        rows = _rows(s.sql(text))
        return rows, getattr(be, "last_path", None), \
            getattr(be, "metrics", {}).get("cond_agg"), getattr(be, "fallback_reason", None)
    for name, (text, floor) in queries.items():
        got, path, how, why = route(text, True)
        got_c, path_c, how_c, why_c = route(text, False)
        _rows(s.sql(floor))
        tf, tc, tw = [], [], []
        for _ in range(args.case_runs):            # alternating, one run each
            s.conf.set(key, "true")
            tf.append(_median_ms(lambda: s.sql(text).collect(), 1, args.device))
            s.conf.set(key, "false")
            tc.append(_median_ms(lambda: s.sql(text).collect(), 1, args.device))
            tw.append(_median_ms(lambda: s.sql(floor).collect(), 1, args.device))
        s.conf.set(key, "true")
        s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
        ref = _rows(s.sql(text))
        th = _median_ms(lambda: s.sql(text).collect(), 3, "cpu")
        s.conf.set("spark.hyperspace.mi.execution.device", args.device)

        def med(ts):
            return sorted(ts)[len(ts) // 2]
        out["queries"][name] = {
            "fused_ms": med(tf), "column_ms": med(tc), "guard_in_where_ms": med(tw),
            "host_ms": th, "fused_ms_min_max": [min(tf), max(tf)],
            "column_ms_min_max": [min(tc), max(tc)],
            "path": path, "cond_agg": how, "fallback_reason": why,
            "column_path": path_c, "column_cond_agg": how_c, "column_fallback_reason": why_c,
            "match": _close(got, ref), "column_match": _close(got_c, ref)}
    out["match"] = all(q["match"] and q["column_match"] for q in out["queries"].values())
    return out


def config_count_distinct(args):
    """``count(DISTINCT x)`` under a range filter on the index key, three shapes: ungrouped, one
    dictionary group column (few groups) and one integer group column (rows / 10 groups).  Each
    is cross-checked against the host engine; reports q/s on both engines, the device time of
    level 1 (the hash aggregate on (g, x): its kernels and extract) and of the level-2 kernels
    per query (stage timers, HIP events), and which level-2 shape ran."""
    import numpy as np
    import pyarrow as pa
    import pyarrow.parquet as pq
    from hyperspace_amd import Hyperspace, IndexConfig, col, count, countDistinct, sum_
    from hyperspace_amd.utils.tracing import PROFILE_ENABLED, TRACER
    n = int(200_000 * args.sf)
    root = os.path.join(args.data_dir, f"cfg_count_distinct_sf{args.sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.join(root, "t"))
    rng = np.random.default_rng(23)
    nk = max(n // 20, 100)
    t = pa.table({"k": rng.integers(0, nk, n).astype(np.int64),
                  "x": pa.array(rng.integers(0, max(n // 4, 10), n).astype(np.int64),
                                mask=rng.random(n) < 0.05),
                  "gd": pa.array([f"region-{i:02d}" for i in range(16)]).take(
                      pa.array(rng.integers(0, 16, n).astype(np.int32))),
                  "gi": rng.integers(0, max(n // 10, 10), n).astype(np.int64),
                  "v": np.round(rng.random(n) * 1000, 2)})
    nfiles = 8
    step = (n + nfiles - 1) // nfiles
    for i in range(nfiles):
        pq.write_table(t.slice(i * step, step), os.path.join(root, "t", f"part-{i}.parquet"))
    del t
    s = _session(root, args.device, args.buckets)
    hs = Hyperspace(s)
    df = s.read.parquet(os.path.join(root, "t"))
    dt, _ = _build(hs, df, IndexConfig("cd_k", ["k"], ["x", "gd", "gi", "v"]), args.device)
    Hyperspace.enable(s)

    def base(i):
        lo = (i % 5) * (nk // 20)
        return df.filter((col("k") >= lo) & (col("k") < lo + (nk * 3) // 4))
    shapes = {
        "ungrouped": lambda i: base(i).agg(countDistinct("x").alias("c")),
        "few_groups": lambda i: base(i).groupBy("gd").agg(
            countDistinct("x").alias("c"), sum_("v").alias("sv"), count("*").alias("n")),
        "many_groups": lambda i: base(i).groupBy("gi").agg(
            countDistinct("x").alias("c"), sum_("v").alias("sv")),
    }
    out = {"config": "count_distinct", "device": args.device, "sf": args.sf, "rows": n,
           "index_build_s": round(dt, 3), "shapes": {}}
    got = {}
    for name, q in shapes.items():
        r = {"index_used": "cd_k" in q(0).queryExecution.executed_plan.tree_string()}
        got[name] = [_rows(q(i)) for i in range(2)]
        be = s.backend()
        r["path"] = getattr(be, "last_path", None)
        r["fallback_reason"] = getattr(be, "fallback_reason", None)
        r["groups"] = len(got[name][0])
        k = args.steps
        el = _timed_loop(lambda i: q(i).collect(), k, args.device)
        r["queries_per_s"] = round(k / el, 2)
        if args.device == "gpu" and r["path"] == "native":
            r["level2_shape"] = be.metrics.get("distinct_level2")
            s.conf.set(PROFILE_ENABLED, "true")
            TRACER.reset()
            for i in range(k):
                q(i).collect()
            rep = TRACER.report()
            s.conf.set(PROFILE_ENABLED, "false")
            TRACER.configure(s.conf)

            def per_query(*stages):
                return round(sum(rep.get(x, {}).get("device_ms", 0.0) for x in stages) / k, 4)
            r["level1_kernels_ms"] = per_query("hagg.kernels", "hagg.extract")
            r["level2_kernels_ms"] = per_query("hagg.distinct_kernels")
        out["shapes"][name] = r
    # the host engine on the same queries (and the cross-check)
    s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
    for name, q in shapes.items():
        ref = [_rows(q(i)) for i in range(2)]
        kh = max(2, min(3, args.steps))
        el_h = _timed_loop(lambda i: q(i).collect(), kh, "cpu")
        out["shapes"][name]["host_engine_queries_per_s"] = round(kh / el_h, 3)
        out["shapes"][name]["match"] = all(_close(a, b) for a, b in zip(got[name], ref))
    out["match"] = all(r["match"] for r in out["shapes"].values())
    return out


def config_window(args):
    """Window functions over ``lineitem`` (index on ``l_orderkey``), each shape aggregated to one
    row so the result copy does not dominate: ``top3`` ranks every order's lines by price
    (partitioned on the index key, ordered by another column: one device sort), ``running``
    sums quantities per supplier by ship date (partitioned on a non-key column: one device
    sort), ``per_order`` takes each order's total (the index order is the window's: no sort).
    Each is cross-checked against the host engine (``HS_CFG_SKIP_HOST=1`` skips that, for a
    kernel-trace run)."""
    from hyperspace_amd import (Hyperspace, IndexConfig, Window, col, count, max_, row_number,
                                sum_)
    sf = args.sf
    data, _ = _tpch(args, sf)
    root = os.path.join(args.data_dir, f"cfg_window_sf{sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    s = _session(root, args.device, args.buckets)
    hs = Hyperspace(s)
    li = s.read.parquet(os.path.join(data, "lineitem"))
    dt, _ = _build(hs, li, IndexConfig("li_win", ["l_orderkey"], [
        "l_suppkey", "l_shipdate", "l_quantity", "l_extendedprice"]), args.device)
    Hyperspace.enable(s)

    def base(i):
        return li.filter(col("l_orderkey") >= i % 4)

    def top3(i):
        w = Window.partitionBy("l_orderkey").orderBy(col("l_extendedprice").desc())
        return base(i).select("l_extendedprice", row_number().over(w).alias("rn")) \
            .filter(col("rn") <= 3).agg(sum_("l_extendedprice").alias("top3_price"),
                                        count("*").alias("n"))

    def running(i):
        w = Window.partitionBy("l_suppkey").orderBy("l_shipdate")
        return base(i).select(sum_("l_quantity").over(w).alias("run")) \
            .agg(max_("run").alias("max_run"), sum_("run").alias("sum_run"), count("*").alias("n"))

    def per_order(i):
        w = Window.partitionBy("l_orderkey")
        return base(i).select("l_quantity", sum_("l_quantity").over(w).alias("tot")) \
            .filter(col("tot") > 150.0).agg(sum_("l_quantity").alias("q"), count("*").alias("n"))
    shapes = {"top3": top3, "running": running, "per_order": per_order}
    out = {"config": "window", "device": args.device, "sf": sf, "index_build_s": round(dt, 3),
           "shapes": {}}
    got = {}
    for name, q in shapes.items():
        r = {"index_used": "li_win" in q(0).queryExecution.executed_plan.tree_string()}
        got[name] = [_rows(q(i)) for i in range(2)]
        be = s.backend()
        r["path"] = getattr(be, "last_path", None)
        r["fallback_reason"] = getattr(be, "fallback_reason", None)
        r["sort_skipped"] = be.metrics.get("window_sort_skipped")
        r["rows"] = got[name][0][0][-1]
        k = args.steps
        el = _timed_loop(lambda i: q(i).collect(), k, args.device)
        r["queries_per_s"] = round(k / el, 3)
        r["ms_per_query"] = round(el / k * 1e3, 2)
        out["shapes"][name] = r
    if os.environ.get("HS_CFG_SKIP_HOST"):
        return out
    s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
    for name, q in shapes.items():
        t0 = time.perf_counter()
        ref = [_rows(q(i)) for i in range(2)]
        out["shapes"][name]["host_engine_queries_per_s"] = round(2 / (time.perf_counter() - t0), 4)
        out["shapes"][name]["match"] = all(_close(a, b) for a, b in zip(got[name], ref))
    out["match"] = all(r["match"] for r in out["shapes"].values())
    return out


def _write_dimensions(root, sf):
    """TPC-H-shaped ``supplier`` (10k x SF rows: the domain of ``l_suppkey``; key and nation only,
    so SF100's 1M rows stay under the 10 MiB broadcast threshold) and ``nation`` (25 rows)."""
    import numpy as np
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = int(10_000 * sf)
    rng = np.random.default_rng(31)
    sup = pa.table({"s_suppkey": rng.permutation(np.arange(1, n + 1, dtype=np.int64)),
                    "s_nationkey": rng.integers(0, 25, n).astype(np.int32)})
    nat = pa.table({"n_nationkey": np.arange(25, dtype=np.int32),
                    "n_name": pa.array([f"NATION-{i:02d}" for i in range(25)]),
                    "n_regionkey": (np.arange(25) % 5).astype(np.int32)})
    for name, t in (("supplier", sup), ("nation", nat)):
        os.makedirs(os.path.join(root, name))
        pq.write_table(t, os.path.join(root, name, "part-0.parquet"))
    return n


def _probe_sweep(rows, reps=15):
    """The probe kernel alone (``hs_hj_probe``, csrc/kernels/hash_join.hip): ``rows`` random int64
    stream keys, ~80 % of them present, against a unique 25-key and a unique 1M-key table, for
    1 / 2 / 4 / 8 stream rows per lane, writing the mark byte alone and the mark plus the build
    row id.  Median of ``reps`` launches by device events; bytes are the stream side's (key,
    mark, row id).  Under ``rocprofv3 --kernel-trace --stats`` use ``HS_CFG_SWEEP_LANES=4
    HS_CFG_SWEEP_REPS=3`` for a short run of the default."""
    import ctypes as C
    import pyarrow as pa
    import torch
    from hyperspace_amd.exec.device_table import DeviceColumn
    from hyperspace_amd.ops import _lib as NL, kernels as K
    dev = torch.device("cuda", torch.cuda.current_device())
    lanes = [int(x) for x in os.environ.get("HS_CFG_SWEEP_LANES", "1,2,4,8").split(",")]
    reps = int(os.environ.get("HS_CFG_SWEEP_REPS", reps))
    L = NL.lib()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    out = []
    for nkeys in (25, 1_000_000):
        bk = (torch.randperm(nkeys, device=dev, generator=g) + 1).to(torch.int64)
        table = K.hash_join_table(DeviceColumn(bk, None, pa.int64()))
        sk = torch.randint(1, nkeys + nkeys // 4 + 2, (rows,), device=dev, generator=g,
                           dtype=torch.int64)
        desc = DeviceColumn(sk, None, pa.int64()).desc()
        mark = torch.empty(rows, dtype=torch.uint8, device=dev)
        build = torch.empty(rows, dtype=torch.int64, device=dev)

        def probe(rpl, want_build):
            NL.check(L.hs_hj_probe(
                C.byref(desc), rows, None, rows, NL.ptr(table.keys), NL.ptr(table.first),
                NL.ptr(table.last), NL.ptr(table.perm), table.slots, table.nbuild, 0, rpl, None,
                None, NL.ptr(mark), NL.ptr(build) if want_build else None, NL.stream_ptr()),
                "hs_hj_probe")
        for want_build in (False, True):
            for rpl in lanes:
                probe(rpl, want_build)
                torch.cuda.synchronize()
                ts = []
                for _ in range(reps):
                    a = torch.cuda.Event(enable_timing=True)
                    b = torch.cuda.Event(enable_timing=True)
                    a.record()
                    probe(rpl, want_build)
                    b.record()
                    b.synchronize()
                    ts.append(a.elapsed_time(b))
                ts.sort()
                nbytes = rows * (8 + 1 + (8 if want_build else 0))
                med = ts[len(ts) // 2]
                out.append({"keys": nkeys, "slots": table.slots, "rows": rows,
                            "rows_per_lane": rpl,
                            "outputs": "mark+row_id" if want_build else "mark",
                            "ms_median": round(med, 4), "ms_min": round(ts[0], 4),
                            "ms_max": round(ts[-1], 4), "stream_bytes": nbytes,
                            "table_bytes": (table.slots + 2) * 16 + table.nbuild * 4,
                            "stream_GBps": round(nbytes / med / 1e6, 1),
                            "hits": int(mark.sum().item())})
    return out


def config_broadcast_join(args):
    """Joins of ``lineitem`` (index on ``l_shipdate``) with small tables under the DEFAULT
    broadcast threshold, so they plan as ``BroadcastHashJoin``: a one-year ship-date range joined
    to ``supplier`` (unique key) and summed; the same grouped by ``s_nationkey``; ``nation``
    chained on top (a second broadcast join); a left-anti join against a 1000-key
    ``createDataFrame`` list.  Each shape is reduced to one row or a handful of groups and
    cross-checked against the host engine (``HS_CFG_SKIP_HOST=1`` skips that).
    ``HS_CFG_BROADCAST_THRESHOLD=-1`` plans the same queries as shuffled sort-merge joins, for
    comparison.  ``--probe-sweep`` runs the probe-kernel sweep alone (``_probe_sweep``)."""
    if getattr(args, "probe_sweep", False):
        from hyperspace_amd.ops import _lib as NL
        return {"config": "broadcast_join", "device": args.device,
                "default_rows_per_lane": int(NL.lib().hs_hj_rows_per_lane()),
                "probe_sweep": _probe_sweep(args.probe_rows)}
    import numpy as np
    from hyperspace_amd import Hyperspace, IndexConfig, col, count, sum_
    sf = args.sf
    data, _ = _tpch(args, sf)
    root = os.path.join(args.data_dir, f"cfg_broadcast_join_sf{sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    nsup = _write_dimensions(root, sf)
    thr = os.environ.get("HS_CFG_BROADCAST_THRESHOLD", "10485760")
    s = _session(root, args.device, args.buckets,
                 **{"spark.sql.autoBroadcastJoinThreshold": thr})
    hs = Hyperspace(s)
    li = s.read.parquet(os.path.join(data, "lineitem"))
    dt, _ = _build(hs, li, IndexConfig("li_ship_bj", ["l_shipdate"], [
        "l_suppkey", "l_extendedprice", "l_discount"]), args.device)
    Hyperspace.enable(s)
    sup = s.read.parquet(os.path.join(root, "supplier"))
    nat = s.read.parquet(os.path.join(root, "nation"))
    keys = np.random.default_rng(5).choice(np.arange(1, nsup + 1, dtype=np.int64),
                                           size=min(1000, nsup), replace=False)
    lst = s.createDataFrame({"k": keys})

    def base(i):
        year = 1993 + i % 5
        lo, hi = datetime.date(year, 1, 1), datetime.date(year + 1, 1, 1)
        return li.filter((col("l_shipdate") >= lo) & (col("l_shipdate") < hi))

    def joined(i):
        return base(i).join(sup, li["l_suppkey"] == sup["s_suppkey"])
    aggs = (sum_("l_extendedprice").alias("price"), count("*").alias("n"))
    shapes = {
        "supplier_sum": lambda i: joined(i).agg(*aggs),
        "by_nation": lambda i: joined(i).groupBy("s_nationkey").agg(*aggs),
        "nation_chain": lambda i: joined(i).join(nat, sup["s_nationkey"] == nat["n_nationkey"])
        .groupBy("n_regionkey").agg(*aggs),
        "anti_list": lambda i: base(i).join(lst, li["l_suppkey"] == lst["k"], "leftanti")
        .agg(*aggs),
    }
    out = {"config": "broadcast_join", "device": args.device, "sf": sf, "threshold": thr,
           "supplier_rows": nsup, "index_build_s": round(dt, 3), "shapes": {}}
    got = {}
    for name, q in shapes.items():
        plan = q(0).queryExecution.executed_plan.tree_string()
        r = {"index_used": "li_ship_bj" in plan, "broadcast_joins": plan.count("BroadcastHashJoin")}
        got[name] = [_rows(q(i)) for i in range(2)]
        be = s.backend()
        r["path"] = getattr(be, "last_path", None)
        r["fallback_reason"] = getattr(be, "fallback_reason", None)
        r["hash_join"] = getattr(be, "metrics", {}).get("hash_join") \
            if r["path"] == "native" and r["broadcast_joins"] else None
        k = args.steps if r["path"] == "native" else max(2, min(3, args.steps))
        el = _timed_loop(lambda i: q(i).collect(), k, args.device)
        r["ms_per_query"] = round(el / k * 1e3, 2)
        out["shapes"][name] = r
    if os.environ.get("HS_CFG_SKIP_HOST"):
        return out
    s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
    for name, q in shapes.items():
        t0 = time.perf_counter()
        ref = [_rows(q(i)) for i in range(2)]
        out["shapes"][name]["host_engine_ms_per_query"] = \
            round((time.perf_counter() - t0) / 2 * 1e3, 1)
        out["shapes"][name]["match"] = all(_close(a, b) for a, b in zip(got[name], ref))
    out["match"] = all(r["match"] for r in out["shapes"].values())
    return out


def _med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _sketch_kernel_times(rel, files, per_file, runs):
    """Median ms of each sketch kernel alone over the uploaded ``c`` and ``id`` columns: MinMax,
    the Bloom filter of the index (global-atomics path at this size) and, for comparison, a
    filter at the LDS limit."""
    import torch
    from hyperspace_amd.exec import device_build as DB
    from hyperspace_amd.ops import kernels as K
    device = torch.device("cuda", torch.cuda.current_device())
    cols = DB.upload_source_columns(rel, files, ["c", "id"], device)
    rows = [per_file] * len(files)
    from hyperspace_amd.index import dataskipping as DS
    _, nw, k = DS.bloom_params(per_file, 0.01)
    lds = K.sketch_bloom_lds_words()
    shapes = {"minmax_c": lambda: K.sketch_minmax(cols["c"], rows),
              f"bloom_id_{nw}_words": lambda: K.sketch_bloom(cols["id"], rows, nw, k),
              f"bloom_id_{lds}_words_lds": lambda: K.sketch_bloom(cols["id"], rows, lds, k)}
    return {n: _median_ms(fn, runs, "gpu") for n, fn in shapes.items()}


def config_data_skipping(args):
    """A data-skipping index over a ``lineitem``-sized table (6M x SF rows) in 128 files: ``c``
    is clustered by file (MinMax), ``id`` holds a disjoint random subset of the ids per file
    (Bloom), ``v`` is the payload.  Reports the sketch build (device build seconds and GB/s of
    decoded sketched bytes, its kernel and upload shares, the host builder over the same
    files), a selective range filter and a point lookup with and without the index (runs
    alternate, a new literal each run, medians; results cross-checked), and the host cost of
    ``prune`` for one equality and for an ``IN`` list of 1000 values."""
    import numpy as np
    import pyarrow as pa
    import pyarrow.parquet as pq
    from hyperspace_amd import (BloomFilterSketch, DataSkippingIndexConfig, Hyperspace,
                                MinMaxSketch, col, count, get_context, sum_)
    from hyperspace_amd.exec import device_sketch
    from hyperspace_amd.index import dataskipping as DS
    from hyperspace_amd.plan import expressions as E
    nfiles, runs = 128, max(5, args.ds_runs)
    per_file = max(1, int(6_000_000 * args.sf) // nfiles)
    root = os.path.join(args.data_dir, f"cfg_data_skipping_sf{args.sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    src = os.path.join(root, "t")
    os.makedirs(src)
    rng = np.random.default_rng(7)
    owner = rng.permutation(nfiles)        # ids congruent to owner[f] mod nfiles live in file f
    for f in range(nfiles):
        ids = rng.permutation(per_file).astype(np.int64) * nfiles + owner[f]
        pq.write_table(pa.table({
            "c": (f * 1000 + rng.integers(0, 1000, per_file)).astype(np.int32),
            "id": ids, "v": rng.random(per_file)}), os.path.join(src, f"part-{f:05d}.parquet"))
    s = _session(root, args.device, args.buckets)
    hs = Hyperspace(s)
    df = s.read.parquet(src)
    out = {"config": "data_skipping", "device": args.device, "sf": args.sf, "files": nfiles,
           "rows": per_file * nfiles, "runs": runs}
    sketched_bytes = per_file * nfiles * 12

    def config(name):
        return DataSkippingIndexConfig(name, MinMaxSketch("c"),
                                       BloomFilterSketch("id", 0.01, per_file))
    builds, stats = [], []
    for i in range(runs):
        _sync(args.device)
        t0 = time.perf_counter()
        hs.createIndex(df, config(f"skip{i}"))
        builds.append(time.perf_counter() - t0)
        stats.append(dict(device_sketch.LAST_SKETCH_STATS))
        if i < runs - 1:
            hs.deleteIndex(f"skip{i}")
            hs.vacuumIndex(f"skip{i}")
    name = f"skip{runs - 1}"
    b = _med(builds)
    out["build"] = {"path": stats[-1].get("path"), "columns": stats[-1].get("columns"),
                    "create_index_s": round(b, 3), "create_index_first_s": round(builds[0], 3),
                    "sketched_gb_per_s": round(sketched_bytes / b / 1e9, 2),
                    "upload_s": round(_med([x["upload_s"] for x in stats]), 4),
                    "kernels_s": round(_med([x["kernels_s"] for x in stats]), 4),
                    "groups": stats[-1].get("groups")}
    entry = [e for e in get_context(s).index_collection_manager.get_indexes()
             if e.name == name][0]
    rel = df.queryExecution.optimized_plan.relation
    ids = {f.name: f.id for f in entry.source_file_info_set}
    host = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ht = DS.host_sketch_rows(rel, sorted(ids), entry.derived_dataset.sketches, ids)
        host.append(time.perf_counter() - t0)
    out["build"]["host_builder_s"] = round(_med(host), 3)
    out["build"]["equals_host"] = DS.read_sketch_table(entry).sort_by("_data_file_id").equals(
        ht.sort_by("_data_file_id"))

    def q_range(i):
        lo = (17 * i + 3) % nfiles * 1000 + 200
        return df.filter((col("c") >= lo) & (col("c") < lo + 500)) \
            .agg(count("*").alias("n"), sum_(col("v")).alias("sv"))

    def q_point(i):
        f = (29 * i + 5) % nfiles
        return df.filter(col("id") == int((1000 + i) * nfiles + owner[f])) \
            .agg(count("*").alias("n"), sum_(col("v")).alias("sv"))
    if args.device == "gpu":
        out["kernels_ms"] = _sketch_kernel_times(rel, sorted(ids), per_file, runs)
    be = s.backend()
    drop = getattr(be, "_drop_resident", lambda: None)

    def timed(q, i, enabled, cold):
        (Hyperspace.enable if enabled else Hyperspace.disable)(s)
        if cold:
            drop()                        # nothing resident: the scan reads its files
        _sync(args.device)
        t0 = time.perf_counter()
        rows = _rows(q(i))
        _sync(args.device)
        return rows, (time.perf_counter() - t0) * 1e3
    out["queries"] = {}
    for qname, q in (("range", q_range), ("point", q_point)):
        res = {"files_read_without_index": nfiles}
        ok = True
        # cold: every run starts with an empty device cache; resident: the device cache keeps
        # what earlier runs loaded (the whole table, once the run without the index read it)
        for mode, cold in (("cold", True), ("resident", False)):
            t_on, t_off, kept = [], [], []
            for i in range(runs):         # alternate: with the index, then without
                DS.LAST_PRUNE.clear()
                a, t = timed(q, i, True, cold)
                t_on.append(t)
                kept.append(DS.LAST_PRUNE.get("kept"))
                r, t = timed(q, i, False, cold)
                t_off.append(t)
                ok = ok and _close(a, r) and a[0][0] > 0
            res[mode] = {"with_index_ms": round(_med(t_on), 2),
                         "without_index_ms": round(_med(t_off), 2)}
            res["files_read_with_index"] = kept
        res["path"] = getattr(be, "last_path", None)
        res["match"] = ok
        out["queries"][qname] = res
    files = rel.location.all_files()
    a = E.Attribute("id", pa.int64())
    eq = [E.EqualTo(a, E.Literal(int(5 * nfiles + owner[3]), pa.int64()))]
    inl = [E.In(a, [E.Literal(int(j * nfiles + owner[j % nfiles]), pa.int64())
                    for j in range(1000)])]
    DS.prune(entry, files, eq)            # loads the sketch table
    probe = {}
    for pname, conj in (("equality", eq), ("in_1000", inl)):
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            k = DS.prune(entry, files, conj)
            ts.append((time.perf_counter() - t0) * 1e3)
        probe[pname] = {"prune_ms": round(_med(ts), 3), "kept": len(k)}
    out["host_probe"] = probe
    out["match"] = all(r["match"] for r in out["queries"].values()) and \
        out["build"]["equals_host"]
    return out


def config_zorder(args):
    """A Z-order covering index on ``lineitem (l_shipdate, l_suppkey)`` including
    ``l_extendedprice`` and ``l_discount``: ``createIndex`` on the device against the host
    builder, the zone-map build and the ``hs_zone_prune`` pass alone, and - for a 5 % range on
    ``l_suppkey`` alone, on ``l_shipdate`` alone and on both - the kept share of zones and the
    query time with the index, with pruning switched off, and with Hyperspace disabled (the
    source table resident in HBM: what runs without this index kind).  Each index variant
    alternates with the disabled run, a new literal every run, medians; 40 consecutive queries
    per variant besides; results cross-checked against the host executor."""
    from hyperspace_amd import Hyperspace, ZOrderCoveringIndexConfig, col, count, sum_
    from hyperspace_amd.ops import kernels as K
    sf, runs = args.zorder_sf, max(5, args.ds_runs)
    data, _ = _tpch(args, sf)
    root = os.path.join(args.data_dir, f"cfg_zorder_sf{sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    src = os.path.join(data, "lineitem")
    cfg = lambda: ZOrderCoveringIndexConfig(                     # noqa: E731
        "li_z", ["l_shipdate", "l_suppkey"], ["l_extendedprice", "l_discount"])
    out = {"config": "zorder", "device": args.device, "sf": sf, "runs": runs}
    # host builder: a CPU session over the same files
    hsess = _session(os.path.join(root, "host"), "cpu", args.buckets)
    t0 = time.perf_counter()
    Hyperspace(hsess).createIndex(hsess.read.parquet(src), cfg())
    out["create_index_host_s"] = round(time.perf_counter() - t0, 3)
    rule = {"spark.hyperspace.index.zorder.filterRule.enabled": "true"}
    if args.zorder_zone_rows:
        rule["spark.hyperspace.mi.zorder.zoneRows"] = str(args.zorder_zone_rows)
    s = _session(os.path.join(root, "dev"), args.device, args.buckets, **rule)
    hs = Hyperspace(s)
    li = s.read.parquet(src)
    dt, _ = _build(hs, li, cfg(), args.device)
    out["create_index_s"] = round(dt, 3)
    nsupp = max(1, int(round(sf * 10_000)))
    day0, days = datetime.date(1992, 1, 2), 2500

    def window(i, span, width):
        lo = (i * 7919) % max(1, span - width)
        return lo, lo + width

    def cond(which, i):
        c = None
        if which in ("suppkey", "both"):
            lo, hi = window(i, nsupp, max(1, nsupp // 20))
            c = (col("l_suppkey") >= lo + 1) & (col("l_suppkey") <= hi)
        if which in ("shipdate", "both"):
            lo, hi = window(i + 3, days, days // 20)
            d = (col("l_shipdate") >= day0 + datetime.timedelta(days=lo)) & \
                (col("l_shipdate") < day0 + datetime.timedelta(days=hi))
            c = d if c is None else c & d
        return c

    def q(df, which, i):
        return df.filter(cond(which, i)).agg(
            sum_(col("l_extendedprice") * col("l_discount")).alias("rev"), count("*").alias("n"))
    # one session per variant over the same files and index store, so the alternating runs
    # flip no session state (enabling Hyperspace or changing the conf between two queries costs
    # the next query its plan-cache entry or a heap settle): with the index, with the index
    # but every zone scanned, and without Hyperspace
    Hyperspace.enable(s)
    s_np = _session(os.path.join(root, "dev"), args.device, args.buckets,
                    **dict(rule, **{"spark.hyperspace.mi.zorder.prune": "false"}))
    Hyperspace.enable(s_np)
    s_off = _session(os.path.join(root, "dev"), args.device, args.buckets)
    sessions = {"index": s, "noprune": s_np, "disabled": s_off}
    frames = {k: x.read.parquet(src) for k, x in sessions.items()}
    be = s.backend()

    def timed(which, i, mode):
        _sync(args.device)
        t0 = time.perf_counter()
        rows = _rows(q(frames[mode], which, i))
        _sync(args.device)
        return rows, (time.perf_counter() - t0) * 1e3
    out["queries"] = {}
    hli = hsess.read.parquet(src)
    for which in ("suppkey", "shipdate", "both"):
        ts = {"index": [], "noprune": [], "disabled": [], "disabled2": []}
        shares, ok = [], True
        for mode in sessions:                  # load tables, plan, compile kernels
            timed(which, 1000, mode)
            timed(which, 1001, mode)
        # alternating pairs, one index variant against the disabled run at a time: the two index
        # sessions run the SAME generated kernel over different tables, and two such sessions
        # taking turns slow each other down on the device, which is not what is measured here
        for mode, off in (("index", "disabled"), ("noprune", "disabled2")):
            for i in range(runs):
                if mode == "index" and args.device == "gpu":
                    be.metrics.pop("scan_zones_kept", None)
                a, t = timed(which, i, mode)
                ts[mode].append(t)
                if mode == "index" and be.metrics.get("scan_zones_kept") is not None:
                    shares.append(int(be.metrics["scan_zones_kept"]) / be.metrics["scan_zones"])
                r, t = timed(which, i, "disabled")
                ts[off].append(t)
                ok = ok and _close(a, r) and a[0][1] > 0
        Hyperspace.disable(hsess)
        ok = ok and _close(_rows(q(hli, which, 0)), timed(which, 0, "index")[0])
        out["queries"][which] = {
            "kept_share": round(_med(shares), 4) if shares else None,
            "with_index_ms": round(_med(ts["index"]), 3),
            "prune_off_ms": round(_med(ts["noprune"]), 3),
            "disabled_ms": round(_med(ts["disabled"]), 3),
            "disabled_beside_prune_off_ms": round(_med(ts["disabled2"]), 3),
            "disabled_spread_ms": round(max(ts["disabled"] + ts["disabled2"]) -
                                        min(ts["disabled"] + ts["disabled2"]), 3),
            "plan_used_index": "Name: li_z" in q(frames["index"], which, 0)
            .queryExecution.executed_plan.tree_string(),
            "path": getattr(be, "last_path", None), "match": ok}
    # the same three variants without alternation: 40 consecutive queries of one session each
    # (l_suppkey range, a new literal every query)
    cons = {}
    for mode in sessions:
        for i in range(2000, 2004):
            timed("suppkey", i, mode)
        _sync(args.device)
        t0 = time.perf_counter()
        for i in range(40):
            q(frames[mode], "suppkey", 3000 + i).collect()
        _sync(args.device)
        cons[mode] = round((time.perf_counter() - t0) / 40 * 1e3, 3)
    out["consecutive_ms"] = cons
    if args.device == "gpu":
        # the zone-map build and the prune pass alone, on the resident index table
        from hyperspace_amd.exec.zorder import resident_zone_maps
        table, names, zone, maps = resident_zone_maps(be)[0]
        cols = [table.columns[c] for c in names]
        lo = K.sortable_image(nsupp // 2, cols[1].hs_type)
        hi = K.sortable_image(nsupp // 2 + nsupp // 20, cols[1].hs_type)
        tm, tp = [], []
        for _ in range(runs):
            _sync("gpu")
            t0 = time.perf_counter()
            K.zone_minmax(cols, zone)
            _sync("gpu")
            tm.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            K.zone_prune(maps, table.num_rows, zone, [(1, lo, hi)])
            _sync("gpu")
            tp.append((time.perf_counter() - t0) * 1e3)
        out.update({"rows": table.num_rows, "zones": int(maps[0].shape[1]), "zone_rows": zone,
                    "zone_map_build_ms": round(_med(tm), 3), "zone_prune_ms": round(_med(tp), 3)})
    out["match"] = all(r["match"] for r in out["queries"].values())
    return out


def config_date_fns(args):
    """Date functions over the lineitem / orders index pair of the bench (TPC-H SF ``--date-sf``),
    every query cross-checked against the host engine; alternating runs in one process, medians
    of ``--date-runs``:

    1. projection cost: ``select(year(l_shipdate))`` against the same-byte arithmetic projection
       ``select(l_linenumber + 1)`` over the same rows (4 B + validity read, 5 B written each);
    2. the Q8 shape - ``sum(CASE WHEN year(o_orderdate) = 1995 ...)`` grouped by
       ``extract(year FROM o_orderdate)`` over the join - against the same query grouped by a
       stored int column with as many groups (``l_linenumber``: 7 values, like the 7 order
       years): the price of the hidden-column route;
    3. ``WHERE year(l_shipdate) = 1994`` with ``datePartRange.enabled`` true against false."""
    from hyperspace_amd import Hyperspace, IndexConfig
    sf = args.date_sf
    data, _ = _tpch(args, sf)
    root = os.path.join(args.data_dir, f"cfg_date_fns_sf{sf:g}")
    shutil.rmtree(root, ignore_errors=True)
    s = _session(root, args.device, args.buckets)
    hs = Hyperspace(s)
    li = s.read.parquet(os.path.join(data, "lineitem"))
    od = s.read.parquet(os.path.join(data, "orders"))
    for df, cfg in ((li, IndexConfig("li_shipdate", ["l_shipdate"],
                                     ["l_discount", "l_quantity", "l_extendedprice"])),
                    (li, IndexConfig("li_orderkey", ["l_orderkey"],
                                     ["l_extendedprice", "l_discount", "l_shipdate",
                                      "l_linenumber"])),
                    (od, IndexConfig("ord_orderkey", ["o_orderkey"],
                                     ["o_orderdate", "o_shippriority"]))):
        _build(hs, df, cfg, args.device)
    Hyperspace.enable(s)
    li.createOrReplaceTempView("lineitem")
    od.createOrReplaceTempView("orders")
    join = "FROM lineitem JOIN orders ON l_orderkey = o_orderkey"
    # a projection is timed through an aggregate over it that reads the computed column, so
    # that no result rows cross to the host: the projection pass is the difference in kind
    pairs = {
        "projection": (
            "SELECT sum(y) s, count(*) n FROM (SELECT year(l_shipdate) y FROM lineitem "
            "WHERE l_orderkey >= 0)",
            "SELECT sum(y) s, count(*) n FROM (SELECT l_linenumber + 1 y FROM lineitem "
            "WHERE l_orderkey >= 0)", {}),
        "q8_grouped": (
            f"SELECT extract(year FROM o_orderdate) g, sum(CASE WHEN year(o_orderdate) = 1995 "
            f"THEN l_extendedprice ELSE 0 END) v, sum(l_extendedprice) t, count(*) n {join} "
            f"GROUP BY extract(year FROM o_orderdate)",
            f"SELECT l_linenumber g, sum(CASE WHEN o_orderdate >= DATE '1995-01-01' AND "
            f"o_orderdate < DATE '1996-01-01' THEN l_extendedprice ELSE 0 END) v, "
            f"sum(l_extendedprice) t, count(*) n {join} GROUP BY l_linenumber", {}),
        "year_filter": (
            "SELECT sum(l_extendedprice * l_discount) r, count(*) n FROM lineitem "
            "WHERE year(l_shipdate) = 1994",
            "SELECT sum(l_extendedprice * l_discount) r, count(*) n FROM lineitem "
            "WHERE year(l_shipdate) = 1994",
            {"spark.hyperspace.mi.datePartRange.enabled": ("true", "false")}),
    }
    be = s.backend()
    out = {"config": "date_fns", "device": args.device, "sf": sf, "runs": args.date_runs,
           "notes": {"projection": "a = year(l_shipdate), b = l_linenumber + 1; each timed as "
                                   "sum / count over the projected column, not a plain select",
                     "q8_grouped": "a grouped by extract(year FROM o_orderdate) with the CASE "
                                   "over year(), b grouped by the stored l_linenumber (7 groups "
                                   "each) with the CASE over a date range",
                     "year_filter": "a = datePartRange.enabled true, b = false"},
           "queries": {}}

    def med(ts):
        return sorted(ts)[len(ts) // 2]
    for name, (a, b, conf) in pairs.items():
        def use(i):
            for k, v in conf.items():
                s.conf.set(k, v[i])
        info = []
        for i, text in enumerate((a, b)):
            use(i)
            rows = _rows(s.sql(text))
            path, why = getattr(be, "last_path", None), getattr(be, "fallback_reason", None)
            s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
            ref = _rows(s.sql(text))
            s.conf.set("spark.hyperspace.mi.execution.device", args.device)
            info.append((rows, path, why, _close(rows, ref)))
        ta, tb = [], []
        for _ in range(max(5, args.date_runs)):        # alternating, one run each
            use(0)
            ta.append(_median_ms(lambda: s.sql(a).collect(), 1, args.device))
            use(1)
            tb.append(_median_ms(lambda: s.sql(b).collect(), 1, args.device))
        use(0)
        out["queries"][name] = {
            "a_ms": med(ta), "b_ms": med(tb), "ratio": round(med(ta) / med(tb), 3),
            "a_runs_ms": [round(x, 3) for x in ta], "b_runs_ms": [round(x, 3) for x in tb],
            "a_path": info[0][1], "b_path": info[1][1],
            "fallback_reason": info[0][2] or info[1][2],
            "rows": len(info[0][0]), "match": info[0][3] and info[1][3]}
    out["match"] = all(r["match"] for r in out["queries"].values())
    return out


CONFIGS = {"csv10k": config_csv10k, "sf10_filter": config_sf10_filter, "hybrid": config_hybrid,
           "q3_3way": config_q3_3way, "tpcds_3way": config_tpcds_3way,
           "streamed": config_streamed, "like": config_like, "case_when": config_case_when,
           "count_distinct": config_count_distinct, "window": config_window,
           "broadcast_join": config_broadcast_join, "data_skipping": config_data_skipping,
           "zorder": config_zorder, "date_fns": config_date_fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["all"] + list(CONFIGS))
    ap.add_argument("--device", default="gpu", choices=["gpu", "cpu"])
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--buckets", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--data-dir", default=os.environ.get("HS_BENCH_DIR", "/tmp/hs_bench"))
    ap.add_argument("--tpcds-sf", type=float, default=300.0)
    ap.add_argument("--hbm-budget-gb", type=float, default=8.0,
                    help="streamed: the build and resident-table HBM budgets")
    ap.add_argument("--like-runs", type=int, default=11,
                    help="like: timed runs per dictionary size and route (medians reported)")
    ap.add_argument("--case-sf", type=float, default=10.0,
                    help="case_when: TPC-H scale factor")
    ap.add_argument("--case-runs", type=int, default=7,
                    help="case_when: alternating timed runs per route (medians reported)")
    ap.add_argument("--date-sf", type=float, default=10.0,
                    help="date_fns: TPC-H scale factor")
    ap.add_argument("--date-runs", type=int, default=7,
                    help="date_fns: alternating timed runs per query pair (at least 5; medians)")
    ap.add_argument("--probe-sweep", action="store_true",
                    help="broadcast_join: time the hash-join probe kernel alone, per rows per lane")
    ap.add_argument("--ds-runs", type=int, default=5,
                    help="data_skipping: runs per measurement (at least 5; medians reported)")
    ap.add_argument("--zorder-sf", type=float, default=10.0,
                    help="zorder: TPC-H scale factor of the lineitem table")
    ap.add_argument("--zorder-zone-rows", type=int, default=0,
                    help="zorder: spark.hyperspace.mi.zorder.zoneRows (0 = automatic)")
    ap.add_argument("--probe-rows", type=int, default=1 << 26,
                    help="broadcast_join --probe-sweep: stream rows")
    args = ap.parse_args()
    if args.device == "gpu":
        import torch
        torch.cuda.set_device(0)
    names = list(CONFIGS) if args.config == "all" else [args.config]
    for name in names:
        t0 = time.perf_counter()
        res = CONFIGS[name](args)
        res["wall_s"] = round(time.perf_counter() - t0, 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
