#!/usr/bin/env python
"""Headline benchmark (BASELINE.json): queries/sec + index-build GB/s on TPC-H SF100-shaped data,
filter (FilterIndexRule, TPC-H Q6) + join (JoinIndexRule, TPC-H Q3-style) on 1/2/4/8 MI355X.

    python bench.py --gpus N --steps K --warmup W [--sf 100] [--full] [--dump-outputs DIR]
    torchrun --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

A plain run does what the headline needs and no more: data (generated once per data dir), the
three index builds, W warm-up steps, K timed steps of the headline placement, and the JSON line
(``value``, ``ms_per_step`` = milliseconds per timed step, the build figures).  ``--full`` adds
every side measurement and check described below (cold first queries, the join-index run, the
replicated placement, per-query latencies, ``q3_full``, the N = 1 side configs and the
cross-check against the un-indexed plan).  ``--dump-outputs DIR`` writes the rows the last timed
step's two queries returned as ``DIR/<name>.npy`` (float64, one array per result column).

One step = one Q6 filter query + one Q3-style join query, each with fresh literals, through
the full engine path (analysis, then a plan-cache lookup: a hit re-binds the new literals into
the cached executed plan and skips the optimizer and the Hyperspace rules; the first query of a
shape runs the optimizer + rules + signature validation), execution on the HIP kernels, and the
cross-rank combine.  ``value`` = whole-job queries/sec.  Data is synthetic TPC-H-shaped
(``hyperspace_amd.models.tpch``) and generated once per data dir.  Index build is timed
separately (three covering indexes: lineitem(l_shipdate), lineitem(l_orderkey),
orders(o_orderkey)); ``index_build_gbps`` = decoded indexed-column bytes / build wall time;
``bytes_over_xgmi`` = build-shuffle bytes all ranks sent to other ranks (RCCL all-to-all).
Queries run with two placements (``--placement``, default both; ``value`` is always the
sharded one - ONE query stream over the N GPUs, ``scaling: strong`` at every N, so a 1->8 curve
compares like with like - and with N > 1 the replicated one is the side key ``replicated``; at
N = 1 they coincide).  (Round 5 reported the replicated placement as ``value`` at N > 1; from
round 6 it is a side key again, so multi-GPU records of round 5 are not comparable.)

* ``sharded`` (headline, ``scaling: strong``): each rank holds only the buckets it owns
  (size-balanced owner map with heavy-bucket key ranges, the same for both sides of a join);
  every query runs on all ranks over their buckets and the partial aggregates combine with one
  RCCL all-gather - the placement for index sets larger than one GPU's HBM, and BASELINE
  config #3's bucket-parallel JoinIndexRule over RCCL.  Every rank plans every query, so its
  rate is bounded by one process's host time per query once the per-rank device time drops
  below it;
* ``replicated`` (side key, ``scaling: weak``): every rank loads all buckets into its HBM (the
  SF100 index set is ~36 GB of a 288 GB MI355X) and serves its own query stream with no
  collective - read replicas, one process per GPU.

At N = 1 two more side keys run the BASELINE configs' real query shapes through the same engine,
each checked against the host oracle (``benchmarks/configs.py``): ``q3_3way`` (TPC-H Q3's
customer x orders x lineitem join with the ``c_mktsegment`` filter over four covering indexes)
and ``hybrid`` (the SF index set + 10% appended Parquet files through Hybrid Scan, then after an
incremental refresh: ``hybrid_vs_refreshed`` = Hybrid Scan q/s / refreshed q/s).  A side key
that fails records its error instead of stopping the headline record.

Extra keys: ``latency`` has single-query latencies (``q3_join_ms`` = merge join,
``q3_join_index_ms`` = through the join index) and the cold first queries after ``createIndex``
(``q6_cold_ms`` / ``q3_cold_ms``: HBM load of the index, kernel compile when the code-object
cache is empty); ``index_build_src_gbps`` is the compressed source-Parquet bytes of the read
columns per second of build.  ``vs_baseline`` divides
by the CPU engine's q/s on the same data (``profiles/cpu_baseline_sf<SF>.json``, written by
``bench.py --device cpu``) when one was recorded.
"""
import argparse
import datetime
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "queries/sec + index-build GB/s, TPC-H SF100 filter+join at 1/2/4/8 MI355X"


def log(rank, *a):
    if rank == 0:
        print(*a, file=sys.stderr, flush=True)


def _dir_bytes(root: str) -> int:
    """Bytes of the index data files under ``root`` (all ranks' buckets: a shared file
    system)."""
    tot = 0
    for dp, _, fs in os.walk(root):
        tot += sum(os.path.getsize(os.path.join(dp, f)) for f in fs if f.endswith(".parquet"))
    return tot


def _decoded_bytes(df, cfg) -> int:
    """Decoded (in-memory, fixed-width) bytes of an index's columns over all source rows — the
    byte count the device build reports as ``source_bytes``."""
    import pyarrow.parquet as pq
    from hyperspace_amd.exec.device_table import storage_numpy_dtype
    from hyperspace_amd.plan import logical as L
    from hyperspace_amd.utils import path_utils as P
    rel = df.queryExecution.analyzed.collect(lambda p: isinstance(p, L.LogicalRelation))[0].relation
    rows = sum(pq.ParquetFile(P.to_local(f.path)).metadata.num_rows
               for f in rel.location.all_files())
    width = sum(storage_numpy_dtype(rel.schema.field(c).type).itemsize
                for c in cfg.indexedColumns + cfg.includedColumns)
    return rows * width


def _source_parquet_bytes(df, cfg) -> int:
    """Compressed on-disk bytes of the column chunks an index build reads (footer metadata)."""
    import pyarrow.parquet as pq
    from hyperspace_amd.plan import logical as L
    from hyperspace_amd.utils import path_utils as P
    rel = df.queryExecution.analyzed.collect(lambda p: isinstance(p, L.LogicalRelation))[0].relation
    want = set(cfg.indexedColumns + cfg.includedColumns)
    total = 0
    for f in rel.location.all_files():
        md = pq.ParquetFile(P.to_local(f.path)).metadata
        for g in range(md.num_row_groups):
            rg = md.row_group(g)
            for c in range(rg.num_columns):
                cc = rg.column(c)
                if cc.path_in_schema in want:
                    total += cc.total_compressed_size
    return total


def _cpu_baseline(sf: float):
    p = os.path.join(ROOT, "profiles", f"cpu_baseline_sf{sf:g}.json")
    if os.path.exists(p):
        with open(p) as f:
            return json.load(f)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--buckets", type=int, default=200)
    ap.add_argument("--files", type=int, default=0, help="source files per table (0=auto)")
    ap.add_argument("--data-dir", default=os.environ.get("HS_BENCH_DIR", "/tmp/hs_bench"))
    ap.add_argument("--workers", type=int, default=int(os.environ.get("HS_BENCH_WORKERS", "0")))
    ap.add_argument("--no-crosscheck", action="store_true")
    ap.add_argument("--codec", default="snappy",
                    help="index file codec: 'snappy' (Spark's default, as the reference writes; "
                         "pages compressed on the device) or 'none'; both use the device "
                         "dictionary/bit-packed encoding (exec/pq_encode.py)")
    ap.add_argument("--placement", default="both", choices=["both", "sharded", "replicated"],
                    help="multi-GPU query placement (spark.hyperspace.mi.index.placement): "
                         "sharded = buckets b %% N per rank, every query on all ranks + one "
                         "all-gather; replicated = every rank holds all buckets and serves its "
                         "own query stream; both = time sharded, then replicated (reported)")
    ap.add_argument("--inflight", type=int, default=4,
                    help="query steps kept in flight (DataFrame.collect_async): 1 = each query "
                         "finishes before the next is planned.  4: a sharded run's cross-rank "
                         "combines of the steps in flight travel together (one collective per "
                         "flush); one GPU measures the same with 2 or 4")
    ap.add_argument("--device", default="gpu", choices=["gpu", "cpu"],
                    help="cpu = the pyarrow host engine (measured baseline, BASELINE.md)")
    ap.add_argument("--record-baseline", action="store_true",
                    help="with --device cpu: save the JSON line as profiles/cpu_baseline_sf<SF>.json "
                         "(the vs_baseline denominator of later GPU runs)")
    ap.add_argument("--no-side", action="store_true",
                    help="skip the N = 1 side configs (q3_3way, hybrid)")
    ap.add_argument("--host-breakdown", type=int, default=0, metavar="N",
                    help="after the timed steps, time N queries phase by phase on the host "
                         "(DataFrame build / plan / submit / result), reported as host_breakdown")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: cold first "
                         "queries, the join-index run, the replicated placement (N > 1), "
                         "per-query latencies, q3_full, the N = 1 side configs (q3_3way, hybrid) "
                         "and the cross-check against the un-indexed plan")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the results of the last timed step "
                         "(what collect() returned) as DIR/<name>.npy, float64")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import numpy as np
    import torch

    from hyperspace_amd import Hyperspace, IndexConfig, Session, col, count, sum_
    from hyperspace_amd.exec import device_build
    from hyperspace_amd.models import tpch
    from hyperspace_amd.parallel.dist import DistContext

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    on_gpu = args.device == "gpu"
    jit_mod = None
    if on_gpu:
        from hyperspace_amd.exec import jit as jit_mod
    dist = DistContext.from_env() if world_env > 1 else None
    rank, world = (dist.rank, dist.world) if dist else (0, 1)
    if on_gpu:
        if dist is None:
            torch.cuda.set_device(0)
        sync = torch.cuda.synchronize
    else:
        sync = (lambda: None)
    barrier = dist.barrier if dist else (lambda: None)

    sf = args.sf
    nfiles = args.files or max(8, int(round(sf * 1.28)))
    data = os.path.join(args.data_dir, f"tpch_sf{sf:g}_f{nfiles}")
    cpus = os.cpu_count() or 8
    workers = args.workers or max(1, min(16, cpus // max(world, 1)))
    # ---------------------------------------------------------------- data generation (once)
    t0 = time.perf_counter()
    mine = [i for i in range(nfiles) if i % world == rank]
    tpch.generate(data, sf, nfiles, mine, workers=workers)
    barrier()
    gen_s = time.perf_counter() - t0
    log(rank, f"[bench] data ready sf={sf} files={nfiles} in {gen_s:.1f}s ({data})")

    idx_root = os.path.join(args.data_dir, f"indexes_sf{sf:g}_b{args.buckets}_w{world}")
    if rank == 0 and os.path.exists(idx_root):
        shutil.rmtree(idx_root)
    barrier()
    s = Session(conf={"spark.hyperspace.system.path": idx_root,
                      "spark.hyperspace.index.numBuckets": str(args.buckets),
                      "spark.sql.autoBroadcastJoinThreshold": "-1",
                      "spark.sql.shuffle.partitions": str(args.buckets),
                      "spark.hyperspace.mi.execution.device": args.device,
                      "spark.hyperspace.mi.index.codec": args.codec,
                      # headline Q3 re-matches keys every query (merge join)
                      "spark.hyperspace.mi.joinIndex.enabled": "false"},
                warehouse_dir=os.path.join(args.data_dir, "wh"))
    # extra session conf for sweeps: HS_BENCH_CONF="key=value,key=value"
    for kv in filter(None, os.environ.get("HS_BENCH_CONF", "").split(",")):
        k, v = kv.split("=", 1)
        s.conf.set(k.strip(), v.strip())
    s.dist = dist
    hs = Hyperspace(s)
    li = s.read.parquet(os.path.join(data, "lineitem"))
    od = s.read.parquet(os.path.join(data, "orders"))

    # engine start (HBM arena, pinned staging pool, staging threads, decode kernels): process
    # start-up, reported as engine_start_s, not part of any build
    te = time.perf_counter()
    if on_gpu:
        s.backend()
        sync()
    engine_s = time.perf_counter() - te
    log(rank, f"[bench] engine start {engine_s:.2f}s")

    # ---------------------------------------------------------------- index build (timed)
    builds = [(li, IndexConfig("li_shipdate", ["l_shipdate"],
                               ["l_discount", "l_quantity", "l_extendedprice"])),
              (li, IndexConfig("li_orderkey", ["l_orderkey"],
                               ["l_extendedprice", "l_discount", "l_shipdate"])),
              (od, IndexConfig("ord_orderkey", ["o_orderkey"], ["o_orderdate", "o_shippriority"]))]
    build_s, build_bytes, src_bytes, xgmi_bytes = 0.0, 0, 0, 0.0
    per_index = {}
    for df, cfg in builds:
        barrier()
        sync()
        tb = time.perf_counter()
        hs.createIndex(df, cfg)
        sync()
        barrier()
        dt = time.perf_counter() - tb
        xg = float(device_build.LAST_BUILD_STATS.get("exchange_sent_bytes", 0)) if on_gpu else 0.0
        if dist:
            xg = dist.all_reduce_sum_float(xg)
        xgmi_bytes += xg
        if on_gpu:
            local_bytes = float(device_build.LAST_BUILD_STATS.get("source_bytes", 0))
        else:  # same definition as the device build: decoded bytes of the indexed columns
            local_bytes = float(_decoded_bytes(df, cfg))
        if dist:
            local_bytes = dist.all_reduce_sum_float(local_bytes)
            dt = dist.all_reduce_max_float(dt)
        sb = _source_parquet_bytes(df, cfg) if rank == 0 else 0
        build_s += dt
        build_bytes += local_bytes
        src_bytes += sb
        per_index[cfg.indexName] = {"s": round(dt, 3), "gbps": round(local_bytes / dt / 1e9, 3),
                                    "src_gbps": round(sb / dt / 1e9, 3)}
        log(rank, f"[bench] built {cfg.indexName} in {dt:.2f}s "
                  f"({local_bytes / 1e9:.2f} GB decoded) {device_build.LAST_BUILD_STATS}")
    build_gbps = build_bytes / build_s / 1e9
    src_gbps = src_bytes / build_s / 1e9

    Hyperspace.enable(s)
    backend = s.backend()

    # ---------------------------------------------------------------- queries
    def d(days):
        return datetime.date(1970, 1, 1) + datetime.timedelta(days=int(days))

    def q6(i):
        year = 1993 + i % 5
        disc = 0.02 + (i % 8) * 0.01
        qty = 24 + (i % 2)
        lo = datetime.date(year, 1, 1)
        hi = datetime.date(year + 1, 1, 1)
        return li.filter((col("l_shipdate") >= lo) & (col("l_shipdate") < hi) &
                         (col("l_discount") >= round(disc - 0.01, 2)) &
                         (col("l_discount") <= round(disc + 0.01, 2)) & (col("l_quantity") < qty)) \
            .agg(sum_(col("l_extendedprice") * col("l_discount")).alias("revenue"))

    def q3(i):
        dd = datetime.date(1995, 3, 1) + datetime.timedelta(days=(i * 7) % 30)
        j = li.join(od, li["l_orderkey"] == od["o_orderkey"]) \
            .filter((col("o_orderdate") < dd) & (col("l_shipdate") > dd))
        return j.groupBy("o_shippriority").agg(
            sum_(col("l_extendedprice") * (1 - col("l_discount"))).alias("revenue"),
            count("*").alias("lines"))

    def q3_full(i):
        """TPC-H Q3's full result shape over the indexed lineitem x orders join:
        GROUP BY l_orderkey, o_orderdate, o_shippriority (millions of groups at SF100, device
        hash aggregate) ORDER BY revenue DESC, o_orderdate LIMIT 10 (device top-k).  The
        c_mktsegment semi-join of the customer table is not part of this shape."""
        dd = datetime.date(1995, 3, 1) + datetime.timedelta(days=(i * 7) % 30)
        j = li.join(od, li["l_orderkey"] == od["o_orderkey"]) \
            .filter((col("o_orderdate") < dd) & (col("l_shipdate") > dd))
        return j.groupBy("l_orderkey", "o_orderdate", "o_shippriority") \
            .agg(sum_(col("l_extendedprice") * (1 - col("l_discount"))).alias("revenue")) \
            .orderBy(col("revenue").desc(), col("o_orderdate")).limit(10)

    def submit(i):
        """One step = one Q6 + one Q3, each planned and submitted through the full engine (a
        warm Q6 scan pipeline replays on the engine's side stream, beside the Q3 merge join:
        spark.hyperspace.mi.sideStreamScans.enabled; two Q3 merge joins on two streams at once
        measured slower, 1.75 vs 1.45 ms per step: profiles/bench_q3_streams_r3.log)."""
        return q6(i).collect_async(), q3(i).collect_async()

    def finish(fs):
        out = tuple(f.result() for f in fs)
        if on_gpu and any(f.path != "native" for f in fs):
            raise RuntimeError(f"query fell back to host: {[f.reason for f in fs]}")
        return out

    def run_steps(idx):
        """Steps ``idx`` with up to ``args.inflight`` steps submitted ahead of the one being
        finished: the host plans and submits step i+1 while the device runs step i."""
        from collections import deque
        pending, out = deque(), []
        for i in idx:
            pending.append(submit(i))
            while len(pending) > max(args.inflight - 1, 0):
                out.append(finish(pending.popleft()))
        while pending:
            out.append(finish(pending.popleft()))
        return out

    def timed(mode):
        """Warm up, then time exactly ``args.steps`` steps bracketed by barrier + sync."""
        s.conf.set("spark.hyperspace.mi.index.placement", mode)
        off = rank * 100000 if mode == "replicated" else 0   # replicas serve distinct queries
        tl = time.perf_counter()
        run_steps(range(1000 + off, 1000 + off + args.warmup))
        sync()
        barrier()
        warm = time.perf_counter() - tl
        log(rank, f"[bench] {mode}: warmup {args.warmup} steps in {warm:.2f}s "
                  f"(includes first HBM load of the indexes)")
        TRACER.reset()  # HS_PROFILE=1: per-stage host/device times of the timed steps only
        prof = None
        if os.environ.get("HS_BENCH_PROFILE") and rank == 0:
            import cProfile
            prof = cProfile.Profile()
        barrier()
        sync()
        t_start = time.perf_counter()
        if prof is not None:
            prof.enable()
        res = run_steps(range(off, off + args.steps))
        sync()
        barrier()
        el = time.perf_counter() - t_start
        if prof is not None:
            import io
            import pstats
            prof.disable()
            buf = io.StringIO()
            pstats.Stats(prof, stream=buf).sort_stats("cumulative").print_stats(40)
            pstats.Stats(prof, stream=buf).sort_stats("tottime").print_stats(30)
            log(rank, buf.getvalue())
        if TRACER.profile:
            log(rank, f"[bench] {mode} stage profile (timed steps)\n" +
                format_report(TRACER.report()))
        if dist:
            el = dist.all_reduce_max_float(el)
        # sharded: every query runs on all ranks; replicated: each rank runs its own stream
        nq = 2 * args.steps * (world if mode == "replicated" else 1)
        return {"qps": nq / el, "ms_per_step": el / args.steps * 1000.0, "warmup_s": warm,
                "results": res, "first": off}

    def one_query_ms(fn, i):
        barrier()
        sync()
        tq = time.perf_counter()
        fn(i).collect()
        sync()
        dtq = time.perf_counter() - tq
        return round((dist.all_reduce_max_float(dtq) if dist else dtq) * 1000, 3)

    # cold: the first query of each kind after createIndex (index HBM load, kernel compile when
    # the on-disk code-object cache is empty, join-index build) — not part of the timed steps
    s.conf.set("spark.hyperspace.mi.index.placement", "sharded")
    from hyperspace_amd.utils.tracing import TRACER, format_report
    cold = {}
    if args.full:
        jit0 = dict(jit_mod.JIT_STATS) if jit_mod is not None else {}
        TRACER.reset()
        cprof = None
        if os.environ.get("HS_BENCH_COLD_PROFILE") and rank == 0:
            import cProfile
            cprof = cProfile.Profile()
            cprof.enable()
        cold = {"q6_cold_ms": one_query_ms(q6, 999), "q3_cold_ms": one_query_ms(q3, 999)}
        if cprof is not None:
            import io
            import pstats
            cprof.disable()
            buf = io.StringIO()
            pstats.Stats(cprof, stream=buf).sort_stats("tottime").print_stats(25)
            log(rank, "[bench] cold queries host profile\n" + buf.getvalue())
        if TRACER.profile:
            log(rank, "[bench] cold queries stage profile\n" + format_report(TRACER.report()))
        if jit_mod is not None:
            # kernels the cold queries compiled with hipRTC vs loaded from the code-object cache
            # (the AOT set of __graft_entry__.build covers the bench's shapes)
            cold["cold_kernels_compiled"] = jit_mod.JIT_STATS["compiled"] - jit0.get("compiled", 0)
            cold["cold_kernels_loaded"] = jit_mod.JIT_STATS["loaded"] - jit0.get("loaded", 0)
        log(rank, f"[bench] cold first queries {cold}")

    # the headline (last) placement is sharded (one query stream over the N GPUs); with --full
    # replicated runs first as a side key
    if world > 1 and args.placement == "both":
        modes = ["replicated", "sharded"] if args.full else ["sharded"]
    else:
        modes = [args.placement if world > 1 else "sharded"]
    ji_key = "spark.hyperspace.mi.joinIndex.enabled"
    ji_run = None
    if on_gpu and args.full:
        # side key: the same steps through the cached join index (headline placement)
        s.conf.set(ji_key, "true")
        ji_run = timed(modes[-1])
        s.conf.set(ji_key, "false")
    runs = {m: timed(m) for m in modes}
    final = modes[-1]
    qps = runs[final]["qps"]
    ms_step = runs[final]["ms_per_step"]
    warm_s = runs[final]["warmup_s"]
    results = runs[final]["results"]

    # ---------------------------------------------------------------- per-query latency
    lat = {}

    def latency(name, fn, reps=5):
        barrier()
        sync()
        tq = time.perf_counter()
        for i in range(reps):
            fn(i).collect()
        sync()
        dtq = (time.perf_counter() - tq) / reps
        lat[name] = round((dist.all_reduce_max_float(dtq) if dist else dtq) * 1000, 3)

    if args.full:
        latency("q6_filter_ms", q6)
        latency("q3_join_ms", q3)
    q3f = None
    if on_gpu and args.full:
        # side key: TPC-H Q3's full shape (3-column group, top 10), fresh literals per query,
        # every query through the full engine path; warm-up first (kernel compile + table size)
        for i in range(2):
            q3_full(2000 + i).collect()
        sync()
        barrier()
        tq = time.perf_counter()
        nq = max(4, args.steps)
        q3f_res = [q3_full(i).collect() for i in range(nq)]
        sync()
        barrier()
        el = time.perf_counter() - tq
        if dist:
            el = dist.all_reduce_max_float(el)
        q3f = {"value": round(nq / el, 3), "ms_per_query": round(el / nq * 1000.0, 3),
               "rows": len(q3f_res[0]), "path": backend.last_path,
               "note": "GROUP BY l_orderkey, o_orderdate, o_shippriority ORDER BY revenue DESC, "
                       "o_orderdate LIMIT 10 (device hash aggregate + top-k)"}
        if backend.last_path != "native":
            raise RuntimeError(f"q3_full fell back: {backend.fallback_reason}")
    if on_gpu and args.full:
        s.conf.set(ji_key, "true")
        latency("q3_join_index_ms", q3)
        s.conf.set(ji_key, "false")
    lat.update(cold)
    hb = _host_breakdown(args.host_breakdown, (q6, q3), backend, sync, barrier) \
        if args.host_breakdown and on_gpu else None
    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, results[-1])
    side = _side_configs(args, sf) \
        if args.full and on_gpu and world == 1 and not args.no_side else {}

    # ---------------------------------------------------------------- cross-check
    check = None
    # multi-rank: the un-indexed plan runs on the host oracle over all files (slow), so only
    # cross-check small scale factors there
    if args.full and not args.no_crosscheck and (world == 1 or sf <= 10):
        s.disableHyperspace()
        tc = time.perf_counter()
        first = runs[final]["first"]   # the literals of this rank's first timed step
        n6 = q6(first).collect()[0][0]
        n3 = sorted(q3(first).collect())
        noidx_s = time.perf_counter() - tc
        s.enableHyperspace()
        i6 = results[0][0][0][0]
        i3 = sorted(results[0][1])
        ok6 = abs(n6 - i6) <= 1e-9 * abs(n6)
        ok3 = len(n3) == len(i3) and all(a[2] == b[2] and abs(a[1] - b[1]) <= 1e-9 * abs(b[1])
                                         for a, b in zip(i3, n3))
        if q3f is not None:
            nf = q3_full(0).collect()
            gf = q3f_res[0]
            okf = len(nf) == len(gf) and all(
                a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and
                abs(a[3] - b[3]) <= 1e-9 * abs(b[3]) for a, b in zip(gf, nf))
            ok3 = ok3 and okf
            if not okf:
                raise RuntimeError(f"q3_full cross-check failed: {gf} vs {nf}")
        check = {"index_vs_full_scan_match": bool(ok6 and ok3),
                 "no_index_q6_plus_q3_s": round(noidx_s, 3)}
        if not (ok6 and ok3):
            raise RuntimeError(f"cross-check failed: {i6} vs {n6}; {i3} vs {n3}")

    base = _cpu_baseline(sf) if on_gpu else None
    vs = round(qps / base["value"], 2) if base and base.get("value") else None
    if rank == 0:
        out = {"metric": METRIC, "value": round(qps, 3), "unit": "queries/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 3),
               "higher_is_better": True,
               "scaling": "weak" if final == "replicated" else "strong", "vs_baseline": vs,
               "dtype": "fp64", "data": "synthetic",
               "config": {"model": f"tpch-sf{sf:g} lineitem/orders covering indexes",
                          "global_batch": 2, "seq_len": 0,
                          "parallelism": (f"replicated-dp{world}" if final == "replicated" else
                                          f"bucket-dp{world}") if on_gpu else "cpu-host",
                          "placement": final,
                          "num_buckets": args.buckets, "source_files": nfiles,
                          "device": args.device},
               "index_build_gbps": round(build_gbps, 3),
               "index_build_src_gbps": round(src_gbps, 3), "engine_start_s": round(engine_s, 3),
               "index_build_s": round(build_s, 3), "index_codec": args.codec,
               "bytes_over_xgmi": int(xgmi_bytes),
               "index_bytes_on_disk": _dir_bytes(idx_root),
               "index_build": per_index, "warmup_s": round(warm_s, 3),
               "datagen_s": round(gen_s, 2), "inflight": args.inflight, "full": args.full}
        if args.full:
            out["latency"] = lat
            out["crosscheck"] = check
        if q3f is not None:
            out["q3_full"] = q3f
        if hb is not None:
            out["host_breakdown"] = hb
        out.update(side)
        if ji_run is not None:
            out["join_index"] = {"value": round(ji_run["qps"], 3),
                                 "ms_per_step": round(ji_run["ms_per_step"], 3),
                                 "note": "Q3 with join indexes enabled: the run-keyed join keeps its key "
                                         "match (per-run right row, right columns copied into run "
                                         "order) instead of re-matching per query"}
        for m in runs:
            if m != final:
                out[m] = {"value": round(runs[m]["qps"], 3),
                          "ms_per_step": round(runs[m]["ms_per_step"], 3),
                          "scaling": "weak" if m == "replicated" else "strong"}
        if base:
            out["cpu_baseline"] = {"value": base["value"], "source": base.get("source")}
        if on_gpu:
            out["device_cache"] = {"hits": backend.cache.hits, "misses": backend.cache.misses}
        if not on_gpu:
            out["n_gpus"] = 0
        print(json.dumps(out), flush=True)
        if args.record_baseline and not on_gpu:
            out["source"] = f"bench.py --device cpu --sf {sf:g} (this repo's pyarrow host engine)"
            with open(os.path.join(ROOT, "profiles", f"cpu_baseline_sf{sf:g}.json"), "w") as f:
                json.dump(out, f, indent=1)
    if dist:
        barrier()
        torch.distributed.destroy_process_group()


def _dump_outputs(out_dir, step_result) -> None:
    """Write what one step's two queries returned to their caller (``collect()``'s rows) as
    ``<out_dir>/<name>.npy``, float64, one array per result column: ``q6_revenue`` (one row) and
    ``q3_o_shippriority`` / ``q3_revenue`` / ``q3_lines`` (one row per group, ordered by the group
    key; a NULL is NaN).  The data and the literals of a step depend only on the arguments, so two
    runs with the same arguments write comparable files."""
    import numpy as np
    q6_rows, q3_rows = step_result
    q3_rows = sorted(q3_rows, key=lambda r: (r[0] is not None, r[0]))
    cols = {"q6_revenue": [r[0] for r in q6_rows],
            "q3_o_shippriority": [r[0] for r in q3_rows],
            "q3_revenue": [r[1] for r in q3_rows],
            "q3_lines": [r[2] for r in q3_rows]}
    os.makedirs(out_dir, exist_ok=True)
    for name, vals in cols.items():
        arr = np.array([np.nan if v is None else v for v in vals], dtype=np.float64)
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def _side_configs(args, sf) -> dict:
    """BASELINE configs #3-#4's real query shapes at N = 1, through ``benchmarks/configs.py``
    (own sessions over the same generated data, each result checked against the host oracle
    with Hyperspace disabled): ``q3_3way`` and ``hybrid``.  Errors are recorded, not raised."""
    import argparse as _ap
    import traceback
    sys.path.insert(0, os.path.join(ROOT, "benchmarks"))
    import configs as CF
    ns = _ap.Namespace(data_dir=args.data_dir, device="gpu", buckets=args.buckets,
                       steps=max(args.steps, 10), sf=sf)
    out = {}
    from hyperspace_amd.exec.gpu import release_process_device_memory
    for name, fn in (("q3_3way", CF.config_q3_3way), ("hybrid", CF.config_hybrid)):
        t0 = time.perf_counter()
        try:
            # each config runs in sessions of its own: free what the earlier ones hold in HBM
            release_process_device_memory()
            r = fn(ns)
            if name == "q3_3way":
                out[name] = {"q3_3way_ms": r["q3_3way_ms"], "value": r["queries_per_s"],
                             "path": r["path"], "match": r["match"],
                             "indexes_in_plan": r["indexes_in_plan"],
                             "semi_join": r.get("semi_join")}
            else:
                out[name] = {"hybrid_qps": r["hybrid_queries_per_s"],
                             "refreshed_qps": r["refreshed_queries_per_s"],
                             "hybrid_vs_refreshed": round(r["hybrid_queries_per_s"] /
                                                          r["refreshed_queries_per_s"], 3),
                             "appended_files": r["appended_files"],
                             "incremental_refresh_s": r["incremental_refresh_s"],
                             "path": r["path"], "match": r["hybrid_matches_refreshed"],
                             "bucket_union_in_plan": r["bucket_union_in_plan"]}
        except Exception as e:  # noqa: BLE001 — a side key never stops the headline record
            out[name] = {"error": f"{type(e).__name__}: {e}",
                         "trace": traceback.format_exc()[-1500:]}
        out[name]["wall_s"] = round(time.perf_counter() - t0, 2)
        print(f"[bench] side config {name}: {out[name]}", file=sys.stderr, flush=True)
    release_process_device_memory()   # the cross-check's un-indexed scans need the room
    return out


def _host_breakdown(n, fns, backend, sync, barrier) -> dict:
    """Host milliseconds per query of each phase of the serving loop (``inflight`` 2), on the
    path the timed steps take (``DataFrame.collect_async``): building the DataFrame; submitting
    it - plan-cache lookup, literal binding into the cached plan and the executor's prepared
    lowering + kernel launches (``QueryExecution._submit_bound``); and waiting for its result
    (which includes device time the host did not overlap).  ``bound`` = share of queries that
    took the bound-plan fast path."""
    from collections import deque
    ph = {"build": 0.0, "submit": 0.0, "result": 0.0}
    pend = deque()
    bound = 0
    barrier()
    sync()
    t_all = time.perf_counter()
    for i in range(n):
        for fn in fns:
            t0 = time.perf_counter()
            df = fn(5000 + i)
            t1 = time.perf_counter()
            qe = df.queryExecution
            fut = qe.to_arrow_async()          # = DataFrame.collect_async's submission
            t3 = time.perf_counter()
            ph["build"] += t1 - t0
            ph["submit"] += t3 - t1
            bound += qe._executed is None
            pend.append(fut)
        while len(pend) > 2:
            t4 = time.perf_counter()
            pend.popleft().result()
            ph["result"] += time.perf_counter() - t4
    while pend:
        t4 = time.perf_counter()
        pend.popleft().result()
        ph["result"] += time.perf_counter() - t4
    sync()
    nq = n * len(fns)
    out = {k: round(v / nq * 1000.0, 4) for k, v in ph.items()}
    out["wall_ms_per_query"] = round((time.perf_counter() - t_all) / nq * 1000.0, 4)
    out["queries"] = nq
    out["bound"] = round(bound / max(nq, 1), 3)
    return out


if __name__ == "__main__":
    main()
