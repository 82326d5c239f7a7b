#!/usr/bin/env python
"""Device timeline of the bench's timed steps from a gpu.sh `benchtrace` kernel trace: finds the
densest stretch of the headline's query kernels (one Q6 scan per step; two-phase join tags and
phase 2 - bits scan or the candidate kernels, single or pair - beside it), then reports the
stretch's wall time, how much of it the GPU had any kernel running (interval union), the idle
gaps, and per-kernel counts and mean durations.

It also splits what surrounds the big kernels:

* join queue: per phase-2 dispatch, the time from its end to the start of the next phase 1 on
  that queue, split into fold / final-reduction kernels, copy kernels and gaps;
* scan queue: per Q6 chain (the nodes between two scans), the time outside ``hs_jit_scan_agg``.

    python scripts/diag/step_timeline.py gpurun_out/X_bench_ktrace.csv [steps]
"""
import collections
import csv
import sys

PHASE1 = ("hs_jit_run_tags2",)
PHASE2 = ("hs_jit_run_bits_scan", "hs_jit_run_bits_cand")   # (cand covers cand2)
SCAN = ("hs_jit_scan_agg",)
HOT = PHASE1 + PHASE2 + SCAN
FOLD = ("hs_agg_final", "hs_agg_fold")
COPY = ("__amd_rocclr_copyBuffer",)
SMALL = FOLD + COPY + ("hs_range_search", "hs_ranges_to_tiles")


def _stats(name, v):
    if not v:
        print(f"  {name:28s} none")
        return
    v = sorted(v)
    print(f"  {name:28s} n={len(v):4d} mean {sum(v) / len(v) / 1e3:7.1f} us  median "
          f"{v[len(v) // 2] / 1e3:7.1f}  min {v[0] / 1e3:7.1f}  max {v[-1] / 1e3:7.1f}")


def tails(seg, steps):
    """The join queue's tails and the scan queue's chains of the timed stretch ``seg``."""
    qj = collections.Counter(q for n, _, _, q in seg if n.startswith(PHASE1)).most_common(1)
    qs = collections.Counter(q for n, _, _, q in seg if n.startswith(SCAN)).most_common(1)
    if qj:
        rows = [r for r in seg if r[3] == qj[0][0]]
        tot, fold, copy, gap, nodes = [], [], [], [], []
        i = 0
        while i < len(rows):
            if not rows[i][0].startswith(PHASE2):
                i += 1
                continue
            j = i + 1
            while j < len(rows) and not rows[j][0].startswith(PHASE1 + PHASE2):
                j += 1
            if j == len(rows) or not rows[j][0].startswith(PHASE1):
                i = j      # (the pair form without a pair phase 2: A's tail precedes B's phase 2)
                continue
            mid = rows[i + 1:j]
            t = rows[j][1] - rows[i][2]
            f = sum(e - s for n, s, e, _ in mid if n.startswith(FOLD))
            c = sum(e - s for n, s, e, _ in mid if n.startswith(COPY))
            k = sum(e - s for n, s, e, _ in mid)
            tot.append(t)
            fold.append(f)
            copy.append(c)
            gap.append(t - k)
            nodes.append(len(mid))
            i = j
        print(f"join queue {qj[0][0]}: end of phase 2 -> start of the next phase 1 "
              f"({len(tot)} tails, {sum(nodes) / max(len(nodes), 1):.1f} nodes each)")
        _stats("tail", tot)
        _stats("fold / final kernels", fold)
        _stats("copy kernels", copy)
        _stats("gaps", gap)
        print(f"  per step: tail {sum(tot) / steps / 1e3:.1f} us = fold {sum(fold) / steps / 1e3:.1f}"
              f" + copies {sum(copy) / steps / 1e3:.1f} + gaps {sum(gap) / steps / 1e3:.1f}")
    if qs:
        rows = [r for r in seg if r[3] == qs[0][0]]
        small = [e - s for n, s, e, _ in rows if n.startswith(SMALL)]
        scans = [e - s for n, s, e, _ in rows if n.startswith(SCAN)]
        per = collections.defaultdict(list)
        for n, s, e, _ in rows:
            if n.startswith(SMALL):
                per[n.split("(")[0]].append(e - s)
        print(f"scan queue {qs[0][0]}: {len(scans)} scans; kernel time outside hs_jit_scan_agg "
              f"{sum(small) / steps / 1e3:.1f} us per step ({len(small) / max(len(scans), 1):.1f} "
              f"nodes per scan), scan {sum(scans) / steps / 1e3:.1f} us per step")
        for n, d in sorted(per.items()):
            _stats(n[:28], d)


def main():
    rows = [(r["name"], int(r["start"]), int(r["end"]), r["queue"])
            for r in csv.DictReader(open(sys.argv[1]))]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    rows.sort(key=lambda x: x[1])
    # the timed run: the densest window of `steps` Q6 scan launches (one per step) with no
    # join-index or top-k kernel inside (those belong to the side runs)
    idx = [i for i, r in enumerate(rows) if r[0].startswith(SCAN)]
    best = None
    for a in range(len(idx) - steps + 1):
        lo, hi = idx[a], idx[a + steps - 1]
        if any(r[0].startswith(("hs_jit_join_index", "hs_jit_run_bits_topk"))
               for r in rows[lo:hi]):
            continue
        span = rows[hi][1] - rows[lo][1]
        if best is None or span < best[2]:
            best = (lo, hi, span)
    if best is None:
        sys.exit("no timed stretch found")
    lo, hi, _ = best
    # widen to the small kernels of the first and the last step
    while lo > 0 and rows[lo - 1][0].startswith(SMALL):
        lo -= 1
    while hi + 1 < len(rows) and rows[hi + 1][0].startswith(FOLD + COPY):
        hi += 1
    seg = rows[lo:hi + 1]
    t0, t1 = seg[0][1], max(r[2] for r in seg)
    busy, cur_s, cur_e = 0, None, None
    gaps = []
    for _, s, e, _ in seg:
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                busy += cur_e - cur_s
                gaps.append(s - cur_e)
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    busy += cur_e - cur_s
    wall = t1 - t0
    print(f"timed stretch: {len(seg)} kernels, wall {wall / 1e6:.3f} ms "
          f"({wall / 1e3 / steps:.1f} us per step over {steps} steps)")
    print(f"GPU busy (union) {busy / 1e6:.3f} ms = {100 * busy / wall:.1f}%; "
          f"idle gaps: {len(gaps)}, total {sum(gaps) / 1e6:.3f} ms, "
          f"largest {max(gaps, default=0) / 1e3:.1f} us")
    per = collections.defaultdict(list)
    for n, s, e, q in seg:
        per[n.split("(")[0]].append(e - s)
    print(f"{'kernel':44s} {'calls':>6s} {'mean us':>9s} {'per step us':>12s}")
    for n, d in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print(f"{n[:44]:44s} {len(d):6d} {sum(d) / len(d) / 1e3:9.1f} "
              f"{sum(d) / steps / 1e3:12.1f}")
    qs = collections.Counter(q for _, _, _, q in seg)
    print("queues:", dict(qs))
    tails(seg, steps)


if __name__ == "__main__":
    main()
