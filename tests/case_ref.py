"""References for the CASE WHEN tests, independent of hyperspace_amd.exec.

* ``case_value`` / ``aggregate``: plain Python, row by row, with Spark's rules - the first branch
  whose condition is TRUE wins (None is not TRUE), no branch taken gives the ELSE value or None;
  aggregates skip None, ``count`` counts the others, an empty ``sum`` / ``min`` / ``max`` / ``avg``
  is None.
* ``scan_guarded``: the numpy reference of tests/scan_ref.py extended by per-aggregate guards.  An
  aggregate is ``(kind, terms, guard)`` with ``guard`` None or ``(preds, const, else_)``: the CNF
  ``preds`` (scan_ref predicate tuples) decides per row between the THEN value - the product of
  ``terms``, or the constant ``const`` when there are none - and the ELSE constant ``else_``
  (None: no ELSE, the row does not count).
"""
import math

import numpy as np

import scan_ref as R


def case_value(branches, else_value=None):
    """``branches``: [(condition, value)] of one row, already evaluated (None = NULL)."""
    for cond, value in branches:
        if cond is True:
            return value
    return else_value


def aggregate(name, values):
    """Spark's sum / count / min / max / avg over a list with None for NULL.  NaN is a value:
    larger than every other one for min / max (Spark's ordering), and it poisons sum / avg."""
    vals = [v for v in values if v is not None]
    if name == "count":
        return len(vals)
    if not vals:
        return None
    if name == "sum":
        return math.fsum(vals) if all(isinstance(v, float) and math.isfinite(v) for v in vals) \
            else sum(vals)
    if name == "avg":
        return math.fsum(float(v) for v in vals) / len(vals) \
            if all(math.isfinite(float(v)) for v in vals) else sum(float(v) for v in vals) / len(vals)

    def key(v):
        return (1, 0) if isinstance(v, float) and v != v else (0, v)
    return min(vals, key=key) if name == "min" else max(vals, key=key)


def scan_guarded(cols, preds, aggs, group_col=-1, num_groups=1, group_base=0, ranges=()):
    """``scan_ref.scan`` with guarded aggregates; same result object."""
    n = len(next(iter(cols.values()))[0])
    passing = R.cnf(preds, cols, n)
    in_range = [np.arange(s, s + ln, dtype=np.int64) for s, ln in ranges]
    rows = np.concatenate(in_range) if in_range else np.zeros(0, np.int64)
    rows = rows[passing[rows]]
    grouped = group_col >= 0
    G = num_groups if grouped else 1
    res = R.ScanResult(rows, G, len(aggs))
    if grouped:
        key = R.image_i64(cols[group_col])[rows].astype(object) - int(group_base)
        kok = R._valid(cols[group_col], n)[rows]
        inside = np.array([bool(v) and 0 <= k < G for k, v in zip(key, kok)], bool)
        slot = np.where(inside, np.where(inside, key, 0).astype(np.int64), -1)
    else:
        slot = np.zeros(len(rows), np.int64)
    for a, (kind, terms, guard) in enumerate(aggs):
        ok = np.ones(len(rows), bool)
        val = np.ones(len(rows))
        if kind != R.AK_COUNT_STAR:
            for c, alpha, beta in terms:
                ok = ok & R._valid(cols[c], n)[rows]
                with np.errstate(invalid="ignore", over="ignore"):
                    val = val * (np.float64(alpha) + np.float64(beta) * R.image_f64(cols[c])[rows])
        if guard is not None:
            gpreds, const, else_ = guard
            g = R.cnf(gpreds, cols, n)[rows] if gpreds is not None else np.zeros(len(rows), bool)
            if not terms:
                val = np.full(len(rows), np.float64(const))
            val = np.where(g, val, np.float64(0.0 if else_ is None else else_))
            ok = np.where(g, ok, else_ is not None)
        ok = ok & (slot >= 0)
        for gi in range(G):
            m = ok & (slot == gi)
            v = val[m]
            res.count[gi, a] = int(m.sum())
            if kind in (R.AK_SUM, R.AK_COUNT):
                fin = bool(np.isfinite(v).all())
                res.sum[gi, a] = math.fsum(v.tolist()) if fin else float(np.sum(v))
                res.abs_sum[gi, a] = math.fsum(np.abs(v).tolist()) if fin else np.inf
            res.mn[gi, a] = np.fmin.reduce(v, initial=np.inf)
            res.mx[gi, a] = np.fmax.reduce(v, initial=-np.inf)
    return res
