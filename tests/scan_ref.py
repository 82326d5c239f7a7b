"""Plain numpy reference of the scan predicate / aggregate contract (csrc/kernels/hs_scan.h).

Independent of hyperspace_amd.exec: it knows the contract only as hs_scan.h documents it.

  * columns     ``(values ndarray, valid ndarray or None, hs_type)`` per slot (dict or list)
  * predicates  ``(kind, op, col, col2, group, ilit, flit, set)`` tuples, equal ``group`` values
                adjacent (the CNF is sorted by group): OR inside a group, AND across groups
  * aggregates  ``(kind, [(col, alpha, beta), ...])``: the value of a row is
                prod_t (alpha_t + beta_t * col_t) in float64
  * grouping    ``group_col`` (slot or -1), ``num_groups``, ``group_base``: a dense key domain
                [base, base + G); a null or outside key contributes to no slot
  * ranges      ``(rstart, rlen)`` pairs, evaluated in the order given

Semantics: a leaf over a null input is false (IS_NULL / NOT_NULL excepted), ``*_COL`` is false
when either side is null; integer kinds compare the int64 image of the column, float kinds the
float64 image, under IEEE rules (NaN fails everything but NE); IN_SET / BITMAP with OP_NE negate
on valid rows only; BITMAP tests bit (value - ilit) of the 64-bit words in ``set`` and finds
nothing outside [0, 64 * len(set)); AK_COUNT counts rows whose every term is valid,
AK_COUNT_STAR counts passing rows.
"""
import math

import numpy as np

I8, I16, I32, I64, F32, F64, BOOL, U32, U64 = range(9)
PK_INT_LIT, PK_FLT_LIT, PK_INT_COL, PK_FLT_COL, PK_IS_NULL, PK_NOT_NULL, PK_IN_SET, PK_BITMAP, \
    PK_TRUE = range(9)
OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE = range(6)
AK_SUM, AK_COUNT, AK_MIN, AK_MAX, AK_COUNT_STAR = range(5)

NP_TYPE = {I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, F32: np.float32,
           F64: np.float64, BOOL: np.uint8, U32: np.uint32, U64: np.uint64}

_CMP = {OP_EQ: np.equal, OP_NE: np.not_equal, OP_LT: np.less, OP_LE: np.less_equal,
        OP_GT: np.greater, OP_GE: np.greater_equal}


def _valid(col, n):
    v = col[1]
    return np.ones(n, bool) if v is None else np.asarray(v).astype(bool)


def image_i64(col):
    """int64 image of a column (a C cast: floats truncate toward zero; non-finite and
    out-of-range floats have no defined image and become 0 here)."""
    x = np.asarray(col[0])
    if x.dtype.kind == "f":
        y = np.trunc(x.astype(np.float64))
        ok = np.isfinite(y) & (np.abs(y) < 2.0 ** 63)
        return np.where(ok, y, 0.0).astype(np.int64)
    return x.astype(np.int64)


def image_f64(col):
    return np.asarray(col[0]).astype(np.float64)


def leaf(pred, cols):
    """Truth value of one leaf for every row of the table."""
    kind, op, c, c2, _group, ilit, flit, pset = pred
    n = len(next(iter(cols.values()))[0]) if isinstance(cols, dict) else len(cols[0][0])
    if kind == PK_TRUE:
        return np.ones(n, bool)
    ok = _valid(cols[c], n)
    if kind == PK_IS_NULL:
        return ~ok
    if kind == PK_NOT_NULL:
        return ok
    with np.errstate(invalid="ignore"):
        if kind == PK_INT_LIT:
            r = _CMP[op](image_i64(cols[c]), np.int64(ilit))
        elif kind == PK_FLT_LIT:
            r = _CMP[op](image_f64(cols[c]), np.float64(flit))
        elif kind == PK_INT_COL:
            ok = ok & _valid(cols[c2], n)
            r = _CMP[op](image_i64(cols[c]), image_i64(cols[c2]))
        elif kind == PK_FLT_COL:
            ok = ok & _valid(cols[c2], n)
            r = _CMP[op](image_f64(cols[c]), image_f64(cols[c2]))
        elif kind == PK_IN_SET:
            found = np.isin(image_i64(cols[c]), np.asarray(pset, np.int64))
            r = found if op == OP_EQ else ~found
        elif kind == PK_BITMAP:
            words = np.asarray(pset).astype(np.uint64)
            bit = image_i64(cols[c]).astype(object) - int(ilit)   # no int64 wrap-around
            found = np.zeros(n, bool)
            for i, b in enumerate(bit):
                if 0 <= b < 64 * len(words):
                    found[i] = (int(words[b >> 6]) >> (b & 63)) & 1
            r = found if op == OP_EQ else ~found
        else:
            raise ValueError(f"predicate kind {kind}")
    return ok & r


def cnf(preds, cols, n):
    """Pass mask of the CNF over every row of the table."""
    res = np.ones(n, bool)
    seen = set()
    i = 0
    while i < len(preds):
        g = preds[i][4]
        assert g not in seen, "predicates of one group must be adjacent"
        seen.add(g)
        gval = np.zeros(n, bool)
        while i < len(preds) and preds[i][4] == g:
            gval |= leaf(preds[i], cols)
            i += 1
        res &= gval
    return res


class ScanResult:
    """rows: passing row ids in range order.  Per output slot [g, a] (g = 0 for a global
    aggregate): count (exact), sum (math.fsum of the per-row products), abs_sum
    (sum of |product|), mn / mx (np.fmin / np.fmax over the products; +inf / -inf when empty)."""

    def __init__(self, rows, G, A):
        self.rows = rows
        self.count = np.zeros((G, A), np.int64)
        self.sum = np.zeros((G, A))
        self.abs_sum = np.zeros((G, A))
        self.mn = np.full((G, A), np.inf)
        self.mx = np.full((G, A), -np.inf)


def scan(cols, preds, aggs, group_col=-1, num_groups=1, group_base=0, ranges=()):
    n = len(next(iter(cols.values()))[0]) if isinstance(cols, dict) else len(cols[0][0])
    passing = cnf(preds, cols, n)
    in_range = [np.arange(s, s + ln, dtype=np.int64) for s, ln in ranges]
    rows = np.concatenate(in_range) if in_range else np.zeros(0, np.int64)
    rows = rows[passing[rows]]
    grouped = group_col >= 0
    G = num_groups if grouped else 1
    res = ScanResult(rows, G, len(aggs))
    if grouped:
        key = image_i64(cols[group_col])[rows].astype(object) - int(group_base)
        kok = _valid(cols[group_col], n)[rows]
        inside = np.array([bool(v) and 0 <= k < G for k, v in zip(key, kok)], bool)
        slot = np.where(inside, np.where(inside, key, 0).astype(np.int64), -1)
    else:
        slot = np.zeros(len(rows), np.int64)
    for a, (kind, terms) in enumerate(aggs):
        ok = slot >= 0
        val = np.ones(len(rows))
        if kind != AK_COUNT_STAR:
            for c, alpha, beta in terms:
                ok = ok & _valid(cols[c], n)[rows]
                with np.errstate(invalid="ignore", over="ignore"):
                    val = val * (np.float64(alpha) + np.float64(beta) * image_f64(cols[c])[rows])
        for g in range(G):
            m = ok & (slot == g)
            v = val[m]
            res.count[g, a] = int(m.sum())
            if kind == AK_SUM:       # (non-finite inputs have no exact sum: plain IEEE result)
                fin = bool(np.isfinite(v).all())
                res.sum[g, a] = math.fsum(v.tolist()) if fin else float(np.sum(v))
                res.abs_sum[g, a] = math.fsum(np.abs(v).tolist()) if fin else np.inf
            res.mn[g, a] = np.fmin.reduce(v, initial=np.inf)
            res.mx[g, a] = np.fmax.reduce(v, initial=-np.inf)
    return res
