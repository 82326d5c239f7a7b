"""Expression evaluation over pyarrow tables (the CPU oracle's expression engine).

Columns inside executors are keyed ``<name>#<exprId>`` so self-joins never collide.
Comparison operands are coerced the way Spark's analyzer would (string literal vs date column ->
date, int vs double -> double).
"""
from __future__ import annotations

import datetime

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from ..plan import expressions as E


def key(a: E.Attribute) -> str:
    return f"{a.name}#{a.expr_id}"


def _coerce_literal(lit: E.Literal, target: pa.DataType):
    v = lit.value
    if v is None:
        return pa.scalar(None, target)
    if pa.types.is_date32(target) and isinstance(v, str):
        return pa.scalar(datetime.date.fromisoformat(v[:10]), pa.date32())
    if pa.types.is_timestamp(target) and isinstance(v, str):
        return pa.scalar(datetime.datetime.fromisoformat(v), target)
    if pa.types.is_timestamp(target) and isinstance(v, datetime.date) and \
            not isinstance(v, datetime.datetime):
        return pa.scalar(datetime.datetime(v.year, v.month, v.day), target)
    if (pa.types.is_string(target) or pa.types.is_large_string(target)) and not isinstance(v, str):
        return pa.scalar(str(v), pa.string())
    if pa.types.is_integer(target) and isinstance(v, float):
        return pa.scalar(v, pa.float64())
    if pa.types.is_floating(target) and isinstance(v, (int, float)) and not isinstance(v, bool):
        return pa.scalar(float(v), pa.float64())
    if pa.types.is_integer(target) and isinstance(v, int) and not isinstance(v, bool):
        return pa.scalar(v, pa.int64())
    if pa.types.is_decimal(target) and isinstance(v, (int, float)):
        return pa.scalar(float(v), pa.float64())
    return pa.scalar(v, lit.data_type)


def _numeric_align(a, b):
    ta, tb = a.type, b.type
    if pa.types.is_decimal(ta):
        a = pc.cast(a, pa.float64())
    if pa.types.is_decimal(tb):
        b = pc.cast(b, pa.float64())
    ta, tb = a.type, b.type
    if (pa.types.is_floating(ta) and pa.types.is_integer(tb)) or \
            (pa.types.is_integer(ta) and pa.types.is_floating(tb)):
        a, b = pc.cast(a, pa.float64()), pc.cast(b, pa.float64())
    elif pa.types.is_integer(ta) and pa.types.is_integer(tb) and ta != tb:
        a, b = pc.cast(a, pa.int64()), pc.cast(b, pa.int64())
    return a, b


def _operands(e: E.BinaryExpression, t: pa.Table):
    l, r = e.left, e.right
    if isinstance(r, E.Literal) and not isinstance(l, E.Literal):
        lv = eval_expr(l, t)
        return _numeric_align(lv, _coerce_literal(r, lv.type))
    if isinstance(l, E.Literal) and not isinstance(r, E.Literal):
        rv = eval_expr(r, t)
        return _numeric_align(_coerce_literal(l, rv.type), rv)
    return _numeric_align(eval_expr(l, t), eval_expr(r, t))


_CMP = {E.EqualTo: pc.equal, E.NotEqual: pc.not_equal, E.LessThan: pc.less,
        E.LessThanOrEqual: pc.less_equal, E.GreaterThan: pc.greater,
        E.GreaterThanOrEqual: pc.greater_equal}
_ARITH = {E.Add: pc.add, E.Subtract: pc.subtract, E.Multiply: pc.multiply}


def _is_num(t: pa.DataType) -> bool:
    return pa.types.is_integer(t) or pa.types.is_floating(t)


def eval_expr(e: E.Expression, t: pa.Table):
    if isinstance(e, E.Attribute):
        return t.column(key(e))
    if isinstance(e, E.Alias):
        return eval_expr(e.child, t)
    if isinstance(e, E.Literal):
        return pa.array([e.value] * t.num_rows, e.data_type if e.value is not None else pa.null())
    if type(e) in _CMP:
        a, b = _operands(e, t)
        return _CMP[type(e)](a, b)
    if isinstance(e, E.And):
        return pc.and_kleene(eval_expr(e.left, t), eval_expr(e.right, t))
    if isinstance(e, E.Or):
        return pc.or_kleene(eval_expr(e.left, t), eval_expr(e.right, t))
    if isinstance(e, E.Not):
        return pc.invert(eval_expr(e.child, t))
    if isinstance(e, E.IsNull):
        return pc.is_null(eval_expr(e.child, t))
    if isinstance(e, E.IsNotNull):
        return pc.is_valid(eval_expr(e.child, t))
    if isinstance(e, (E.In, E.InSet)):
        v = eval_expr(e.value, t)
        raw = [x.value for x in e.values] if isinstance(e, E.In) else list(e.hset)
        lits = [_coerce_literal(E.Literal(x), v.type).as_py() for x in raw if x is not None]
        vtype = v.type
        if pa.types.is_integer(vtype) and any(isinstance(x, float) for x in lits):
            v = pc.cast(v, pa.float64())
            vtype = pa.float64()
        vs = pa.array(lits, vtype if not pa.types.is_dictionary(vtype) else vtype.value_type)
        return pc.is_in(v, value_set=vs)
    if isinstance(e, E.Like):
        v = eval_expr(e.child, t)
        if pa.types.is_dictionary(v.type):
            v = pc.cast(v, v.type.value_type)
        return pc.match_like(v, e.pattern)
    if type(e) in _ARITH:
        a, b = _operands(e, t)
        return _ARITH[type(e)](a, b)
    if isinstance(e, E.Remainder):
        return _remainder(*_operands(e, t), t.num_rows, e.data_type)
    if isinstance(e, E.Divide):
        # Spark: a double division, NULL for a zero divisor
        a, b = _operands(e, t)
        b = pc.cast(b, pa.float64())
        q = pc.divide(pc.cast(a, pa.float64()), b)
        return pc.if_else(pc.equal(b, 0.0), pa.scalar(None, pa.float64()), q)
    if isinstance(e, E.NormalizeNaNAndZero):
        v = eval_expr(e.child, t)
        if not pa.types.is_floating(v.type):
            return v
        return pc.if_else(pc.is_nan(v), pa.scalar(float("nan"), v.type),
                          pc.add(v, pa.scalar(0.0, v.type)))
    if isinstance(e, E.CaseWhen):
        # the first branch whose condition is TRUE (not NULL) wins; no branch: ELSE, or NULL
        rt = e.data_type

        def value(x):
            v = eval_expr(x, t)
            if pa.types.is_dictionary(v.type):
                v = pc.cast(v, v.type.value_type)
            if pa.types.is_decimal(v.type) and pa.types.is_floating(rt):
                v = pc.cast(v, pa.float64())
            return v if v.type == rt else pc.cast(v, rt, safe=False)
        out = value(e.else_value) if e.else_value is not None else pa.nulls(t.num_rows, rt)
        for c, v in reversed(e.branches):
            cond = eval_expr(c, t)
            if pa.types.is_null(cond.type):
                continue
            out = pc.if_else(pc.fill_null(cond, False), value(v), out)
        return out
    if isinstance(e, E.DateFunction):
        return _date_function(e, t)
    if isinstance(e, E.Cast):
        v = eval_expr(e.child, t)
        if _is_num(v.type) and _is_num(e.dtype):
            if pa.types.is_floating(v.type) and pa.types.is_integer(e.dtype):
                return _float_to_int(v, e.dtype)
            # Spark's numeric casts truncate toward zero and wrap (non-ANSI)
            return pc.cast(v, e.dtype, safe=False)
        return pc.cast(v, e.dtype)
    raise NotImplementedError(f"cannot evaluate {type(e).__name__}")


def _flat(v):
    return v.combine_chunks() if isinstance(v, pa.ChunkedArray) else v


def _date_arg(x: E.Expression, t: pa.Table):
    """A date argument as a date32 array: a timestamp is its UTC date (floor of the day)."""
    v = _flat(eval_expr(x, t))
    if pa.types.is_null(v.type):
        return pa.nulls(len(v), pa.date32())
    if pa.types.is_timestamp(v.type):
        per_day = {"s": 86400, "ms": 86400 * 10 ** 3, "us": 86400 * 10 ** 6,
                   "ns": 86400 * 10 ** 9}[v.type.unit]
        ticks = np.asarray(pc.fill_null(v.cast(pa.int64()), 0).to_numpy(zero_copy_only=False))
        days = np.floor_divide(ticks, per_day).astype(np.int32)
        return pa.array(days, pa.int32(), mask=_null_mask(v)).cast(pa.date32())
    return v if pa.types.is_date32(v.type) else pc.cast(v, pa.date32())


def _null_mask(*arrays) -> np.ndarray:
    bad = np.zeros(len(arrays[0]), dtype=bool)
    for a in arrays:
        if a.null_count:
            bad |= np.asarray(pc.is_null(a).to_numpy(zero_copy_only=False))
    return bad


def _days(v) -> np.ndarray:
    """int32 day numbers of a date32 array (NULLs as 0)."""
    return np.asarray(pc.fill_null(v.cast(pa.int32()), 0).to_numpy(zero_copy_only=False))


def _int_arg(x: E.Expression, t: pa.Table):
    v = _flat(eval_expr(x, t))
    if pa.types.is_null(v.type):
        return pa.nulls(len(v), pa.int32())
    return pc.cast(v, pa.int32())


def _month_start(m: np.ndarray) -> np.ndarray:
    """Day numbers (int64) of the first days of the ``datetime64[M]`` months ``m``."""
    return m.astype("datetime64[D]").astype(np.int64)


def _date_function(e: E.DateFunction, t: pa.Table):
    """The date functions: the parts through ``pyarrow.compute``, day arithmetic on int32 day
    numbers, month arithmetic through numpy ``datetime64[M]`` (pyarrow has no add_months)."""
    d = _date_arg(e.children[0], t)
    part = {E.Year: pc.year, E.Quarter: pc.quarter, E.Month: pc.month, E.DayOfMonth: pc.day,
            E.DayOfYear: pc.day_of_year, E.WeekOfYear: pc.iso_week}.get(type(e))
    if part is not None:
        return pc.cast(part(d), pa.int32())
    if isinstance(e, E.WeekDay):
        return pc.cast(pc.day_of_week(d), pa.int32())               # Monday = 0
    if isinstance(e, E.DayOfWeek):
        wd = pc.cast(pc.day_of_week(d, count_from_zero=False, week_start=7), pa.int32())
        return wd                                                   # Sunday = 1
    dn = _days(d)
    if isinstance(e, (E.DateAdd, E.DateSub, E.AddMonths)):
        n = _int_arg(e.children[1], t)
        bad = _null_mask(d, n)
        nv = np.asarray(pc.fill_null(n, 0).to_numpy(zero_copy_only=False)).astype(np.int32)
        if not isinstance(e, E.AddMonths):
            with np.errstate(over="ignore"):
                out = dn + nv if isinstance(e, E.DateAdd) else dn - nv
            return pa.array(out.astype(np.int32), pa.int32(), mask=bad).cast(pa.date32())
        m = dn.astype("datetime64[D]").astype("datetime64[M]")
        dom = dn.astype(np.int64) - _month_start(m)                 # day of month - 1
        m2 = m + nv.astype(np.int64)
        first = _month_start(m2)
        out = first + np.minimum(dom, _month_start(m2 + 1) - first - 1)
        return pa.array(out.astype(np.int32), pa.int32(), mask=bad).cast(pa.date32())
    if isinstance(e, E.DateDiff):
        s = _date_arg(e.children[1], t)
        out = dn.astype(np.int64) - _days(s).astype(np.int64)
        return pa.array(out.astype(np.int32), pa.int32(), mask=_null_mask(d, s))
    bad = _null_mask(d)
    m = dn.astype("datetime64[D]").astype("datetime64[M]")
    if isinstance(e, E.LastDay):
        out = _month_start(m + 1) - 1
    else:
        level = e.level
        if level is None:
            return pa.nulls(len(d), pa.date32())
        if level == "week":
            out = dn.astype(np.int64) - np.mod(dn.astype(np.int64) + 3, 7)   # 1970-01-01: Thursday
        elif level == "month":
            out = _month_start(m)
        elif level == "quarter":
            mi = m.astype(np.int64)                                  # months since 1970-01
            out = _month_start((mi - np.mod(mi, 3)).astype("datetime64[M]"))
        else:
            out = m.astype("datetime64[Y]").astype("datetime64[D]").astype(np.int64)
    return pa.array(out.astype(np.int32), pa.int32(), mask=bad).cast(pa.date32())


def _remainder(a, b, n: int, dtype=None):
    """Spark ``%``: truncated remainder (sign of the dividend), NULL for a zero divisor or a
    NULL operand; ``fmod`` for floating-point operands; Long.MIN_VALUE % -1 = 0.  Either operand
    may be a scalar (a literal dividend or divisor): both are broadcast to the ``n`` rows first.
    The result takes the expression's type ``dtype``."""
    import numpy as np

    def arr(x):
        if isinstance(x, pa.Scalar):
            return pa.array([x.as_py()] * n, x.type)
        return x.combine_chunks() if isinstance(x, pa.ChunkedArray) else x
    a, b = arr(a), arr(b)
    f = pa.types.is_floating(a.type) or pa.types.is_floating(b.type)
    out_t = pa.float64() if f else pa.int64()
    av = np.asarray(pc.fill_null(pc.cast(a, out_t), 0).to_numpy(zero_copy_only=False))
    bv = np.asarray(pc.fill_null(pc.cast(b, out_t), 0).to_numpy(zero_copy_only=False))
    bad = np.asarray(pc.or_kleene(pc.is_null(a), pc.is_null(b)).to_numpy(zero_copy_only=False))
    bad = bad | (bv == 0)
    if f:
        with np.errstate(invalid="ignore"):
            r = np.fmod(av, np.where(bad, 1.0, bv))
    else:
        safe = np.where(bad | (bv == -1), 1, bv)
        r = np.fmod(av, safe)          # C / JVM truncated remainder
        r = np.where(bv == -1, 0, r)
    out = pa.array(r, out_t, mask=bad)
    if dtype is not None and out.type != dtype and (pa.types.is_integer(dtype) or
                                                    pa.types.is_floating(dtype)):
        out = pc.cast(out, dtype, safe=False)
    return out


def _float_to_int(v, dtype: pa.DataType):
    """Spark (non-ANSI) float -> integral cast: truncate toward zero, NaN -> 0, saturate to the
    long range (d2l) for a long target, to the int range (d2i) otherwise; a short / byte target
    then wraps (``toInt.toShort``).  Explicit clamps: an out-of-range ``pc.cast`` is undefined."""
    lo, hi = ((-2.0 ** 63, 2.0 ** 63) if pa.types.is_int64(dtype)
              else (-2147483648.0, 2147483647.0))
    f = pc.cast(v, pa.float64())
    f = pc.if_else(pc.is_nan(f), 0.0, f)
    f = pc.trunc(pc.min_element_wise(pc.max_element_wise(f, lo, skip_nulls=False), hi,
                                     skip_nulls=False))
    if pa.types.is_int64(dtype):
        big = pc.greater_equal(f, 2.0 ** 63)
        out = pc.cast(pc.if_else(big, 0.0, f), pa.int64(), safe=False)
        return pc.if_else(big, pa.scalar(2**63 - 1, pa.int64()), out)
    return pc.cast(pc.cast(f, pa.int64(), safe=False), dtype, safe=False)


def eval_predicate(e: E.Expression, t: pa.Table) -> pa.Table:
    mask = eval_expr(e, t)
    if isinstance(mask, pa.ChunkedArray):
        mask = mask.combine_chunks()
    return t.filter(mask, null_selection_behavior="drop")


def to_numpy(col) -> np.ndarray:
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    return col.to_numpy(zero_copy_only=False)
