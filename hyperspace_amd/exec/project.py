"""Computed projections on the device: ``select(a * 2 + b)``, ``select((x > 0) & (y < 5))``.

FilterIndexRule rewrites ``Project(Filter(Relation))`` with an arbitrary project list
(FilterIndexRule.scala:155-191); the reference leaves the expressions to Spark's executors.
Here every computed column of a projection is evaluated by ONE generated elementwise kernel
(hipRTC, ``exec/jit.py``) over the relation's rows: column loads, the expression trees with
Spark's semantics, and one store per output column.  The kernel is cached per expression
*shape* (operators, input types, nullability); literals are kernel arguments, so a new literal
reuses the compiled kernel.

Semantics (Spark non-ANSI, and the host oracle ``exec/arrow_eval.py``):

* arithmetic on integers wraps at the result width; a mixed integer / floating (or decimal)
  operation runs in double;
* ``/`` is a double division; a zero divisor gives NULL;
* casts between numeric types truncate toward zero (integer targets) and wrap;
* comparisons give booleans; AND / OR / NOT follow three-valued (Kleene) logic;
* NULL in, NULL out for everything else.

Date functions (``year(d)``, ``date_add(d, n)``, ``add_months``, ``trunc``, ...) read and produce
dates as int32 day numbers.  Their calendar arithmetic (``DATE_PRELUDE``) is the
days-from-0000-03-01 form in 32-bit unsigned registers: that count is non-negative for every day
of 0001-01-01 ... 9999-12-31, so no era branch is needed, every division is by a constant (a
multiply-high on gfx950, which has no integer divide) and nothing is ever 64 bits wide.  Outside
that range the result is unspecified but still plain integer arithmetic.  The prelude is appended
only to kernels that use it, and it is plain C++ (no HIP builtin), so a host compiler can check
it over every day of the range.
"""
from __future__ import annotations

import datetime
from typing import Dict, List, Tuple

import pyarrow as pa

from ..ops import _lib as NL
from ..plan import expressions as E
from . import jit
from .compile import Unsupported
from .device_table import DeviceColumn

BLOCK = 256

_CTYPE = {NL.I8: "signed char", NL.I16: "short", NL.I32: "int", NL.I64: "long long",
          NL.F32: "float", NL.F64: "double", NL.BOOL: "unsigned char", NL.U32: "unsigned"}
_CMP = {E.EqualTo: "==", E.NotEqual: "!=", E.LessThan: "<", E.LessThanOrEqual: "<=",
        E.GreaterThan: ">", E.GreaterThanOrEqual: ">="}
_ARITH = {E.Add: "+", E.Subtract: "-", E.Multiply: "*"}


DATE_PRELUDE_MARK = "// -- date functions --"
DATE_PRELUDE = DATE_PRELUDE_MARK + r"""
// Proleptic Gregorian calendar over int32 day numbers (days since 1970-01-01), exact for
// 0001-01-01 ... 9999-12-31.  z = days + 719468 counts from 0000-03-01 and is >= 306 there.
struct HsCivil { unsigned y, m, d; };
__device__ inline HsCivil hs_civil(int days) {
  const unsigned z = (unsigned)days + 719468u;
  const unsigned era = z / 146097u;
  const unsigned doe = z - era * 146097u;
  const unsigned yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
  const unsigned doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
  const unsigned mp = (5u * doy + 2u) / 153u;
  HsCivil c;
  c.d = doy - (153u * mp + 2u) / 5u + 1u;
  c.m = mp < 10u ? mp + 3u : mp - 9u;
  c.y = yoe + era * 400u + (c.m <= 2u ? 1u : 0u);
  return c;
}
__device__ inline int hs_days(unsigned y, unsigned m, unsigned d) {
  y -= m <= 2u ? 1u : 0u;
  const unsigned era = y / 400u;
  const unsigned yoe = y - era * 400u;
  const unsigned doy = (153u * (m > 2u ? m - 3u : m + 9u) + 2u) / 5u + d - 1u;
  const unsigned doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
  return (int)(era * 146097u + doe - 719468u);
}
// Monday = 0 ... Sunday = 6 (0000-03-01 is a Wednesday)
__device__ inline unsigned hs_weekday(int days) { return ((unsigned)days + 719470u) % 7u; }
__device__ inline int hs_year(int days) { return (int)hs_civil(days).y; }
__device__ inline int hs_quarter(int days) { return (int)((hs_civil(days).m + 2u) / 3u); }
__device__ inline int hs_month(int days) { return (int)hs_civil(days).m; }
__device__ inline int hs_dayofmonth(int days) { return (int)hs_civil(days).d; }
__device__ inline int hs_dayofyear(int days) {
  return (int)((unsigned)days - (unsigned)hs_days(hs_civil(days).y, 1u, 1u)) + 1;
}
// 1 = Sunday ... 7 = Saturday
__device__ inline int hs_dayofweek(int days) { return (int)(((unsigned)days + 719471u) % 7u) + 1; }
// ISO-8601: the week of the year that holds this week's Thursday
__device__ inline int hs_weekofyear(int days) {
  const int thu = (int)((unsigned)days - hs_weekday(days) + 3u);
  const unsigned into = (unsigned)thu - (unsigned)hs_days(hs_civil(thu).y, 1u, 1u);
  return (int)(into / 7u) + 1;
}
__device__ inline int hs_month_first(unsigned y, unsigned m) { return hs_days(y, m, 1u); }
__device__ inline int hs_next_month_first(unsigned y, unsigned m) {
  return m == 12u ? hs_days(y + 1u, 1u, 1u) : hs_days(y, m + 1u, 1u);
}
__device__ inline int hs_last_day(int days) {
  const HsCivil c = hs_civil(days);
  return (int)((unsigned)hs_next_month_first(c.y, c.m) - 1u);
}
// Spark 3: the day of month is kept, clamped to the target month's length
__device__ inline int hs_add_months(int days, int n) {
  const HsCivil c = hs_civil(days);
  const unsigned total = c.y * 12u + (c.m - 1u) + (unsigned)n;
  const unsigned y = total / 12u;
  const unsigned m = total - y * 12u + 1u;
  const unsigned first = (unsigned)hs_month_first(y, m);
  const unsigned len = (unsigned)hs_next_month_first(y, m) - first;
  return (int)(first + (c.d < len ? c.d : len) - 1u);
}
__device__ inline int hs_trunc_year(int days) { return hs_days(hs_civil(days).y, 1u, 1u); }
__device__ inline int hs_trunc_quarter(int days) {
  const HsCivil c = hs_civil(days);
  return hs_days(c.y, (c.m - 1u) / 3u * 3u + 1u, 1u);
}
__device__ inline int hs_trunc_month(int days) {
  return (int)((unsigned)days - hs_civil(days).d + 1u);
}
__device__ inline int hs_trunc_week(int days) { return (int)((unsigned)days - hs_weekday(days)); }
"""

_DATE_PART = {E.Year: "hs_year", E.Quarter: "hs_quarter", E.Month: "hs_month",
              E.DayOfMonth: "hs_dayofmonth", E.DayOfYear: "hs_dayofyear",
              E.DayOfWeek: "hs_dayofweek", E.WeekOfYear: "hs_weekofyear",
              E.LastDay: "hs_last_day"}


def _kind(t: pa.DataType) -> str:
    """'i' integral, 'f' double (floating / decimal), 'b' boolean; else unsupported."""
    if pa.types.is_boolean(t):
        return "b"
    if pa.types.is_integer(t):
        return "i"
    if pa.types.is_floating(t) or pa.types.is_decimal(t):
        return "f"
    raise Unsupported(f"computed projection over {t}")


def _is_date(e: E.Expression) -> bool:
    try:
        return pa.types.is_date32(e.data_type)
    except ValueError:
        return False


def _date_compare(e: E.BinaryComparison) -> bool:
    """Date against date, or against a string literal (which the analyzer reads as a date)."""
    def text(x):
        return isinstance(x, E.Literal) and isinstance(x.value, str)
    l, r = e.left, e.right
    return (_is_date(l) and (_is_date(r) or text(r))) or (text(l) and _is_date(r))


def _out_storage(t: pa.DataType):
    import torch
    if pa.types.is_boolean(t):
        return torch.uint8, "unsigned char"
    if pa.types.is_date32(t):
        return torch.int32, "int"
    if pa.types.is_integer(t):
        bw = t.bit_width
        return ({8: torch.int8, 16: torch.int16, 32: torch.int32, 64: torch.int64}[bw],
                {8: "signed char", 16: "short", 32: "int", 64: "long long"}[bw])
    if pa.types.is_float32(t):
        return torch.float32, "float"
    return torch.float64, "double"


class _Gen:
    """Expression -> C statements over row ``i``; every node yields (value var, valid var)."""

    def __init__(self, cols: Dict[int, DeviceColumn]):
        self.cols = cols            # expr_id -> device column
        self.slot: Dict[int, int] = {}
        self.args = jit.Args()
        self.lines: List[str] = []
        self.values: Dict[str, object] = {}
        self.shape: List[object] = []
        self.n = 0
        self.in_case = 0            # depth of CaseWhen nodes around the node being emitted
        self.uses_dates = False     # a date function was emitted: the kernel needs DATE_PRELUDE
        self.date_exprs = False     # the output expression being emitted holds a date function

    def _var(self) -> str:
        self.n += 1
        return f"t{self.n}"

    def attr(self, a: E.Attribute, dates: bool = False) -> Tuple[str, str, str]:
        c = self.cols.get(a.expr_id)
        if c is None:
            raise Unsupported(f"attribute {a.sql()} not on device")
        if c.dictionary is not None:
            raise Unsupported("computed projection over a string column")
        # a date is its day number where a CASE selects or compares dates (``dates``)
        k = "i" if dates and pa.types.is_date32(c.atype) else _kind(c.atype)
        s = self.slot.get(a.expr_id)
        if s is None:
            s = self.slot[a.expr_id] = len(self.slot)
            self.args.add("p", f"c{s}", f"const {_CTYPE[c.hs_type]}*")
            self.args.add("p", f"v{s}", "const unsigned char*")
            self.values[f"c{s}"] = c.data.data_ptr()
            self.values[f"v{s}"] = c.valid.data_ptr() if c.valid is not None else 0
            self.shape.append(("col", s, c.hs_type, c.valid is not None))
        v, ok = self._var(), self._var()
        ct = "double" if k == "f" else ("bool" if k == "b" else "long long")
        self.lines.append(f"const {ct} {v} = ({ct})a.c{s}[i];")
        self.lines.append(f"const bool {ok} = !a.v{s} || a.v{s}[i];" if c.valid is not None
                          else f"const bool {ok} = true;")
        return v, ok, k

    def lit(self, e: E.Literal, dates: bool = False) -> Tuple[str, str, str]:
        v, ok = self._var(), self._var()
        if e.value is None:
            self.shape.append(("null",))
            self.lines.append(f"const long long {v} = 0; const bool {ok} = false;")
            return v, ok, "i"
        val = e.value
        if dates and isinstance(val, str):
            try:
                val = datetime.date.fromisoformat(val[:10])
            except ValueError:
                raise Unsupported(f"literal {val!r} compared with a date") from None
        if dates and isinstance(val, datetime.date) and not isinstance(val, datetime.datetime):
            val = (val - datetime.date(1970, 1, 1)).days
        if isinstance(val, bool):
            k = "b"
        elif isinstance(val, int):
            k = "i"
        elif isinstance(val, float) or hasattr(val, "as_tuple"):
            k = "f"
        else:
            raise Unsupported(f"literal {val!r} in a computed projection")
        name = f"l{len(self.values)}"
        if k == "f":
            self.args.add("d", name, "double")
            self.values[name] = float(val)
            self.lines.append(f"const double {v} = a.{name};")
        else:
            self.args.add("q", name, "long long")
            self.values[name] = int(val)
            ct = "bool" if k == "b" else "long long"
            self.lines.append(f"const {ct} {v} = ({ct})a.{name};")
        self.shape.append(("lit", k))
        self.lines.append(f"const bool {ok} = true;")
        return v, ok, k

    def operand(self, e: E.Expression, dates: bool) -> Tuple[str, str, str]:
        """``emit`` with date columns and date literals as day numbers when ``dates``."""
        while isinstance(e, E.Alias):
            e = e.child
        if isinstance(e, E.Attribute):
            return self.attr(e, dates)
        if isinstance(e, E.Literal):
            return self.lit(e, dates)
        return self.emit(e)

    def case_when(self, e: E.CaseWhen) -> Tuple[str, str, str]:
        """Nested selects over the (value, valid) pairs of the branches: the first branch whose
        condition is valid and true gives both; every operand is computed, nothing branches."""
        rt = e.data_type
        if pa.types.is_string(rt) or pa.types.is_large_string(rt):
            raise Unsupported("string-valued CASE in a computed projection")
        dates = pa.types.is_date32(rt)
        rk = "i" if dates else _kind(rt)
        ct = {"i": "long long", "f": "double", "b": "bool"}[rk]
        self.shape.append(("case", len(e.branches), e.else_value is not None, rk))

        def value(x):
            v, ok, k = self.operand(x, dates)
            null = isinstance(x, E.Literal) and x.value is None
            if not null and k != rk and not (k == "i" and rk == "f"):
                raise Unsupported(f"CASE value {x.sql()} in a {rt} result")
            return f"({ct}){v}", ok
        self.in_case += 1
        try:
            arms = []
            for c, x in e.branches:
                cv, cok, ck = self.emit(c)
                if ck != "b" and not (isinstance(c, E.Literal) and c.value is None):
                    raise Unsupported("CASE condition that is not a boolean")
                arms.append((f"({cok} && {cv})", *value(x)))
            tail_v, tail_ok = value(e.else_value) if e.else_value is not None else \
                (f"({ct})0", "false")
        finally:
            self.in_case -= 1
        v, ok = self._var(), self._var()
        ve, oke = tail_v, tail_ok
        for g, bv, bok in reversed(arms):
            ve, oke = f"({g} ? {bv} : {ve})", f"({g} ? {bok} : {oke})"
        self.lines.append(f"const {ct} {v} = {ve};")
        self.lines.append(f"const bool {ok} = {oke};")
        return v, ok, rk

    def date_function(self, e: E.DateFunction) -> Tuple[str, str, str]:
        """A date function over day numbers: every argument is narrowed to ``int`` once, the
        calendar arithmetic of ``DATE_PRELUDE`` runs in 32 bits, and the result widens back to
        the kernel's ``long long`` value convention.  Integer arguments (``n`` of date_add /
        add_months) are ordinary operands: a literal is a kernel argument."""
        self.uses_dates = True
        args = []
        for i, x in enumerate(e.children):
            if i in e.DATES:
                t = x.data_type
                if pa.types.is_timestamp(t):
                    raise Unsupported(f"timestamp argument of {e.name}()")
                if not (pa.types.is_date32(t) or pa.types.is_null(t)):
                    raise Unsupported(f"{t} argument of {e.name}()")
            v, ok, k = self.operand(x, True)
            if k != "i":
                raise Unsupported(f"argument {x.sql()} of {e.name}()")
            args.append((f"(int){v}", ok))
        v, ok = self._var(), self._var()
        valid = " && ".join(o for _, o in args)
        a = args[0][0]
        if type(e) in _DATE_PART:
            expr = f"{_DATE_PART[type(e)]}({a})"
        elif isinstance(e, E.WeekDay):
            expr = f"(int)hs_weekday({a})"
        elif isinstance(e, E.DateAdd):
            expr = f"(int)((unsigned){a} + (unsigned){args[1][0]})"
        elif isinstance(e, (E.DateSub, E.DateDiff)):
            expr = f"(int)((unsigned){a} - (unsigned){args[1][0]})"
        elif isinstance(e, E.AddMonths):
            expr = f"hs_add_months({a}, {args[1][0]})"
        elif isinstance(e, E.TruncDate):
            level = e.level
            self.shape.append(("trunc", level))
            if level is None:
                expr, valid = "0", "false"
            else:
                expr = f"hs_trunc_{level}({a})"
        else:
            raise Unsupported(f"computed projection of {type(e).__name__}")
        self.lines.append(f"const bool {ok} = {valid};")
        self.lines.append(f"const long long {v} = (long long)({expr});")
        return v, ok, "i"

    def in_list(self, e: E.In) -> Tuple[str, str, str]:
        """``x IN (literals)`` over an integral value: TRUE on a match, else NULL when ``x`` or
        a list entry is NULL, else FALSE."""
        a, av, ak = self.emit(e.value)
        if ak != "i" or not all(isinstance(x, E.Literal) for x in e.values):
            raise Unsupported("IN over a value that is not integral, or a list of non-literals")
        hits, nulls = [], False
        for x in e.values:
            if x.value is None:
                nulls = True
                continue
            b, _, bk = self.lit(x)
            if bk != "i":
                raise Unsupported("IN list entry that is not an integer")
            hits.append(f"{a} == {b}")
        self.shape.append(("in", len(hits), nulls))
        v, ok = self._var(), self._var()
        self.lines.append(f"const bool {v} = {av} && ({' || '.join(hits) if hits else 'false'});")
        self.lines.append(f"const bool {ok} = {av} && ({v} || {'false' if nulls else 'true'});")
        return v, ok, "b"

    def emit(self, e: E.Expression) -> Tuple[str, str, str]:
        if isinstance(e, E.Alias):
            return self.emit(e.child)
        if isinstance(e, E.Attribute):
            return self.attr(e)
        if isinstance(e, E.Literal):
            return self.lit(e)
        self.shape.append(type(e).__name__)
        if isinstance(e, E.CaseWhen):
            return self.case_when(e)
        if isinstance(e, E.DateFunction):
            return self.date_function(e)
        if (self.in_case or self.date_exprs) and type(e) in _CMP and _date_compare(e):
            # inside a CASE, or in an expression that holds a date function (a WHERE conjunct
            # on dates alone never comes here): day numbers
            (a, av, ak), (b, bv, bk) = self.operand(e.left, True), self.operand(e.right, True)
            v, ok = self._var(), self._var()
            self.lines.append(f"const bool {ok} = {av} && {bv};")
            self.lines.append(f"const bool {v} = (long long){a} {_CMP[type(e)]} (long long){b};")
            return v, ok, "b"
        if type(e) in _ARITH or isinstance(e, (E.Divide, E.Remainder)) or type(e) in _CMP:
            (a, av, ak), (b, bv, bk) = self.emit(e.left), self.emit(e.right)
            if "b" in (ak, bk):
                raise Unsupported("arithmetic / comparison on booleans")
            v, ok = self._var(), self._var()
            f = "f" in (ak, bk)
            if isinstance(e, E.Remainder):
                # Spark: sign of the dividend, NULL for a zero divisor; x % -1 = 0 (no trap on
                # LLONG_MIN % -1)
                if f:
                    self.lines.append(f"const bool {ok} = {av} && {bv} && (double){b} != 0.0;")
                    self.lines.append(f"const double {v} = {ok} ? fmod((double){a}, (double){b})"
                                      f" : 0.0;")
                    return v, ok, "f"
                self.lines.append(f"const bool {ok} = {av} && {bv} && (long long){b} != 0;")
                self.lines.append(f"const long long {v} = (!{ok} || (long long){b} == -1) ? 0 : "
                                  f"(long long){a} % (long long){b};")
                return v, ok, "i"
            if isinstance(e, E.Divide):
                self.lines.append(f"const bool {ok} = {av} && {bv} && (double){b} != 0.0;")
                self.lines.append(f"const double {v} = {ok} ? (double){a} / (double){b} : 0.0;")
                return v, ok, "f"
            self.lines.append(f"const bool {ok} = {av} && {bv};")
            if type(e) in _CMP:
                ct = "double" if f else "long long"
                self.lines.append(f"const bool {v} = ({ct}){a} {_CMP[type(e)]} ({ct}){b};")
                return v, ok, "b"
            op = _ARITH[type(e)]
            if f:
                self.lines.append(f"const double {v} = (double){a} {op} (double){b};")
                return v, ok, "f"
            # integers wrap: two's-complement arithmetic in unsigned 64 bits, narrowed at store
            self.lines.append(f"const long long {v} = (long long)((unsigned long long){a} {op} "
                              f"(unsigned long long){b});")
            return v, ok, "i"
        if isinstance(e, (E.And, E.Or)):
            (a, av, ak), (b, bv, bk) = self.emit(e.left), self.emit(e.right)
            if ak != "b" or bk != "b":
                raise Unsupported("AND / OR of non-booleans")
            v, ok = self._var(), self._var()
            if isinstance(e, E.And):
                # false wins over NULL
                self.lines.append(f"const bool {ok} = ({av} && {bv}) || ({av} && !{a}) || "
                                  f"({bv} && !{b});")
                self.lines.append(f"const bool {v} = {a} && {b} && {av} && {bv};")
            else:
                # true wins over NULL
                self.lines.append(f"const bool {ok} = ({av} && {bv}) || ({av} && {a}) || "
                                  f"({bv} && {b});")
                self.lines.append(f"const bool {v} = ({av} && {a}) || ({bv} && {b});")
            return v, ok, "b"
        if isinstance(e, E.In):
            return self.in_list(e)
        if isinstance(e, E.InSet):
            # OptimizeIn's form of a long literal list
            return self.in_list(E.In(e.value, [E.Literal(x) for x in sorted(e.hset, key=repr)]))
        if isinstance(e, E.Not):
            a, av, ak = self.emit(e.child)
            if ak != "b":
                raise Unsupported("NOT of a non-boolean")
            v = self._var()
            self.lines.append(f"const bool {v} = !{a};")
            return v, av, "b"
        if isinstance(e, (E.IsNull, E.IsNotNull)):
            a, av, _ = self.emit(e.child)
            v, ok = self._var(), self._var()
            self.lines.append(f"const bool {v} = {'!' if isinstance(e, E.IsNull) else ''}{av};")
            self.lines.append(f"const bool {ok} = true;")
            return v, ok, "b"
        if isinstance(e, E.Cast):
            a, av, ak = self.emit(e.child)
            tk = _kind(e.dtype)
            self.shape.append(str(e.dtype))
            v = self._var()
            if tk == "f":
                self.lines.append(f"const double {v} = (double){a};")
            elif tk == "b":
                self.lines.append(f"const bool {v} = {a} != 0;")
            elif ak == "f" and pa.types.is_int64(e.dtype):
                # truncation toward zero; NaN / out of range saturate like the JVM's d2l
                self.lines.append(f"const long long {v} = {a} != {a} ? 0LL : ({a} >= 9.2233720368547758e18 ? "
                                  f"0x7fffffffffffffffLL : ({a} <= -9.2233720368547758e18 ? "
                                  f"(-0x7fffffffffffffffLL - 1) : (long long){a}));")
            elif ak == "f":
                # Spark: d2i saturates to the int range (NaN -> 0); a short / byte target is
                # toInt then a wrapping narrow, which the store performs
                self.lines.append(f"const long long {v} = {a} != {a} ? 0LL : ({a} >= 2147483647.0 ? "
                                  f"2147483647LL : ({a} <= -2147483648.0 ? -2147483648LL : "
                                  f"(long long){a}));")
            else:
                self.lines.append(f"const long long {v} = (long long){a};")
            return v, av, tk
        raise Unsupported(f"computed projection of {type(e).__name__}")


def evaluate(exprs: List[E.Expression], cols: Dict[int, DeviceColumn], n: int,
             device) -> List[DeviceColumn]:
    """Device columns of ``exprs`` (over attributes in ``cols``: expr_id -> column of ``n``
    rows), all computed by one generated kernel launch."""
    k, values, outs = build(exprs, cols, n, device)
    if n:
        grid = max(1, min(4096, -(-n // BLOCK)))
        k.launch(grid, values, NL.stream_ptr(), 0)
    return outs


def build(exprs: List[E.Expression], cols: Dict[int, DeviceColumn], n: int, device):
    """(kernel, argument values, output columns) of ``evaluate`` without the launch."""
    import torch
    g = _Gen(cols)
    outs = []
    body: List[str] = []
    for j, e in enumerate(exprs):
        t = e.data_type
        if pa.types.is_integer(t) and e.data_type.bit_width > 64:
            raise Unsupported("wide integer result")
        g.date_exprs = E.contains_date_function(e)
        v, ok, k = g.emit(e)
        tdt, ct = _out_storage(t)
        if (k == "b") != pa.types.is_boolean(t):
            raise Unsupported(f"result type {t} of {e.sql()}")
        data = torch.empty(n, dtype=tdt, device=device)
        valid = torch.empty(n, dtype=torch.uint8, device=device)
        g.args.add("p", f"o{j}", f"{ct}*")
        g.args.add("p", f"ov{j}", "unsigned char*")
        g.values[f"o{j}"] = data.data_ptr()
        g.values[f"ov{j}"] = valid.data_ptr()
        g.shape.append(("out", str(t)))
        g.lines.append(f"a.o{j}[i] = {v} ? ({ct}){v} : ({ct})0;" if k == "b" else
                       f"a.o{j}[i] = {ok} ? ({ct}){v} : ({ct})0;")
        g.lines.append(f"a.ov{j}[i] = {ok} ? 1 : 0;")
        outs.append((data, valid, t))
    g.args.add("q", "n", "long long")
    g.values["n"] = n
    body = ["  const long long stride = (long long)gridDim.x * blockDim.x;",
            "  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; "
            "i += stride) {"] + ["    " + x for x in g.lines] + ["  }"]
    shape = ("project", tuple(map(str, g.shape)), tuple(s for _, s, _ in g.args.slots))

    def make():
        src = (jit._PRELUDE + (DATE_PRELUDE if g.uses_dates else "") + g.args.struct_src() +
               f'extern "C" __global__ __launch_bounds__({BLOCK}) void hs_jit_project(Args a) {{\n'
               + "\n".join(body) + "\n}\n")
        return jit.Kernel(src, "hs_jit_project", g.args, 0, BLOCK)
    k = jit.kernel_for(shape, make)
    return k, g.values, [DeviceColumn(data, valid, t) for data, valid, t in outs]


__all__ = ["evaluate"]
