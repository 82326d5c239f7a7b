"""Expression trees of the query front-end (the subset of Catalyst the index rules need,
SURVEY §7.4 item 8): attributes, literals, comparisons, boolean logic, IN, null tests,
arithmetic, aliases and aggregate functions.

Attributes carry a unique ``expr_id`` (Catalyst's ``ExprId``); equality of attributes is by id,
which is what ``JoinIndexRule.ensureAttributeRequirements`` relies on when it canonicalizes
join-condition attributes (``JoinIndexRule.scala:232-271``).
"""
from __future__ import annotations

import datetime
import itertools
from typing import Iterable, List

import pyarrow as pa

from .types import common_numeric

_ids = itertools.count(1)


def new_expr_id() -> int:
    return next(_ids)


class Expression:
    children: tuple = ()

    # -- tree utilities -----------------------------------------------------------------------
    def references(self) -> List["Attribute"]:
        out: list = []
        seen = set()
        for e in self.iter_tree():
            if isinstance(e, Attribute) and e.expr_id not in seen:
                seen.add(e.expr_id)
                out.append(e)
        return out

    def iter_tree(self):
        yield self
        for c in self.children:
            yield from c.iter_tree()

    def with_children(self, children) -> "Expression":
        raise NotImplementedError(type(self).__name__)

    def transform_up(self, fn) -> "Expression":
        if self.children:
            new_children = tuple(c.transform_up(fn) for c in self.children)
            node = self.with_children(new_children) if any(
                a is not b for a, b in zip(new_children, self.children)) else self
        else:
            node = self
        r = fn(node)
        return node if r is None else r

    @property
    def data_type(self) -> pa.DataType:
        raise NotImplementedError

    @property
    def nullable(self) -> bool:
        return any(c.nullable for c in self.children)

    def semantic_equals(self, other) -> bool:
        return self.canonical_key() == other.canonical_key()

    def canonical_key(self):
        return (type(self).__name__,) + tuple(c.canonical_key() for c in self.children)

    def __repr__(self):
        return self.sql()

    def sql(self) -> str:
        raise NotImplementedError


class LeafExpression(Expression):
    def with_children(self, children):
        return self


class Attribute(LeafExpression):
    def __init__(self, name: str, dtype: pa.DataType, nullable: bool = True, expr_id: int = None,
                 qualifier: str = None):
        self.name = name
        self.dtype = dtype
        self._nullable = nullable
        self.expr_id = expr_id if expr_id is not None else new_expr_id()
        self.qualifier = qualifier

    @property
    def data_type(self):
        return self.dtype

    @property
    def nullable(self):
        return self._nullable

    def with_nullability(self, nullable: bool) -> "Attribute":
        return Attribute(self.name, self.dtype, nullable, self.expr_id, self.qualifier)

    def new_instance(self) -> "Attribute":
        return Attribute(self.name, self.dtype, self._nullable, None, self.qualifier)

    def canonical_key(self):
        return ("Attribute", self.expr_id)

    def __eq__(self, o):
        return isinstance(o, Attribute) and o.expr_id == self.expr_id

    def __hash__(self):
        return hash(("attr", self.expr_id))

    def sql(self):
        return f"{self.name}#{self.expr_id}"


class Literal(LeafExpression):
    def __init__(self, value, dtype: pa.DataType = None):
        if dtype is None:
            dtype = infer_literal_type(value)
        self.value = value
        self.dtype = dtype

    @property
    def data_type(self):
        return self.dtype

    @property
    def nullable(self):
        return self.value is None

    def canonical_key(self):
        return ("Literal", repr(self.value), str(self.dtype))

    def sql(self):
        v = self.value
        if v is None:
            return "null"
        if isinstance(v, str):
            return v
        if isinstance(v, datetime.date):
            return v.isoformat()
        return str(v)


def infer_literal_type(v) -> pa.DataType:
    if v is None:
        return pa.null()
    if isinstance(v, bool):
        return pa.bool_()
    if isinstance(v, int):
        return pa.int32() if -2 ** 31 <= v < 2 ** 31 else pa.int64()
    if isinstance(v, float):
        return pa.float64()
    if isinstance(v, str):
        return pa.string()
    if isinstance(v, datetime.datetime):
        return pa.timestamp("us")
    if isinstance(v, datetime.date):
        return pa.date32()
    if isinstance(v, bytes):
        return pa.binary()
    raise TypeError(f"unsupported literal {v!r}")


class Alias(Expression):
    def __init__(self, child: Expression, name: str, expr_id: int = None):
        self.children = (child,)
        self.name = name
        self.expr_id = expr_id if expr_id is not None else new_expr_id()

    @property
    def child(self):
        return self.children[0]

    def with_children(self, children):
        return Alias(children[0], self.name, self.expr_id)

    @property
    def data_type(self):
        return self.child.data_type

    def to_attribute(self) -> Attribute:
        return Attribute(self.name, self.data_type, self.child.nullable, self.expr_id)

    def canonical_key(self):
        return ("Alias", self.child.canonical_key())

    def sql(self):
        return f"{self.child.sql()} AS {self.name}#{self.expr_id}"


class UnresolvedAttribute(LeafExpression):
    """A column referenced by name before analysis (``col("a")``)."""

    def __init__(self, name: str):
        self.name = name

    @property
    def data_type(self):
        raise ValueError(f"unresolved attribute {self.name}")

    def canonical_key(self):
        return ("Unresolved", self.name)

    def sql(self):
        return f"'{self.name}"


# ---------------------------------------------------------------------------------------------
# Predicates
# ---------------------------------------------------------------------------------------------
class BinaryExpression(Expression):
    symbol = "?"

    def __init__(self, left: Expression, right: Expression):
        self.children = (left, right)

    @property
    def left(self):
        return self.children[0]

    @property
    def right(self):
        return self.children[1]

    def with_children(self, children):
        return type(self)(children[0], children[1])

    def sql(self):
        return f"({self.left.sql()} {self.symbol} {self.right.sql()})"


class Predicate(Expression):
    @property
    def data_type(self):
        return pa.bool_()


class BinaryComparison(BinaryExpression, Predicate):
    op = "?"


class EqualTo(BinaryComparison):
    symbol, op = "=", "eq"


class NotEqual(BinaryComparison):
    symbol, op = "!=", "ne"

    def sql(self):
        return f"NOT ({self.left.sql()} = {self.right.sql()})"


class LessThan(BinaryComparison):
    symbol, op = "<", "lt"


class LessThanOrEqual(BinaryComparison):
    symbol, op = "<=", "le"


class GreaterThan(BinaryComparison):
    symbol, op = ">", "gt"


class GreaterThanOrEqual(BinaryComparison):
    symbol, op = ">=", "ge"


FLIP = {EqualTo: EqualTo, NotEqual: NotEqual, LessThan: GreaterThan,
        LessThanOrEqual: GreaterThanOrEqual, GreaterThan: LessThan,
        GreaterThanOrEqual: LessThanOrEqual}


class And(BinaryExpression, Predicate):
    symbol = "AND"


class Or(BinaryExpression, Predicate):
    symbol = "OR"


class Not(Predicate):
    def __init__(self, child):
        self.children = (child,)

    @property
    def child(self):
        return self.children[0]

    def with_children(self, children):
        return Not(children[0])

    def sql(self):
        return f"NOT {self.child.sql()}"


class IsNull(Predicate):
    def __init__(self, child):
        self.children = (child,)

    @property
    def child(self):
        return self.children[0]

    @property
    def nullable(self):
        return False

    def with_children(self, children):
        return IsNull(children[0])

    def sql(self):
        return f"isnull({self.child.sql()})"


class IsNotNull(Predicate):
    def __init__(self, child):
        self.children = (child,)

    @property
    def child(self):
        return self.children[0]

    @property
    def nullable(self):
        return False

    def with_children(self, children):
        return IsNotNull(children[0])

    def sql(self):
        return f"isnotnull({self.child.sql()})"


class In(Predicate):
    def __init__(self, value: Expression, values: List[Expression]):
        self.children = (value, *values)

    @property
    def value(self):
        return self.children[0]

    @property
    def values(self):
        return self.children[1:]

    def with_children(self, children):
        return In(children[0], list(children[1:]))

    def sql(self):
        return f"{self.value.sql()} IN ({','.join(v.sql() for v in self.values)})"


class InSet(Predicate):
    """``OptimizeIn`` output for large literal lists (``HybridScanSuite.scala:138-165``)."""

    def __init__(self, value: Expression, hset: frozenset):
        self.children = (value,)
        self.hset = frozenset(hset)

    @property
    def value(self):
        return self.children[0]

    def with_children(self, children):
        return InSet(children[0], self.hset)

    def canonical_key(self):
        return ("InSet", self.value.canonical_key(), tuple(sorted(map(repr, self.hset))))

    def sql(self):
        return f"{self.value.sql()} INSET ({','.join(map(str, sorted(self.hset, key=repr)))})"


def check_like_pattern(pattern: str) -> str:
    """Spark's LIKE escape rule: ``\\`` may only precede ``%``, ``_`` or ``\\``."""
    if not isinstance(pattern, str):
        raise TypeError(f"LIKE pattern must be a string literal, got {pattern!r}")
    i, n = 0, len(pattern)
    while i < n:
        if pattern[i] == "\\":
            if i + 1 >= n:
                raise ValueError(f"the LIKE pattern {pattern!r} is invalid: "
                                 "it is not allowed to end with the escape character")
            if pattern[i + 1] not in "%_\\":
                raise ValueError(f"the LIKE pattern {pattern!r} is invalid: the escape character "
                                 f"is not allowed to precede {pattern[i + 1]!r}")
            i += 2
        else:
            i += 1
    return pattern


def escape_like(s: str) -> str:
    """``s`` with LIKE's special characters escaped: a pattern that matches ``s`` literally."""
    return s.replace("\\", "\\\\").replace("%", "\\%").replace("_", "\\_")


def like_simple_shape(pattern: str):
    """("prefix" | "suffix" | "contains", literal) when ``pattern`` is ``lit%``, ``%lit`` or
    ``%lit%`` with a non-empty wildcard-free literal (escapes resolved), else None."""
    toks, i = [], 0
    while i < len(pattern):
        ch = pattern[i]
        if ch == "\\":
            toks.append(pattern[i + 1])
            i += 2
        else:
            toks.append(None if ch == "%" else (False if ch == "_" else ch))
            i += 1
    if any(t is False for t in toks):
        return None
    lead, trail = bool(toks) and toks[0] is None, len(toks) > 1 and toks[-1] is None
    body = toks[1 if lead else 0:len(toks) - 1 if trail else len(toks)]
    if not body or any(t is None for t in body) or not (lead or trail):
        return None
    lit = "".join(body)
    return ("contains" if lead and trail else "suffix" if lead else "prefix"), lit


def _is_string_type(t: pa.DataType) -> bool:
    if pa.types.is_dictionary(t):
        t = t.value_type
    return pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_null(t)


class Like(Predicate):
    """``child LIKE 'pattern'`` with Spark's semantics: ``%`` any run, ``_`` one character,
    ``\\`` escapes ``%``, ``_`` and itself; case-sensitive, anchored, NULL in -> NULL out.
    The pattern is a plain field (not a Literal child), so two patterns are two plan shapes."""

    def __init__(self, child: Expression, pattern: str):
        self.children = (child,)
        self.pattern = check_like_pattern(pattern)
        # resolution rebuilds the node over the resolved child (with_children): a resolved
        # child that is not a string is an analysis error
        t = getattr(child, "dtype", None) if isinstance(child, (Attribute, Literal, Cast)) else None
        if t is not None and not _is_string_type(t):
            raise TypeError(f"cannot resolve '{self.sql()}' due to data type mismatch: "
                            f"LIKE requires a string input, not {t}")

    @property
    def child(self):
        return self.children[0]

    @property
    def nullable(self):
        return self.child.nullable

    def with_children(self, children):
        return Like(children[0], self.pattern)

    def canonical_key(self):
        return ("Like", self.child.canonical_key(), self.pattern)

    def sql(self):
        p = self.pattern.replace("\\", "\\\\").replace("'", "''")
        return f"{self.child.sql()} LIKE '{p}'"


# ---------------------------------------------------------------------------------------------
# Arithmetic
# ---------------------------------------------------------------------------------------------
class BinaryArithmetic(BinaryExpression):
    op = "?"

    @property
    def data_type(self):
        return common_numeric(self.left.data_type, self.right.data_type)


class Add(BinaryArithmetic):
    symbol, op = "+", "add"


class Subtract(BinaryArithmetic):
    symbol, op = "-", "sub"


class Multiply(BinaryArithmetic):
    symbol, op = "*", "mul"


class Remainder(BinaryArithmetic):
    """``a % b``: Spark's (and the JVM's) remainder - the sign follows the dividend, NULL for a
    zero divisor; ``fmod`` for floating-point operands."""
    symbol, op = "%", "mod"


class Divide(BinaryArithmetic):
    symbol, op = "/", "div"

    @property
    def data_type(self):
        return pa.float64()


class Cast(Expression):
    def __init__(self, child, dtype: pa.DataType):
        self.children = (child,)
        self.dtype = dtype

    @property
    def child(self):
        return self.children[0]

    @property
    def data_type(self):
        return self.dtype

    def with_children(self, children):
        return Cast(children[0], self.dtype)

    def canonical_key(self):
        return ("Cast", str(self.dtype), self.child.canonical_key())

    def sql(self):
        return f"cast({self.child.sql()} as {self.dtype})"


# ---------------------------------------------------------------------------------------------
# Conditional
# ---------------------------------------------------------------------------------------------
def _plain_type(t: pa.DataType) -> pa.DataType:
    return t.value_type if pa.types.is_dictionary(t) else t


def _case_family(t: pa.DataType) -> str:
    if pa.types.is_integer(t) or pa.types.is_floating(t) or pa.types.is_decimal(t):
        return "numeric"
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        return "string"
    if pa.types.is_date32(t) or pa.types.is_date64(t):
        return "date"
    if pa.types.is_boolean(t):
        return "boolean"
    return str(t)


def common_case_type(a: pa.DataType, b: pa.DataType, what="CASE") -> pa.DataType:
    """The type two branch values of a CASE share: integers widen to the widest integer, an
    integer with a floating or decimal value is a double (the rule of the host engine's
    ``_numeric_align``), strings go with strings, dates with dates, booleans with booleans; a
    NULL literal takes the other side's type.  Anything else is an analysis error that names
    both types (``what``: the expression's text, or a function that builds it - only then)."""
    a, b = _plain_type(a), _plain_type(b)
    if pa.types.is_null(a):
        return b
    if pa.types.is_null(b) or a == b:
        return a
    fa, fb = _case_family(a), _case_family(b)
    if fa == fb == "numeric":
        if pa.types.is_integer(a) and pa.types.is_integer(b):
            return a if a.bit_width >= b.bit_width else b
        return pa.float64()
    if fa == fb and fa in ("string", "date"):
        return pa.string() if fa == "string" else a
    from ..exceptions import HyperspaceException
    what = what() if callable(what) else what
    raise HyperspaceException(
        f"cannot resolve '{what}' due to data type mismatch: THEN and ELSE expressions should "
        f"all be same type or coercible to a common type, got {a} and {b}")


class CaseWhen(Expression):
    """``CASE WHEN c1 THEN v1 [WHEN c2 THEN v2 ...] [ELSE e] END`` with Spark's semantics: the
    first branch whose condition is TRUE wins (a NULL condition is not taken); without an ELSE
    the result of a row no branch takes is NULL.  The children are the conditions and values in
    order, then the ELSE value if there is one - so every literal in it is an ordinary
    ``Literal`` child (which the plan cache parameterises) and the node has no other field."""

    def __init__(self, branches, else_value: Expression = None):
        branches = [(c, v) for c, v in branches]
        if not branches:
            raise ValueError("CASE needs at least one WHEN branch")
        flat = [x for b in branches for x in b]
        self.children = tuple(flat) + ((else_value,) if else_value is not None else ())
        # resolution rebuilds the node over resolved children (with_children): then the
        # branch types are known, and values without a common type are an analysis error
        try:
            self.data_type
        except ValueError:      # an unresolved attribute below: checked once it is resolved
            pass
        for c in self.children[:len(branches) * 2:2]:
            try:
                t = c.data_type
            except ValueError:
                continue
            if not (pa.types.is_boolean(t) or pa.types.is_null(t)):
                from ..exceptions import HyperspaceException
                raise HyperspaceException(
                    f"cannot resolve '{self.sql()}' due to data type mismatch: WHEN expressions "
                    f"should all be boolean type, but {c.sql()} is {t}")

    @property
    def branches(self) -> list:
        n = len(self.children) // 2
        return [(self.children[2 * i], self.children[2 * i + 1]) for i in range(n)]

    @property
    def else_value(self):
        return self.children[-1] if len(self.children) % 2 else None

    @property
    def values(self) -> list:
        """The branch values, then the ELSE value if there is one."""
        out = [v for _, v in self.branches]
        if self.else_value is not None:
            out.append(self.else_value)
        return out

    def with_children(self, children):
        children = tuple(children)
        n = len(children) // 2
        return CaseWhen([(children[2 * i], children[2 * i + 1]) for i in range(n)],
                        children[-1] if len(children) % 2 else None)

    @property
    def data_type(self):
        vals = self.values
        t = vals[0].data_type
        for v in vals[1:]:
            t = common_case_type(t, v.data_type, self.sql)
        return _plain_type(t)

    @property
    def nullable(self):
        return self.else_value is None or any(v.nullable for v in self.values)

    def canonical_key(self):
        return ("CaseWhen", len(self.children)) + tuple(c.canonical_key() for c in self.children)

    def sql(self):
        parts = ["CASE"]
        for c, v in self.branches:
            cs = c.sql()
            if not (cs.startswith("(") and cs.endswith(")")):
                cs = f"({cs})"
            parts.append(f"WHEN {cs} THEN {v.sql()}")
        if self.else_value is not None:
            parts.append(f"ELSE {self.else_value.sql()}")
        parts.append("END")
        return " ".join(parts)


def contains_case(e: Expression) -> bool:
    return any(isinstance(x, CaseWhen) for x in e.iter_tree())


def references_outside_case(e: Expression) -> List["Attribute"]:
    """``e.references()`` without the attributes that only occur inside a ``CaseWhen``: a
    predicate over a CASE says nothing about the nullness of the columns the CASE reads
    (``coalesce(x, 0) > 1`` is true for a NULL ``x``)."""
    out: list = []

    def walk(x):
        if isinstance(x, CaseWhen):
            return
        if isinstance(x, Attribute):
            if all(a.expr_id != x.expr_id for a in out):
                out.append(x)
            return
        for c in x.children:
            walk(c)
    walk(e)
    return out


# ---------------------------------------------------------------------------------------------
# Date functions
# ---------------------------------------------------------------------------------------------
_EPOCH = datetime.date(1970, 1, 1)


def _as_date(v):
    """The date a literal value stands for where a date is expected: a date, a timestamp (its
    UTC date) or a string that reads as one; None when it is none of these."""
    if isinstance(v, datetime.datetime):
        if v.tzinfo is not None:
            v = v.astimezone(datetime.timezone.utc)
        return v.date()
    if isinstance(v, datetime.date):
        return v
    if isinstance(v, str):
        try:
            return datetime.date.fromisoformat(v.strip()[:10])
        except ValueError:
            return None
    return None


class DateFunction(Expression):
    """A scalar function over dates with Spark 3's typing and NULL rules (NULL in, NULL out).
    ``DATES`` / ``INTS`` name the argument positions that take a date and an integer.  A date
    argument is a ``date32`` expression, a timestamp expression (taken as its UTC date: session
    time zones are not modelled) or a string literal that reads as a date, which becomes a date
    literal here, as the analyzer reads ``l_shipdate >= '1994-01-01'``.  The calendar is the
    proleptic Gregorian one; the contract covers 0001-01-01 ... 9999-12-31 for inputs and results.

    The nodes hold their children only (``TruncDate``: and ``fmt``), so every literal argument
    is an ordinary ``Literal`` child that the plan cache parameterises.  Build them through
    ``date_function``, which folds a call over literals."""
    name = "?"
    DATES: tuple = (0,)
    INTS: tuple = ()
    RESULT = "int"

    def __init__(self, *children):
        if len(children) != len(self.DATES) + len(self.INTS):
            raise TypeError(f"{self.name}() takes {len(self.DATES) + len(self.INTS)} arguments")
        self.children = tuple(self._checked(i, c) for i, c in enumerate(children))

    def _checked(self, i: int, c: Expression) -> Expression:
        """Argument ``i`` once its type is known (resolution rebuilds the node over resolved
        children): a string literal in a date position as a date literal; a type the function
        does not take is an analysis error."""
        try:
            t = c.data_type
        except ValueError:          # an unresolved attribute below: checked once it is resolved
            return c
        if pa.types.is_null(t):
            return c
        if i in self.DATES:
            if isinstance(c, Literal) and isinstance(c.value, str):
                d = _as_date(c.value)
                return Literal(d, pa.date32())      # (not a date: NULL, as in Spark)
            if pa.types.is_date32(t) or pa.types.is_timestamp(t):
                return c
            want = "a date"
        else:
            if pa.types.is_signed_integer(t) and t.bit_width <= 32:
                return c
            want = "an int"
        from ..exceptions import HyperspaceException
        raise HyperspaceException(
            f"cannot resolve '{self.name}(...)' due to data type mismatch: argument {i + 1} "
            f"({c.sql()}) of {self.name}() requires {want}, not {t}")

    def with_children(self, children):
        return type(self)(*children)

    @property
    def data_type(self):
        return pa.date32() if self.RESULT == "date" else pa.int32()

    def sql(self):
        return f"{self.name}({', '.join(c.sql() for c in self.children)})"

    # the value for plain Python arguments (dates as datetime.date): folding and documentation
    @staticmethod
    def compute(*args):
        raise NotImplementedError


def _month_len(y: int, m: int) -> int:
    import calendar
    return calendar.monthrange(y, m)[1]


def _add_months(d: datetime.date, n: int) -> datetime.date:
    y, m = divmod(d.year * 12 + d.month - 1 + n, 12)
    return datetime.date(y, m + 1, min(d.day, _month_len(y, m + 1)))


class Year(DateFunction):
    name = "year"
    compute = staticmethod(lambda d: d.year)


class Quarter(DateFunction):
    name = "quarter"
    compute = staticmethod(lambda d: (d.month + 2) // 3)


class Month(DateFunction):
    name = "month"
    compute = staticmethod(lambda d: d.month)


class DayOfMonth(DateFunction):
    name = "dayofmonth"
    compute = staticmethod(lambda d: d.day)


class DayOfYear(DateFunction):
    name = "dayofyear"
    compute = staticmethod(lambda d: d.timetuple().tm_yday)


class DayOfWeek(DateFunction):
    """1 = Sunday ... 7 = Saturday."""
    name = "dayofweek"
    compute = staticmethod(lambda d: (d.weekday() + 1) % 7 + 1)


class WeekDay(DateFunction):
    """0 = Monday ... 6 = Sunday."""
    name = "weekday"
    compute = staticmethod(lambda d: d.weekday())


class WeekOfYear(DateFunction):
    """The ISO-8601 week: weeks start on Monday, week 1 holds the year's first Thursday."""
    name = "weekofyear"
    compute = staticmethod(lambda d: d.isocalendar()[1])


class DateAdd(DateFunction):
    name, INTS, RESULT = "date_add", (1,), "date"
    compute = staticmethod(lambda d, n: d + datetime.timedelta(days=n))


class DateSub(DateFunction):
    name, INTS, RESULT = "date_sub", (1,), "date"
    compute = staticmethod(lambda d, n: d - datetime.timedelta(days=n))


class DateDiff(DateFunction):
    """``datediff(end, start)``: the days from ``start`` to ``end``."""
    name, DATES = "datediff", (0, 1)
    compute = staticmethod(lambda end, start: (end - start).days)


class AddMonths(DateFunction):
    """Spark 3: the day of month is kept and clamped to the target month's length; a month's
    last day is not snapped to the target's last day."""
    name, INTS, RESULT = "add_months", (1,), "date"
    compute = staticmethod(_add_months)


class LastDay(DateFunction):
    name, RESULT = "last_day", "date"
    compute = staticmethod(lambda d: d.replace(day=_month_len(d.year, d.month)))


TRUNC_LEVELS = {"year": "year", "yyyy": "year", "yy": "year", "quarter": "quarter",
                "month": "month", "mon": "month", "mm": "month", "week": "week"}


def _trunc(d: datetime.date, level):
    if level == "year":
        return d.replace(month=1, day=1)
    if level == "quarter":
        return d.replace(month=(d.month - 1) // 3 * 3 + 1, day=1)
    if level == "month":
        return d.replace(day=1)
    if level == "week":
        return d - datetime.timedelta(days=d.weekday())
    return None


class TruncDate(DateFunction):
    """``trunc(d, fmt)``: the first day of ``d``'s year / quarter / month, or the Monday of its
    week; ``fmt`` (a plain field: a part of the plan's shape) is compared without case, and one
    that names none of these gives NULL, as in Spark."""
    name, RESULT = "trunc", "date"

    def __init__(self, child, fmt: str):
        if not isinstance(fmt, str):
            raise TypeError(f"trunc() takes a string literal format, got {fmt!r}")
        self.fmt = fmt
        super().__init__(child)

    @property
    def level(self):
        """'year' | 'quarter' | 'month' | 'week', or None for an unknown format."""
        return TRUNC_LEVELS.get(self.fmt.lower())

    def with_children(self, children):
        return TruncDate(children[0], self.fmt)

    @property
    def nullable(self):
        return self.level is None or self.children[0].nullable

    def canonical_key(self):
        return ("TruncDate", self.fmt.lower(), self.children[0].canonical_key())

    def sql(self):
        return f"trunc({self.children[0].sql()}, {self.fmt})"

    def compute(self, d):
        return _trunc(d, self.level)


DATE_FUNCTIONS = {c.name: c for c in (Year, Quarter, Month, DayOfMonth, DayOfYear, DayOfWeek,
                                      WeekDay, WeekOfYear, DateAdd, DateSub, DateDiff, AddMonths,
                                      LastDay, TruncDate)}
DATE_FUNCTIONS["day"] = DayOfMonth


def date_function(name: str, *args) -> Expression:
    """The date function ``name`` over ``args`` (``trunc``: the date and the format string).
    A call whose arguments are all non-NULL literals is folded here, at construction, into its
    ``Literal``: ``DATE '1998-12-01' - INTERVAL '90' DAY`` is a date literal before the plan is
    fingerprinted, so the plan cache parameterises it and the index rules see a plain
    column / literal comparison.  (A result outside 0001 ... 9999 is left unfolded.)"""
    node = DATE_FUNCTIONS[name.lower()](*args)
    if not all(isinstance(c, Literal) and c.value is not None for c in node.children):
        return node
    vals = [_as_date(c.value) if i in node.DATES else c.value
            for i, c in enumerate(node.children)]
    try:
        out = node.compute(*vals)
    except (OverflowError, ValueError):
        return node
    return Literal(out, node.data_type)


def contains_date_function(e: Expression) -> bool:
    return any(isinstance(x, DateFunction) for x in e.iter_tree())


# ---------------------------------------------------------------------------------------------
# Aggregates
# ---------------------------------------------------------------------------------------------
class AggregateFunction(Expression):
    name = "agg"

    def __init__(self, child: Expression = None):
        self.children = (child,) if child is not None else ()

    @property
    def child(self):
        return self.children[0] if self.children else None

    def with_children(self, children):
        return type(self)(children[0] if children else None)

    def sql(self):
        return f"{self.name}({self.child.sql() if self.child is not None else '1'})"


class Sum(AggregateFunction):
    name = "sum"

    @property
    def data_type(self):
        t = self.child.data_type
        return pa.int64() if pa.types.is_integer(t) else pa.float64()


class Count(AggregateFunction):
    name = "count"

    @property
    def data_type(self):
        return pa.int64()

    @property
    def nullable(self):
        return False


class CountDistinct(AggregateFunction):
    """``count(DISTINCT x)``: the number of different non-NULL values of ``x``.  A class of its
    own (not a flag on ``Count``): it has no partial / final decomposition, so every site that
    dispatches on the aggregate's type rejects it unless it was written for it."""
    name = "count"

    @property
    def data_type(self):
        return pa.int64()

    @property
    def nullable(self):
        return False

    def sql(self):
        return f"count(DISTINCT {self.child.sql()})"


class Min(AggregateFunction):
    name = "min"

    @property
    def data_type(self):
        return self.child.data_type


class Max(AggregateFunction):
    name = "max"

    @property
    def data_type(self):
        return self.child.data_type


class Avg(AggregateFunction):
    name = "avg"

    @property
    def data_type(self):
        return pa.float64()


class NormalizeNaNAndZero(Expression):
    """A float with ``-0.0`` as ``0.0`` and every NaN as the one canonical NaN: values that are
    equal as keys then have equal bits (what a hash of the bits needs)."""

    def __init__(self, child: Expression):
        self.children = (child,)

    @property
    def child(self):
        return self.children[0]

    def with_children(self, children):
        return NormalizeNaNAndZero(children[0])

    @property
    def data_type(self):
        return self.child.data_type

    def sql(self):
        return f"knownfloatingpointnormalized(normalizenanandzero({self.child.sql()}))"


# ---------------------------------------------------------------------------------------------
# Window functions
# ---------------------------------------------------------------------------------------------
class RankingFunction(LeafExpression):
    """``row_number()`` / ``rank()`` / ``dense_rank()``: only meaningful inside a
    ``WindowExpression`` whose specification has an ORDER BY."""
    name = "rank"

    @property
    def data_type(self):
        return pa.int32()

    @property
    def nullable(self):
        return False

    def sql(self):
        return f"{self.name}()"


class RowNumber(RankingFunction):
    name = "row_number"


class Rank(RankingFunction):
    name = "rank"


class DenseRank(RankingFunction):
    name = "dense_rank"


def _frame_error(what: str):
    from ..exceptions import HyperspaceException
    return HyperspaceException(
        f"explicit window frames ({what}) are not supported: a window takes Spark's default "
        "frame - the whole partition without ORDER BY, RANGE BETWEEN UNBOUNDED PRECEDING AND "
        "CURRENT ROW with it")


class WindowSpecDefinition(Expression):
    """``(PARTITION BY p... ORDER BY o [ASC|DESC]...)``.  ``order_by`` takes sort orders (anything
    with ``child`` and ``ascending``) or (expression, ascending) pairs.  The keys are the node's
    children (so they resolve and rewrite like any expression); the split between them and the
    directions are plain fields, which keeps two specifications apart in every plan key."""

    def __init__(self, partition_by=(), order_by=(), frame=None):
        if frame is not None:
            raise _frame_error(str(frame))
        orders = [(o.child, o.ascending) if hasattr(o, "ascending") else (o[0], o[1])
                  for o in order_by]
        self.children = tuple(partition_by) + tuple(e for e, _ in orders)
        self.n_part = len(tuple(partition_by))
        self.ascending = tuple(bool(a) for _, a in orders)

    @property
    def partition_by(self) -> list:
        return list(self.children[:self.n_part])

    @property
    def order_by(self) -> list:
        """[(expression, ascending)]"""
        return list(zip(self.children[self.n_part:], self.ascending))

    def with_children(self, children):
        children = tuple(children)
        return WindowSpecDefinition(children[:self.n_part],
                                    list(zip(children[self.n_part:], self.ascending)))

    @property
    def data_type(self):
        raise ValueError("a window specification has no value")

    @property
    def nullable(self):
        return False

    def canonical_key(self):
        return ("WindowSpecDefinition",
                tuple(e.canonical_key() for e in self.partition_by),
                tuple((e.canonical_key(), a) for e, a in self.order_by))

    def sql(self):
        parts = []
        if self.n_part:
            parts.append("PARTITION BY " + ", ".join(e.sql() for e in self.partition_by))
        if self.ascending:
            parts.append("ORDER BY " + ", ".join(
                f"{e.sql()} {'ASC NULLS FIRST' if a else 'DESC NULLS LAST'}"
                for e, a in self.order_by))
        return "(" + " ".join(parts) + ")"


class WindowExpression(Expression):
    """``function OVER spec``: a ranking function, or ``sum`` / ``count`` / ``min`` / ``max`` /
    ``avg`` over Spark's default frame.  With an ORDER BY the frame runs from the partition's
    first row to the current row's last peer (rows that tie on every order key share one value);
    without one it is the whole partition."""

    def __init__(self, function: Expression, spec: WindowSpecDefinition):
        from ..exceptions import HyperspaceException
        if not isinstance(spec, WindowSpecDefinition):
            raise TypeError(f"OVER needs a window specification, got {spec!r}")
        if isinstance(function, RankingFunction):
            if not spec.ascending:
                raise HyperspaceException(
                    f"window function {function.name}() requires the window to be ordered: "
                    f"add an ORDER BY to {spec.sql()}")
        elif isinstance(function, CountDistinct) or \
                not isinstance(function, (Sum, Count, Min, Max, Avg)):
            raise HyperspaceException(
                f"{function.sql()} is not a window function: OVER takes row_number, rank, "
                "dense_rank, sum, count, min, max or avg")
        elif contains_window(function):
            raise HyperspaceException("a window function cannot be nested in another one")
        self.children = (function, spec)

    @property
    def function(self):
        return self.children[0]

    @property
    def spec(self) -> WindowSpecDefinition:
        return self.children[1]

    def with_children(self, children):
        return WindowExpression(children[0], children[1])

    @property
    def data_type(self):
        return self.function.data_type

    @property
    def nullable(self):
        return not isinstance(self.function, (RankingFunction, Count))

    def canonical_key(self):
        return ("WindowExpression", self.function.canonical_key(), self.spec.canonical_key())

    def sql(self):
        return f"{self.function.sql()} OVER {self.spec.sql()}"


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def split_conjuncts(e: Expression) -> List[Expression]:
    if isinstance(e, And):
        return split_conjuncts(e.left) + split_conjuncts(e.right)
    return [e]


def conjoin(preds: Iterable[Expression]):
    preds = list(preds)
    if not preds:
        return None
    out = preds[0]
    for p in preds[1:]:
        out = And(out, p)
    return out


def attr_set(exprs) -> set:
    out = set()
    for e in exprs:
        for r in e.references():
            out.add(r.expr_id)
    return out


def contains_aggregate(e: Expression) -> bool:
    """Whether ``e`` holds an aggregate function of its own: one wrapped in a
    ``WindowExpression`` (``sum(x) OVER w``) is a per-row value, not an aggregate."""
    if isinstance(e, WindowExpression):
        return False
    if isinstance(e, AggregateFunction):
        return True
    return any(contains_aggregate(c) for c in e.children)


def contains_window(e: Expression) -> bool:
    return any(isinstance(x, WindowExpression) for x in e.iter_tree())
