"""User-facing ``Column`` API (``col("a") > 5``, ``df["a"] == df2["b"]``, ``sum_("x")``)."""
from __future__ import annotations

from . import expressions as E


def _expr(v) -> E.Expression:
    if isinstance(v, Column):
        return v.expr
    if isinstance(v, E.Expression):
        return v
    return E.Literal(v)


class Column:
    def __init__(self, expr: E.Expression):
        self.expr = expr

    # comparisons
    def __eq__(self, o):  # noqa: D105
        return Column(E.EqualTo(self.expr, _expr(o)))

    def __ne__(self, o):
        return Column(E.NotEqual(self.expr, _expr(o)))

    def __lt__(self, o):
        return Column(E.LessThan(self.expr, _expr(o)))

    def __le__(self, o):
        return Column(E.LessThanOrEqual(self.expr, _expr(o)))

    def __gt__(self, o):
        return Column(E.GreaterThan(self.expr, _expr(o)))

    def __ge__(self, o):
        return Column(E.GreaterThanOrEqual(self.expr, _expr(o)))

    # boolean
    def __and__(self, o):
        return Column(E.And(self.expr, _expr(o)))

    def __or__(self, o):
        return Column(E.Or(self.expr, _expr(o)))

    def __invert__(self):
        return Column(E.Not(self.expr))

    # arithmetic
    def __add__(self, o):
        return Column(E.Add(self.expr, _expr(o)))

    def __radd__(self, o):
        return Column(E.Add(_expr(o), self.expr))

    def __sub__(self, o):
        return Column(E.Subtract(self.expr, _expr(o)))

    def __rsub__(self, o):
        return Column(E.Subtract(_expr(o), self.expr))

    def __mul__(self, o):
        return Column(E.Multiply(self.expr, _expr(o)))

    def __rmul__(self, o):
        return Column(E.Multiply(_expr(o), self.expr))

    def __mod__(self, o):
        return Column(E.Remainder(self.expr, _expr(o)))

    def __rmod__(self, o):
        return Column(E.Remainder(_expr(o), self.expr))

    def __truediv__(self, o):
        return Column(E.Divide(self.expr, _expr(o)))

    def __neg__(self):
        return Column(E.Subtract(E.Literal(0), self.expr))

    __hash__ = object.__hash__

    def isin(self, *values):
        if len(values) == 1 and isinstance(values[0], (list, tuple, set)):
            values = tuple(values[0])
        return Column(E.In(self.expr, [_expr(v) for v in values]))

    def isNull(self):
        return Column(E.IsNull(self.expr))

    def isNotNull(self):
        return Column(E.IsNotNull(self.expr))

    def like(self, pattern: str):
        """SQL ``LIKE``: ``%`` any run, ``_`` one character, ``\\`` escapes either."""
        return Column(E.Like(self.expr, pattern))

    def startswith(self, s: str):
        return Column(E.Like(self.expr, E.escape_like(s) + "%"))

    def endswith(self, s: str):
        return Column(E.Like(self.expr, "%" + E.escape_like(s)))

    def contains(self, s: str):
        return Column(E.Like(self.expr, "%" + E.escape_like(s) + "%"))

    def between(self, lo, hi):
        return (self >= lo) & (self <= hi)

    def asc(self):
        """Sort order for ``orderBy`` (ascending, nulls first — Spark's default)."""
        c = Column(self.expr)
        c.sort_ascending = True
        return c

    def desc(self):
        """Sort order for ``orderBy`` (descending, nulls last)."""
        c = Column(self.expr)
        c.sort_ascending = False
        return c

    def over(self, window: "WindowSpec"):
        """This function over a window: ``sum_("x").over(Window.partitionBy("k"))``."""
        if isinstance(window, type) and issubclass(window, Window):
            window = WindowSpec()
        if not isinstance(window, WindowSpec):
            raise TypeError(f"over() takes a Window specification, got {window!r}")
        return Column(E.WindowExpression(self.expr, window.definition()))

    def alias(self, name: str):
        return Column(E.Alias(self.expr, name))

    def cast(self, dtype):
        """``dtype``: a pyarrow type or a Spark type name ("int", "bigint", "double", ...)."""
        if isinstance(dtype, str):
            import pyarrow as pa
            names = {"byte": pa.int8(), "tinyint": pa.int8(), "short": pa.int16(),
                     "smallint": pa.int16(), "int": pa.int32(), "integer": pa.int32(),
                     "long": pa.int64(), "bigint": pa.int64(), "float": pa.float32(),
                     "double": pa.float64(), "string": pa.string(), "boolean": pa.bool_(),
                     "date": pa.date32()}
            if dtype.lower() not in names:
                raise ValueError(f"unknown type name {dtype!r}")
            dtype = names[dtype.lower()]
        return Column(E.Cast(self.expr, dtype))

    def __repr__(self):
        return f"Column<{self.expr.sql()}>"


def col(name: str) -> Column:
    return Column(E.UnresolvedAttribute(name))


def lit(v) -> Column:
    return Column(E.Literal(v))


def sum_(c) -> Column:
    return Column(E.Sum(_expr(col(c) if isinstance(c, str) else c)))


def count(c="*") -> Column:
    if c == "*":
        return Column(E.Count(None))
    return Column(E.Count(_expr(col(c) if isinstance(c, str) else c)))


def countDistinct(c, *more) -> Column:
    """``count(DISTINCT c)``: the number of different non-NULL values of one column or
    expression."""
    if more:
        from ..exceptions import HyperspaceException
        raise HyperspaceException("countDistinct over several columns is not supported: "
                                  "it takes one argument")
    return Column(E.CountDistinct(_expr(col(c) if isinstance(c, str) else c)))


count_distinct = countDistinct


def min_(c) -> Column:
    return Column(E.Min(_expr(col(c) if isinstance(c, str) else c)))


def max_(c) -> Column:
    return Column(E.Max(_expr(col(c) if isinstance(c, str) else c)))


def avg(c) -> Column:
    return Column(E.Avg(_expr(col(c) if isinstance(c, str) else c)))


def row_number() -> Column:
    """1, 2, 3, ... within the partition, in the window's order (ties in an unspecified
    order)."""
    return Column(E.RowNumber())


def rank() -> Column:
    """The row's rank in the window's order: peers share a rank, the next one skips."""
    return Column(E.Rank())


def dense_rank() -> Column:
    """Like ``rank`` without gaps."""
    return Column(E.DenseRank())


def _key_expr(c) -> E.Expression:
    if isinstance(c, str):
        from .parser import parse_expression
        return E.UnresolvedAttribute(c) if c.isidentifier() else parse_expression(c)
    return _expr(c)


class WindowSpec:
    """An immutable ``PARTITION BY ... ORDER BY ...`` (``Window.partitionBy("k").orderBy("d")``).
    Frames are Spark's defaults; ``rowsBetween`` / ``rangeBetween`` raise."""

    def __init__(self, partition_by=(), order_by=()):
        self._partition = tuple(partition_by)
        self._order = tuple(order_by)      # (expression, ascending)

    @staticmethod
    def _flat(cols):
        if len(cols) == 1 and isinstance(cols[0], (list, tuple)):
            return tuple(cols[0])
        return cols

    def partitionBy(self, *cols) -> "WindowSpec":
        return WindowSpec([_key_expr(c) for c in self._flat(cols)], self._order)

    def orderBy(self, *cols) -> "WindowSpec":
        orders = [(_key_expr(c), bool(getattr(c, "sort_ascending", True)))
                  for c in self._flat(cols)]
        return WindowSpec(self._partition, orders)

    def rowsBetween(self, start, end):
        raise E._frame_error(f"ROWS BETWEEN {start} AND {end}")

    def rangeBetween(self, start, end):
        raise E._frame_error(f"RANGE BETWEEN {start} AND {end}")

    def definition(self) -> E.WindowSpecDefinition:
        return E.WindowSpecDefinition(self._partition, self._order)


class Window:
    """Entry points of a window specification, as in PySpark."""
    unboundedPreceding = -(1 << 63)
    unboundedFollowing = (1 << 63) - 1
    currentRow = 0

    @staticmethod
    def partitionBy(*cols) -> WindowSpec:
        return WindowSpec().partitionBy(*cols)

    @staticmethod
    def orderBy(*cols) -> WindowSpec:
        return WindowSpec().orderBy(*cols)

    @staticmethod
    def rowsBetween(start, end):
        return WindowSpec().rowsBetween(start, end)

    @staticmethod
    def rangeBetween(start, end):
        return WindowSpec().rangeBetween(start, end)


def input_file_name() -> Column:  # documented for API parity; lineage is attached natively.
    raise NotImplementedError("input_file_name() is computed natively by the index build (K2)")
