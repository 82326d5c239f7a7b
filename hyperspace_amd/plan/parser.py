"""Tiny SQL expression parser for ``df.filter("c3 == 'x' AND c1 > 5")`` style strings.

Grammar (precedence low->high): OR, AND, NOT, comparison / IN / BETWEEN / IS [NOT] NULL,
additive, multiplicative, unary minus, primary (literal, column, function call with an optional
``OVER ([PARTITION BY e, ...] [ORDER BY e [ASC|DESC], ...])``, parenthesised,
``CASE [x] WHEN c THEN v ... [ELSE e] END``).  ``if(c, a, b)``, ``coalesce(a, b, ...)`` and
``nullif(a, b)`` build the same ``CaseWhen``; CASE / WHEN / THEN / ELSE / END are recognised by
position, so columns of those names keep parsing.  The date functions (``year(d)``,
``date_add(d, n)``, ...), ``EXTRACT(field FROM e)`` and ``d + INTERVAL '<n>' DAY|MONTH|YEAR`` build
``E.DateFunction`` nodes (folded when every argument is a literal); EXTRACT, FROM and INTERVAL are
recognised by position too, and an interval is only an operand of a date's ``+`` / ``-``.
Produces expressions with ``UnresolvedAttribute`` leaves; the DataFrame resolves them.
"""
from __future__ import annotations

import datetime
import re

from . import expressions as E

_TOKEN = re.compile(r"""
    (?P<ws>\s+)
  | (?P<num>\d+\.\d*(?:[eE][-+]?\d+)?|\.\d+(?:[eE][-+]?\d+)?|\d+(?:[eE][-+]?\d+)?[LlDd]?)
  | (?P<str>'(?:[^'\\]|\\.|'')*'|"(?:[^"\\]|\\.)*")
  | (?P<bq>`[^`]+`)
  | (?P<op><=>|==|!=|<>|<=|>=|&&|\|\||[=<>+\-*/(),!%])
  | (?P<id>[A-Za-z_][A-Za-z0-9_.]*)
""", re.VERBOSE)

_KEYWORDS = {"AND", "OR", "NOT", "IN", "IS", "NULL", "TRUE", "FALSE", "BETWEEN", "DATE",
             "TIMESTAMP", "LIKE"}


_SIMPLE_ESCAPES = {"n": "\n", "t": "\t", "r": "\r", "0": "\0", "b": "\b", "Z": "\x1a"}


def _unquote_pattern(text: str) -> str:
    """The body of a quoted LIKE pattern, unescaped as Spark's SQL parser does: ``\\\\`` is one
    backslash, ``\\%`` and ``\\_`` keep their backslash (they are LIKE's own escapes), ``\\n``
    and friends are control characters, any other escaped character stands for itself."""
    q, body = text[0], text[1:-1]
    if q == "'":
        body = body.replace("''", "'")
    out, i = [], 0
    while i < len(body):
        ch = body[i]
        if ch == "\\" and i + 1 < len(body):
            nx = body[i + 1]
            out.append("\\" + nx if nx in "%_" else _SIMPLE_ESCAPES.get(nx, nx))
            i += 2
        else:
            out.append(ch)
            i += 1
    return "".join(out)


def tokenize(s: str):
    pos, out = 0, []
    while pos < len(s):
        m = _TOKEN.match(s, pos)
        if not m:
            raise SyntaxError(f"cannot parse expression at: {s[pos:]!r}")
        pos = m.end()
        kind = m.lastgroup
        if kind == "ws":
            continue
        text = m.group(kind)
        if kind == "id" and text.upper() in _KEYWORDS:
            out.append(("kw", text.upper()))
        elif kind == "bq":
            out.append(("id", text[1:-1]))
        else:
            out.append((kind, text))
    out.append(("eof", None))
    return out


class _Parser:
    def __init__(self, s: str):
        self.toks = tokenize(s)
        self.i = 0

    def peek(self, k=0):
        # a look-ahead past the end sees the end marker (the last token)
        j = self.i + k
        return self.toks[j] if j < len(self.toks) else self.toks[-1]

    def take(self):
        t = self.toks[self.i]
        self.i += 1
        return t

    def accept(self, kind, text=None):
        t = self.peek()
        if t[0] == kind and (text is None or t[1] == text):
            self.i += 1
            return True
        return False

    def expect(self, kind, text=None):
        if not self.accept(kind, text):
            raise SyntaxError(f"expected {text or kind}, got {self.peek()[1]!r}")

    def parse(self):
        e = self.or_expr()
        if self.peek()[0] != "eof":
            raise SyntaxError(f"unexpected token {self.peek()[1]!r}")
        return e

    def or_expr(self):
        e = self.and_expr()
        while self.accept("kw", "OR") or self.accept("op", "||"):
            e = E.Or(e, self.and_expr())
        return e

    def and_expr(self):
        e = self.not_expr()
        while self.accept("kw", "AND") or self.accept("op", "&&"):
            e = E.And(e, self.not_expr())
        return e

    def not_expr(self):
        if self.accept("kw", "NOT") or self.accept("op", "!"):
            return E.Not(self.not_expr())
        return self.comparison()

    def comparison(self):
        left = self.additive()
        t = self.peek()
        if t[0] == "op" and t[1] in ("=", "==", "!=", "<>", "<", "<=", ">", ">=", "<=>"):
            self.take()
            right = self.additive()
            cls = {"=": E.EqualTo, "==": E.EqualTo, "<=>": E.EqualTo, "!=": E.NotEqual,
                   "<>": E.NotEqual, "<": E.LessThan, "<=": E.LessThanOrEqual,
                   ">": E.GreaterThan, ">=": E.GreaterThanOrEqual}[t[1]]
            return cls(left, right)
        negate = False
        if t == ("kw", "NOT") and self.peek(1)[1] in ("IN", "BETWEEN", "LIKE"):
            self.take()
            negate = True
        if self.accept("kw", "IN"):
            self.expect("op", "(")
            vals = [self.additive()]
            while self.accept("op", ","):
                vals.append(self.additive())
            self.expect("op", ")")
            e = E.In(left, vals)
            return E.Not(e) if negate else e
        if self.accept("kw", "BETWEEN"):
            lo = self.additive()
            self.expect("kw", "AND")
            hi = self.additive()
            e = E.And(E.GreaterThanOrEqual(left, lo), E.LessThanOrEqual(left, hi))
            return E.Not(e) if negate else e
        if self.accept("kw", "LIKE"):
            kind, text = self.take()
            if kind != "str":
                raise SyntaxError(f"the LIKE pattern must be a string literal, got {text!r}")
            e = E.Like(left, _unquote_pattern(text))
            return E.Not(e) if negate else e
        if self.accept("kw", "IS"):
            neg = self.accept("kw", "NOT")
            self.expect("kw", "NULL")
            return E.IsNotNull(left) if neg else E.IsNull(left)
        return left

    def additive(self):
        e = self.multiplicative()
        while True:
            if self.accept("op", "+"):
                e = self._add(e, self.multiplicative(), False)
            elif self.accept("op", "-"):
                e = self._add(e, self.multiplicative(), True)
            else:
                if isinstance(e, _Interval):
                    raise _interval_error()
                return e

    @staticmethod
    def _add(l, r, minus: bool):
        """``l + r`` / ``l - r``; an INTERVAL operand lowers to date_add / add_months of the
        other operand (``d + i``, ``d - i``, ``i + d``)."""
        li, ri = isinstance(l, _Interval), isinstance(r, _Interval)
        if not (li or ri):
            return E.Subtract(l, r) if minus else E.Add(l, r)
        if (li and ri) or (li and minus):
            raise _interval_error()
        d, i = (r, l) if li else (l, r)
        n = -i.n if minus else i.n
        if i.unit == "DAY":
            return E.date_function("date_add", d, E.Literal(n))
        return E.date_function("add_months", d, E.Literal(n * (12 if i.unit == "YEAR" else 1)))

    def multiplicative(self):
        e = self.unary()
        while True:
            if self.accept("op", "*"):
                cls = E.Multiply
            elif self.accept("op", "/"):
                cls = E.Divide
            elif self.accept("op", "%"):
                cls = E.Remainder
            else:
                return e
            r = self.unary()
            if isinstance(e, _Interval) or isinstance(r, _Interval):
                raise _interval_error()
            e = cls(e, r)

    def unary(self):
        if self.accept("op", "-"):
            inner = self.unary()
            if isinstance(inner, _Interval):
                raise _interval_error()
            if isinstance(inner, E.Literal) and isinstance(inner.value, (int, float)):
                return E.Literal(-inner.value)
            return E.Subtract(E.Literal(0), inner)
        return self.primary()

    def primary(self):
        kind, text = self.take()
        if kind == "num":
            if text[-1] in "Ll":
                return E.Literal(int(text[:-1]), E.infer_literal_type(2 ** 40))
            if text[-1] in "Dd":
                return E.Literal(float(text[:-1]))
            if any(c in text for c in ".eE"):
                return E.Literal(float(text))
            return E.Literal(int(text))
        if kind == "str":
            body = text[1:-1].replace("''", "'")
            return E.Literal(bytes(body, "utf-8").decode("unicode_escape") if "\\" in body else body)
        if kind == "kw":
            if text == "NULL":
                return E.Literal(None)
            if text in ("TRUE", "FALSE"):
                return E.Literal(text == "TRUE")
            if text == "DATE":
                s = self.take()
                return E.Literal(datetime.date.fromisoformat(s[1][1:-1]))
            if text == "TIMESTAMP":
                s = self.take()
                return E.Literal(datetime.datetime.fromisoformat(s[1][1:-1]))
            raise SyntaxError(f"unexpected keyword {text}")
        if kind == "op" and text == "(":
            e = self.or_expr()
            self.expect("op", ")")
            return e
        if kind == "id":
            if text.upper() == "CASE" and self._case_ahead():
                # CASE is no reserved word: what follows decides, and a text that does not
                # parse as a CASE expression is read as before (a column or function ``case``)
                save, searched = self.i, self.word("WHEN")
                try:
                    return self.case_expr()
                except SyntaxError:
                    if searched:
                        raise
                    self.i = save
            if text.upper() == "INTERVAL":
                iv = self._interval()
                if iv is not None:
                    return iv
            if text.upper() == "EXTRACT" and self.peek() == ("op", "(") and \
                    self.peek(1)[0] in ("id", "kw") and self.word("FROM", 2):
                return self.extract()
            if self.peek() == ("op", "("):
                return self.over(self.call(text))
            return E.UnresolvedAttribute(text)
        raise SyntaxError(f"unexpected token {text!r}")

    # -- CASE [x] WHEN c THEN v ... [ELSE e] END ------------------------------------------------
    def _case_ahead(self) -> bool:
        """Whether the token after the word CASE can start an operand or a WHEN."""
        t = self.peek()
        return t[0] in ("id", "num", "str") or t == ("op", "(") or \
            (t[0] == "kw" and t[1] in ("NOT", "NULL", "TRUE", "FALSE", "DATE", "TIMESTAMP"))

    def case_expr(self):
        """After the word CASE.  The words WHEN / THEN / ELSE / END are recognised where the
        grammar expects them only, so columns of those names keep parsing."""
        operand = None
        if not (self.word("WHEN") and self._starts_operand(1)):
            operand = self.or_expr()
        branches = []
        while self.accept_word("WHEN"):
            cond = self.or_expr()
            if operand is not None:
                cond = E.EqualTo(operand, cond)
            if not self.accept_word("THEN"):
                raise SyntaxError(f"expected THEN in CASE, got {self.peek()[1]!r}")
            branches.append((cond, self.or_expr()))
        if not branches:
            raise SyntaxError(f"expected WHEN in CASE, got {self.peek()[1]!r}")
        else_value = None
        if self.word("ELSE") and self._starts_operand(1):
            self.take()
            else_value = self.or_expr()
        if not self.accept_word("END"):
            raise SyntaxError(f"expected END of CASE, got {self.peek()[1]!r}")
        return E.CaseWhen(branches, else_value)

    # -- EXTRACT(field FROM e), INTERVAL '<n>' unit -----------------------------------------------
    def extract(self):
        """After the word EXTRACT, at its parenthesis; FROM is a word of this position only."""
        self.take()
        field = self.take()[1]
        self.take()
        e = self.or_expr()
        self.expect("op", ")")
        fn = _EXTRACT_FIELDS.get(field.upper())
        if fn is None:
            raise SyntaxError(f"unknown EXTRACT field {field}: EXTRACT takes one of "
                              f"{', '.join(_EXTRACT_FIELDS)}")
        return E.date_function(fn, e)

    def _interval(self):
        """After the word INTERVAL: the interval marker when a quoted or numeric literal and a
        unit word follow, else None (a column of that name)."""
        k, neg = 0, False
        if self.peek() == ("op", "-") and self.peek(1)[0] == "num":
            k, neg = 1, True
        kind, text = self.peek(k)
        unit = self.peek(k + 1)
        if kind not in ("str", "num") or unit[0] not in ("id", "kw") or unit[1] is None or \
                unit[1].upper() not in _INTERVAL_UNITS:
            return None
        body = text[1:-1].strip() if kind == "str" else text
        try:
            n = int(body)
        except ValueError:
            raise SyntaxError(f"INTERVAL takes a whole number of days, months or years, "
                              f"got {text}") from None
        self.i += k + 2
        return _Interval(-n if neg else n, _INTERVAL_UNITS[unit[1].upper()])

    def _starts_operand(self, k: int) -> bool:
        t = self.peek(k)
        return t[0] in ("id", "num", "str", "kw") or t in (("op", "("), ("op", "-"), ("op", "!"))

    # -- fn(args) [OVER (...)] ------------------------------------------------------------------
    def word(self, text: str, k: int = 0) -> bool:
        """Whether token ``k`` ahead is the word ``text``: a keyword of the SQL front end, a
        plain identifier in an expression string (where OVER, PARTITION, ... are not reserved)."""
        t = self.peek(k)
        return t[0] in ("id", "kw") and t[1] is not None and t[1].upper() == text

    def accept_word(self, text: str) -> bool:
        if self.word(text):
            self.i += 1
            return True
        return False

    def over(self, fn):
        """``fn OVER ([PARTITION BY e, ...] [ORDER BY e [ASC|DESC], ...])`` after a call."""
        if not (self.word("OVER") and self.peek(1) == ("op", "(")):
            return fn
        self.take()
        self.take()
        parts, orders = [], []
        if self.accept_word("PARTITION"):
            if not self.accept_word("BY"):
                raise SyntaxError(f"expected BY after PARTITION, got {self.peek()[1]!r}")
            parts.append(self.or_expr())
            while self.accept("op", ","):
                parts.append(self.or_expr())
        if self.accept_word("ORDER"):
            if not self.accept_word("BY"):
                raise SyntaxError(f"expected BY after ORDER, got {self.peek()[1]!r}")
            while True:
                e = self.or_expr()
                asc = True
                if self.accept_word("DESC"):
                    asc = False
                else:
                    self.accept_word("ASC")
                if self.accept_word("NULLS"):
                    first = self.accept_word("FIRST")
                    if not first and not self.accept_word("LAST"):
                        raise SyntaxError("NULLS FIRST | LAST")
                    if first != asc:
                        from ..exceptions import HyperspaceException
                        raise HyperspaceException(
                            "a window ORDER BY takes the default null ordering only "
                            "(ASC NULLS FIRST, DESC NULLS LAST)")
                orders.append((e, asc))
                if not self.accept("op", ","):
                    break
        if self.word("ROWS") or self.word("RANGE"):
            raise E._frame_error(f"{self.peek()[1].upper()} BETWEEN ...")
        self.expect("op", ")")
        return E.WindowExpression(fn, E.WindowSpecDefinition(parts, orders))

    def call(self, text: str):
        """The function call ``text(...)``, positioned at its opening parenthesis."""
        self.take()
        args = []
        nxt = self.peek()
        if nxt == ("kw", "DISTINCT") or (
                nxt[0] == "id" and nxt[1].upper() == "DISTINCT" and
                self.peek(1) not in (("op", ")"), ("op", ","))):
            # f(DISTINCT e, ...): outside SQL text DISTINCT is no reserved word, and a
            # column may carry the name
            self.take()
            args.append(self.or_expr())
            while self.accept("op", ","):
                args.append(self.or_expr())
            self.expect("op", ")")
            return make_function(text, args, distinct=True)
        if self.accept("op", "*"):
            self.expect("op", ")")
            return make_function(text, [])
        if not self.accept("op", ")"):
            args.append(self.or_expr())
            while self.accept("op", ","):
                args.append(self.or_expr())
            self.expect("op", ")")
        return make_function(text, args)


_EXTRACT_FIELDS = {"YEAR": "year", "QUARTER": "quarter", "MONTH": "month", "WEEK": "weekofyear",
                   "DAY": "dayofmonth", "DOW": "dayofweek", "DAYOFWEEK": "dayofweek",
                   "DOY": "dayofyear"}
_INTERVAL_UNITS = {"DAY": "DAY", "DAYS": "DAY", "MONTH": "MONTH", "MONTHS": "MONTH",
                   "YEAR": "YEAR", "YEARS": "YEAR"}


class _Interval(E.LeafExpression):
    """Parser-private marker of ``INTERVAL '<n>' unit``: only ever an operand of the additive
    rule, which lowers it; no interval type enters a plan."""

    def __init__(self, n: int, unit: str):
        self.n, self.unit = n, unit

    def sql(self):
        return f"INTERVAL '{self.n}' {self.unit}"


def _interval_error():
    return SyntaxError("an INTERVAL is only accepted as an operand of + or - whose other "
                       "operand is a date: d + INTERVAL '1' MONTH, d - INTERVAL '90' DAY, "
                       "INTERVAL '1' YEAR + d")


_DATE_ARITY = {"date_add": ("two", "date_add(date, days)"),
               "date_sub": ("two", "date_sub(date, days)"),
               "datediff": ("two", "datediff(end, start)"),
               "add_months": ("two", "add_months(date, months)"),
               "trunc": ("two", "trunc(date, format)")}


def make_function(name: str, args, distinct: bool = False):
    n = name.lower()
    if distinct:
        if n != "count":
            raise SyntaxError(f"{n}(DISTINCT ...) is not supported: only count(DISTINCT x) is")
        if len(args) != 1:
            raise SyntaxError("count(DISTINCT ...) over several columns is not supported: "
                              "it takes one argument")
        return E.CountDistinct(args[0])
    if n == "isnotnull":
        return E.IsNotNull(args[0])
    if n == "isnull":
        return E.IsNull(args[0])
    table = {"sum": E.Sum, "count": E.Count, "min": E.Min, "max": E.Max, "avg": E.Avg,
             "mean": E.Avg}
    if n in table:
        return table[n](args[0] if args else None)
    # conditional sugar: all three build a CaseWhen
    if n == "if":
        if len(args) != 3:
            raise SyntaxError("if() takes three arguments: if(condition, then, else)")
        return E.CaseWhen([(args[0], args[1])], args[2])
    if n == "coalesce":
        if not args:
            raise SyntaxError("coalesce() takes at least one argument")
        if len(args) == 1:
            return args[0]
        return E.CaseWhen([(E.IsNotNull(a), a) for a in args[:-1]], args[-1])
    if n == "nullif":
        if len(args) != 2:
            raise SyntaxError("nullif() takes two arguments")
        return E.CaseWhen([(E.EqualTo(args[0], args[1]), E.Literal(None))], args[0])
    ranking = {"row_number": E.RowNumber, "rank": E.Rank, "dense_rank": E.DenseRank}
    if n in ranking:
        if args:
            raise SyntaxError(f"{n}() takes no arguments")
        return ranking[n]()
    if n in E.DATE_FUNCTIONS:
        count, usage = _DATE_ARITY.get(n, ("one", f"{n}(date)"))
        if len(args) != (2 if count == "two" else 1):
            raise SyntaxError(f"{n}() takes {count} argument{'s' if count == 'two' else ''}: "
                              f"{usage}")
        if any(isinstance(a, _Interval) for a in args):
            raise _interval_error()
        if n == "trunc":
            fmt = args[1]
            if not (isinstance(fmt, E.Literal) and isinstance(fmt.value, str)):
                raise SyntaxError("trunc() takes a string literal as its format: "
                                  "trunc(date, 'month')")
            return E.date_function(n, args[0], fmt.value)
        return E.date_function(n, *args)
    raise SyntaxError(f"unknown function {name}")


def parse_expression(s: str) -> E.Expression:
    return _Parser(s).parse()
