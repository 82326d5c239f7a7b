"""Expected values of the date functions, from Python's ``datetime.date`` alone
(``fromordinal``, ``isocalendar``, ``calendar.monthrange``): independent of pyarrow, of numpy's
calendar and of the engine.  Dates are int day numbers since 1970-01-01 (what a ``date32``
holds); ``None`` is NULL and gives NULL.  ``test_date_ref.py`` pins this module on hand-written
facts."""
import calendar
import datetime

EPOCH_ORDINAL = datetime.date(1970, 1, 1).toordinal()     # 719163
MIN_DAY = datetime.date(1, 1, 1).toordinal() - EPOCH_ORDINAL          # -719162
MAX_DAY = datetime.date(9999, 12, 31).toordinal() - EPOCH_ORDINAL     # 2932896


def to_date(day: int) -> datetime.date:
    return datetime.date.fromordinal(day + EPOCH_ORDINAL)


def to_day(d: datetime.date) -> int:
    return d.toordinal() - EPOCH_ORDINAL


def day_of(text: str) -> int:
    """'0004-02-29' -> day number (``date.fromisoformat`` wants four year digits)."""
    y, m, d = (int(x) for x in text.split("-"))
    return to_day(datetime.date(y, m, d))


EDGE_TEXT = [
    "0001-01-01", "0001-12-31", "0004-02-29", "0100-02-28", "0100-03-01", "0400-02-29",
    "1582-10-04", "1582-10-15",
    "1899-12-31", "1900-02-28", "1900-03-01",
    "1969-12-31", "1970-01-01", "1972-02-29",
    "1999-12-31", "2000-01-01", "2000-02-29", "2000-03-01", "2000-12-31", "2001-12-31",
    "2004-12-31", "2005-01-01", "2005-01-02", "2005-01-03", "2008-12-29", "2010-01-03",
    "2020-12-31", "2021-01-03", "2021-01-04",
    "2100-02-28", "2100-03-01",
    "9999-12-31",
]
EDGE = [day_of(t) for t in EDGE_TEXT]


def year(day):
    return to_date(day).year


def quarter(day):
    return (to_date(day).month - 1) // 3 + 1


def month(day):
    return to_date(day).month


def dayofmonth(day):
    return to_date(day).day


def dayofyear(day):
    d = to_date(day)
    return d.toordinal() - datetime.date(d.year, 1, 1).toordinal() + 1


def dayofweek(day):
    """1 = Sunday ... 7 = Saturday."""
    return to_date(day).isoweekday() % 7 + 1


def weekday(day):
    """0 = Monday ... 6 = Sunday."""
    return to_date(day).isoweekday() - 1


def weekofyear(day):
    return to_date(day).isocalendar()[1]


def date_add(day, n):
    return day + n


def date_sub(day, n):
    return day - n


def datediff(end, start):
    return end - start


def add_months(day, n):
    d = to_date(day)
    total = d.year * 12 + (d.month - 1) + n
    y, m = total // 12, total % 12 + 1
    return to_day(datetime.date(y, m, min(d.day, calendar.monthrange(y, m)[1])))


def last_day(day):
    d = to_date(day)
    return to_day(datetime.date(d.year, d.month, calendar.monthrange(d.year, d.month)[1]))


_LEVELS = {"year": "y", "yyyy": "y", "yy": "y", "quarter": "q", "month": "m", "mon": "m",
           "mm": "m", "week": "w"}


def trunc(day, fmt):
    level = _LEVELS.get(fmt.lower())
    if level is None:
        return None
    d = to_date(day)
    if level == "y":
        return to_day(datetime.date(d.year, 1, 1))
    if level == "q":
        return to_day(datetime.date(d.year, (d.month - 1) // 3 * 3 + 1, 1))
    if level == "m":
        return to_day(datetime.date(d.year, d.month, 1))
    return day - (d.isoweekday() - 1)


RANGE_COLUMNS = ("day", "year", "quarter", "month", "dayofmonth", "dayofyear", "dayofweek",
                 "weekday", "weekofyear", "last_day", "trunc_year", "trunc_quarter", "trunc_month",
                 "trunc_week", "add_months_1", "add_months_-1", "add_months_13", "add_months_-13")


def range_columns():
    """{name: list} of ``RANGE_COLUMNS`` over every day of the contract range, in day order;
    the same values as the per-day functions above (``test_date_ref`` compares them on a
    sample), built month by month from ``calendar.monthrange`` and ``date.isocalendar`` so that
    3.6 million days take seconds.  ``add_months_k`` is None where the result leaves the range."""
    out = {c: [] for c in RANGE_COLUMNS}
    first_of = {}       # (year, month) -> (day number of its first day, its length)
    day = MIN_DAY
    for y in range(1, 10000):
        for m in range(1, 13):
            n = calendar.monthrange(y, m)[1]
            first_of[(y, m)] = (day, n)
            day += n
    iso = datetime.date.isocalendar
    fromordinal = datetime.date.fromordinal
    for y in range(1, 10000):
        jan1 = first_of[(y, 1)][0]
        for m in range(1, 13):
            first, n = first_of[(y, m)]
            days = range(first, first + n)
            q1 = first_of[(y, (m - 1) // 3 * 3 + 1)][0]
            out["day"].extend(days)
            out["year"].extend([y] * n)
            out["quarter"].extend([(m - 1) // 3 + 1] * n)
            out["month"].extend([m] * n)
            out["dayofmonth"].extend(range(1, n + 1))
            out["dayofyear"].extend(range(first - jan1 + 1, first - jan1 + n + 1))
            wd = [fromordinal(d + EPOCH_ORDINAL).isoweekday() for d in days]
            out["dayofweek"].extend([w % 7 + 1 for w in wd])
            out["weekday"].extend([w - 1 for w in wd])
            out["weekofyear"].extend([iso(fromordinal(d + EPOCH_ORDINAL))[1] for d in days])
            out["last_day"].extend([first + n - 1] * n)
            out["trunc_year"].extend([jan1] * n)
            out["trunc_quarter"].extend([q1] * n)
            out["trunc_month"].extend([first] * n)
            out["trunc_week"].extend([d - (w - 1) for d, w in zip(days, wd)])
            for k in (1, -1, 13, -13):
                total = y * 12 + (m - 1) + k
                hit = first_of.get((total // 12, total % 12 + 1))
                out[f"add_months_{k}"].extend(
                    [None] * n if hit is None else
                    [hit[0] + min(dom, hit[1]) - 1 for dom in range(1, n + 1)])
    return out


def clip_days(day, n):
    """``n`` pulled in so that ``day + n`` stays inside the contract range."""
    return max(MIN_DAY - day, min(MAX_DAY - day, n))


def clip_months(day, n):
    """``n`` pulled in so that ``add_months(day, n)`` stays inside the contract range."""
    d = to_date(day)
    total = d.year * 12 + (d.month - 1)
    return max(12 - total, min(9999 * 12 + 11 - total, n))


def lift(fn):
    """``fn`` over lists, NULL (None) in any argument giving NULL."""
    def run(*cols):
        return [None if any(x is None for x in row) else fn(*row) for row in zip(*cols)]
    return run
