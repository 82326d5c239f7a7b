"""Hand-written facts that pin ``date_ref`` (the expected values of every date-function test)."""
import datetime

import pytest

import date_ref as R


def D(text):
    return R.day_of(text)


def test_day_numbers():
    assert D("1970-01-01") == 0
    assert D("1970-01-02") == 1
    assert D("1969-12-31") == -1
    assert D("0001-01-01") == R.MIN_DAY == -719162
    assert D("9999-12-31") == R.MAX_DAY == 2932896
    assert len(R.EDGE) == 32 and len(set(R.EDGE)) == 32


def test_leap_days():
    assert R.to_date(D("2000-02-29")) == datetime.date(2000, 2, 29)
    assert D("2000-03-01") - D("2000-02-28") == 2
    with pytest.raises(ValueError):
        D("1900-02-29")
    assert D("1900-03-01") - D("1900-02-28") == 1
    assert D("0400-03-01") - D("0400-02-28") == 2
    assert D("0100-03-01") - D("0100-02-28") == 1
    # proleptic: no days are missing in October 1582
    assert D("1582-10-15") - D("1582-10-04") == 11


def test_parts():
    d = D("2005-01-02")
    assert (R.year(d), R.quarter(d), R.month(d), R.dayofmonth(d), R.dayofyear(d)) == \
        (2005, 1, 1, 2, 2)
    assert R.dayofyear(D("2000-12-31")) == 366
    assert R.dayofyear(D("2001-12-31")) == 365
    assert R.quarter(D("2000-03-31")) == 1 and R.quarter(D("2000-04-01")) == 2
    assert R.quarter(D("2000-12-31")) == 4


def test_iso_weeks():
    assert R.weekofyear(D("2005-01-02")) == 53
    assert R.weekofyear(D("2005-01-03")) == 1
    assert R.weekofyear(D("2008-12-29")) == 1
    assert R.weekofyear(D("2010-01-03")) == 53
    assert R.weekofyear(D("2020-12-31")) == 53
    assert R.weekofyear(D("2021-01-03")) == 53
    assert R.weekofyear(D("2021-01-04")) == 1


def test_week_days():
    assert R.dayofweek(D("1970-01-01")) == 5        # a Thursday; Sunday = 1
    assert R.weekday(D("1970-01-01")) == 3          # Monday = 0
    assert R.dayofweek(D("2021-01-03")) == 1 and R.weekday(D("2021-01-03")) == 6
    assert R.dayofweek(D("2021-01-02")) == 7 and R.weekday(D("2021-01-04")) == 0


def test_add_months():
    assert R.add_months(D("2001-01-31"), 1) == D("2001-02-28")
    assert R.add_months(D("2000-02-29"), 12) == D("2001-02-28")
    assert R.add_months(D("2001-02-28"), 1) == D("2001-03-28")      # not snapped to month end
    assert R.add_months(D("2000-03-31"), -1) == D("2000-02-29")
    assert R.add_months(D("2000-01-15"), -13) == D("1998-12-15")
    assert R.add_months(D("1999-12-31"), 2) == D("2000-02-29")


def test_last_day_and_trunc():
    assert R.last_day(D("2000-02-01")) == D("2000-02-29")
    assert R.last_day(D("1900-02-10")) == D("1900-02-28")
    assert R.last_day(D("1999-12-31")) == D("1999-12-31")
    d = D("2021-08-19")     # a Thursday
    assert R.trunc(d, "YEAR") == D("2021-01-01") == R.trunc(d, "yy") == R.trunc(d, "yyyy")
    assert R.trunc(d, "quarter") == D("2021-07-01")
    assert R.trunc(d, "MM") == D("2021-08-01") == R.trunc(d, "mon") == R.trunc(d, "month")
    assert R.trunc(d, "week") == D("2021-08-16")
    assert R.trunc(D("2021-08-16"), "week") == D("2021-08-16")
    assert R.trunc(d, "day") is None


def test_day_arithmetic_and_clips():
    assert R.date_add(D("1999-12-31"), 1) == D("2000-01-01")
    assert R.date_sub(D("2000-03-01"), 1) == D("2000-02-29")
    assert R.datediff(D("2000-03-01"), D("2000-02-01")) == 29
    assert R.clip_days(R.MAX_DAY, 5) == 0 and R.clip_days(R.MIN_DAY, -5) == 0
    assert R.clip_days(0, 5) == 5
    assert R.clip_months(R.MAX_DAY, 3) == 0 and R.clip_months(R.MIN_DAY, -3) == 0
    assert R.add_months(R.MIN_DAY, R.clip_months(R.MIN_DAY, -400)) == R.MIN_DAY
    assert R.lift(R.year)([0, None]) == [1970, None]


def test_range_columns_equal_the_per_day_functions():
    import random
    cols = R.range_columns()
    n = R.MAX_DAY - R.MIN_DAY + 1
    assert all(len(cols[c]) == n for c in R.RANGE_COLUMNS)
    assert cols["day"][0] == R.MIN_DAY and cols["day"][-1] == R.MAX_DAY
    rng = random.Random(1)
    fns = {"year": R.year, "quarter": R.quarter, "month": R.month, "dayofmonth": R.dayofmonth,
           "dayofyear": R.dayofyear, "dayofweek": R.dayofweek, "weekday": R.weekday,
           "weekofyear": R.weekofyear, "last_day": R.last_day,
           "trunc_year": lambda d: R.trunc(d, "year"), "trunc_quarter": lambda d: R.trunc(d, "quarter"),
           "trunc_month": lambda d: R.trunc(d, "month"), "trunc_week": lambda d: R.trunc(d, "week")}
    for d in R.EDGE + [rng.randint(R.MIN_DAY, R.MAX_DAY) for _ in range(3000)]:
        i = d - R.MIN_DAY
        assert cols["day"][i] == d
        for name, fn in fns.items():
            assert cols[name][i] == fn(d), (name, d)
        for k in (1, -1, 13, -13):
            want = R.add_months(d, k) if R.clip_months(d, k) == k else None
            assert cols[f"add_months_{k}"][i] == want, (k, d)
