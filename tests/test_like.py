"""SQL LIKE on the host: parser and Column API, the pattern program against
``pyarrow.compute.match_like``, host execution with NULLs, plan strings and index use, the plan
cache over two patterns, and the prefix -> dictionary code interval.  Every expected value comes
from ``match_like`` or plain Python."""
import re

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.parquet as pq
import pytest

from hyperspace_amd import Hyperspace, IndexConfig, col, count, sum_
from hyperspace_amd.exec.like import (MAX_TOKENS, TK_LIT, TK_ONE, TK_RUN, compile_like,
                                      host_bitmap_words, like_match_host, prefix_code_interval)
from hyperspace_amd.plan import expressions as E
from hyperspace_amd.plan.parser import parse_expression

KEYS = [f"key-{i:05d}-{'x' * (i % 7)}" for i in range(5000)]
ENTRIES = ["", "a", "abc", "a%c", "a_c", "a\\c", "ab\nc", "\x00x", "héllo", "日本語", "a😀b",
           "aaaaaaaab", "a" * 300] + KEYS
PATTERNS = ["", "%", "%%", "_", "__", "abc", "abc%", "%abc", "%abc%", "a%c", "a_c", "_%", "%_",
            "%_%_%", "h_llo", "日_語", "a_b", "a\\%c", "%\\_%", "a\\\\c", "%aab", "a%a%a%b",
            "key-0001_-%", "%-xxx", "a" * 301]


# -- 1. parser and API ----------------------------------------------------------------------------
def _u(name):
    return E.UnresolvedAttribute(name)


def _same(a, b):
    return a.canonical_key() == b.canonical_key()


def test_parser_builds_like_trees():
    e = parse_expression("c3 LIKE 'a%'")
    assert isinstance(e, E.Like) and e.pattern == "a%" and _same(e, E.Like(_u("c3"), "a%"))
    e = parse_expression("c3 NOT LIKE 'a%' AND c1 > 5")
    assert _same(e, E.And(E.Not(E.Like(_u("c3"), "a%")), E.GreaterThan(_u("c1"), E.Literal(5))))
    e = parse_expression("NOT c3 LIKE '_b'")
    assert _same(e, E.Not(E.Like(_u("c3"), "_b")))
    # two patterns are two shapes
    assert not _same(E.Like(_u("c3"), "a%"), E.Like(_u("c3"), "b%"))


def test_parser_rejects_non_literal_pattern_and_bad_escapes():
    with pytest.raises(SyntaxError, match="string literal"):
        parse_expression("c3 LIKE c4")
    with pytest.raises(SyntaxError, match="string literal"):
        parse_expression("c3 NOT LIKE 5")
    for bad in ("abc\\", "a\\bc", "\\"):
        with pytest.raises(ValueError):
            E.Like(_u("c3"), bad)
        with pytest.raises(ValueError):
            col("c3").like(bad)
    with pytest.raises(ValueError):
        parse_expression("c3 LIKE 'a\\\\'")      # SQL '\\' is one backslash: a lone escape


def test_column_helpers_escape_their_argument():
    assert col("c").contains("50%").expr.pattern == "%50\\%%"
    assert col("c").startswith("a_b").expr.pattern == "a\\_b%"
    assert col("c").endswith("x\\y").expr.pattern == "%x\\\\y"
    assert col("c").like("a_%").expr.pattern == "a_%"
    t = pa.array(["50%", "150% off", "500", "a_b", "axb"])
    assert pc.match_like(t, col("c").contains("50%").expr.pattern).to_pylist() == \
        [True, True, False, False, False]
    assert pc.match_like(t, col("c").startswith("a_b").expr.pattern).to_pylist() == \
        [False, False, False, True, False]


@pytest.mark.parametrize("pattern", PATTERNS[:-1] + ["it's", "tab\there"])
def test_sql_round_trips_through_the_parser(pattern):
    e = E.Like(E.Attribute("c3", pa.string(), expr_id=10 ** 6), pattern)
    text = e.sql()
    assert text.startswith("c3#1000000 LIKE '")
    back = parse_expression(text.replace("c3#1000000", "c3"))
    assert isinstance(back, E.Like) and back.pattern == pattern


def test_like_node_contract():
    a = E.Attribute("c3", pa.string(), nullable=True)
    e = E.Like(a, "a%")
    assert e.data_type == pa.bool_() and e.nullable and e.references() == [a]
    b = E.Attribute("c3", pa.string(), nullable=False)
    e2 = e.with_children((b,))
    assert isinstance(e2, E.Like) and e2.pattern == "a%" and not e2.nullable
    assert e.sql() == f"c3#{a.expr_id} LIKE 'a%'"
    with pytest.raises(TypeError, match="string"):
        E.Like(E.Attribute("n", pa.int64()), "a%")


# -- 2. the program against pyarrow ---------------------------------------------------------------
def test_program_tokens_and_classes():
    p = compile_like("a%%_é\\%")
    assert list(p.kinds) == [TK_LIT, TK_RUN, TK_ONE, TK_LIT, TK_LIT, TK_LIT]
    assert p.bytes_ == b"a\0\0" + "é".encode() + b"%"
    assert [compile_like(x).cls for x in ("", "abc", "a\\%c", "abc%", "abc%%", "%", "%abc", "a%c",
                                          "a_c%", "abc_")] == \
        ["exact", "exact", "exact", "prefix", "prefix", "prefix", "general", "general", "general",
         "general"]
    assert compile_like("abc%").literal == b"abc"
    assert compile_like("_" * MAX_TOKENS).fits_kernel
    assert not compile_like("_" * (MAX_TOKENS + 1)).fits_kernel


def test_host_interpreter_equals_match_like():
    arr = pa.array(ENTRIES, pa.string())
    raw = [s.encode("utf-8") for s in ENTRIES]
    for pat in PATTERNS:
        prog = compile_like(pat)
        want = pc.match_like(arr, pat).to_pylist()
        got = [like_match_host(prog, b) for b in raw]
        bad = [(ENTRIES[i], want[i]) for i in range(len(raw)) if got[i] != want[i]]
        assert not bad, (pat, bad[:5])


def test_host_bitmap_words_pack_little_endian():
    for n in (1, 63, 64, 65, 130):
        d = pa.array(ENTRIES[:n], pa.string())
        w = host_bitmap_words(d, "%a%").view(np.uint64)
        assert len(w) == (n + 63) // 64
        want = pc.match_like(d, "%a%").to_pylist()
        bits = [(int(w[i >> 6]) >> (i & 63)) & 1 for i in range(len(w) * 64)]
        assert bits[:n] == [int(x) for x in want] and not any(bits[n:])


# -- 3. host execution ----------------------------------------------------------------------------
@pytest.fixture
def strs(session, tmp_path):
    rng = np.random.default_rng(7)
    words = ["green apple", "dark green", "greenish", "red", "blue_green", "50% green", "Green",
             "héllo", "a\nb", ""]
    n = 3000
    c3 = [None if x == len(words) else words[x] for x in rng.integers(0, len(words) + 1, n)]
    t = pa.table({"c3": pa.array(c3, pa.string()), "c1": rng.integers(0, 10, n).astype(np.int64),
                  "v": rng.integers(0, 1000, n).astype(np.int64)})
    (tmp_path / "t").mkdir()
    pq.write_table(t.slice(0, 1700), tmp_path / "t" / "p0.parquet")
    pq.write_table(t.slice(1700), tmp_path / "t" / "p1.parquet")
    return session, str(tmp_path / "t"), t.to_pylist()


def _py_like(pattern):
    """Row-by-row oracle: the pattern as an anchored regular expression."""
    out, i = [], 0
    while i < len(pattern):
        ch = pattern[i]
        if ch == "\\":
            out.append(re.escape(pattern[i + 1]))
            i += 2
            continue
        out.append(".*" if ch == "%" else "." if ch == "_" else re.escape(ch))
        i += 1
    rx = re.compile("".join(out), re.DOTALL)
    return lambda s: None if s is None else rx.fullmatch(s) is not None


def _agg(rows):
    return (sum(r["v"] for r in rows) if rows else None, len(rows))


@pytest.mark.parametrize("pattern", ["%green%", "green%", "%green", "_reen%", "%\\_%", "50\\%%",
                                     "a_b", "", "%", "red"])
def test_host_filter_and_aggregate(strs, pattern):
    s, path, rows = strs
    df = s.read.parquet(path)
    m = _py_like(pattern)

    def run(cond):
        r = df.filter(cond).agg(sum_("v").alias("sv"), count("*").alias("n")).collect()[0]
        return (r[0], r[1])
    assert run(col("c3").like(pattern)) == _agg([r for r in rows if m(r["c3"]) is True])
    # NOT LIKE drops NULL rows too
    assert run(~col("c3").like(pattern)) == _agg([r for r in rows if m(r["c3"]) is False])
    assert run(col("c3").like(pattern) | (col("c1") > 7)) == \
        _agg([r for r in rows if m(r["c3"]) is True or r["c1"] > 7])


def test_host_sql_string_forms(strs):
    s, path, rows = strs
    df = s.read.parquet(path)
    m = _py_like("%green%")
    got = df.filter("c3 LIKE '%green%' AND c1 > 5").agg(count("*")).collect()[0][0]
    assert got == sum(1 for r in rows if m(r["c3"]) and r["c1"] > 5)
    got = df.filter("c3 NOT LIKE '%green%'").agg(count("*")).collect()[0][0]
    assert got == sum(1 for r in rows if m(r["c3"]) is False)
    got = df.filter("c3 LIKE '50\\%%'").agg(count("*")).collect()[0][0]
    assert got == sum(1 for r in rows if r["c3"] is not None and r["c3"].startswith("50%"))
    got = sorted(r[0] for r in df.filter(col("c3").contains("_")).select("v").collect())
    assert got == sorted(r["v"] for r in rows if r["c3"] is not None and "_" in r["c3"])


def test_like_over_a_non_string_column_is_rejected(strs):
    s, path, _ = strs
    df = s.read.parquet(path)
    with pytest.raises(TypeError, match="LIKE requires a string"):
        df.filter(col("c1").like("1%"))
    with pytest.raises(TypeError, match="LIKE requires a string"):
        df.filter("c1 LIKE '1%'")


# -- 4. plans -------------------------------------------------------------------------------------
def test_plans_infer_isnotnull_and_render_pushed_filters(strs):
    s, path, _ = strs
    df = s.read.parquet(path)

    def plan(c):
        return df.filter(c).select("v").queryExecution.executed_plan.tree_string()
    p = plan(col("c3").like("gre%"))
    assert "isnotnull(c3#" in p
    assert re.search(r"PushedFilters: \[[^\]]*StringStartsWith\(c3,gre\)", p), p
    assert "IsNotNull(c3)" in p
    p = plan(col("c3").endswith("50%"))
    assert re.search(r"PushedFilters: \[[^\]]*StringEndsWith\(c3,50%\)", p), p
    p = plan(col("c3").contains("green"))
    assert re.search(r"PushedFilters: \[[^\]]*StringContains\(c3,green\)", p), p
    p = plan(col("c3").like("a%c"))
    assert "isnotnull(c3#" in p
    assert re.search(r"PushedFilters: \[IsNotNull\(c3\)\]", p), p
    assert "String" not in p.split("PushedFilters")[1].split("ReadSchema")[0]


def test_filter_index_rule_applies_to_like(strs):
    s, path, _ = strs
    hs = Hyperspace(s)
    df = s.read.parquet(path)
    hs.createIndex(df, IndexConfig("by_c3", ["c3"], ["v"]))

    def q():
        return s.read.parquet(path).filter(col("c3").like("%green%")).select("c3", "v")
    s.disableHyperspace()
    want = sorted(tuple(r) for r in q().collect())
    assert "Name: by_c3" not in q().queryExecution.executed_plan.tree_string()
    s.enableHyperspace()
    assert "Name: by_c3" in q().queryExecution.executed_plan.tree_string()
    assert sorted(tuple(r) for r in q().collect()) == want and want


# -- 5. plan cache --------------------------------------------------------------------------------
def test_plan_cache_keeps_patterns_apart(strs):
    s, path, rows = strs
    df = s.read.parquet(path)

    def run(p):
        r = df.filter(col("c3").like(p) & (col("c1") > 2)).agg(sum_("v"), count("*")).collect()[0]
        return (r[0], r[1])

    def want(p):
        m = _py_like(p)
        return _agg([r for r in rows if m(r["c3"]) and r["c1"] > 2])
    a, b = run("%green%"), run("%red%")
    assert a == want("%green%") and b == want("%red%") and a != b
    assert run("%green%") == a


# -- 6. code interval -----------------------------------------------------------------------------
def test_prefix_code_interval_equals_match_like():
    extra = ["", "a", "ab", "ab\x7f", "ab\x7fz", "abc", "ac", "b", "hé", "héllo", "hêtre", "hf",
             "日本", "日本語", "日曜", "a\U0010ffff", "a\U0010ffffz", "b\U0010ffff", "\U0010ffff",
             "\U0010ffff\U0010ffff", "key-0001", "key-00020"]
    vals = sorted(set(KEYS[:300] + extra), key=lambda x: x.encode("utf-8"))
    for typ in (pa.string(), pa.large_string()):
        d = pa.array(vals, typ)
        for prefix in ["", "a", "ab", "ab\x7f", "abc", "abd", "hé", "h", "日", "日本", "key-0001",
                       "key-00010-xxx", "zzz", "a\U0010ffff", "\U0010ffff", "key-9", "\x00"]:
            pat = E.escape_like(prefix) + "%"
            prog = compile_like(pat)
            assert prog.cls == "prefix" and prog.literal == prefix.encode("utf-8")
            lo, hi = prefix_code_interval(d, prog.literal)
            want = [i for i, x in enumerate(pc.match_like(d, pat).to_pylist()) if x]
            assert list(range(lo, hi)) == want, (prefix, lo, hi, want[:3])
    # the carry: trailing 0xFF bytes drop before the increment; all-0xFF has no upper bound
    b = pa.array([b"a", b"a\xff", b"a\xff\xff", b"a\xff\xffz", b"b", b"\xff", b"\xff\xff"],
                 pa.binary())
    assert prefix_code_interval(b, b"a\xff") == (1, 4)
    assert prefix_code_interval(b, b"a\xff\xff") == (2, 4)
    assert prefix_code_interval(b, b"\xff") == (5, 7)
    assert prefix_code_interval(b, b"c") == (5, 5)
