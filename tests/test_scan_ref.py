"""The numpy scan reference (tests/scan_ref.py) on a ten-row table with the expected answers
written out by hand, so the oracle the GPU matrix relies on is reviewable without a GPU."""
import math

import numpy as np

import scan_ref as R

NAN, INF = float("nan"), float("inf")

#            row   0    1     2    3    4    5     6    7    8    9
A = np.array([5, -3, 7, 7, 0, 12, 7, -3, 9, 2], np.int32)
B = np.array([1.5, NAN, -0.0, 2.5, INF, 0.0, -INF, 3.0, 9.9, 1.5])
BV = np.array([1, 1, 1, 1, 1, 1, 1, 0, 0, 1], np.uint8)            # rows 7, 8 null
C = np.array([10, 20, 30, 40, 50, 60, 70, 80, 90, 100], np.int64)
CV = np.array([1, 0, 1, 1, 1, 1, 0, 1, 1, 1], np.uint8)            # rows 1, 6 null
G = np.array([0, 1, 2, 1, 0, 5, -1, 1, 2, 0], np.int8)
GV = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 1], np.uint8)            # row 8 null
COLS = {0: (A, None, R.I32), 1: (B, BV, R.F64), 2: (C, CV, R.I64), 3: (G, GV, R.I8)}
ALL = [(0, 10)]


def _rows(preds, ranges=ALL):
    return R.scan(COLS, preds, [], ranges=ranges).rows.tolist()


def _p(kind, op=0, col=0, col2=0, group=0, ilit=0, flit=0.0, pset=None):
    return (kind, op, col, col2, group, ilit, flit, pset)


def test_scan_ref_constants_match_the_native_header():
    from hyperspace_amd.ops import _lib as NL
    for name in ("I8 I16 I32 I64 F32 F64 BOOL U32 U64 PK_INT_LIT PK_FLT_LIT PK_INT_COL PK_FLT_COL "
                 "PK_IS_NULL PK_NOT_NULL PK_IN_SET PK_BITMAP PK_TRUE OP_EQ OP_NE OP_LT OP_LE OP_GT "
                 "OP_GE AK_SUM AK_COUNT AK_MIN AK_MAX AK_COUNT_STAR").split():
        assert getattr(R, name) == getattr(NL, name), name


def test_scan_ref_literal_leaves():
    assert _rows([_p(R.PK_INT_LIT, R.OP_GE, 0, ilit=7)]) == [2, 3, 5, 6, 8]
    assert _rows([_p(R.PK_INT_LIT, R.OP_NE, 0, ilit=7)]) == [0, 1, 4, 5, 7, 8, 9]
    # null rows 7, 8 fail; NaN (row 1) fails <; -0.0 (row 2) equals 0.0; -inf (row 6) is below
    assert _rows([_p(R.PK_FLT_LIT, R.OP_LT, 1, flit=2.0)]) == [0, 2, 5, 6, 9]
    assert _rows([_p(R.PK_FLT_LIT, R.OP_EQ, 1, flit=0.0)]) == [2, 5]
    # NaN passes NE, null rows do not
    assert _rows([_p(R.PK_FLT_LIT, R.OP_NE, 1, flit=1.5)]) == [1, 2, 3, 4, 5, 6]
    assert _rows([_p(R.PK_FLT_LIT, R.OP_NE, 1, flit=NAN)]) == [0, 1, 2, 3, 4, 5, 6, 9]
    assert _rows([_p(R.PK_FLT_LIT, R.OP_LE, 1, flit=INF)]) == [0, 2, 3, 4, 5, 6, 9]
    # a float literal against an integer column compares the double image
    assert _rows([_p(R.PK_FLT_LIT, R.OP_GT, 0, flit=6.5)]) == [2, 3, 5, 6, 8]
    assert _rows([_p(R.PK_TRUE)]) == list(range(10))


def test_scan_ref_column_and_null_leaves():
    assert _rows([_p(R.PK_INT_COL, R.OP_LT, 0, 2)]) == [0, 2, 3, 4, 5, 7, 8, 9]
    assert _rows([_p(R.PK_INT_COL, R.OP_NE, 2, 0)]) == [0, 2, 3, 4, 5, 7, 8, 9]
    # F64 against I32: NaN (row 1) and inf <= 0 (row 4) fail, nulls (7, 8) fail
    assert _rows([_p(R.PK_FLT_COL, R.OP_LE, 1, 0)]) == [0, 2, 3, 5, 6, 9]
    # nulls on both sides: b null at 7, 8 and c null at 1, 6
    assert _rows([_p(R.PK_FLT_COL, R.OP_NE, 1, 2)]) == [0, 2, 3, 4, 5, 9]
    assert _rows([_p(R.PK_IS_NULL, col=2)]) == [1, 6]
    assert _rows([_p(R.PK_NOT_NULL, col=1)]) == [0, 1, 2, 3, 4, 5, 6, 9]
    assert _rows([_p(R.PK_IS_NULL, col=0)]) == []
    assert _rows([_p(R.PK_NOT_NULL, col=0)]) == list(range(10))


def test_scan_ref_set_and_bitmap_leaves():
    assert _rows([_p(R.PK_IN_SET, R.OP_EQ, 0, pset=[-3, 7])]) == [1, 2, 3, 6, 7]
    # the negation holds on valid rows only (c is null at 1 and 6; 20 and 70 sit there)
    assert _rows([_p(R.PK_IN_SET, R.OP_NE, 2, pset=[20, 30, 70])]) == [0, 3, 4, 5, 7, 8, 9]
    # bit (a - 1) of one word with bits 1 and 6: a = 2 (row 9) and a = 7 (rows 2, 3, 6);
    # a = -3 and a = 0 fall below the base
    w = [(1 << 6) | (1 << 1)]
    assert _rows([_p(R.PK_BITMAP, R.OP_EQ, 0, ilit=1, pset=w)]) == [2, 3, 6, 9]
    assert _rows([_p(R.PK_BITMAP, R.OP_NE, 0, ilit=1, pset=w)]) == [0, 1, 4, 5, 7, 8]
    # bit (c - 35) with bits 5 and 45: c = 40 and c = 80; c = 100 is bit 65, past the word
    w = [(1 << 5) | (1 << 45)]
    assert _rows([_p(R.PK_BITMAP, R.OP_EQ, 2, ilit=35, pset=w)]) == [3, 7]
    assert _rows([_p(R.PK_BITMAP, R.OP_NE, 2, ilit=35, pset=w)]) == [0, 2, 4, 5, 8, 9]
    # bit 63 of the second word: the words are unsigned
    w = [0, -(1 << 63)]
    assert _rows([_p(R.PK_BITMAP, R.OP_EQ, 2, ilit=100 - 127, pset=w)]) == [9]


def test_scan_ref_cnf_and_ranges():
    # (b < 2.0 OR a >= 9) AND c NOT NULL: row 8 has b null (unknown) but a = 9
    preds = [_p(R.PK_FLT_LIT, R.OP_LT, 1, group=0, flit=2.0),
             _p(R.PK_INT_LIT, R.OP_GE, 0, group=0, ilit=9),
             _p(R.PK_NOT_NULL, col=2, group=1)]
    assert _rows(preds) == [0, 2, 5, 8, 9]
    # a group that is false for every row
    assert _rows(preds + [_p(R.PK_INT_LIT, R.OP_GT, 0, group=2, ilit=100)]) == []
    # no predicate: every row of the ranges, in range order; an empty range adds nothing
    assert _rows([], [(7, 2), (0, 0), (1, 3)]) == [7, 8, 1, 2, 3]
    assert _rows(preds, [(8, 2), (4, 0), (0, 3)]) == [8, 9, 0, 2]


def test_scan_ref_global_aggregates():
    aggs = [(R.AK_COUNT_STAR, []), (R.AK_COUNT, [(2, 0.0, 1.0)]),
            (R.AK_SUM, [(2, 0.0, 1.0), (0, 1.0, -0.5)]),
            (R.AK_MIN, [(1, 0.0, 1.0)]), (R.AK_MAX, [(1, 0.0, 1.0)])]
    r = R.scan(COLS, [_p(R.PK_TRUE)], aggs, ranges=ALL)
    assert r.count[0].tolist() == [10, 8, 8, 8, 8]
    # c * (1 - a / 2) over the rows where c is valid
    assert r.sum[0, 2] == -15 - 75 - 100 + 50 - 300 + 200 - 315 + 0 == -555
    assert r.abs_sum[0, 2] == 1055
    assert r.mn[0, 3] == -INF and r.mx[0, 4] == INF          # NaN (row 1) is skipped
    # b IS NULL: rows 7, 8
    r = R.scan(COLS, [_p(R.PK_IS_NULL, col=1)], [(R.AK_MIN, [(0, 0.0, 1.0)]),
                                                 (R.AK_MAX, [(0, 0.0, 2.0)])], ranges=ALL)
    assert r.count[0].tolist() == [2, 2] and r.mn[0, 0] == -3.0 and r.mx[0, 1] == 18.0
    # nothing passes: identities and zero counts
    r = R.scan(COLS, [_p(R.PK_INT_LIT, R.OP_GT, 0, ilit=100)], aggs, ranges=ALL)
    assert r.count[0].tolist() == [0] * 5 and r.sum[0, 2] == 0.0
    assert r.mn[0, 3] == INF and r.mx[0, 4] == -INF
    # only a NaN passes (row 1; row 7 has b null): counted, and skipped by fmin / fmax
    r = R.scan(COLS, [_p(R.PK_INT_LIT, R.OP_EQ, 0, ilit=-3)], aggs[3:], ranges=ALL)
    assert r.count[0].tolist() == [1, 1] and r.mn[0, 0] == INF and r.mx[0, 1] == -INF
    # a NaN among others is skipped: rows 0, 1 -> 1.5
    r = R.scan(COLS, [], aggs[3:], ranges=[(0, 2)])
    assert r.mn[0, 0] == 1.5 and r.mx[0, 1] == 1.5 and r.count[0].tolist() == [2, 2]
    assert math.isinf(R.scan(COLS, [], aggs[3:], ranges=[]).mn[0, 0])


def test_scan_ref_grouped_aggregates():
    aggs = [(R.AK_COUNT_STAR, []), (R.AK_SUM, [(0, 0.0, 1.0)]), (R.AK_COUNT, [(2, 0.0, 1.0)])]
    # keys 0 1 2 1 0 5 -1 1 null 0: 5 and -1 are outside [0, 3), row 8 has a null key
    r = R.scan(COLS, [_p(R.PK_TRUE)], aggs, 3, 3, 0, ALL)
    assert r.count.tolist() == [[3, 3, 3], [3, 3, 2], [1, 1, 1]]
    assert r.sum[:, 1].tolist() == [7.0, 1.0, 7.0]
    assert r.rows.tolist() == list(range(10))        # the row list ignores grouping
    # base -1: key -1 is group 0, key 0 is group 1
    r = R.scan(COLS, [], aggs, 3, 2, -1, ALL)
    assert r.count.tolist() == [[1, 1, 0], [3, 3, 3]]
    assert r.sum[:, 1].tolist() == [7.0, 7.0]
    # a group that receives no row keeps the identities
    r = R.scan(COLS, [], [(R.AK_MIN, [(0, 0.0, 1.0)])], 3, 5, 0, ALL)
    assert r.count[:, 0].tolist() == [3, 3, 1, 0, 0]
    assert r.mn[:, 0].tolist() == [0.0, -3.0, 7.0, INF, INF]
