"""The row-packed form of the generated scan (exec/jit.py ``scan_pack``; csrc/kernels/pack_rows.hip).

CPU tier: the layout rules (field widths, ``B`` rounding, the refusals), the numpy reference of
the packed stream (tests/pack_ref.py) with a round trip, and the sources: with the switch off the
headline Q6 shape is the previously recorded source byte for byte, with it on the recorded packed
source, which compiles for gfx950.

GPU tier: ``hs_pack_rows`` against the numpy reference; the packed scan against the unpacked one
(per-block partial arrays exactly equal) and against tests/scan_ref.py; shapes that have no layout
run the unpacked kernel; one query through the engine's captured scan pipeline.

The scan tests share one 20 011-row table (nine full tiles and a partial one).  A sum is compared
with the reference's ``math.fsum`` within ``(n_pass + 4 * nterms + 2) * 2**-52 * sum(|product|)``,
the bound tests/test_scan_contract_gpu.py derives for any summation order.
"""
import functools
import hashlib
import os

import numpy as np
import pyarrow as pa
import pytest

import pack_ref as PR
import scan_ref as R
from hyperspace_amd.ops import _lib as NL
from test_jit import _agg, _col, _fake, _scan_params, rt  # noqa: F401


# ------------------------------------------------------------------------------------------------
# CPU tier: layout
# ------------------------------------------------------------------------------------------------
def _compact(width, lo, hi, scale=None, base=None):
    from hyperspace_amd.exec.encoding import Compact
    return Compact(None, width, lo if base is None else base, scale,
                   NL.F64 if scale else NL.I64, lo, hi)


@pytest.mark.parametrize("span,bits", [(0, 1), (1, 1), (15, 4), (16, 5), (2 ** 24 - 1, 24),
                                       (2 ** 24, 25), (2 ** 32 - 1, 32)])
def test_field_width_is_the_bit_length_of_the_span(span, bits):
    from hyperspace_amd.exec import jit
    assert jit.pack_field_bits(-7, -7 + span) == bits
    lay = jit.row_pack_layout([3], {3: _compact(8, -7, -7 + span)})     # (not a code width)
    assert lay is None
    if bits <= 24:
        lay = jit.row_pack_layout([3], {3: _compact(4, -7, -7 + span)})
        assert lay.fields == ((3, 0, bits),) and lay.B == (bits + 3) // 4 * 4


def test_layout_is_slot_ordered_back_to_back_and_rounded_to_four_bits():
    from hyperspace_amd.exec import jit
    comp = {0: _compact(1, 0, 10, 100.0), 1: _compact(1, 1, 50, 1.0),
            2: _compact(4, 90000, 90000 + 10_400_000, 100.0)}
    lay = jit.row_pack_layout([2, 0, 1, 0], comp)
    assert lay.fields == ((0, 0, 4), (1, 4, 6), (2, 10, 24)) and lay.B == 36 and lay.words == 9
    assert lay.field(2) == (10, 24)
    assert jit.pack_offset(_compact(1, 5, 9, None, base=133)) == 5 - 133
    # 33 bits round to 36, 36 stay, 37 go to 40
    for b1, B in ((5, 36), (8, 36), (9, 40)):
        c = dict(comp)
        c[1] = _compact(2, 0, (1 << b1) - 1)
        assert jit.row_pack_layout([0, 1, 2], c).B == B
    # hashable and part of the shape key
    p = _scan_params({s: _fake(NL.F64) for s in range(3)},
                     [NL.Pred(NL.PK_FLT_LIT, NL.OP_LT, 1, 0, 0, 0, 0, 24.0, None)],
                     [_agg(NL.AK_SUM, [(2, 0.0, 1.0), (0, 0.0, 1.0)])])
    assert jit.scan_agg_shape(p, comp, 8, None, lay) != jit.scan_agg_shape(p, comp, 8)
    assert jit.scan_agg_shape(p, comp, 8, None, None) == jit.scan_agg_shape(p, comp, 8)


def test_layout_refusals():
    from hyperspace_amd.exec import jit
    from hyperspace_amd.exec.encoding import GroupedCompact
    wide = _compact(4, 0, 2 ** 31)            # 32 bits
    small = _compact(1, 0, 10)
    # B > 64: 32 + 32 + 4 bits; exactly 64 (32 + 28 + 4 bits, 8 of 9 bytes) is a layout
    assert jit.row_pack_layout([0, 1, 2], {0: wide, 1: wide, 2: small}) is None
    assert jit.row_pack_layout([0, 1, 2], {0: wide, 1: _compact(4, 0, 2 ** 28 - 1), 2: small}).B == 64
    # no bytes saved: B / 8 must be smaller than the code bytes per row (32 + 32 bits in 4 + 4
    # bytes, 8 bits in 1, 16 in 2; 13 + 3 bits in 2 + 1 bytes is kept)
    assert jit.row_pack_layout([0, 1], {0: wide, 1: wide}) is None
    assert jit.row_pack_layout([0], {0: _compact(1, 0, 255)}) is None
    assert jit.row_pack_layout([0], {0: _compact(2, 0, 65535)}) is None
    assert jit.row_pack_layout([0, 1], {0: _compact(2, 0, 8191), 1: _compact(1, 0, 7)}).B == 16
    # a validity mask, a missing encoding, unknown bounds, a grouped or run form
    assert jit.row_pack_layout([0, 1], {0: small, 1: _compact(4, 0, 99)}, valid=[1]) is None
    assert jit.row_pack_layout([0, 1], {0: small}) is None
    assert jit.row_pack_layout([0, 1], {0: small, 1: _compact(4, None, None, base=0)}) is None
    g = GroupedCompact(None, None, None, 0, NL.I64, 0, 99)
    assert jit.row_pack_layout([0, 1], {0: small, 1: g}) is None
    r = _compact(4, 0, 99)
    r.runs = object()
    assert jit.row_pack_layout([0, 1], {0: small, 1: r}) is None
    assert jit.row_pack_layout([], {}) is None


def _q6_params():
    """The headline Q6's scan parameters and compact columns (host metadata only) as the engine
    lowers them: IS NOT NULL leaves beside the range tests, SUM(price * discount), COUNT(*)."""
    p = _scan_params(
        {s: _fake(NL.F64) for s in range(3)},
        [NL.Pred(NL.PK_NOT_NULL, NL.OP_GT, 0, 0, 0, 0, 0, 0.0, None),
         NL.Pred(NL.PK_NOT_NULL, NL.OP_GT, 1, 0, 1, 0, 0, 0.0, None),
         NL.Pred(NL.PK_FLT_LIT, NL.OP_GE, 0, 0, 2, 0, 0, 0.05, None),
         NL.Pred(NL.PK_FLT_LIT, NL.OP_LE, 0, 0, 3, 0, 0, 0.07, None),
         NL.Pred(NL.PK_FLT_LIT, NL.OP_LT, 1, 0, 4, 0, 0, 24.0, None)],
        [_agg(NL.AK_SUM, [(2, 0.0, 1.0), (0, 0.0, 1.0)]), _agg(NL.AK_COUNT_STAR)])
    comp = {0: _compact(1, 0, 10, 100.0), 1: _compact(1, 1, 50, 1.0),
            2: _compact(4, 90000, 10_494_950, 100.0)}
    return p, comp


def test_scan_layout_covers_the_ungrouped_vectorized_scan_only():
    from hyperspace_amd.exec import jit, kernel_config
    p, comp = _q6_params()
    assert kernel_config.KernelConfig().scan_pack is True
    assert jit.scan_pack_layout(p, comp, 8) == (((0, 0, 4), (1, 4, 6), (2, 10, 24)), 36)
    assert jit.scan_pack_layout(p, comp, 0) is None and jit.scan_pack_layout(p, comp, 16) is None
    with kernel_config.use(scan_pack=False):
        assert jit.scan_pack_layout(p, comp, 8) is None
    with kernel_config.use(scan_compact=False):
        assert jit.scan_pack_layout(p, comp, 8) is None
    p.group_col, p.num_groups = 1, 50
    assert jit.scan_pack_layout(p, comp, 8) is None
    p.group_col = -1
    p.cols[2] = _fake(NL.F64, True)
    assert jit.scan_pack_layout(p, comp, 8) is None


def test_off_source_is_the_recorded_parent_source_and_on_source_is_recorded(rt, tmp_path):
    jit = rt
    from hyperspace_amd.exec import kernel_config
    p, comp = _q6_params()
    with kernel_config.use(scan_pack=False):
        off = jit.gen_scan_agg(p, comp, 8, None, jit.scan_pack_layout(p, comp, 8))
    with open(os.path.join(jit.AOT_DIR, "hs_jit_scan_agg.8e8205354881e551.hip")) as fh:
        assert off.src == fh.read()
    lay = jit.scan_pack_layout(p, comp, 8)
    shape_on = jit.scan_agg_shape(p, comp, 8, None, lay)
    on = jit.gen_scan_agg(p, comp, 8, None, lay)
    h = hashlib.sha1(on.src.encode()).hexdigest()[:16]
    with open(os.path.join(jit.AOT_DIR, f"hs_jit_scan_agg.{h}.hip")) as fh:
        assert on.src == fh.read()
    # one stream, no gather: the full tiles read PK only, the list holds 28-bit entries
    assert "pload<9>(a.PK, (g0P >> 3) * 9, pkvP);" in on.src
    assert "typedef unsigned int crow_t; __shared__ crow_t crow_s[4][512];" in on.src
    full = on.src[on.src.index("for (; t < t1 && fullP; ++t)"):on.src.index("for (; t < t1; ++t)")]
    assert "a.c0[" not in full and "a.c1[" not in full and "a.c2[" not in full
    assert [n for _, n, _ in on.args.slots if n.startswith("P")] == ["PK", "PO0", "PO1", "PO2"]
    # a u64 list when the aggregate inputs need more than 32 bits
    comp[0] = _compact(2, 0, 1000, 100.0)
    wide = jit.gen_scan_agg(p, comp, 8, None, jit.scan_pack_layout(p, comp, 8))
    assert "typedef u64 crow_t;" in wide.src
    # the lane-coalesced load shape: the same fields out of an LDS transpose
    with kernel_config.use(scan_pack_lds=True):
        assert jit.scan_agg_shape(p, comp, 8, None, lay) != shape_on
        lds = jit.gen_scan_agg(p, comp, 8, None, jit.scan_pack_layout(p, comp, 8))
    assert "ploadc<10>(a.PK, ((g0P >> 3) - cln) * 10, cln, pkvP);" in lds.src
    assert "hs_pk_t<10>(pks_s[wv], cln, pkv);" in lds.src and "ploadc<" not in wide.src
    for k in (on, wide, lds):
        rc = jit.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                                   str(tmp_path).encode())
        assert rc == 0, jit.runtime().hs_jit_last_error().decode()


# ------------------------------------------------------------------------------------------------
# CPU tier: the numpy reference
# ------------------------------------------------------------------------------------------------
# (column dtypes, offsets, first bits, widths, B): fields that straddle dwords, 1 and 31 bits
LAYOUTS = {
    "B4": ((np.int8, np.int8), (-128, 3), (0, 1), (1, 3), 4),
    "B36": ((np.int8, np.int8, np.int32), (-5, 1, -90000), (0, 4, 10), (4, 6, 24), 36),
    "B64": ((np.int16, np.int32, np.int8, np.int32), (-4000, -(2 ** 30), -128, 7),
            (0, 13, 44, 45), (13, 31, 1, 19), 64),
}


def _codes(name, n, seed=5):
    """Code columns of ``LAYOUTS[name]``: uniform over each field's span, both ends present."""
    dts, offs, _, bits, _ = LAYOUTS[name]
    rng = np.random.default_rng(seed)
    cols = []
    for dt, off, w in zip(dts, offs, bits):
        c = off + rng.integers(0, 1 << w, n, dtype=np.int64)
        if n >= 1:
            c[0] = off + (1 << w) - 1
        if n >= 2:
            c[-1] = off
        assert np.iinfo(dt).min <= c.min() and c.max() <= np.iinfo(dt).max
        cols.append(c.astype(dt))
    return cols


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_reference_round_trip(name):
    _, offs, pos, bits, B = LAYOUTS[name]
    for n in (1, 9, 2049):
        cols = _codes(name, n)
        w = PR.pack(cols, offs, pos, bits, B)
        assert w.dtype == np.uint32 and len(w) == PR.padded_rows(n) // 8 * (B // 4)
        back = PR.unpack(w, n, offs, pos, bits, B)
        for c, b in zip(cols, back):
            assert np.array_equal(c.astype(np.int64), b)
        # padding rows are zero
        assert not w[-(-n // 8) * (B // 4):].any()


def test_reference_bit_positions():
    """Row i starts at bit i * B; a field at its first bit: spelled out for two rows of B = 36."""
    _, offs, pos, bits, B = LAYOUTS["B36"]
    cols = [np.array([-5 + 0xA, -5 + 1], np.int8), np.array([1 + 0x21, 1], np.int8),
            np.array([-90000 + 0xABCDEF, -90000 + 3], np.int32)]
    w = PR.pack(cols, offs, pos, bits, B)
    row0 = 0xA | (0x21 << 4) | (0xABCDEF << 10)
    row1 = 1 | (0 << 4) | (3 << 10)
    stream = row0 | (row1 << 36)
    assert [int(x) for x in w[:3]] == [(stream >> (32 * k)) & 0xFFFFFFFF for k in range(3)]


# ------------------------------------------------------------------------------------------------
# GPU: hs_pack_rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_pack_rows_equals_the_reference(device, name):
    import torch
    from hyperspace_amd.ops import kernels as K
    _, offs, pos, bits, B = LAYOUTS[name]
    for n in (1, 7, 8, 9, 63, 2047, 2048, 2049, 5000):
        cols = _codes(name, n, seed=n)
        want = PR.pack(cols, offs, pos, bits, B)
        dev = [torch.from_numpy(c).to(device) for c in cols]
        got = K.pack_rows(dev, offs, pos, bits, B).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), (name, n)
        # columns whose bases are not vector aligned take the element loads
        if n >= 9:
            dev1 = [torch.from_numpy(np.concatenate([c[:1], c])).to(device)[1:] for c in cols]
            assert all(d.data_ptr() % (8 * d.element_size()) for d in dev1)
            got = K.pack_rows(dev1, offs, pos, bits, B).cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want), (name, n, "unaligned")


# ------------------------------------------------------------------------------------------------
# GPU: packed against unpacked scan
# ------------------------------------------------------------------------------------------------
N = 20011
TILE = 2048
MIXED = [(37, 5000), (5100, 0), (5203, 700), (6001, 2048), (9000, 4103), (15000, N - 15000)]
ONE = [(1003, 9001)]
MANY = [(97 * i + i % 8, 37 + (i * 13) % 60) for i in range(200)]
GRIDS = (1, 3, None)


@functools.lru_cache(maxsize=None)
def _table():
    """name -> (numpy values, validity or None, hs type, device column, compact or None)."""
    import torch
    from hyperspace_amd.exec.encoding import encode
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(77)
    c = {"d": rng.integers(0, 11, N) / 100.0,
         "q": rng.integers(1, 51, N).astype(np.float64),
         "x": np.round(rng.random(N) * 1e5, 2),
         "w": rng.integers(-500_000, 500_001, N),     # (int64: 4-byte codes)
         "s": rng.integers(-3000, 3001, N).astype(np.int32),
         "k": 10 ** 12 + rng.integers(0, 3_000_000_000, N),
         "k2": -(10 ** 9) + rng.integers(0, 4_000_000_000, N),
         "fr": rng.random(N)}
    c["x"][:2] = (0.0, 99999.99)
    valid = {"dn": rng.random(N) >= 0.1}
    c["dn"] = c["d"]
    hs = {v: k for k, v in R.NP_TYPE.items()}
    out = {}
    for name, a in c.items():
        v = valid.get(name)
        col = _col(pa.array(a, mask=None if v is None else ~v), dev)
        out[name] = (a, None if v is None else v.astype(np.uint8), hs[a.dtype.type], col,
                     encode(col))
    return out


def _query(names, preds, aggs):
    """(ScanParams, compacts, reference columns, predicate tuples, aggregate tuples)."""
    t = _table()
    p = _scan_params({s: t[n][3].desc() for s, n in names.items()},
                     [NL.Pred(k, op, c, 0, g, 0, 0, float(lit), None)
                      if k == R.PK_FLT_LIT else NL.Pred(k, op, c, 0, g, 0, int(lit), 0.0, None)
                      for g, (k, op, c, lit) in enumerate(preds)],
                     [_agg(k, terms) for k, terms in aggs])
    comp = {s: t[n][4] for s, n in names.items() if t[n][4] is not None}
    ref_cols = {s: t[n][:3] for s, n in names.items()}
    ref_preds = [(k, op, c, 0, g, int(lit) if k == R.PK_INT_LIT else 0,
                  float(lit) if k == R.PK_FLT_LIT else 0.0, None)
                 for g, (k, op, c, lit) in enumerate(preds)]
    return p, comp, ref_cols, ref_preds, aggs


def _run(p, comp, ranges, grid, pack):
    import torch
    from hyperspace_amd.exec import jit, kernel_config
    dev = torch.device("cuda:0")
    rs = torch.tensor([s for s, _ in ranges], dtype=torch.int64, device=dev)
    rl = torch.tensor([n for _, n in ranges], dtype=torch.int64, device=dev)
    over = {"scan_grid": grid} if grid else {}
    with kernel_config.use(scan_pack=pack, **over):
        assert jit.scan_vec(p, comp, N) == 8
        parts = []
        out = jit.scan_agg(p, rs, rl, None, comp, N, parts_out=parts)
        return ([x.cpu().numpy() for x in out], [x.cpu().numpy() for x in parts],
                jit.scan_pack_layout(p, comp, 8))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check(q, ranges, grids=GRIDS, packed=True):
    """Packed and unpacked partials agree exactly; the result agrees with the reference."""
    p, comp, ref_cols, ref_preds, aggs = q
    ref = R.scan(ref_cols, ref_preds, aggs, ranges=ranges)
    for g in grids:
        on, pon, lay = _run(p, comp, ranges, g, True)
        off, poff, none = _run(p, comp, ranges, g, False)
        assert none is None and (lay is not None) == packed, (lay, packed)
        for a, b in zip(pon, poff):           # psum, pcnt, pmin, pmax of every block
            assert np.array_equal(_bits(a), _bits(b)), (g, a[:8], b[:8])
        for a, b in zip(on, off):
            assert np.array_equal(_bits(a), _bits(b))
        s, c, mn, mx = on
        for i, (kind, terms) in enumerate(aggs):
            assert c[i] == ref.count[0, i], (g, i, c[i], ref.count[0, i])
            if kind == R.AK_SUM:
                bound = (ref.count[0, i] + 4 * len(terms) + 2) * 2.0 ** -52 * ref.abs_sum[0, i]
                assert abs(s[i] - ref.sum[0, i]) <= bound, (g, i, s[i], ref.sum[0, i], bound)
            elif kind == R.AK_MAX:
                assert mx[i] == ref.mx[0, i]
            elif kind == R.AK_MIN:
                assert mn[i] == ref.mn[0, i]
    return ref, lay


def _q6(lo=0.05, hi=0.07, qty=24.0):
    return _query({0: "d", 1: "q", 2: "x"},
                  [(R.PK_FLT_LIT, R.OP_GE, 0, lo), (R.PK_FLT_LIT, R.OP_LE, 0, hi),
                   (R.PK_FLT_LIT, R.OP_LT, 1, qty)],
                  [(R.AK_SUM, [(2, 0.0, 1.0), (0, 0.0, 1.0)]), (R.AK_COUNT_STAR, []),
                   (R.AK_MAX, [(2, 0.0, 1.0)]), (R.AK_MIN, [(2, 0.0, 1.0)])])


@pytest.mark.gpu
@pytest.mark.parametrize("ranges", [MIXED, ONE, MANY], ids=["mixed", "R1", "R200"])
def test_packed_scan_equals_unpacked_and_reference(device, ranges):
    ref, lay = _check(_q6(), ranges)
    assert lay == (((0, 0, 4), (1, 4, 6), (2, 10, 24)), 36)
    assert 0 < ref.count[0, 1] < sum(n for _, n in ranges)
    if ranges is MIXED:     # the last range's third tile (from row 19096) is the partial one
        assert (ref.rows >= 19096).any() and (ref.rows < 19096).any()


@pytest.mark.gpu
@pytest.mark.parametrize("ranges", [[(5100, 0)], [(8, 16)], [(4099, 5)], [(N - 3, 3)],
                                    [(N - N % TILE - 5, N % TILE + 5)]],
                         ids=["empty", "aligned", "short", "tail", "into-partial"])
def test_packed_scan_small_ranges(device, ranges):
    _check(_q6(0.0, 0.1, 100.0), ranges, grids=(None,))


@pytest.mark.gpu
def test_no_row_and_every_row_of_a_tile_pass(device):
    ref, _ = _check(_q6(0.5, 0.9, 24.0), MIXED, grids=(3,))
    assert ref.count[0, 1] == 0
    # every row passes: 512 list entries per wavefront in each full tile
    ref, _ = _check(_q6(0.0, 0.1, 100.0), MIXED, grids=(3,))
    assert ref.count[0, 1] == sum(n for _, n in MIXED)


@pytest.mark.gpu
def test_u64_list_entries(device):
    """SUM(x * w): 24 + 20 bits of aggregate inputs per passing row."""
    q = _query({0: "d", 1: "x", 2: "w"}, [(R.PK_FLT_LIT, R.OP_GE, 0, 0.03)],
               [(R.AK_SUM, [(1, 0.0, 1.0), (2, 0.0, 1.0)]), (R.AK_COUNT_STAR, [])])
    ref, lay = _check(q, MIXED, grids=(3, None))
    assert lay == (((0, 0, 4), (1, 4, 24), (2, 28, 20)), 48) and ref.count[0, 1] > 0


@pytest.mark.gpu
def test_lane_coalesced_load_shape(device):
    """``scan_pack_lds``: an odd and an even number of dwords per lane."""
    from hyperspace_amd.exec import kernel_config
    q = _query({0: "d", 1: "x", 2: "w"}, [(R.PK_FLT_LIT, R.OP_GE, 0, 0.03)],
               [(R.AK_SUM, [(1, 0.0, 1.0), (2, 0.0, 1.0)]), (R.AK_COUNT_STAR, [])])
    with kernel_config.use(scan_pack_lds=True):
        _check(_q6(), MIXED, grids=(3, None))
        _check(q, MIXED, grids=(3,))


@pytest.mark.gpu
def test_aggregate_inputs_among_the_predicate_columns(device):
    """No list at all: SUM(s * d) with both columns under predicates."""
    q = _query({0: "s", 1: "d"}, [(R.PK_INT_LIT, R.OP_GT, 0, -1000), (R.PK_FLT_LIT, R.OP_NE, 1, 0.04)],
               [(R.AK_SUM, [(0, 1.0, 2.0), (1, 0.0, 1.0)]), (R.AK_COUNT_STAR, [])])
    ref, lay = _check(q, MIXED, grids=(3, None))
    assert lay == (((0, 0, 13), (1, 13, 4)), 20) and ref.count[0, 1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("names", [{0: "dn", 1: "q", 2: "x"}, {0: "d", 1: "fr", 2: "x"},
                                   {0: "k", 1: "k2", 2: "x"}],
                         ids=["nullable", "float", "B>64"])
def test_shapes_without_a_layout_run_the_unpacked_kernel(device, names):
    leaf = {"dn": (R.PK_FLT_LIT, 0.05), "d": (R.PK_FLT_LIT, 0.05), "k": (R.PK_INT_LIT, 10 ** 12 + 10 ** 9),
            "q": (R.PK_FLT_LIT, 24.0), "fr": (R.PK_FLT_LIT, 0.5), "k2": (R.PK_INT_LIT, 10 ** 9)}
    q = _query(names, [(leaf[names[0]][0], R.OP_GE, 0, leaf[names[0]][1]),
                       (leaf[names[1]][0], R.OP_LT, 1, leaf[names[1]][1])],
               [(R.AK_SUM, [(2, 0.0, 1.0)]), (R.AK_COUNT_STAR, [])])
    ref, lay = _check(q, MIXED, grids=(None,), packed=False)
    assert lay is None and ref.count[0, 1] > 0


# ------------------------------------------------------------------------------------------------
# GPU: through the engine (captured scan pipeline)
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_engine_scan_pipeline_reads_the_pack(device, tmp_path):
    import pyarrow.parquet as pq
    from hyperspace_amd import Hyperspace, IndexConfig, Session, col, sum_
    from hyperspace_amd.exec import graphs
    rng = np.random.default_rng(3)
    n = 30_000
    os.makedirs(tmp_path / "li")
    pq.write_table(pa.table({"l_ship": rng.integers(8000, 10500, n).astype(np.int32),
                             "l_price": np.round(rng.random(n) * 1e5, 2),
                             "l_disc": rng.integers(0, 11, n) / 100.0,
                             "l_qty": rng.integers(1, 51, n).astype(np.float64)}),
                   tmp_path / "li" / "part-0.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.numBuckets": "4",
                      "spark.hyperspace.mi.execution.device": "gpu"})
    hs = Hyperspace(s)
    li = s.read.parquet(str(tmp_path / "li"))
    hs.createIndex(li, IndexConfig("li_ship", ["l_ship"], ["l_disc", "l_qty", "l_price"]))
    Hyperspace.enable(s)

    def q(lo, hi, disc, qty):
        return li.filter((col("l_ship") >= lo) & (col("l_ship") < hi) & (col("l_disc") >= disc) &
                         (col("l_qty") < qty)).agg(sum_(col("l_price") * col("l_disc")))

    lits = [(9000, 9365, 0.05, 24), (8100, 10400, 0.02, 40), (9000, 9001, 0.0, 51)]
    be = s.backend()
    got = []
    for x in lits:
        got.append(q(*x).collect()[0][0])
        assert be.last_path == "native", be.fallback_reason
    prep = be._last_graph_prep
    assert prep.pack is not None and "PK" in prep.values and "pload<" in prep.k.src
    assert prep.g.replays >= 1
    counts = [graphs.node_counts(sl.graph) for sl in prep.g.slots if sl.graph is not None]
    assert counts and set(counts) == {(4, 0, 0)}
    s.conf.set("spark.hyperspace.mi.execution.device", "cpu")
    for x, r in zip(lits, got):
        e = q(*x).collect()[0][0]
        assert abs(r - e) <= 1e-9 * abs(e), (x, r, e)
