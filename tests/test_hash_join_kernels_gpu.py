"""The hash-join kernels (csrc/kernels/hash_join.hip: hs_hj_build, hs_hj_probe, hs_hj_emit) through
``K.hash_join_table`` / ``K.hash_join_probe`` against the numpy reference of
tests/hash_join_ref.py (itself checked against ``pyarrow.Table.join`` in test_hash_join_ref.py):
exactly the same ids in the same order, for every build size, probe size around the block and
tile sizes, with and without a row-id list, in all three modes."""
import numpy as np
import pyarrow as pa
import pytest

import hash_join_ref as R

gpu = pytest.mark.gpu


def _col(values, valid, device):
    import torch
    from hyperspace_amd.exec.device_table import DeviceColumn
    a = np.ascontiguousarray(values)
    data = torch.from_numpy(a.copy()).to(device)
    v = torch.from_numpy(np.ascontiguousarray(valid).copy()).to(device) \
        if valid is not None else None
    return DeviceColumn(data, v, pa.from_numpy_dtype(a.dtype))


def _rows(rows, device):
    import torch
    return torch.from_numpy(rows.copy()).to(device) if rows is not None else None


def _check_table(table, ref):
    assert table.nbuild == ref["nbuild"]
    assert table.nkeys == ref["nkeys"]
    assert table.unique == ref["unique"]
    assert table.slots == ref["slots"]
    assert np.array_equal(table.perm.cpu().numpy().astype(np.int64), ref["perm"])
    assert table.keys.numel() == table.slots + 2
    assert table.first.numel() == table.slots + 2 and table.last.numel() == table.slots + 2


def _check_probe(K, table, ref, scol, skeys, svalid, rows, device, how, **kw):
    got = K.hash_join_probe(table, scol, _rows(rows, device), how=how, **kw)
    want = R.ref_probe(ref, skeys, svalid, rows, how)
    if how == "mark":
        assert str(got.dtype) == "torch.uint8"
        assert np.array_equal(got.cpu().numpy(), want), how
        return
    sid, bid = (x.cpu().numpy() for x in got)
    assert sid.dtype == np.int64 and bid.dtype == np.int64
    assert np.array_equal(sid, want[0]), how
    assert np.array_equal(bid, want[1]), how


@gpu
def test_rows_per_lane_is_what_the_probe_sizes_assume(device):
    from hyperspace_amd.ops import _lib as NL
    assert NL.lib().hs_hj_rows_per_lane() == R.ROWS_PER_LANE


@gpu
@pytest.mark.parametrize("name", sorted(R.cases()))
def test_build_and_probe_match_reference(name, device):
    from hyperspace_amd.ops import kernels as K
    case = R.cases()[name]
    table = K.hash_join_table(_col(case.bkeys, case.bvalid, device))
    ref = R.ref_build(case.bkeys, case.bvalid)
    _check_table(table, ref)
    sizes = R.PROBE_SIZES + ((300,) if name == "same1000" else ())
    for n in sizes:
        skeys, svalid = case.stream(n)
        scol = _col(skeys, svalid, device)
        for rows in (None, R.row_list(n, n // 2 + (n > 0))):
            for how in R.MODES:
                _check_probe(K, table, ref, scol, skeys, svalid, rows, device, how)


@gpu
def test_build_over_a_row_id_list(device):
    from hyperspace_amd.ops import kernels as K
    for name in ("mixed1000", "nulls", "unique65"):
        case = R.cases()[name]
        nb = len(case.bkeys)
        rows = R.row_list(nb, nb // 3)
        table = K.hash_join_table(_col(case.bkeys, case.bvalid, device), _rows(rows, device))
        ref = R.ref_build(case.bkeys, case.bvalid, rows)
        _check_table(table, ref)
        skeys, svalid = case.stream(R.TILE + 1)
        scol = _col(skeys, svalid, device)
        for how in R.MODES:
            _check_probe(K, table, ref, scol, skeys, svalid, None, device, how)


@gpu
@pytest.mark.parametrize("rpl", [1, 2, 4, 8])
def test_every_rows_per_lane_variant_gives_the_same_rows(rpl, device):
    from hyperspace_amd.ops import kernels as K
    for name in ("mixed1000", "collisions", "special_present", "nulls"):
        case = R.cases()[name]
        table = K.hash_join_table(_col(case.bkeys, case.bvalid, device))
        ref = R.ref_build(case.bkeys, case.bvalid)
        for n in (256 * rpl - 1, 256 * rpl, 256 * rpl + 1, 3 * 256 * rpl + 5):
            skeys, svalid = case.stream(n)
            scol = _col(skeys, svalid, device)
            for how in R.MODES:
                _check_probe(K, table, ref, scol, skeys, svalid, None, device, how,
                             rows_per_lane=rpl)


@gpu
def test_output_is_reproducible(device):
    from hyperspace_amd.ops import kernels as K
    case = R.cases()["mixed1000"]
    skeys, _ = case.stream(3 * R.TILE + 5)
    scol = _col(skeys, None, device)
    outs = []
    for _ in range(2):
        table = K.hash_join_table(_col(case.bkeys, None, device))
        sid, bid = K.hash_join_probe(table, scol, how="preserve")
        outs.append((sid.cpu().numpy(), bid.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@gpu
def test_float_and_unsigned_64_bit_keys_are_refused(device):
    from hyperspace_amd.ops import kernels as K
    with pytest.raises(ValueError):
        K.hash_join_table(_col(np.zeros(4, np.float64), None, device))
    with pytest.raises(ValueError):
        K.hash_join_table(_col(np.zeros(4, np.uint64), None, device))
    table = K.hash_join_table(_col(np.arange(4, dtype=np.int64), None, device))
    with pytest.raises(ValueError):
        K.hash_join_probe(table, _col(np.zeros(4, np.float32), None, device))
    with pytest.raises(ValueError):
        K.hash_join_probe(table, _col(np.zeros(4, np.int64), None, device), how="full")
