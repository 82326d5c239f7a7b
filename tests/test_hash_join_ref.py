"""The numpy reference the hash-join kernel tests compare with (tests/hash_join_ref.py), checked
where there is no GPU: against ``pyarrow.Table.join`` on every case and probe size of the GPU
tests (the same set of (stream row, build row) pairs - Arrow does not promise an order), and
against two plain Python loops for the order, the -1 padding and the NULL rules."""
import numpy as np
import pyarrow as pa
import pytest

import hash_join_ref as R


def _arrow_pairs(case, skeys, svalid, rows, how):
    bk = pa.array(case.bkeys.astype(np.int64),
                  mask=None if case.bvalid is None else case.bvalid == 0)
    ids = np.arange(len(skeys), dtype=np.int64) if rows is None else rows
    sk = pa.array(skeys.astype(np.int64)[ids],
                  mask=None if svalid is None else svalid[ids] == 0)
    st = pa.table({"k": sk, "sid": ids})
    bt = pa.table({"k": bk, "bid": np.arange(len(case.bkeys), dtype=np.int64)})
    jt = {"pairs": "inner", "preserve": "left outer", "mark": "left semi"}[how]
    j = st.join(bt, "k", join_type=jt, use_threads=False)
    if how == "mark":
        mark = np.zeros(len(skeys), np.uint8)
        mark[j.column("sid").to_numpy()] = 1
        return mark[ids]
    bid = j.column("bid").fill_null(-1).to_numpy()
    return sorted(zip(j.column("sid").to_numpy().tolist(), bid.tolist()))


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_reference_matches_arrow_join(name):
    case = R.cases()[name]
    table = R.ref_build(case.bkeys, case.bvalid)
    sizes = R.PROBE_SIZES + ((300,) if name == "same1000" else ())
    for n in sizes:
        skeys, svalid = case.stream(n)
        for rows in (None, R.row_list(n, n // 2 + (n > 0))):
            for how in R.MODES:
                got = R.ref_probe(table, skeys, svalid, rows, how)
                want = _arrow_pairs(case, skeys, svalid, rows, how)
                if how == "mark":
                    assert np.array_equal(got, want), (name, n, how)
                else:
                    assert sorted(zip(got[0].tolist(), got[1].tolist())) == want, (name, n, how)


@pytest.mark.parametrize("name", ["mixed65", "nulls", "special_present", "special_absent",
                                  "unique2", "unique0", "collisions", "width_int8_int64"])
def test_reference_order_and_padding(name):
    case = R.cases()[name]
    table = R.ref_build(case.bkeys, case.bvalid)
    for n in (0, 1, 97):
        skeys, svalid = case.stream(n)
        for rows in (None, R.row_list(n, n // 2)):
            for how in R.MODES:
                got = R.ref_probe(table, skeys, svalid, rows, how)
                want = R.brute_probe(case.bkeys, case.bvalid, skeys, svalid, rows, how)
                if how == "mark":
                    assert np.array_equal(got, want)
                else:
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_reference_build_contract():
    for name, case in R.cases().items():
        t = R.ref_build(case.bkeys, case.bvalid)
        ok = np.ones(len(case.bkeys), bool) if case.bvalid is None else case.bvalid != 0
        assert sorted(t["perm"].tolist()) == np.nonzero(ok)[0].tolist(), name
        k = case.bkeys.astype(np.int64)[t["perm"]]
        assert np.all(k[1:] >= k[:-1]), name
        same = k[1:] == k[:-1]
        assert np.all(t["perm"][1:][same] > t["perm"][:-1][same]), name     # stable
        assert t["unique"] == (len(set(k.tolist())) == len(k)), name
        assert t["slots"] >= max(64, 2 * t["nkeys"]) and t["slots"] & (t["slots"] - 1) == 0
    # a row-id list restricts the build side
    case = R.cases()["mixed65"]
    rows = R.row_list(65, 20)
    t = R.ref_build(case.bkeys, None, rows)
    assert sorted(t["perm"].tolist()) == rows.tolist()


def test_collision_set_shares_a_home_slot_and_wraps():
    case = R.cases()["collisions"]
    slots = R.ref_slots(len(case.bkeys))
    home = R.mix64(case.bkeys) & np.uint64(slots - 1)
    assert int((home == slots - 3).sum()) >= 40          # the cluster passes slot 127 -> 0
    absent = np.setdiff1d(case.pool, case.bkeys)
    assert int(((R.mix64(absent) & np.uint64(slots - 1)) == slots - 3).sum()) >= 10
    # mix64 as the device computes it: two values worked out by hand from the definition
    assert int(R.mix64(np.array([0]))[0]) == 0
    h = 1
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) % (1 << 64)
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) % (1 << 64)
    h ^= h >> 33
    assert int(R.mix64(np.array([1]))[0]) == h
