"""``HashJoinOps._local_table_rel`` (the device relation of a ``createDataFrame`` table) on the
CPU: columns of types the device does not hold are left out instead of failing the upload, and
reading one is ``Unsupported`` - which the executor turns into a host run - never another
exception."""
import numpy as np
import pyarrow as pa
import pytest
import torch

from hyperspace_amd.exec.gpu_common import Unsupported
from hyperspace_amd.exec.gpu_hash_join import HashJoinOps, _device_type
from hyperspace_amd.plan import physical as X


class _Backend(HashJoinOps):
    device = torch.device("cpu")

    def __init__(self, world=1):
        self.world = world

    def _dist(self):
        if self.world == 1:
            return None
        return type("D", (), {"world": self.world, "rank": 0})()


def _scan(session, table):
    plan = session.createDataFrame(table).queryExecution.executed_plan
    nodes = plan.collect(lambda x: isinstance(x, X.LocalTableScanExec))
    assert len(nodes) == 1
    return nodes[0]


ODD = pa.table({
    "k": pa.array([1, 2, None, 4], pa.int32()),
    "tags": pa.array([[1], [], None, [2, 3]], pa.list_(pa.int64())),
    "raw": pa.array([b"a", b"", None, b"zz"], pa.binary()),
    "st": pa.array([{"x": 1}, {"x": 2}, None, {"x": 4}], pa.struct([("x", pa.int64())])),
    "nothing": pa.nulls(4),
    "half": pa.array(np.arange(4, dtype=np.float16)),
    "t": pa.array([1, 2, 3, 4], pa.time64("us")),
    "s": pa.array(["b", None, "a", "b"]),
    "d": pa.array([1, 2, 3, None], pa.date32()),
    "ts": pa.array([1, 2, 3, 4], pa.timestamp("us")),
    "b": pa.array([True, False, None, True]),
    "f": pa.array([0.5, 1.5, 2.5, 3.5]),
    "dec": pa.array([1, 2, 3, 4], pa.int32()).cast(pa.decimal128(12, 2)),
})
HELD = ("k", "s", "d", "ts", "b", "f", "dec")


def test_unsupported_column_types_are_left_out_not_raised(session):
    p = _scan(session, ODD)
    r = _Backend()._local_table_rel(p)
    by_name = {a.name: a for a in p.output}
    assert r.table.num_rows == 4
    assert list(r.table.bucket_offsets_host) == [0, 4]
    for name in HELD:
        c = r.col(by_name[name])
        assert len(c) == 4 and c.hs_transient
        assert c.to_arrow().to_pylist() == ODD.column(name).to_pylist(), name
    assert len(r.table.columns) == len(HELD)
    for name in set(ODD.column_names) - set(HELD):
        with pytest.raises(Unsupported, match=f"createDataFrame column {name} of type"):
            r.col(by_name[name])
    assert getattr(r.table, "_hs_cache_key", None) is None


def test_device_type_agrees_with_the_upload():
    for name in ODD.column_names:
        assert _device_type(ODD.column(name).type) == (name in HELD), name


def test_empty_table_and_several_ranks(session):
    p = _scan(session, pa.table({"k": pa.array([], pa.int64()),
                                 "l": pa.array([], pa.list_(pa.int8()))}))
    r = _Backend()._local_table_rel(p)
    assert r.table.num_rows == 0 and len(r.col(p.output[0])) == 0
    with pytest.raises(Unsupported, match="more than one rank"):
        _Backend(world=2)._local_table_rel(p)
