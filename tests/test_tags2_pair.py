"""The pair form of merge-join phase 1 (exec/jit_runs.py ``rt2_pair``, exec/pairing.py): one pass
over the keys, the right predicate column and the run bounds tags two in-flight queries of one
shape, each with its own literal slots and bitmap.

CPU tier: which lowerings get the form, its source compiles for gfx950, and the hold / release
rules of ``pairing.PairGate`` driven by a fake launcher with fake events.  GPU tier, kernel
level: one pair launch equals two single launches on both bitmaps (``torch.equal``) and in both
results, over run counts 1 / 255 / 256 / 257 / ~3000, literal sets identical / nested / disjoint /
none-beside-all, with and without the prune bound, and inputs that force the 64-run fall-back (a
wide key group on either side, left keys without a right row, a guess that leaves the bucket).
GPU tier, end to end: interleaved asynchronous join and filter queries equal one-by-one
``collect()`` exactly, with the expected split of pairs and singles.
"""
import datetime
import functools
import os

import numpy as np
import pyarrow as pa
import pytest

from hyperspace_amd.exec.pairing import HeldQuery, PairGate
from hyperspace_amd.ops import _lib as NL
from test_jit import _col, _q3_params, rt  # noqa: F401
from test_run_prune import _params
from test_tags2_keys16 import _k16_compacts


# ------------------------------------------------------------------------------------------------
# CPU tier: the form and its source
# ------------------------------------------------------------------------------------------------
def test_lowering_selects_the_pair_form():
    from hyperspace_amd.exec import jit_runs, kernel_config
    p, c = _q3_params(), _k16_compacts()
    pr = jit_runs.prune_plan(p, c, 1)
    assert pr
    with kernel_config.use(rt2_k16=True, rt2_pair=True):
        assert jit_runs.tags2_pair(p, c, 1, True, "", True)
        for q in ((), pr):
            one = jit_runs.gen_run_tags2(p, c, 1, True, "", q, True)
            two = jit_runs.gen_run_tags2(p, c, 1, True, "", q, True, True)
            assert jit_runs.tags2_shape(p, c, 1, True, "", q, True, True) != \
                jit_runs.tags2_shape(p, c, 1, True, "", q, True)
            assert "tags_b" not in one.src and "_b;" not in one.src
            # both paths store both bitmaps: the 256-run stages and the 64-run fall-back
            assert two.src.count("a.tags_b[(nb + ") == two.src.count("a.tags[(nb + ") > 0
            assert two.src.count("a.tags_b[((gi + ") == two.src.count("a.tags[((gi + ") > 0
            # the second literal set: the right predicate's bounds and the prune bound
            names = [n for _, n, _ in two.args.slots]
            assert "CL1_b" in names and "CH1_b" in names and ("CL0_b" in names) == bool(q)
            assert [n for n in names if not n.endswith("_b")] == [n for _, n, _ in one.args.slots]
            # the keys are loaded once
            assert two.src.count("(a.LO16 +") == one.src.count("(a.LO16 +")
        # not covered: the 32-bit form, wider tags, the recording / recorded forms, one run
        assert not jit_runs.tags2_pair(p, c, 1, True, "", False)
        assert not jit_runs.tags2_pair(p, c, 2, True, "", True)
        for mode in ("rec", "match", "copy"):
            assert not jit_runs.tags2_pair(p, c, 1, True, mode, True)
        assert not jit_runs.tags2_pair(p, c, 1, False, "", True)
        with kernel_config.use(rt2_wide=1):
            assert not jit_runs.tags2_pair(p, c, 1, True, "", True)
        assert jit_runs.tags2_shape(p, c, 2, True, "", (), True, True) == \
            jit_runs.tags2_shape(p, c, 2, True, "", (), True)
    with kernel_config.use(rt2_k16=True, rt2_pair=False):
        assert not jit_runs.tags2_pair(p, c, 1, True, "", True)
        assert jit_runs.tags2_shape(p, c, 1, True, "", pr, True, True) == \
            jit_runs.tags2_shape(p, c, 1, True, "", pr, True)
    with kernel_config.use(rt2_k16=False, rt2_pair=True):
        assert not jit_runs.tags2_pair(p, c, 1, True, "", True)


def test_pair_sources_compile(rt, tmp_path):  # noqa: F811
    from hyperspace_amd.exec import jit_runs, kernel_config
    p, c = _q3_params(), _k16_compacts()
    with kernel_config.use(rt2_k16=True, rt2_pair=True):
        ks = [jit_runs.gen_run_tags2(p, c, 1, True, "", q, True, True)
              for q in ((), jit_runs.prune_plan(p, c, 1))]
        with kernel_config.use(rt2_unroll=1):
            ks.append(jit_runs.gen_run_tags2(p, c, 1, True, "", (), True, True))
    assert len({k.src for k in ks}) == 3
    for k in ks:
        rc = rt.runtime().hs_jit_compile_to_cache(k.src.encode(), k.name.encode(), b"gfx950",
                                                  str(tmp_path).encode())
        assert rc == 0, rt.runtime().hs_jit_last_error().decode()


# ------------------------------------------------------------------------------------------------
# CPU tier: hold / release
# ------------------------------------------------------------------------------------------------
class _FakePending:
    def __init__(self, log, what):
        self.log, self.what = log, what

    def result(self):
        return self.what

    def done(self):
        return True


class _FakeLauncher:
    """``busy_for``: how many more ``busy()`` calls report the latest launch unfinished after
    it was made (the fake completion event); None: never finishes by itself."""

    def __init__(self, log, name="L", pairs=True, busy_for=None):
        self.log, self.name, self.pairs, self.busy_for = log, name, pairs, busy_for
        self.held = None
        self.match = None
        self.running = False
        self.left = 0

    def supports_pair(self):
        return self.pairs and self.match is None

    def busy(self):
        if self.running and self.busy_for is not None:
            self.left -= 1
            if self.left < 0:
                self.running = False
        return self.running

    def finish(self):
        self.running = False

    def _started(self):
        self.running, self.left = True, self.busy_for or 0

    def launch(self, p, key=None, graph=False):
        if self.held is not None:       # as TwoPhaseLauncher.launch: submission order
            self.held.release()
        self.log.append((self.name, "single", key))
        self._started()
        return _FakePending(self.log, key)

    def launch_pair(self, pa_, ka, pb, kb):
        assert self.held is None
        self.log.append((self.name, "pair", ka, kb))
        self._started()
        return _FakePending(self.log, ka), _FakePending(self.log, kb)


EPOCH = [0]       # the fake device cache's epoch


def _new_gate(metrics=None):
    EPOCH[0] = 0
    return PairGate(metrics, lambda: EPOCH[0])


def _gate():
    log = []
    return _new_gate(), _FakeLauncher(log), log


def test_gate_pairs_behind_a_busy_predecessor():
    g, lz, log = _gate()
    a = g.submit(lz, "p", 1, True)              # nothing in flight: launched at once
    assert not isinstance(a, HeldQuery) and log == [("L", "single", 1)]
    b = g.submit(lz, "p", 2, True)              # predecessor busy: held
    assert isinstance(b, HeldQuery) and lz.held is b and g.held == [b] and len(log) == 1
    c = g.submit(lz, "p", 3, True)              # its partner
    assert log[-1] == ("L", "pair", 2, 3) and lz.held is None and not g.held
    assert b.result() == 2 and c.result() == 3 and len(log) == 2
    d = g.submit(lz, "p", 4, True)
    e = g.submit(lz, "p", 5, True)
    assert isinstance(d, HeldQuery) and log[-1] == ("L", "pair", 4, 5) and e.result() == 5
    assert (g.pairs, g.singles) == (2, 1)
    # order per launcher: 1, (2, 3), (4, 5)
    assert [x[2:] for x in log] == [(1,), (2, 3), (4, 5)]


def test_gate_never_holds_when_it_may_not():
    # not through the async path / conf off / several ranks (``hold`` false), a launcher
    # without the pair form, one that may still record its match, and an idle device
    for kw, hold in (({}, False), ({"pairs": False}, True)):
        log = []
        g, lz = _new_gate(), _FakeLauncher(log, **kw)
        for k in range(4):
            assert not isinstance(g.submit(lz, "p", k, hold), HeldQuery)
        assert [x[1] for x in log] == ["single"] * 4 and (g.pairs, g.singles) == (0, 4)
    g, lz, log = _gate()
    lz.match = (1, 2, 3)
    for k in range(3):
        assert not isinstance(g.submit(lz, "p", k, True), HeldQuery)
    g, lz, log = _gate()
    for k in range(3):                          # an ``--inflight 1`` loop: each finished first
        out = g.submit(lz, "p", k, True)
        assert not isinstance(out, HeldQuery)
        lz.finish()
    assert (g.pairs, g.singles) == (0, 3)


def test_gate_releases_on_its_own_wait():
    for wait in ("result", "done"):
        g, lz, log = _gate()
        g.submit(lz, "p", 1, True)
        h = g.submit(lz, "p", 2, True)
        assert isinstance(h, HeldQuery) and len(log) == 1
        assert getattr(h, wait)() in (2, True)
        assert log[-1] == ("L", "single", 2) and lz.held is None and not g.held
        assert (g.pairs, g.singles) == (0, 2)
        assert h.result() == 2 and h.done() and len(log) == 2      # launched once
    # polling done() ends
    g, lz, log = _gate()
    g.submit(lz, "p", 1, True)
    h = g.submit(lz, "p", 2, True)
    n = 0
    while not h.done():
        n += 1
        assert n < 10
    assert log[-1] == ("L", "single", 2)


def test_gate_releases_when_the_predecessor_has_finished():
    g, lz, log = _gate()
    g.submit(lz, "p", 1, True)
    h = g.submit(lz, "p", 2, True)
    g.poll()                                    # an engine entry, predecessor still running
    assert h.pending is None and g.held == [h]
    lz.finish()
    g.poll()                                    # ... finished: the device would idle
    assert log[-1] == ("L", "single", 2) and not g.held and h.result() == 2
    # the fake event completing by itself between two entries
    log = []
    g, lz = _new_gate(), _FakeLauncher(log, busy_for=2)
    g.submit(lz, "p", 1, True)
    h = g.submit(lz, "p", 2, True)              # busy() call 1
    g.poll()                                    # call 2: still busy
    assert h.pending is None
    g.poll()                                    # call 3: finished
    assert h.pending is not None and log[-1] == ("L", "single", 2)


def test_gate_another_shape_does_not_release():
    log = []
    g, q3, q3b = _new_gate(), _FakeLauncher(log, "A"), _FakeLauncher(log, "B")
    g.submit(q3, "p", 1, True)
    h = g.submit(q3, "p", 2, True)
    g.poll()                                    # the filter query between two joins
    g.submit(q3b, "p", 7, True)                 # another launcher
    hb = g.submit(q3b, "p", 8, True)
    assert h.pending is None and isinstance(hb, HeldQuery) and g.held == [h, hb]
    g.submit(q3, "p", 3, True)
    assert log[-1] == ("A", "pair", 2, 3) and g.held == [hb]
    assert hb.result() == 8 and not g.held


def test_gate_keeps_submission_order_and_one_held():
    g, lz, log = _gate()
    g.submit(lz, "p", 1, True)
    h = g.submit(lz, "p", 2, True)
    out = g.submit(lz, "p", 3, False)           # a synchronous collect of the same shape
    assert not isinstance(out, HeldQuery) and h.pending is not None
    assert [x[1:] for x in log] == [("single", 1), ("single", 2), ("single", 3)]
    # a direct launch (the planning path) flushes first as well
    h = g.submit(lz, "p", 4, True)
    assert isinstance(h, HeldQuery)
    lz.launch("p", 5)
    assert [x[2] for x in log[-2:]] == [4, 5] and not g.held and lz.held is None
    # never two held on one launcher
    for k in range(6, 20):
        g.submit(lz, "p", k, True)
        assert len(g.held) <= 1 and (lz.held is None) == (not g.held)
    g.release_all()
    keys = [k for x in log for k in x[2:]]
    assert keys == sorted(keys) and keys == list(range(1, 20))      # nothing lost, in order


def test_gate_flushes_before_invalidation():
    # release_all: a synchronous collect, a stale prep, a program that returns to the planning
    # path, released device memory; an epoch change found at the next engine entry
    metrics = {}
    log = []
    g, lz = _new_gate(metrics), _FakeLauncher(log)
    g.submit(lz, "p", 1, True)
    h = g.submit(lz, "p", 2, True)
    g.release_all()
    assert h.pending is not None and not g.held and log[-1] == ("L", "single", 2)
    h = g.submit(lz, "p", 3, True)
    assert isinstance(h, HeldQuery)
    g.poll()
    assert h.pending is None
    EPOCH[0] = 1                                # the device cache evicted something
    g.poll()
    assert h.pending is not None and not g.held
    assert metrics == {"join_pairs": 0, "join_singles": 3}


def _recording_launcher(monkeypatch, log):
    """A real ``TwoPhaseLauncher`` whose device work is faked: ``_record`` and ``supports_pair``
    are the launcher's own; its launches only log, and its launches never finish."""
    import torch
    from hyperspace_amd.exec import device_cache, jit_runs

    class _M:       # the match record
        def data_ptr(self):
            return 64

    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (1 << 40, 1 << 40))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda dev=None: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda dev=None: 0)
    monkeypatch.setattr(jit_runs, "RT2_COPY", False)
    monkeypatch.setattr(jit_runs, "record_matches", lambda *a: log.append("record") or _M())
    monkeypatch.setattr(jit_runs, "tags2_shape", lambda *a: ("shape",) + a[3:])
    monkeypatch.setattr(jit_runs.J, "kernel_for", lambda shape, make: ("kernel",) + shape)
    monkeypatch.setattr(device_cache, "track_derived", lambda t: None)

    class _Lz(jit_runs.TwoPhaseLauncher):
        def busy(self):
            return self.launches > 0

        def launch(self, p, key=None, graph=False):
            if self.held is not None:
                self.held.release()
            self.launches += 1
            if self.match is not None and self.launches == 2:
                self._record()
            log.append(("single", key))
            return _FakePending(log, key)

        def launch_pair(self, pa_, ka, pb, kb):
            assert self.supports_pair()
            log.append(("pair", ka, kb))
            return _FakePending(log, ka), _FakePending(log, kb)

    return _Lz("kt", "ks", 1, 1, 1, 0, {}, {}, {}, (), None, None)


def test_a_launcher_that_recorded_never_holds_or_pairs(monkeypatch):
    """The recorded-match and copy forms keep the single kernel: a launcher holds nothing while
    its switch is pending, flushes before it switches and has no pair form afterwards - also
    one that had the pair kernel before."""
    log = []
    lz = _recording_launcher(monkeypatch, log)
    g = _new_gate()
    lz.ktp = "pair kernel"
    lz.tags_b, lz.tplp = "bitmap", b"blk"
    lz.pblocks[(1, 2)] = "block"
    lz.match = (1, 100, "params")           # the switch is pending: the second launch records
    assert not lz.supports_pair()
    for k in (1, 2, 3):
        assert not isinstance(g.submit(lz, "p", k, True), HeldQuery) and not g.held
    assert log == [("single", 1), "record", ("single", 2), ("single", 3)]
    assert lz.match is None and lz.kt == ("kernel", "shape", True, "match")
    assert lz.vt["MATCH"] == 64 and lz.graph is None
    # recorded: no pair kernel, no second bitmap, no pair blocks - and never held or paired
    assert lz.ktp is None and lz.tags_b is None and lz.tplp is None and not lz.pblocks
    assert not lz.supports_pair()
    for k in range(4, 10):
        assert not isinstance(g.submit(lz, "p", k, True), HeldQuery)
        assert lz.held is None and not g.held
    assert [x[0] for x in log[4:]] == ["single"] * 6 and g.pairs == 0
    # ``_record`` itself launches a held query first, with the kernel it was submitted under
    log.clear()
    lz = _recording_launcher(monkeypatch, log)
    lz.ktp = "pair kernel"
    g.submit(lz, "p", 1, True)
    h = g.submit(lz, "p", 2, True)
    assert isinstance(h, HeldQuery) and lz.held is h
    lz.match, lz.launches = (1, 100, "params"), 5
    lz._record()
    assert log == [("single", 1), ("single", 2), "record"] and h.pending is not None
    assert lz.held is None and not g.held and lz.ktp is None


def test_a_program_that_returns_to_planning_flushes_the_gate():
    """``_AggProgram.submit`` returning None (an epoch change here) hands the query back to the
    planning path, which may re-lower: what is held launches first."""
    from hyperspace_amd.exec.gpu_common import _AggProgram

    class _Cache:
        epoch = 0

    class _Be:
        pass

    g, lz, log = _gate()
    be = _Be()
    be.pair_gate, be.cache = g, _Cache()
    prog = _AggProgram(be, None, None, None, None, 0)
    g.submit(lz, "p", 1, True)
    h = g.submit(lz, "p", 2, True)
    assert isinstance(h, HeldQuery) and h.pending is None
    be.cache.epoch = 1
    assert prog.submit(be, None, 0.0) is None
    assert h.pending is not None and not g.held and log[-1] == ("L", "single", 2)


def test_futures_poll_the_gate():
    """``QueryFuture.result`` / ``done`` are engine entries, before and after the wait; a wait on
    an earlier, launched future does not by itself release a held query."""
    from hyperspace_amd.exec.gpu_common import QueryFuture

    class _Cache:
        epoch = 0

    class _Be:
        def __init__(self, gate):
            self.pair_gate, self.cache, self.metrics = gate, _Cache(), {}

    g, lz, log = _gate()
    be = _Be(g)
    first = g.submit(lz, "p", 1, True)
    h = g.submit(lz, "p", 2, True)

    def fin(pending, hook=None):
        def finish():
            if hook:
                hook()
            return pending.result()
        finish.pending = pending
        return finish
    f1 = QueryFuture(be, None, fin(first, lz.finish), "native", None, 0.0)
    f2 = QueryFuture(be, None, fin(h), "native", None, 0.0)
    other = QueryFuture(be, None, fin(_FakePending(log, "q6")), "native", None, 0.0)
    assert other.result() == "q6" and other.done() and h.pending is None   # still held
    assert f1.result() == 1                     # the predecessor finished during this wait
    assert h.pending is not None and log[-1] == ("L", "single", 2)
    assert f2.done() and f2.result() == 2 and (g.pairs, g.singles) == (0, 2)


# ------------------------------------------------------------------------------------------------
# GPU tier, kernel level
# ------------------------------------------------------------------------------------------------
def _join_data(nkeys: int, kind: str = "plain", seed: int = 3):
    """Bucket-sorted join inputs (host): ``nkeys`` keys 40 apart over four buckets (45 % / none
    / 35 % / 20 %; one bucket when there are fewer than 8), 2-4 left rows per key.  ``kind``:

    "plain"    every left key has a right row and every right key left rows;
    "nomatch"  a tenth of the right keys and a twentieth of the left keys are missing, and a
               tenth more left keys lie between the right keys: guesses miss and gallop;
    "lwide" / "rwide"  past key 700 of the first bucket (inside its second 512-run stage) the
               keys jump by 90 000; one side fills the gap with 100 keys 800 apart, so the
               group around the jump is wide on the left / on the right only;
    "leave"    the first bucket's right side holds only the first half of its keys: the
               range-relative guesses of its second stage lie past the bucket's right rows."""
    rng = np.random.default_rng(seed)
    share = (0.45, 0.0, 0.35, 0.2) if nkeys >= 8 else (1.0, 0.0, 0.0, 0.0)
    sizes = [int(round(nkeys * x)) for x in share]
    sizes[0] += nkeys - sum(sizes)
    lks, rks, key0 = [], [], 1 << 20
    for b, n in enumerate(sizes):
        keys = key0 + 40 * np.arange(1, n + 1, dtype=np.int64)
        lkeys = rkeys = keys
        if kind == "nomatch" and n:
            lkeys = np.sort(np.concatenate([keys[rng.random(n) >= 0.05],
                                            keys[rng.integers(0, n, n // 10 + 1)] + 1]))
            rkeys = keys[rng.random(n) >= 0.1]
        elif kind in ("lwide", "rwide") and b == 0:
            assert n > 1100
            keys = keys.copy()
            keys[700:] += 90_000
            fill = np.sort(np.concatenate([keys, keys[699] + 800 * np.arange(1, 101)]))
            lkeys, rkeys = (keys, fill) if kind == "lwide" else (fill, keys)
        elif kind == "leave" and b == 0:
            rkeys = keys[:n // 2]
        key0 = (int(max(lkeys[-1], rkeys[-1])) if n else key0) + 400_000
        lks.append(np.repeat(lkeys, rng.integers(2, 5, len(lkeys))))
        rks.append(rkeys)
    lk, rk = np.concatenate(lks), np.concatenate(rks)
    assert (np.diff(lk) >= 0).all() and (np.diff(rk) > 0).all()
    d = {"lk": lk, "rk": rk,
         "loff": np.concatenate([[0], np.cumsum([len(x) for x in lks])]).astype(np.int64),
         "roff": np.concatenate([[0], np.cumsum([len(x) for x in rks])]).astype(np.int64),
         "ldate": rng.integers(0, 1000, len(lk)).astype(np.int32),
         "lprice": np.round(rng.random(len(lk)) * 1000, 2),
         "lqty": rng.integers(0, 1 << 30, len(lk)).astype(np.int64),
         "rdate": rng.integers(0, 1000, len(rk)).astype(np.int32)}
    d["starts"] = np.flatnonzero(np.concatenate([[True], lk[1:] != lk[:-1]]))
    return d


def test_join_data_holds_the_fall_back_cases():
    from test_tags2_keys16 import _ref32

    def wide(x):        # the stored codes: value - (smallest value + 2^31)
        return _ref32((x - x.min() - (1 << 31)).astype(np.int32))[2]
    for kind in ("lwide", "rwide"):
        d = _join_data(3000, kind)
        lw, rw = wide(d["lk"][d["starts"]]), wide(d["rk"])
        one, other = (lw, rw) if kind == "lwide" else (rw, lw)
        # the group around key 700 (runs 512 .. 1023: a stage inside the first bucket)
        assert one[700 // 32] and not other[16:32].any() and not one[16:21].any()
    d = _join_data(3000, "leave")
    nr0 = int(np.searchsorted(d["starts"], d["loff"][1]))
    assert nr0 >= 1024 and d["roff"][1] - d["roff"][0] < 1024
    d = _join_data(3000, "nomatch")
    runkeys = d["lk"][d["starts"]]
    hit = np.isin(runkeys, d["rk"])
    assert 0.7 < hit.mean() < 0.95 and not np.isin(d["rk"], runkeys).all()
    for n in (1, 255, 256, 257, 3000):
        d = _join_data(n)
        assert len(d["starts"]) == n and len(d["rk"]) == n
    assert (np.diff(_join_data(3000)["loff"]) == 0).any()        # an empty bucket


@functools.lru_cache(maxsize=None)
def _inputs(nkeys: int, kind: str = "plain"):
    import torch
    from hyperspace_amd.exec.encoding import Compact, encode
    dev = torch.device("cuda:0")
    d = _join_data(nkeys, kind)
    cols = {0: pa.array(d["lk"]), 1: pa.array(d["ldate"]), 2: pa.array(d["lprice"]),
            3: pa.array(d["lqty"]), 8: pa.array(d["rk"]), 9: pa.array(d["rdate"])}
    dc = {s: _col(a, dev) for s, a in cols.items()}
    comp = {s: e for s, e in ((s, encode(c)) for s, c in dc.items()) if e is not None}
    for s in (0, 8):
        if comp[s].width != 4:
            # a key range below 2^16 (the one-key table) encodes narrower; the join forms under
            # test read 32-bit key codes: value - (smallest value + 2^31), as ``encode`` biases them
            v = dc[s].data.long()
            lo, hi = int(v.min()), int(v.max())
            comp[s] = Compact((v - lo - (1 << 31)).to(torch.int32), 4, lo + (1 << 31), None,
                              dc[s].hs_type, lo, hi)
    B = len(d["loff"]) - 1
    rt_ = (torch.from_numpy(d["loff"][:-1].copy()).to(dev),
           torch.from_numpy(np.diff(d["loff"])).to(dev),
           torch.arange(B, dtype=torch.int32, device=dev), torch.from_numpy(d["roff"]).to(dev))
    return d, dc, comp, rt_


def _query(dc, lo: int, hi: int, rlit: int):
    """lo <= ldate < hi on the left (two conjuncts: the pruned phase 1 reads the runs' maximum
    and minimum), rdate < rlit on the right."""
    return _params(dc, [(">=", lo, 0), ("<", hi, 1)], rlit)


def _lower(dc, comp, rt_, nrows, prune: bool, monkeypatch, **cfg):
    """A launcher of the headline's form (one eager query ran through it).  Small tables get
    the 16-bit key form too: the group that holds a column's smallest code is always wide, which
    alone is above ``K16_MAX_WIDE`` of a table with a few groups."""
    from hyperspace_amd.exec import jit, jit_runs, kernel_config
    monkeypatch.setattr(jit_runs, "K16_MAX_WIDE", 1.0)
    kw = dict(rt2_match=False, rt2_copy=False, mj_2p=True, rt2_k16=True, rt2_pair=True,
              rs_prune=prune)
    kw.update(cfg)
    with kernel_config.use(**kw):
        jit.merge_join_agg(_query(dc, 300, 700, 500), *rt_, comp, nrows=nrows, rdup=False,
                           record=False, cache_spans=False)
        lz = jit.LAST_MJ_LAUNCHER[0]
    assert isinstance(lz, jit_runs.TwoPhaseLauncher) and lz.supports_pair(), cfg
    # (the one-key table's dates span less than 2^8: no 16-bit codes, so no pruned form there)
    assert "a.LO16 +" in lz.kt.src and ("a.RMX1" in lz.kt.src) == (prune and nrows > 8)
    return lz


# (left lo, left hi, right literal) of query A and of query B
LITERALS = {"identical": ((300, 700, 500), (300, 700, 500)),
            "nested": ((100, 900, 800), (300, 500, 400)),
            "disjoint": ((0, 300, 300), (600, 1000, 1500)),
            "none_all": ((600, 500, -5), (-5, 2000, 1500))}   # no run passes A, every run B


def _check_pair(lz, d, dc, lits, tag=""):
    """One pair launch against two single launches: both bitmaps and both results."""
    import torch
    nw = (len(d["starts"]) + 31) // 32
    ps = [_query(dc, *x) for x in lits]
    keys = [(tag, "a") + lits[0], (tag, "b") + lits[1]]
    want_t, want_r = [], []
    for p, k in zip(ps, keys):
        want_r.append(lz.launch(p, key=k, graph=True).result())
        torch.cuda.synchronize()
        want_t.append(lz.tags[:nw].clone())
    # poison both bitmaps: the pair kernel has to store every word of every run group
    lz.tags.fill_(0x5A5A5A5A)
    if lz.tags_b is not None:
        lz.tags_b.fill_(0x5A5A5A5A)
    a, b = lz.launch_pair(ps[0], keys[0], ps[1], keys[1])
    got_r = [a.result(), b.result()]
    torch.cuda.synchronize()
    assert torch.equal(lz.tags[:nw], want_t[0]), (tag, lits, "bitmap 1")
    assert torch.equal(lz.tags_b[:nw], want_t[1]), (tag, lits, "bitmap 2")
    for g, w in zip(got_r, want_r):
        for x, y in zip(g, w):
            assert np.array_equal(np.asarray(x), np.asarray(y)), (tag, lits)
    return want_t, want_r


@pytest.mark.gpu
@pytest.mark.parametrize("prune", [True, False])
def test_pair_launch_equals_two_single_launches(device, monkeypatch, prune):
    some = False
    for nkeys in (1, 255, 256, 257, 3000):
        d, dc, comp, rt_ = _inputs(nkeys)
        assert len(d["starts"]) == nkeys
        lz = _lower(dc, comp, rt_, len(d["lk"]), prune, monkeypatch)
        for name, lits in LITERALS.items():
            # three pairs of one launcher: the eager one, the capture and a replay
            for rep in range(3 if name == "nested" else 1):
                want_t, want_r = _check_pair(lz, d, dc, lits, (nkeys, name, rep))
            if name == "none_all":
                assert not want_t[0].any() and int(np.asarray(want_r[0][1]).reshape(-1)[1]) == 0
                assert int(np.asarray(want_r[1][1]).reshape(-1)[1]) == len(d["lk"])
            some |= bool(want_t[0].any()) and bool(want_t[1].any())
        assert "a.tags_b[" in lz.ktp.src and lz.ktp.src != lz.kt.src
    assert some


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lwide", "rwide", "nomatch", "leave"])
def test_pair_fall_back_paths_write_both_bitmaps(device, monkeypatch, kind):
    """Inputs whose stages leave the 256-run pipeline for the 64-run code (or gallop):
    ``test_join_data_holds_the_fall_back_cases``."""
    d, dc, comp, rt_ = _inputs(3000, kind)
    for prune in (True, False):
        # (grids: one stage per wavefront; one wavefront walks every stage, so a fall-back
        # stage follows fast ones)
        for cfg in ({}, {"rt2_wide_grid": 1}):
            lz = _lower(dc, comp, rt_, len(d["lk"]), prune, monkeypatch, **cfg)
            for name in ("nested", "none_all"):
                want_t, _ = _check_pair(lz, d, dc, LITERALS[name], (kind, prune, name))
                assert name == "none_all" or (want_t[0].any() and want_t[1].any())


# ------------------------------------------------------------------------------------------------
# GPU tier, end to end
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from conftest import gpu_available
    if not gpu_available():
        pytest.skip("no GPU")
    import pyarrow.parquet as pq
    from hyperspace_amd import Hyperspace, IndexConfig, Session
    tmp_path = tmp_path_factory.mktemp("pair")
    rng = np.random.default_rng(5)
    n_ord = 20_000
    okeys = rng.permutation(np.arange(1, n_ord + 1, dtype=np.int64) * 4)
    od = pa.table({"o_orderkey": okeys,
                   "o_orderdate": pa.array(rng.integers(8000, 10500, n_ord).astype(np.int32))
                   .view(pa.date32()),
                   "o_shippriority": np.zeros(n_ord, np.int32)})     # one group: 1-bit tags
    lk = np.repeat(okeys, rng.integers(1, 8, n_ord))
    n = len(lk)
    li = pa.table({"l_orderkey": lk,
                   "l_quantity": rng.integers(1, 51, n).astype(np.float64),
                   "l_extendedprice": np.round(rng.random(n) * 1e5, 2),
                   "l_discount": rng.integers(0, 11, n) / 100.0,
                   "l_shipdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32))
                   .view(pa.date32())})
    for name, t in (("lineitem", li), ("orders", od)):
        os.makedirs(tmp_path / name)
        pq.write_table(t, tmp_path / name / "part-0.parquet")
    s = Session(conf={"spark.hyperspace.system.path": str(tmp_path / "idx"),
                      "spark.hyperspace.index.numBuckets": "8",
                      "spark.sql.autoBroadcastJoinThreshold": "-1",
                      "spark.hyperspace.mi.execution.device": "gpu"},
                warehouse_dir=str(tmp_path / "wh"))
    hs = Hyperspace(s)
    lidf = s.read.parquet(str(tmp_path / "lineitem"))
    oddf = s.read.parquet(str(tmp_path / "orders"))
    hs.createIndex(lidf, IndexConfig("li_ship", ["l_shipdate"],
                                     ["l_discount", "l_quantity", "l_extendedprice"]))
    hs.createIndex(lidf, IndexConfig("li_ok", ["l_orderkey"],
                                     ["l_extendedprice", "l_discount", "l_shipdate"]))
    hs.createIndex(oddf, IndexConfig("od_ok", ["o_orderkey"], ["o_orderdate", "o_shippriority"]))
    Hyperspace.enable(s)
    # one query of each shape through the planner, then two through the prepared program
    for i in (100, 101, 102):
        _q3(lidf, oddf, i).collect()
        _q6(lidf, i).collect()
    yield s, lidf, oddf
    _SPIN.clear()


def _q6(li, i):
    from hyperspace_amd import col, count, sum_
    y = 1993 + i % 5
    return li.filter((col("l_shipdate") >= datetime.date(y, 1, 1)) &
                     (col("l_shipdate") < datetime.date(y + 1, 1, 1)) &
                     (col("l_discount") >= 0.01 * (i % 9)) & (col("l_quantity") < 20 + i % 7)) \
        .agg(sum_(col("l_extendedprice") * col("l_discount")).alias("r"), count("*").alias("n"))


def _q3(li, od, i):
    from hyperspace_amd import col, count, sum_
    dd = datetime.date(1995, 3, 1) + datetime.timedelta(days=i * 11 % 200)
    return li.join(od, li["l_orderkey"] == od["o_orderkey"]) \
        .filter((col("o_orderdate") < dd) & (col("l_shipdate") > dd)) \
        .groupBy("o_shippriority") \
        .agg(sum_(col("l_extendedprice") * (1 - col("l_discount"))).alias("rev"),
             count("*").alias("n"))


def _rows(x):
    return sorted(tuple(r) for r in x)


def _counts(s):
    g = s.backend().pair_gate
    return g.pairs, g.singles


_SPIN = []        # the buffer ``_behind_busy_device`` passes over; freed with ``env``


def _behind_busy_device(s, li, od, primer: int):
    """Keep the device busy (300 passes over a 2 GB buffer on the query stream: 1.2 TB of
    traffic, 0.15 s or more) and queue one join query behind it: later submissions of the shape
    find their predecessor unfinished.  ``_still_busy`` says afterwards whether they did."""
    import torch
    if not _SPIN:
        _SPIN.append(torch.zeros(1 << 29, dtype=torch.int32, device="cuda:0"))
    torch.cuda.synchronize()
    for _ in range(300):
        _SPIN[0].add_(1)
    return _q3(li, od, primer).collect_async()


def _still_busy(primer) -> None:
    """The counts asserted below hold only if every submission was made while the primer had not
    finished; a host too slow for that fails here, by name, not in a count."""
    assert not primer.done(), "the host took longer to submit than the device was kept busy"


@pytest.mark.gpu
@pytest.mark.parametrize("n,pairs,singles", [(2, 1, 0), (3, 1, 1), (5, 2, 1)])
def test_interleaved_async_queries_pair_up(env, n, pairs, singles):
    s, li, od = env
    ids = [10 * n + k for k in range(n)]
    want = [(_rows(_q3(li, od, i).collect()), _rows(_q6(li, i).collect())) for i in ids]
    for seen in (True, False):          # the literal vectors lowered before / first seen here
        if not seen:
            ids = [500 + i for i in ids]
            want = None
        p0, s0 = _counts(s)
        primer = _behind_busy_device(s, li, od, 100)
        futs = []
        for i in ids:
            futs.append((_q3(li, od, i).collect_async(), _q6(li, i).collect_async()))
            if len(futs) == min(n, 3):
                # (the fourth launch takes the primer's ring slot and waits for it; the fifth
                # query runs single whether or not it is held first)
                _still_busy(primer)
        got = [(_rows(a.result()), _rows(b.result())) for a, b in futs]
        primer.result()
        p1, s1 = _counts(s)
        # the primer runs single; the odd one out is released by its result()
        assert (p1 - p0, s1 - s0) == (pairs, singles + 1), (n, seen)
        assert all(a.path == "native" and b.path == "native" for a, b in futs)
        if want is None:
            want = [(_rows(_q3(li, od, i).collect()), _rows(_q6(li, i).collect())) for i in ids]
        assert got == want, (n, seen)               # exactly: same kernels, same order of sums
    assert not s.backend().pair_gate.held
    m = s.backend().metrics
    assert (m["join_pairs"], m["join_singles"]) == _counts(s)


@pytest.mark.gpu
def test_held_query_is_released_by_its_own_wait(env):
    s, li, od = env
    want = [_rows(_q3(li, od, i).collect()) for i in (61, 62)]
    for k, wait in enumerate(("result", "done")):
        p0, s0 = _counts(s)
        primer = _behind_busy_device(s, li, od, 101)
        f = _q3(li, od, 61 + k).collect_async()
        _still_busy(primer)
        assert len(s.backend().pair_gate.held) == 1
        if wait == "done":
            polls = 0
            while not f.done():
                polls += 1
            assert not s.backend().pair_gate.held
        assert _rows(f.result()) == want[k]
        assert _counts(s) == (p0, s0 + 2)
        primer.result()


@pytest.mark.gpu
def test_no_pairs_with_conf_off_or_one_in_flight(env):
    s, li, od = env
    ids = [71, 72, 73, 74]
    want = [_rows(_q3(li, od, i).collect()) for i in ids]
    key = "spark.hyperspace.mi.join.pairInFlight"
    s.conf.set(key, "false")
    try:
        p0, s0 = _counts(s)
        primer = _behind_busy_device(s, li, od, 102)
        futs = [_q3(li, od, i).collect_async() for i in ids]
        assert not s.backend().pair_gate.held
        assert [_rows(f.result()) for f in futs] == want
        primer.result()
        # (a query re-planned after the conf change launches from the planner, outside the gate)
        assert _counts(s)[0] == p0 and _counts(s)[1] > s0
    finally:
        s.conf.set(key, "true")
    # one step in flight: each result is read before the next submission
    p0, s0 = _counts(s)
    for i, w in zip(ids, want):
        f = _q3(li, od, i).collect_async()
        assert _rows(f.result()) == w
    # synchronous collects are never held, even behind a busy device
    primer = _behind_busy_device(s, li, od, 100)
    assert _rows(_q3(li, od, 71).collect()) == want[0]
    primer.result()
    assert _counts(s)[0] == p0 and _counts(s)[1] > s0 and not s.backend().pair_gate.held


@pytest.mark.gpu
def test_released_device_memory_flushes_a_held_query(env):
    s, li, od = env
    want = _rows(_q3(li, od, 81).collect())
    p0, s0 = _counts(s)
    primer = _behind_busy_device(s, li, od, 101)
    f = _q3(li, od, 81).collect_async()
    _still_busy(primer)
    held = list(s.backend().pair_gate.held)
    assert len(held) == 1 and held[0].pending is None
    from hyperspace_amd.exec.gpu import release_process_device_memory
    release_process_device_memory()         # every live backend's ``release_device_memory``
    # launched alone before anything was dropped; its result survives the release
    assert held[0].pending is not None and not s.backend().pair_gate.held
    assert _rows(f.result()) == want and _counts(s) == (p0, s0 + 2)
    primer.result()
    assert _rows(_q3(li, od, 81).collect()) == want         # the next query reloads


@pytest.mark.gpu
def test_pairs_leave_single_query_graphs_behind(device, monkeypatch):
    """A stream of pairs captures its ring slots' single-query graphs as it goes (one per pair
    launch), so a query that later runs alone - a synchronous collect - replays."""
    d, dc, comp, rt_ = _inputs(3000)
    lz = _lower(dc, comp, rt_, len(d["lk"]), True, monkeypatch)
    lits = LITERALS["nested"]
    ps = [_query(dc, *x) for x in lits]
    want = lz.launch(ps[0], key=("s", 0), graph=True).result()      # the eager first query
    g = lz.graph
    assert [sl.graph is not None for sl in g.slots] == [False] * g.RING
    captures, capture = [], g._capture
    monkeypatch.setattr(g, "_capture", lambda *a: captures.append(a[0]) or capture(*a))
    for rep in range(g.RING + 1):       # the eager pair, then captures and replays
        a, b = lz.launch_pair(ps[0], ("s", 0), ps[1], ("s", 1))
        a.result(), b.result()
    assert all(sl.graph is not None for sl in g.slots) and g.pairs
    assert len(captures) == g.RING == len(set(map(id, captures)))   # one per slot
    r0 = g.replays
    for rep in range(g.RING):           # every slot replays its own graph
        got = lz.launch(ps[0], key=("s", 0), graph=True).result()
        for x, y in zip(got, want):
            assert np.array_equal(np.asarray(x), np.asarray(y))
    assert g.replays == r0 + g.RING and len(captures) == g.RING      # nothing captured again
