"""hipGraph-captured scan pipelines (BASELINE.json north star; SURVEY.md §2.3 K7 "kernel chain
captured in a hipGraph", §7.4 item 6).

An indexed filter + aggregate (TPC-H Q6 shape) is four device steps on the device-resident index
table, each a kernel:

1. per-bucket range search of the leading indexed column (``hs_range_search_val``: the bounds
   travel in its by-value argument struct);
2. ranges -> tile prefix (``hs_ranges_to_tiles``);
3. the query's generated scan kernel (``exec/jit.py``);
4. the deterministic final reduction that also delivers the result (``hs_agg_fold``): it writes
   the device result block and the replay's pinned host block.

The two-phase merge join (``TwoPhaseGraph``) is three: phase 1, phase 2, fold; a pair of queries
with the pair phase 2 is three as well (pair phase 1, pair phase 2, ONE fold of both partial sets
into the two queries' host blocks).

Every size in such a chain is fixed by the table (one range per bucket, a fixed grid), so it is
captured ONCE per (query shape, table) into a HIP graph.  The graph has no copy node and no
input buffer: what changes per query - the range bounds, the generated kernels' literals, the
address of the host block the result goes to - sits in by-value argument structs of its kernel
nodes, which a replay rewrites (``hs_graph_replay``).  No node outside those holds an address that
belongs to one in-flight instance, so the one captured graph is instantiated once per ring slot
(``hs_graph_clone``) instead of being captured per slot.

The first execution of a key runs the same sequence eagerly (that also loads the kernel module);
the second captures and instantiates every slot's executable graph; later executions replay.
With several ranks (sharded placement) the replay's device output block is all-gathered across
ranks right after it (exec/gpu.py); the host block then only feeds single-rank callers.
"""
from __future__ import annotations

import ctypes as C
import threading
import time
from collections import OrderedDict
from typing import Optional, Tuple

import numpy as np

from ..ops import _lib as NL
from . import jit

# host time of making executable graphs: a capture (stream capture + node table + instantiate)
# against a clone (instantiate of the kept graph)
STATS = {"captures": 0, "capture_s": 0.0, "clones": 0, "clone_s": 0.0}


class _LibKernel:
    """A kernel of libhs_kernels with ONE by-value argument struct, named in a capture's
    rewritten list beside the generated kernels (``function()``: the address its captured
    kernel node carries)."""

    def __init__(self, getter: str):
        self.getter = getter
        self._fn = None

    def function(self):
        if self._fn is None:
            self._fn = getattr(NL.lib(), self.getter)()
        return self._fn


_FOLD = _LibKernel("hs_agg_fold_func")
_RANGE = _LibKernel("hs_range_search_val_func")


class _Pinned:
    """A hipHostMalloc block (capture-safe: no allocator bookkeeping on the copies)."""

    def __init__(self, nbytes: int):
        self.nbytes = nbytes
        self.ptr = jit.runtime().hs_host_alloc(nbytes)
        if not self.ptr:
            raise MemoryError(f"hipHostMalloc({nbytes}) failed")

    def view(self) -> np.ndarray:
        v = getattr(self, "_view", None)
        if v is None:       # the block never moves: one numpy view for its lifetime
            v = self._view = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))
        return v

    def __del__(self):
        if getattr(self, "ptr", None):
            jit.runtime().hs_host_free(self.ptr)
            self.ptr = None


class _Slot:
    """One in-flight instance of a captured pipeline: its own pinned result block (the fold
    kernel writes it when the graph EXECUTES, so a query queued behind another must not share
    it), the fold's argument struct that names that block, its own executable graph (whose
    kernel arguments are rewritten per launch), and the event that marks its result ready."""

    def __init__(self, out_bytes: int):
        self.h_out = _Pinned(out_bytes)
        self.fold = None           # NL.AggFoldArgs of this slot alone (``_RingGraph._fold_args``)
        self.graph = None          # native handle (csrc/runtime/hs_graph.cpp)
        # native timing-disabled event: recorded by hs_graph_replay in the same call as the
        # launch (a torch.cuda.Event costs a few Python-level calls per query)
        self.event = jit.runtime().hs_event_create()
        if not self.event:
            raise RuntimeError(f"hs_event_create: {jit.runtime().hs_graph_last_error().decode()}")
        self.launched = False
        self.current = None   # _Launch whose result the slot's h_out holds / will hold

    def done(self) -> bool:
        rc = jit.runtime().hs_event_query(self.event)
        _rt_check(rc if rc < 0 else 0, "hs_event_query")
        return rc == 0

    def wait(self) -> None:
        _rt_check(jit.runtime().hs_event_sync(self.event), "hs_event_sync")

    def __del__(self):
        R = jit.runtime()
        if getattr(self, "graph", None):
            R.hs_graph_destroy(self.graph)
            self.graph = None
        if getattr(self, "event", None):
            R.hs_event_destroy(self.event)
            self.event = None


class _Launch:
    """One query launched into a slot; ``value`` is filled when it is read (by the caller, or
    by the next launch that needs the slot first)."""

    __slots__ = ("slot", "value")

    def __init__(self, slot: _Slot):
        self.slot = slot
        self.value = None


def _rt_check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what}: {jit.runtime().hs_graph_last_error().decode()}")


def _clone(h):
    """Another executable graph of the captured graph behind ``h`` (no second capture)."""
    R = jit.runtime()
    t0 = time.perf_counter()
    c = R.hs_graph_clone(h)
    STATS["clones"] += 1
    STATS["clone_s"] += time.perf_counter() - t0
    if not c:
        raise RuntimeError(f"hs_graph_clone: {R.hs_graph_last_error().decode()}")
    return c


def node_counts(h) -> Tuple[int, int, int]:
    """(kernel, memcpy, other) node counts of the captured graph behind the handle ``h``."""
    k, m, o = C.c_int(0), C.c_int(0), C.c_int(0)
    _rt_check(jit.runtime().hs_graph_node_counts(h, C.byref(k), C.byref(m), C.byref(o)),
              "hs_graph_node_counts")
    return k.value, m.value, o.value


class _RingGraph:
    """A captured pipeline with ``RING`` in-flight instances (one pinned result block and one
    executable graph per slot; device intermediates shared, since replays on one stream execute
    in order).  Subclasses define ``kernels`` (the kernels whose by-value argument blocks change
    per query: the generated ones, ``_RANGE`` and ``_FOLD``), ``_enqueue(slot, stream, blocks)``
    (the work one query queues, eager or under capture), ``GA`` and ``out`` (the device result
    block, ``K.agg_outputs``).

    A replay rewrites the captured kernel nodes' argument blocks and launches the executable
    graph: the kernels keep their by-value kernarg struct (a struct read from device memory
    makes every column load a flat load, ~2x slower on gfx950 -
    ``profiles/graph_byptr_r5.txt``).  The shape is captured once; every slot's executable
    graph is instantiated from that capture (``hs_graph_clone``)."""
    # in-flight instances per captured shape: a pipelined query stream (exec/gpu.py
    # collect_async) keeps a few replays of the same shape queued at once
    RING = 4

    def _init_ring(self) -> None:
        self.slots = [_Slot(self.out[0].hs_buf.numel()) for _ in range(self.RING)]
        self._next = 0
        self._warm = False
        self._proto = None     # the handle of the shape's capture (a slot's; clones come from it)
        self.replays = 0
        self.on_side = False   # replays moved to the backend's side stream (exec/gpu.py)
        self.side_stream = None

    @property
    def graph(self):
        return self.slots[0].graph

    def _fold_set(self, parts, nblk: int, slot: _Slot, dout: bool) -> NL.AggFoldSet:
        """``parts`` folded into ``slot``'s host block, and into the device result block with
        ``dout``."""
        return NL.AggFoldSet(parts[0].data_ptr(), parts[1].data_ptr(), parts[2].data_ptr(),
                             parts[3].data_ptr(),
                             self.out[0].hs_buf.data_ptr() if dout else None, slot.h_out.ptr,
                             nblk, 0)

    def _fold_args(self, slot: _Slot, nblk: int) -> NL.AggFoldArgs:
        """``slot``'s fold block of a single query: the graph's partials into the device result
        block (the sharded placement's cross-rank combine reads it) and the slot's host block."""
        a = slot.fold
        if a is None:
            a = slot.fold = NL.AggFoldArgs(self.GA, 1)
            a.set[0] = self._fold_set(self.parts, nblk, slot, True)
        return a

    def _fold(self, args: NL.AggFoldArgs, stream: int) -> None:
        NL.check(NL.lib().hs_agg_fold(C.byref(args), stream), "hs_agg_fold")

    def _capture(self, slot: _Slot, blocks, cur) -> None:
        """Give ``slot`` its executable graph: the shape's one capture (from this slot's
        launch), or for every later slot a clone of it - the slots' chains differ only in what
        a replay rewrites."""
        if self._proto is None:
            self._proto = slot.graph = self._capture_of(
                lambda st: self._enqueue(slot, st, blocks), self.kernels, cur)
        else:
            slot.graph = _clone(self._proto)

    def _capture_of(self, enqueue, kernels, cur):
        """The executable graph (native handle) of what ``enqueue(stream)`` queues;
        ``kernels``: the kernels whose argument blocks a replay rewrites, in launch order."""
        import torch
        R = jit.runtime()
        t0 = time.perf_counter()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        _rt_check(R.hs_graph_capture_begin(side.cuda_stream), "hs_graph_capture_begin")
        try:
            enqueue(side.cuda_stream)
        finally:
            fns = [k.function() for k in kernels]
            arr = (C.c_void_p * len(fns))(*fns)
            h = R.hs_graph_capture_end(side.cuda_stream, arr, len(fns))
        if not h:
            raise RuntimeError(f"graph capture: {R.hs_graph_last_error().decode()}")
        cur.wait_stream(side)
        STATS["captures"] += 1
        STATS["capture_s"] += time.perf_counter() - t0
        return h

    def _take_slot(self) -> _Slot:
        """The ring's next slot, free for a new query: a slot still holding an unread earlier
        result is drained first (wait for it and keep its result on the earlier handle), one
        whose replay is still running is waited for."""
        slot = self.slots[self._next]
        self._next = (self._next + 1) % len(self.slots)
        prev = slot.current
        if prev is not None and prev.value is None:
            prev.value = self._read(slot)
        elif slot.launched and not slot.done():
            slot.wait()    # back-pressure: the slot's replay is still running
        return slot

    def busy(self) -> bool:
        """Whether the most recent launch has not finished on the device."""
        slot = self.slots[self._next - 1]
        return slot.launched and not slot.done()

    def _launch_slot(self, blocks_of, stream=None, after=None) -> _Launch:
        """Queue one query on ``stream`` (default: the current stream), ordered after the work
        queued on ``after`` when given: ``blocks_of(slot)`` gives the argument blocks (ctypes)
        of ``kernels`` for the slot the query takes.  A slot still holding an unread earlier
        result is drained first (wait for it and keep its result on the earlier handle:
        back-pressure, no lost results); a slot's graph gets new kernel arguments only once its
        previous replay has finished.  A replay is one native call (``hs_graph_replay``:
        ordering, argument rewrite, launch, completion event)."""
        import torch
        slot = self._take_slot()
        blocks = blocks_of(slot)
        R = jit.runtime()
        if slot.graph is None and self._warm:
            # the shape's one capture (or, behind a stream of pairs, a clone of it), and with
            # it every other slot's executable graph
            self._capture(slot, blocks,
                          stream if stream is not None else torch.cuda.current_stream())
            for other in self.slots:
                if other.graph is None:
                    other.graph = _clone(self._proto)
        if slot.graph is not None:
            st = stream.cuda_stream if stream is not None else NL.raw_stream()
            ptrs = (C.c_void_p * len(blocks))(*[C.addressof(b) for b in blocks])
            _rt_check(R.hs_graph_replay(slot.graph, len(blocks), ptrs, st,
                                        after.cuda_stream if after is not None else None,
                                        slot.event), "hs_graph_replay")
            self.replays += 1
        else:
            cur = stream if stream is not None else torch.cuda.current_stream()
            st = cur.cuda_stream
            if after is not None:
                cur.wait_stream(after)
            self._enqueue(slot, st, blocks)   # first run of the shape: eager (loads modules)
            self._warm = True
            _rt_check(R.hs_event_record(slot.event, st), "hs_event_record")
        slot.launched = True
        h = _Launch(slot)
        slot.current = h
        return h

    def result(self, h: _Launch):
        """(sum, count, min, max) numpy arrays of the launched query ``h``."""
        if h.value is None:
            h.value = self._read(h.slot)
        return h.value

    def _read(self, slot: _Slot):
        slot.wait()
        h = slot.h_out.view()
        n = 8 * self.GA
        return (h[0:n].view(np.float64).copy(), h[n:2 * n].view(np.int64).copy(),
                h[2 * n:3 * n].view(np.float64).copy(), h[3 * n:4 * n].view(np.float64).copy())


def _cbuf(block) -> "C.Array":
    """A ctypes copy of a packed argument block (kept with the cached block, so a replay passes
    its address without a per-query copy)."""
    b = bytes(block)
    return C.create_string_buffer(b, len(b))


class ScanAggGraph(_RingGraph):
    def __init__(self, kernel: jit.Kernel, kd: NL.ColDesc, bucket_off, nb: int, grid: int,
                 GA: int, shmem: int, device, vec: int = 0):
        import torch
        from ..ops import kernels as K
        self.kernel = kernel
        self.kernels = (_RANGE, kernel, _FOLD)
        self.kd = kd
        self.bucket_off = bucket_off
        self.nb, self.grid, self.GA, self.shmem = nb, grid, GA, shmem
        self.vec = vec   # rows per thread of a vectorized kernel (tiles over aligned ranges)
        self.tile = jit.BLOCK * (vec or jit.SCAN_ITEMS)
        # device intermediates are shared: replays on one stream execute in order
        self.rstart = torch.empty(nb, dtype=torch.int64, device=device)
        self.rlen = torch.empty(nb, dtype=torch.int64, device=device)
        self.rbk = torch.empty(nb, dtype=torch.int32, device=device)
        self.tp = torch.empty(nb + 1, dtype=torch.int64, device=device)
        self.parts = jit._partials(grid, GA, device)
        self.out = K.agg_outputs(GA, device)
        self._init_ring()
        # the range search's argument struct, one per slot; a launch writes its bounds
        for slot in self.slots:
            slot.range = NL.RangeValArgs(kd, bucket_off.data_ptr(), None, self.rstart.data_ptr(),
                                         self.rlen.data_ptr(), self.rbk.data_ptr(),
                                         (C.c_int64 * 6)(), nb, 0)

    def _enqueue(self, slot: _Slot, stream: int, blocks) -> None:
        """``blocks``: the range search's, the scan kernel's and the fold's argument blocks."""
        K = NL.lib()
        NL.check(K.hs_range_search_val(C.byref(blocks[0]), stream), "hs_range_search_val")
        if self.vec:
            NL.check(K.hs_ranges_to_tiles_aligned(NL.ptr(self.rstart), NL.ptr(self.rlen), self.nb,
                                                  self.tile, self.vec, NL.ptr(self.tp), stream),
                     "hs_ranges_to_tiles_aligned")
        else:
            NL.check(K.hs_ranges_to_tiles(NL.ptr(self.rlen), self.nb, self.tile,
                                          NL.ptr(self.tp), stream), "hs_ranges_to_tiles")
        self.kernel.launch_packed(self.grid, blocks[1], stream, self.shmem)
        self._fold(blocks[2], stream)

    def buffers(self) -> list:
        """Device intermediates a replay reads and writes."""
        return [self.rstart, self.rlen, self.rbk, self.tp, self.bucket_off,
                *self.parts, self.out[0].hs_buf]

    def values_template(self) -> dict:
        return {"rstart": self.rstart.data_ptr(), "rlen": self.rlen.data_ptr(),
                "tile_prefix": self.tp.data_ptr(), "R": self.nb,
                "psum": self.parts[0].data_ptr(), "pcnt": self.parts[1].data_ptr(),
                "pmin": self.parts[2].data_ptr(), "pmax": self.parts[3].data_ptr()}

    def launch(self, bounds: Tuple[int, int, int, int, int, int], args_block, stream=None,
               after=None) -> _Launch:
        """Queue one query on ``stream`` (default current), after ``after``'s queued work when
        given; ``result(handle)`` waits for it.  ``args_block``: the scan kernel's packed
        arguments (bytes or a ``_cbuf``)."""
        if not isinstance(args_block, C.Array):
            args_block = _cbuf(args_block)

        def blocks_of(slot):
            # (the launch and a replay's rewrite copy the struct: the slot's one is free again
            # when the call returns)
            slot.range.bp[:] = bounds
            return slot.range, args_block, self._fold_args(slot, self.grid)
        return self._launch_slot(blocks_of, stream, after)

    def run(self, bounds: Tuple[int, int, int, int, int, int], args_block):
        """(sum, count, min, max) numpy arrays for one query (launch + wait)."""
        return self.result(self.launch(bounds, args_block))


class TwoPhaseGraph(_RingGraph):
    """The run-keyed two-phase merge-join aggregate (exec/jit_runs.py) captured: phase 1 (run
    tags), phase 2 (bits scan into the graph's partials) and the fold that reduces the partials
    into the result blocks - one replay per query instead of three launches and their host-side
    argument packing.  The tag bitmap and the run tables are the launcher's (fixed per
    lowering)."""

    def __init__(self, kt: jit.Kernel, ks: jit.Kernel, grid_t: int, grid_s: int, GA: int,
                 shmem: int, device):
        from ..ops import kernels as K
        self.kt, self.ks = kt, ks
        self.kernels = (kt, ks, _FOLD)
        self.grid_t, self.grid_s, self.GA, self.shmem = grid_t, grid_s, GA, shmem
        self.parts = jit._partials(grid_s, GA, device)
        # the second query's partials of a pair whose phase 2 is one pass (``launch_pair`` with
        # the pair kernel ``ksp``)
        self.parts_b = jit._partials(grid_s, GA, device)
        self.out = K.agg_outputs(GA, device)
        self._init_ring()
        # executable graphs of pairs (``launch_pair``): index of the first query's slot ->
        # native handle; one capture (``_pair_proto``), the other positions are clones of it
        self.pairs: dict = {}
        self._pair_proto = None
        self._pair_folds: dict = {}    # index of the first slot -> the pair's one fold block
        self._pair_warm = False
        self.pair_replays = 0

    def _enqueue(self, slot: _Slot, stream: int, blocks) -> None:
        self.kt.launch_packed(self.grid_t, blocks[0], stream, 0)
        self.ks.launch_packed(self.grid_s, blocks[1], stream, self.shmem)
        self._fold(blocks[2], stream)

    def _pair_fold(self, ia: int, sa: _Slot, sb: _Slot) -> NL.AggFoldArgs:
        """The one fold of a pair with the pair phase 2: A's partials into A's host block, B's
        into B's host block and into the device result block - which then holds what it held
        after the two final reductions this fold replaces, B's result."""
        a = self._pair_folds.get(ia)
        if a is None:
            a = self._pair_folds[ia] = NL.AggFoldArgs(self.GA, 2)
            a.set[0] = self._fold_set(self.parts, self.grid_s, sa, False)
            a.set[1] = self._fold_set(self.parts_b, self.grid_s, sb, True)
        return a

    def _enqueue_pair(self, ktp: jit.Kernel, stream: int, blocks,
                      ksp: Optional[jit.Kernel] = None) -> None:
        """One linear chain: pair phase 1, then per query phase 2 and the fold into its own
        slot's result block (the partials and the device result block are reused in stream
        order, as between two single queries).  With the pair phase 2 ``ksp`` (three blocks):
        pair phase 1, pair phase 2 into both partial sets, then one fold of both."""
        ktp.launch_packed(self.grid_t, blocks[0], stream, 0)
        if ksp is not None:
            ksp.launch_packed(self.grid_s, blocks[1], stream, self.shmem)
            self._fold(blocks[2], stream)
            return
        for blk, fold in ((blocks[1], blocks[2]), (blocks[3], blocks[4])):
            self.ks.launch_packed(self.grid_s, blk, stream, self.shmem)
            self._fold(fold, stream)

    def launch_pair(self, ktp: jit.Kernel, block_tp, block_sa, block_sb, single,
                    ksp: Optional[jit.Kernel] = None) -> tuple:
        """Queue two queries behind one pass of the pair phase-1 kernel ``ktp`` (``_cbuf``
        blocks: the pair kernel's, and each query's phase 2 - or, with the pair phase-2 kernel
        ``ksp``, its one block as ``block_sa`` and no ``block_sb``: a three-kernel chain whose
        second kernel writes A's partials into ``parts`` and B's into ``parts_b`` and whose
        third folds both; A's result then waits for the shared phase 2 instead of its own).
        Each query takes its own ring slot; both slots' events are recorded behind the whole
        chain.  The first pair runs eagerly (that loads the pair kernel's module); the second
        captures the chain, and every later position of a pair in the ring gets a clone of that
        capture.  (A sharded session never pairs - ``exec/pairing.py`` - so nothing reads the
        device result block between the two queries of a pair.)

        ``single``: the (phase 1, phase 2) blocks of either query alone.  A stream of pairs
        never runs its slots alone, so their single-query graphs would be made by the first
        queries that do - synchronous collects, which wait for each.  Instead each pair launch
        makes one missing single-query graph of its slots (the first is the shape's capture,
        the others clones), after the pair is queued: the host does it while the device runs
        the pair."""
        import torch
        ia = self._next
        sa, sb = self._take_slot(), self._take_slot()
        if ksp is not None:
            blocks = (block_tp, block_sa, self._pair_fold(ia, sa, sb))
            kernels = (ktp, ksp, _FOLD)
        else:
            # (``ks`` and the fold twice: the native side takes kernel nodes of one function in
            # dependency order, so the first of each is A's and the second is B's)
            blocks = (block_tp, block_sa, self._fold_args(sa, self.grid_s),
                      block_sb, self._fold_args(sb, self.grid_s))
            kernels = (ktp, self.ks, _FOLD, self.ks, _FOLD)
        R = jit.runtime()
        h = self.pairs.get(ia)
        if h is None and self._pair_warm:
            if self._pair_proto is None:
                self._pair_proto = h = self._capture_of(
                    lambda s_: self._enqueue_pair(ktp, s_, blocks, ksp), kernels,
                    torch.cuda.current_stream())
                for i in range(len(self.slots)):    # the other positions of a pair in the ring
                    if i != ia:
                        self.pairs[i] = _clone(h)
            else:
                h = _clone(self._pair_proto)
            self.pairs[ia] = h
        st = NL.raw_stream()
        if h is not None:
            ptrs = (C.c_void_p * len(blocks))(*[C.addressof(b) for b in blocks])
            _rt_check(R.hs_graph_replay(h, len(blocks), ptrs, st, None, sa.event),
                      "hs_graph_replay")
            self.pair_replays += 1
        else:
            self._enqueue_pair(ktp, st, blocks, ksp)
            self._pair_warm = True
            _rt_check(R.hs_event_record(sa.event, st), "hs_event_record")
        _rt_check(R.hs_event_record(sb.event, st), "hs_event_record")
        out = []
        for slot in (sa, sb):
            slot.launched = True
            slot.current = _Launch(slot)
            out.append(slot.current)
        if self._warm and (sa.graph is None or sb.graph is None):
            # (made, not launched: a replay rewrites every block)
            slot = sa if sa.graph is None else sb
            self._capture(slot, (*single, self._fold_args(slot, self.grid_s)),
                          torch.cuda.current_stream())
        return tuple(out)

    def __del__(self):
        pairs = getattr(self, "pairs", None)
        while pairs:
            jit.runtime().hs_graph_destroy(pairs.popitem()[1])

    def buffers(self) -> list:
        return [*self.parts, *self.parts_b, self.out[0].hs_buf]

    def partial_ptrs(self, sfx: str = "", parts=None) -> dict:
        p = self.parts if parts is None else parts
        return {"psum" + sfx: p[0].data_ptr(), "pcnt" + sfx: p[1].data_ptr(),
                "pmin" + sfx: p[2].data_ptr(), "pmax" + sfx: p[3].data_ptr()}

    def launch(self, block_t, block_s) -> _Launch:
        """``block_t`` / ``block_s``: ``_cbuf`` argument blocks of the two phases."""
        return self._launch_slot(
            lambda slot: (block_t, block_s, self._fold_args(slot, self.grid_s)))


class GraphPending:
    """A replayed pipeline whose result block is still in flight."""
    __slots__ = ("graph", "handle")

    def __init__(self, graph, handle):
        self.graph, self.handle = graph, handle

    def result(self):
        return self.graph.result(self.handle)

    def done(self) -> bool:
        """Whether ``result()`` returns without waiting for the device."""
        h = self.handle
        return h.value is not None or h.slot.current is not h or h.slot.done()


class GraphCache:
    """Per-backend LRU of captured pipelines (graphs pin their buffers)."""

    def __init__(self, capacity: int = 64):
        self.capacity = capacity
        self._lru: "OrderedDict[tuple, ScanAggGraph]" = OrderedDict()
        self._lock = threading.Lock()

    def get(self, key: tuple, make) -> ScanAggGraph:
        with self._lock:
            g = self._lru.get(key)
            if g is not None:
                self._lru.move_to_end(key)
                return g
        g = make()
        with self._lock:
            self._lru[key] = g
            while len(self._lru) > self.capacity:
                _, old = self._lru.popitem(last=False)
                side = getattr(old, "side_stream", None)
                if side is not None:
                    # its last replays may still run on the side stream: let them finish before
                    # the executable graphs are destroyed
                    side.synchronize()
        return g

    def peek(self, key: tuple) -> Optional[ScanAggGraph]:
        """The cached pipeline of ``key`` (touched as most recent), or None."""
        with self._lock:
            g = self._lru.get(key)
            if g is not None:
                self._lru.move_to_end(key)
            return g

    def __len__(self):
        return len(self._lru)


def range_bounds(lo: Optional[int], lo_incl: bool, hi: Optional[int], hi_incl: bool):
    """The 6-int64 bound block read by ``hs_range_search_dev`` (images as signed int64 bits)."""
    def s64(v):
        v = int(v or 0) & 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >= (1 << 63) else v
    return (1 if lo is not None else 0, s64(lo), 1 if lo_incl else 0,
            1 if hi is not None else 0, s64(hi), 1 if hi_incl else 0)
