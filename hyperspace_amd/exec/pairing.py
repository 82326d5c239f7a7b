"""Pairing of in-flight merge-join queries of one shape (``jit_runs.TwoPhaseLauncher.launch_pair``:
one phase-1 pass tags both).

A pipelined caller (``DataFrame.collect_async``, a few steps in flight) usually submits the next
query of a shape while the previous one still runs.  Such a submission is *held* - queued
nowhere - until its partner arrives, and the two launch as a pair.  ``PairGate`` decides; it knows
nothing of the device beyond the launcher's ``busy()`` (the completion event of its latest
launch), so fakes drive it in the CPU tests.

A submission is held only when the caller allows it (``hold``, passed down from
``collect_async`` through the prepared program to the join prep: the asynchronous path, the conf
key, a single-rank session, a lowered literal vector), the launcher has the pair form and an
earlier launch of it has not finished.  At most one query is held per launcher.  It leaves the
gate

* as a pair, with the next holdable submission to the same launcher;
* alone, with the single kernel, when its own result is asked for (``result()`` / ``done()``),
  when any other submission reaches the launcher (so a launcher's queries launch in submission
  order), when an engine entry (a submission of any shape, a wait on any future of the backend,
  before and after the wait) finds the predecessor finished - the device would idle - or at
  ``release_all`` (a synchronous collect, and anything that invalidates lowerings: a device-cache
  epoch change, a placement change, a stale prep, released device memory).

A wait on another, already launched future does not by itself release the held query: that
future's device work is queued and finishes without it, so nothing can deadlock, and a caller that
keeps a fixed number of steps in flight waits on the oldest one after every submission - releasing
there would undo every pair.

Sessions with several ranks never hold: a replay's cross-rank all-gather is queued at launch, and
a decision that depends on device timing could order the collectives differently on different
ranks.
"""
from __future__ import annotations

from typing import List


class HeldQuery:
    """A submitted query whose launch waits for a partner; stands in for the launched query's
    ``graphs.GraphPending`` (``result()`` / ``done()``) and becomes it on release."""
    __slots__ = ("gate", "launcher", "p", "key", "pending", "epoch")

    def __init__(self, gate, launcher, p, key):
        self.gate, self.launcher, self.p, self.key = gate, launcher, p, key
        self.pending = None
        self.epoch = gate.epoch()   # device-cache epoch it was submitted under

    def release(self) -> None:
        """Launch alone (no-op once launched)."""
        if self.pending is None:
            self.gate._drop(self)
            self.gate._count(0, 1)
            self.pending = self.launcher.launch(self.p, self.key, graph=True)

    def result(self):
        self.release()
        return self.pending.result()

    def done(self) -> bool:
        self.release()
        return self.pending.done()


class PairGate:
    """The held queries of one backend and the pair / single counts (mirrored into ``metrics``
    as ``join_pairs`` / ``join_singles``).  ``epoch()``: the device-table cache's epoch."""

    def __init__(self, metrics=None, epoch=None):
        self.held: List[HeldQuery] = []
        self.pairs = 0
        self.singles = 0
        self.metrics = metrics
        self.epoch = epoch or (lambda: None)

    def _count(self, pairs: int, singles: int) -> None:
        self.pairs += pairs
        self.singles += singles
        if self.metrics is not None:
            self.metrics["join_pairs"], self.metrics["join_singles"] = self.pairs, self.singles

    def _drop(self, h: HeldQuery) -> None:
        if h.launcher.held is h:
            h.launcher.held = None
        if h in self.held:
            self.held.remove(h)

    def submit(self, launcher, p, key, hold: bool):
        """Launch, pair or hold one graph-replay submission of ``launcher``; returns its pending
        result (``GraphPending`` or ``HeldQuery``)."""
        h = launcher.held
        if hold and launcher.supports_pair():
            if h is not None:
                self._drop(h)
                self._count(1, 0)
                h.pending, out = launcher.launch_pair(h.p, h.key, p, key)
                return out
            if launcher.busy():
                h = launcher.held = HeldQuery(self, launcher, p, key)
                self.held.append(h)
                return h
        if h is not None:
            h.release()
        self._count(0, 1)
        return launcher.launch(p, key, graph=True)

    def poll(self) -> None:
        """An engine entry (callers test ``held`` first): release what would leave the device
        idle - the predecessor has finished - and what was submitted under another device-cache
        epoch."""
        epoch = self.epoch()
        for h in list(self.held):
            if h.epoch != epoch or not h.launcher.busy():
                h.release()

    def release_all(self) -> None:
        for h in list(self.held):
            h.release()
