"""FilterIndexRule (reference ``index/rules/FilterIndexRule.scala:38-191``).

Replaces the relation under ``Project(Filter(Relation))`` / ``Filter(Relation)`` with a covering
index whose first indexed column appears in the predicate and which covers every referenced
column.  The index is read *without* its bucket spec to keep scan parallelism (``:59-65``).
When no covering index qualifies, a Z-order covering index (``index/zorder.py``) whose indexed
columns include ANY filtered column and which covers the plan is used instead.
Any exception leaves the plan unchanged — an index must never break a query.
"""
from __future__ import annotations

import logging

from ..actions import states
from ..plan import expressions as E
from ..plan import logical as L
from ..telemetry.events import (AppInfo, HyperspaceIndexUsageEvent, NoOpEventLogger,
                                get_event_logger)
from ..utils.resolver import resolve, resolve_one
from . import rule_utils as RU
from .rankers import rank_filter

log = logging.getLogger(__name__)


def extract_filter_node(plan):
    """Returns (original, filter, output_cols, filter_cols, relation) or None."""
    if isinstance(plan, L.Project) and isinstance(plan.child, L.Filter) and \
            isinstance(plan.child.child, L.LogicalRelation) and \
            not RU.is_index_applied(plan.child.child.relation):
        f = plan.child
        out_cols = [a.name for e in plan.project_list for a in e.references()]
        filt_cols = [a.name for a in f.condition.references()]
        return plan, f, out_cols, filt_cols, f.child
    if isinstance(plan, L.Filter) and isinstance(plan.child, L.LogicalRelation) and \
            not RU.is_index_applied(plan.child.relation):
        return plan, plan, [a.name for a in plan.child.output], \
            [a.name for a in plan.condition.references()], plan.child
    return None


def index_covers_plan(session, out_cols, filt_cols, indexed, included) -> bool:
    cs = session.case_sensitive
    return resolve_one(indexed[0], filt_cols, cs) is not None and \
        resolve(out_cols + filt_cols, list(indexed) + list(included), cs) is not None


def find_covering_indexes(session, filt, out_cols, filt_cols) -> list:
    from ..hyperspace import get_context
    rel = RU.get_logical_relation(filt)
    if rel is None:
        return []
    all_idx = get_context(session).index_collection_manager.get_indexes([states.ACTIVE])
    cands = [i for i in all_idx
             if i.is_covering and index_covers_plan(session, out_cols, filt_cols,
                                                    i.indexed_columns, i.included_columns)]
    return RU.get_candidate_indexes(session, cands, rel)


def zorder_index_covers_plan(session, out_cols, filt_cols, indexed, included) -> bool:
    """A Z-order index serves a filter on ANY of its indexed columns."""
    cs = session.case_sensitive
    return any(resolve_one(c, filt_cols, cs) is not None for c in indexed) and \
        resolve(out_cols + filt_cols, list(indexed) + list(included), cs) is not None


def find_zorder_indexes(session, filt, out_cols, filt_cols) -> list:
    """Z-order candidates: active, covering the plan, source signature matching exactly
    (Hybrid Scan never applies to this kind).  None unless
    ``spark.hyperspace.index.zorder.filterRule.enabled`` is set: the kind is opt-in."""
    from ..hyperspace import get_context
    from ..utils.conf import HyperspaceConf
    if not HyperspaceConf.zorder_filter_rule_enabled(session.conf):
        return []
    rel = RU.get_logical_relation(filt)
    if rel is None:
        return []
    all_idx = get_context(session).index_collection_manager.get_indexes([states.ACTIVE])
    cands = [i for i in all_idx
             if i.is_zorder and zorder_index_covers_plan(session, out_cols, filt_cols,
                                                         i.indexed_columns, i.included_columns)]
    return RU.get_signature_matched_indexes(session, cands, rel)


def rank_zorder(session, filt_cols, candidates: list):
    """Largest share of indexed columns named in the filter, then the smallest index."""
    if not candidates:
        return None
    cs = session.case_sensitive

    def key(i):
        named = sum(resolve_one(c, filt_cols, cs) is not None for c in i.indexed_columns)
        return (-named / len(i.indexed_columns), sum(f.size for f in i.content.file_infos),
                i.name)
    return min(candidates, key=key)


def _window_keys(p):
    """The partition column names of a Window directly over a filter node, else None."""
    if isinstance(p, L.Window) and p.partition_by and \
            all(isinstance(e, E.Attribute) for e in p.partition_by):
        return [e.name for e in p.partition_by]
    return None


def _log_usage(session, index, filt, transformed) -> None:
    logger = get_event_logger(session.conf)
    if not isinstance(logger, NoOpEventLogger):  # plan strings only when someone listens
        logger.log_event(HyperspaceIndexUsageEvent(
            AppInfo(session.user, session.app_id, session.app_name), [index],
            filt.tree_string(), transformed.tree_string(), "Filter index rule applied."))


def FilterIndexRule(session, plan):
    def fn(p):
        # a Window partitioned on exactly the index's indexed columns reads the index with its
        # bucket spec: the buckets are the window's partitioning (and their sort order its
        # ordering), so it needs no shuffle - worth more than the scan parallelism given up
        wkeys = _window_keys(p)
        m = extract_filter_node(p.children[0] if wkeys else p)
        if m is None:
            return None
        original, filt, out_cols, filt_cols, _ = m
        try:
            cands = find_covering_indexes(session, filt, out_cols, filt_cols)
            index = rank_filter(session, filt, cands)
            if index is None:
                # no covering index leads with a filtered column: a Z-order index serves a
                # filter on any of its indexed columns
                index = rank_zorder(session, filt_cols,
                                    find_zorder_indexes(session, filt, out_cols, filt_cols))
                if index is None or wkeys is not None:
                    return None      # under a Window: the child is visited next, unbucketed
                transformed = RU.transform_plan_to_use_index_only_scan(session, index, original,
                                                                       False)
                _log_usage(session, index, filt, transformed)
                return _Done(transformed)
            if wkeys is not None:
                cs = session.case_sensitive
                fold = (lambda n: n) if cs else str.lower
                if [fold(n) for n in wkeys] != [fold(n) for n in index.indexed_columns]:
                    return None      # the child is visited next and rewritten as usual
            transformed = RU.transform_plan_to_use_index(session, index, original,
                                                         wkeys is not None)
            _log_usage(session, index, filt, transformed)
            if wkeys is not None:
                return p.with_children((_Done(transformed),))
            return _Done(transformed)
        except Exception as e:  # noqa: BLE001
            log.warning("Non fatal exception in running filter index rule: %s", e)
            return None
    return _undone(plan.transform_down(fn))


class _Done(L.LogicalPlan):
    """Wraps a rewritten subtree so transform_down does not revisit it."""

    def __init__(self, inner):
        self.inner = inner
        self.children = ()

    @property
    def output(self):
        return self.inner.output

    def with_children(self, children):
        return self


def _undone(plan):
    return plan.transform_up(lambda p: p.inner if isinstance(p, _Done) else None)
