"""ApplyDataSkipping: attach a data-skipping index to a filtered source relation.

On ``Filter(Relation)`` / ``Project(Filter(Relation))`` over a source relation that no covering
index replaced, the rule picks an ACTIVE data-skipping index of that relation with a sketch on a
column the condition references and records it on the relation (``HadoopFsRelation.skipping``).

The rule prunes nothing itself: cached plans are reused for other literal values
(``plan/plan_cache.py``), so the file list is cut when the scan executes
(``index.dataskipping.prune``), from the literals of that execution.  Any exception leaves the
plan unchanged.
"""
from __future__ import annotations

import logging

from ..actions import states
from ..plan import logical as L
from . import rule_utils as RU
from .filter_rule import extract_filter_node

log = logging.getLogger(__name__)


def _candidates(session, rel: L.LogicalRelation) -> list:
    from ..hyperspace import get_context
    all_idx = get_context(session).index_collection_manager.get_indexes([states.ACTIVE])
    return RU.get_candidate_indexes(session, [i for i in all_idx if i.is_data_skipping], rel)


def _pick(cands: list, filt_cols: list):
    cols = {c.lower() for c in filt_cols}
    best = None
    for i in sorted(cands, key=lambda e: e.name):
        n = sum(1 for s in i.derived_dataset.sketches if s["column"].lower() in cols)
        if n and (best is None or n > best[0]):
            best = (n, i)
    return best[1] if best else None


def ApplyDataSkipping(session, plan):
    def fn(p):
        m = extract_filter_node(p)
        if m is None:
            return None
        _, _, _, filt_cols, lr = m
        rel = lr.relation
        if rel.is_index() or rel.skipping is not None:
            return None
        try:
            index = _pick(_candidates(session, lr), filt_cols)
            if index is None:
                return None
            loc = rel.location
            if type(loc) is L.FileIndex:
                loc = L.DataSkippingFileIndex(loc)
            new_lr = lr.copy(relation=rel.copy(location=loc, skipping=index))
            return p.transform_up(lambda x: new_lr if x is lr else None)
        except Exception as e:  # noqa: BLE001 - an index must never break a query
            log.warning("Non fatal exception in running data skipping rule: %s", e)
            return None
    return plan.transform_down(fn)
