"""Record what the merge-join phase-1 generator (``jit_runs.gen_run_tags2``) and
``gen_match_gather`` emit, as hashes, so that a restructuring of the generator can be checked
byte for byte on the CPU (``tests/test_tags2_sources.py`` against
``tests/golden/tags2_sources.json``):

    python scripts/dev/tags2_manifest.py [--root TREE] --out FILE

``--root``: the tree ``hyperspace_amd``, ``tests`` and ``scripts/dev/gen_join_src`` are imported
from (default: this file's), so the manifest of another commit is
``git worktree add ../parent <commit>`` and ``--root ../parent``.  Only ``gen_run_tags2``,
``gen_match_gather`` and the predicates ``tag_width``, ``prune_plan``, ``tags2_k16``,
``tags2_pair`` and ``copy_ok`` are called.

One group per shape (``GROUPS``): the Q3 join of ``gen_join_src.q3_params`` with 1, 3 and 200
right-side groups (W = 1, 2, 8), the headline's shape, and variants of the first that reach the
generator's other branches - grouped by a left column, a plain (not compact) or nullable right
predicate column, a nullable or grouped-16-bit right key, and a ``<`` left predicate (an
``RMN<slot>`` bound).  Per group the product of ``SWEEP`` under ``kernel_config.use``, ``ix32``,
the six modes, with and without ``prune_plan``'s bounds (mode ""), ``k16`` and ``pair`` where
``tags2_k16`` / ``tags2_pair`` allow them - skipping only what the generator's asserts forbid
("rec", "lo16", "lo16prep" without ``ix32``; "copy" without ``copy_ok``) - and last one
``gen_match_gather`` source.  The record per case and the file form: ``source_manifest.py``.
"""
import functools
import itertools

import source_manifest as S
from source_manifest import cfg_key

SWEEP = (("rt2_unroll", (1, 2, 4)), ("rt2_wide", (1, 4)), ("rt2_k16", (True, False)))
MODES = ("", "rec", "match", "copy", "lo16", "lo16prep")
GROUPS = ("q3g1", "q3g3", "q3g200", "headline", "left_grouped", "plain_pred_col",
          "nullable_pred_col", "nullable_key", "grouped_key", "lt_pred")


def _nullable(x):
    """A DeviceColumn of the numpy array ``x`` with a tenth of its rows null."""
    import numpy as np
    import pyarrow as pa
    from hyperspace_amd.exec.device_table import DeviceColumn
    return DeviceColumn.from_arrow(
        pa.array(x, mask=np.random.default_rng(2).random(len(x)) < 0.1), "cpu")


def shape(group: str):
    """(params, compacts, objects to keep alive) of ``group``."""
    import numpy as np
    G = S.gen_join_src()
    from hyperspace_amd.exec.encoding import GroupedCompact, encode
    from hyperspace_amd.ops import _lib as NL
    if group.startswith("q3g"):
        return G.q3_params(int(group[3:]))
    if group == "headline":
        from test_bits_cand_keep import _headline_params
        return _headline_params()
    p, comp, keep = G.q3_params(1)
    if group == "left_grouped":
        p.group_col, p.num_groups, p.group_base = 1, 16, 9000
    elif group == "plain_pred_col":
        del comp[9]
    elif group in ("nullable_pred_col", "nullable_key"):
        sl = 9 if group == "nullable_pred_col" else 8
        n = len(keep[1][0])
        c = _nullable(np.random.default_rng(3).integers(8000, 10000, n).astype(np.int32)
                      if sl == 9 else np.arange(1, n + 1, dtype=np.int64) * 4)
        p.cols[sl] = c.desc()
        e = encode(c)
        comp.pop(sl, None)
        if e is not None:
            comp[sl] = e
        keep = (keep, c)
    elif group == "grouped_key":
        c = comp[8]
        comp[8] = GroupedCompact(None, None, None, c.base, c.logical_type, c.lo, c.hi)
    elif group == "lt_pred":
        p.preds[0] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 1, 0, 0, 0, 9000, 0.0, None)
    else:
        raise KeyError(group)
    return p, comp, keep


def cases(group: str):
    """Yield (case key, thunk generating the kernel) of ``group``; a thunk runs inside its
    ``kernel_config.use``."""
    from hyperspace_amd.exec import jit_runs, kernel_config

    # (a group's parameters and compact columns are built once: they depend on no tunable, and
    # the generators do not change them)
    @functools.lru_cache(maxsize=None)
    def shape_params():
        return shape(group)

    def under(cfg, fn):
        def run():
            with kernel_config.use(**cfg):
                return fn(*shape_params()[:2])
        return run

    def settings(p, comp):
        """(ix32, mode, prune, k16, pair) under the bound tunables."""
        W = jit_runs.tag_width(p)
        for ix32, mode in itertools.product((True, False), MODES):
            if (mode in ("rec", "lo16", "lo16prep") and not ix32) or \
                    (mode == "copy" and not jit_runs.copy_ok(p, comp)):
                continue
            plan = jit_runs.prune_plan(p, comp, W) if mode == "" else ()
            for prune in ((), plan) if plan else ((),):
                for k16 in (False, True) if jit_runs.tags2_k16(p, comp, ix32, mode) else (False,):
                    for pair in (False, True) \
                            if jit_runs.tags2_pair(p, comp, W, ix32, mode, k16) else (False,):
                        yield ix32, mode, prune, k16, pair

    for vs in itertools.product(*[v for _, v in SWEEP]):
        cfg = dict(zip([n for n, _ in SWEEP], vs))
        with kernel_config.use(**cfg):
            todo = list(settings(*shape_params()[:2]))
        for ix32, mode, prune, k16, pair in todo:
            key = (f"{cfg_key(cfg)};ix32={int(ix32)},mode={mode or '-'},prune={int(bool(prune))},"
                   f"k16={int(k16)},pair={int(pair)}")
            yield key, under(cfg, lambda p, comp, a=(ix32, mode, prune, k16, pair):
                             jit_runs.gen_run_tags2(p, comp, jit_runs.tag_width(p), *a))
    yield "gather", under({}, jit_runs.gen_match_gather)


def generate(group: str):
    """``source_manifest.generate`` over ``group``."""
    return S.generate(cases(group))


if __name__ == "__main__":
    S.main(__doc__, GROUPS, cases)
