"""Record what the bit-parallel phase-2 generator (``jit_runs.gen_run_sparse_scan``) and
``gen_run_scan`` emit, as hashes, so that a restructuring of the generators can be checked byte
for byte on the CPU (``tests/test_bits_scan_sources.py`` against
``tests/golden/bits_scan_sources.json``):

    python scripts/dev/bits_scan_manifest.py [--root TREE] --out FILE

``--root``: the tree ``hyperspace_amd``, ``tests`` and ``scripts/dev/gen_join_src`` are imported
from (default: this file's), so the manifest of another commit is
``git worktree add ../parent <commit>`` and ``--root ../parent``.

Cases, by group (one test case each):

* ``headline/{stream,cand,cand2}`` and ``q3/{stream,hash,topk}``: the product of the nine phase-2
  tunables (``SWEEP``); the candidate forms where ``prune_plan`` / ``pack_layout`` / ``cand_pair``
  allow them under the setting.
* ``extra/<shape>``: streaming sources of four shapes that reach branches the two above do not
  (left-grouped, a float predicate, a plain predicate column, a nullable one) under ``EXTRA_CFGS``.
* ``scan/q3g3``: one ``gen_run_scan`` source (the argument header it shares).

The record per case and the file form: ``source_manifest.py``.  A group's cases come in the
order ``cases(group)`` yields them (the base groups: ``itertools.product`` over ``SWEEP``, last
setting fastest).
"""
import functools
import itertools

import source_manifest as S
from source_manifest import cfg_key

SWEEP = (("rs_keep", (True, False)), ("rs_lut", (True, False)), ("rs_pipe", (0, 1, 2)),
         ("rs_lds", (False, True)), ("rs_pk16", (True, False)), ("rs_pack12", (True, False)),
         ("rs_walk", (1, 4)), ("rs_pack", (True, False)), ("rs_waves", (0, 6)))
EXTRA_CFGS = ({}, {"rs_pack12": False}, {"rs_pack12": False, "rs_pk16": False},
              {"rs_pack12": False, "rs_lds": True}, {"rs_pipe": 2, "rs_pack12": False})
BASE_GROUPS = ("headline/stream", "headline/cand", "headline/cand2",
               "q3/stream", "q3/hash", "q3/topk")
EXTRA_GROUPS = ("extra/left_grouped", "extra/float_pred", "extra/plain_pred_col",
                "extra/nullable_pred_col")
GROUPS = BASE_GROUPS + EXTRA_GROUPS + ("scan/q3g3",)


def _extra_shape(group: str):
    """(params, compacts, objects to keep alive) of an ``extra/`` group."""
    import numpy as np
    import pyarrow as pa
    G = S.gen_join_src()
    from hyperspace_amd.exec.device_table import DeviceColumn
    from hyperspace_amd.exec.encoding import encode
    from hyperspace_amd.ops import _lib as NL
    p, comp, keep = G.q3_params(1)
    if group == "extra/left_grouped":
        p.group_col, p.num_groups, p.group_base = 1, 16, 9000
    elif group == "extra/float_pred":
        p.preds[0] = NL.Pred(NL.PK_FLT_LIT, NL.OP_GT, 2, 0, 0, 0, 0, 5000.0, None)
    elif group == "extra/plain_pred_col":
        del comp[1]
    elif group == "extra/nullable_pred_col":
        n = len(keep[0][1])
        rng = np.random.default_rng(2)
        c = DeviceColumn.from_arrow(pa.array(rng.integers(8000, 10000, n).astype(np.int32),
                                             mask=rng.random(n) < 0.1), "cpu")
        p.cols[1] = c.desc()
        e = encode(c)
        comp.pop(1, None)
        if e is not None:
            comp[1] = e
        keep = (keep, c)
    else:
        raise KeyError(group)
    return p, comp, keep


def cases(group: str):
    """Yield (configuration key, thunk generating the kernel) of ``group``; a thunk runs inside
    its ``kernel_config.use`` and returns None where the form does not apply."""
    import types
    import pyarrow as pa
    G = S.gen_join_src()
    from hyperspace_amd.exec import hash_agg as H
    from hyperspace_amd.exec import jit_runs, kernel_config
    from hyperspace_amd.ops import _lib as NL

    # (a group's parameters and compact columns are built once: they depend on no tunable, and
    # the generators do not change them)
    @functools.lru_cache(maxsize=None)
    def shape_params():
        if shape == "headline":
            from test_bits_cand_keep import _headline_params
            return _headline_params()
        return _extra_shape(group) if shape == "extra" else G.q3_params(3)

    def headline(form):
        p, comp, _keep = shape_params()
        if form == "stream":
            return jit_runs.gen_run_sparse_scan(p, comp)
        pr = jit_runs.prune_plan(p, comp, 1)
        cand = tuple(dict.fromkeys(sl for _, sl, _ in pr))
        if not cand or jit_runs.pack_layout(p, comp, cand) is None:
            return None
        if form == "cand":
            return jit_runs.gen_run_sparse_scan(p, comp, None, None, cand)
        if not jit_runs.cand_pair(p, comp, cand):
            return None
        return jit_runs.gen_run_sparse_scan(p, comp, None, None, cand, True)

    def q3(form):
        from test_jit import _q3_compacts, _q3_params
        j, jc = _q3_params(), _q3_compacts()
        if form == "stream":
            return jit_runs.gen_run_sparse_scan(j, jc)
        c = types.SimpleNamespace(hs_type=NL.I64, valid=None, dictionary=None, offsets=None,
                                  atype=pa.int64())
        hk = H.plan_keys([(0, None, c, (1, 600_000_000, None))], (False, False), False)
        tk = H.TopKPlan(0, False, True, 2, 16) if form == "topk" else None
        return jit_runs.gen_run_sparse_scan(j, jc, hk, tk)

    def extra():
        p, comp, _keep = shape_params()
        return jit_runs.gen_run_sparse_scan(p, comp)

    def scan():
        p, comp, _keep = shape_params()
        return jit_runs.gen_run_scan(p, comp, 2, jit_runs.RS_ITEMS)

    shape, form = group.split("/")
    if group in BASE_GROUPS:
        fn = {"headline": headline, "q3": q3}[shape]
        cfgs = [dict(zip([n for n, _ in SWEEP], vs))
                for vs in itertools.product(*[v for _, v in SWEEP])]
        thunk = lambda: fn(form)  # noqa: E731
    elif group in EXTRA_GROUPS:
        cfgs, thunk = list(EXTRA_CFGS), extra
    else:
        cfgs, thunk = [{}], scan

    def under(cfg):
        def run():
            with kernel_config.use(**cfg):
                return thunk()
        return run
    for cfg in cfgs:
        yield cfg_key(cfg), under(cfg)


def generate(group: str):
    """``source_manifest.generate`` over ``group``."""
    return S.generate(cases(group))


if __name__ == "__main__":
    S.main(__doc__, GROUPS, cases)
