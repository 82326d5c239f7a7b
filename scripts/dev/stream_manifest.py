"""Record what the streaming kernel generators of ``exec/jit.py`` emit - ``gen_scan_agg``,
``gen_join_index_agg``, ``gen_pred_bitmap`` - and the consumers of the helpers they share
(``gen_join_agg``, ``jit_join.gen_merge_join_agg``, ``jit_runs.gen_run_scan``), as hashes, so
that a restructuring of the generators can be checked byte for byte on the CPU
(``tests/test_stream_sources.py`` against ``tests/golden/stream_sources.json``):

    python scripts/dev/stream_manifest.py [--root TREE] --out FILE

``--root``: the tree ``hyperspace_amd``, ``tests`` and ``scripts/dev/gen_join_src`` are imported
from (default: this file's), so the manifest of another commit is
``git worktree add ../parent <commit>`` and ``--root ../parent``.  Host metadata only: the
columns are fake descriptors, nothing is compiled or launched.

Groups (one test case each) and their cases, in the order ``cases(group)`` yields them:

* ``scan/<shape>``: ``gen_scan_agg`` on the shapes of ``scan_shape`` under ``SCAN_CFGS``, ``vec``
  in (0, 8, 16), and where ``scan_pack_layout`` gives a layout under the setting, packed too.
* ``ji/<shape>``: ``gen_join_index_agg`` under ``JI_CFGS``; on the two ``JI_FULL`` shapes ``vec``
  in (0, 4, 8, 16) x (jw, jlog) in ((4, 0), (2, 8), (1, 7)) x {plain, stage, bitmap} under the
  defaults, on the others and under every other setting ``vec`` in (0, 8) x ((4, 0), (1, 7))
  (x {plain, stage, bitmap} under the defaults only); last, one ``gen_pred_bitmap`` source (the
  three mixed shapes raise there: their left/right compare reads a slot the bitmap's column map
  drops, which the engine never asks for).
* ``join_agg``: ``gen_join_agg`` on the join shapes (the first with a float key too) under
  ``JA_CFGS``.
* ``merge_join``: ``gen_merge_join_agg`` on ``MJ_VARIANTS`` under ``MJ_CFGS``.
* ``run_scan``: ``gen_run_scan`` of ``gen_join_src.q3_params(1 | 3 | 200)`` at ``NI`` 8 and 16
  under ``RS_CFGS``.

Every ``*_CFGS`` is the defaults, each tunable of the family one step away from its default, and
the corner with every boolean one off - not their product; the shapes in ``CORNERS_ONLY`` take
the defaults and that corner only (the full product is some 1100 distinct sources, three times
the largest manifest in the tree).  The record per case and the file form:
``source_manifest.py``.
"""
import functools

import source_manifest as S
from source_manifest import cfg_key


def _sweep(alts: dict) -> tuple:
    """The defaults, one knob of ``alts`` away from them at a time, and every boolean off."""
    return ({},) + tuple({k: v} for k, v in alts.items()) + \
        ({k: False for k, v in alts.items() if isinstance(v, bool)},)


SCAN_CFGS = _sweep({"scan_items": 2, "scan_compact": False, "scan_eager": True,
                    "scan_pack_lds": True, "vec_prefetch": False, "wave_sync": False})
JI_CFGS = _sweep({"ji_items": 2, "ji_compact": False, "vec_prefetch": False, "wave_sync": False})
JA_CFGS = _sweep({"join_eager": True, "join_stage_right": False, "join_pipeline": False,
                  "join_direct": True})
MJ_CFGS = _sweep({"mj_prefetch": True, "mj_rpf": True, "mj_eager": True, "mj_dbuf": True,
                  "mj_sparse": False, "mj_runs_prefetch": True, "mj_hash_lanemajor": True,
                  "mj_steps": 2})
RS_CFGS = ({}, {"vec_prefetch": False}, {"wave_sync": False})

SCAN_SHAPES = ("float_inset", "grouped_null", "compact", "q6", "q6_wide", "hk2", "hk3", "guard")
JOIN_SHAPES = ("mixed", "mixed_g10", "mixed_g1", "q3c", "q3", "q3_nullable")
JI_FULL = ("q3c", "mixed_g10")
# shapes that differ from a swept one in a branch no tunable touches: defaults and corner only
CORNERS_ONLY = ("scan/q6_wide", "scan/hk3", "ji/mixed", "ji/mixed_g1", "ji/q3", "ji/q3_nullable",
                "join_agg/mixed_g1", "join_agg/q3", "merge_join/float_key", "merge_join/key16",
                "merge_join/hash_plain")
MJ_VARIANTS = ("plain", "grouped", "float_key", "compact", "image32", "key16", "runs",
               "hash_compact", "hash_plain")
GROUPS = tuple(f"scan/{s}" for s in SCAN_SHAPES) + tuple(f"ji/{s}" for s in JOIN_SHAPES) + \
    ("join_agg", "merge_join", "run_scan")


def _key_col(t, valid=False):
    import types
    import pyarrow as pa
    return types.SimpleNamespace(hs_type=t, valid=1 if valid else None, dictionary=None,
                                 offsets=None, atype=pa.int64())


def scan_shape(name: str):
    """(ScanParams, compact columns, hash key plan) of a scan shape: those of
    ``tests/test_jit.py``'s compile checks, the headline Q6 (and its variant whose list entries
    need 64 bits), the two hash-key shapes and the CASE WHEN guard shape."""
    from hyperspace_amd.exec import hash_agg as H
    from hyperspace_amd.exec.encoding import Compact
    from hyperspace_amd.ops import _lib as NL
    from test_jit import _agg, _fake, _scan_params
    if name == "float_inset":
        return _scan_params(
            {0: _fake(NL.I32), 1: _fake(NL.F64), 2: _fake(NL.F64, True), 3: _fake(NL.F64)},
            [NL.Pred(NL.PK_FLT_LIT, NL.OP_GE, 1, 0, 0, 0, 0, 0.05, None),
             NL.Pred(NL.PK_FLT_LIT, NL.OP_LT, 2, 0, 1, 0, 0, 24.0, None),
             NL.Pred(NL.PK_INT_LIT, NL.OP_EQ, 0, 0, 2, 0, 7, 0.0, None),
             NL.Pred(NL.PK_IN_SET, NL.OP_NE, 0, 0, 2, 3, 0, 0.0, 0x5000)],
            [_agg(NL.AK_SUM, [(3, 0.0, 1.0), (1, 1.0, -1.0)]), _agg(NL.AK_COUNT_STAR)]), None, None
    if name == "grouped_null":
        return _scan_params(
            {0: _fake(NL.I64, True), 1: _fake(NL.F32), 2: _fake(NL.BOOL)},
            [NL.Pred(NL.PK_IS_NULL, 0, 0, 0, 0, 0, 0, 0.0, None),
             NL.Pred(NL.PK_INT_COL, NL.OP_LT, 0, 2, 0, 0, 0, 0.0, None),
             NL.Pred(NL.PK_BITMAP, NL.OP_NE, 0, 0, 1, 4, 0, 0.0, 0x6000)],
            [_agg(NL.AK_MIN, [(1, 0.0, 1.0)]), _agg(NL.AK_MAX, [(1, 0.0, 2.0)]),
             _agg(NL.AK_COUNT, [(0, 0.0, 1.0)])], group_col=2, num_groups=2), None, None
    if name == "compact":
        p = _scan_params({0: _fake(NL.F64), 1: _fake(NL.F64), 2: _fake(NL.I64, True)},
                         [NL.Pred(NL.PK_FLT_LIT, NL.OP_GE, 0, 0, 0, 0, 0, 0.05, None),
                          NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 2, 0, 1, 0, 9, 0.0, None)],
                         [_agg(NL.AK_SUM, [(1, 0.0, 1.0), (0, 1.0, -1.0)])])
        return p, {0: Compact(None, 1, 0, 100.0, NL.F64), 1: Compact(None, 4, 0, 100.0, NL.F64),
                   2: Compact(None, 2, 5, None, NL.I64)}, None
    if name in ("q6", "q6_wide"):
        from test_scan_pack import _compact, _q6_params
        p, comp = _q6_params()
        if name == "q6_wide":
            comp[0] = _compact(2, 0, 1000, 100.0)
        return p, comp, None
    if name in ("hk2", "hk3"):
        p = _scan_params({0: _fake(NL.I64, True), 1: _fake(NL.F64), 2: _fake(NL.F32),
                          3: _fake(NL.F64)},
                         [NL.Pred(NL.PK_FLT_LIT, NL.OP_GE, 1, 0, 0, 0, 0, 0.05, None)],
                         [_agg(NL.AK_SUM, [(3, 0.0, 1.0)]), _agg(NL.AK_MIN, [(3, 0.0, 1.0)]),
                          _agg(NL.AK_MAX, [(3, 0.0, 1.0)]), _agg(NL.AK_COUNT_STAR)])
        if name == "hk2":
            hk = H.plan_keys([(0, None, _key_col(NL.I64, True), (-5, 100, None)),
                              (1, None, _key_col(NL.F64), (0, 11, 100.0)),
                              (2, None, _key_col(NL.F32), (0, 0, None))],
                             (False, False, False, False), True)
        else:
            hk = H.plan_keys([(3, None, _key_col(NL.F64), (0, 0, 0.0))],
                             (False, False, False, False))
        return p, None, hk
    if name == "guard":
        from test_case_when import _scan_case
        return _scan_case(), {0: Compact(None, 2, 0, None, NL.I32),
                              1: Compact(None, 1, 0, 100.0, NL.F64),
                              3: Compact(None, 4, 0, 100.0, NL.F64),
                              4: Compact(None, 2, 5, None, NL.I32)}, None
    raise KeyError(name)


def join_shape(name: str):
    """(JoinParams, compact columns) of a join shape: the mixed shape of ``tests/test_jit.py``
    (a left/right column compare, a nullable aggregate input and group column) ungrouped and
    grouped by slot 10 and slot 1, and the Q3 shape with compact columns, without, and with a
    nullable right predicate column."""
    from hyperspace_amd.ops import _lib as NL
    from test_jit import _agg, _fake, _q3_compacts, _q3_params
    if name.startswith("mixed"):
        j = NL.JoinParams()
        j.cols[0], j.cols[1], j.cols[2] = _fake(NL.I64), _fake(NL.I32), _fake(NL.F64, True)
        j.cols[8], j.cols[9], j.cols[10] = _fake(NL.I64), _fake(NL.I32), _fake(NL.I32, True)
        j.preds[0] = NL.Pred(NL.PK_INT_LIT, NL.OP_GT, 1, 0, 0, 0, 9000, 0.0, None)
        j.preds[1] = NL.Pred(NL.PK_INT_LIT, NL.OP_LT, 9, 0, 1000, 0, 9000, 0.0, None)
        j.preds[2] = NL.Pred(NL.PK_INT_COL, NL.OP_LT, 1, 9, 1001, 0, 0, 0.0, None)
        j.nlp, j.npreds = 1, 3
        j.aggs[0] = _agg(NL.AK_SUM, [(2, 0.0, 1.0), (2, 1.0, -1.0)])
        j.aggs[1] = _agg(NL.AK_COUNT_STAR)
        j.naggs, j.lkey, j.rkey, j.key_is_float = 2, 0, 8, 0
        j.group_col, j.num_groups = {"mixed": -1, "mixed_g10": 10, "mixed_g1": 1}[name], 3
        return j, None
    j = _q3_params()
    if name == "q3_nullable":
        j.cols[9] = _fake(NL.I32, True)
    return j, (None if name == "q3" else _q3_compacts())


def _float_key(j):
    from hyperspace_amd.ops import _lib as NL
    f = NL.JoinParams.from_buffer_copy(j)
    f.key_is_float = 1
    return f


def merge_join_variant(name: str):
    """(JoinParams, compact columns, hash key plan) of a ``gen_merge_join_agg`` variant that
    ``tests/test_jit.py`` builds."""
    import torch
    from hyperspace_amd.exec import hash_agg as H
    from hyperspace_amd.exec.encoding import Compact, GroupedCompact, RunCompact
    from hyperspace_amd.ops import _lib as NL
    from test_jit import _fake, _q3_compacts, _q3_params
    if name in ("plain", "grouped", "float_key"):
        j, _ = join_shape("mixed_g10" if name == "grouped" else "mixed")
        return (_float_key(j) if name == "float_key" else j), None, None
    if name == "compact":
        return _q3_params(), _q3_compacts(), None
    c32 = dict(_q3_compacts())
    c32[0] = Compact(None, 4, 1 + (1 << 31), None, NL.I64, 1, 600_000_000)
    c32[8] = Compact(None, 4, 1 + (1 << 31), None, NL.I64, 1, 600_000_000)
    if name == "image32":
        return _q3_params(), c32, None
    if name == "key16":
        c32[0] = GroupedCompact(None, None, None, 1 + (1 << 31), NL.I64, 1, 600_000_000)
        return _q3_params(), c32, None
    if name == "runs":
        c32[0] = RunCompact(c32[0], torch.zeros(1, dtype=torch.int32),
                            torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
        return _q3_params(), c32, None
    if name in ("hash_compact", "hash_plain"):
        j = _q3_params()
        j.cols[10] = _fake(NL.I32)
        hk = H.plan_keys([(0, None, _key_col(NL.I64), (1, 600_000_000, None)),
                          (9, None, _key_col(NL.I32), (8000, 2500, None)),
                          (10, None, _key_col(NL.I32), (0, 1, None))], (False, False), False)
        return j, (c32 if name == "hash_compact" else None), hk
    raise KeyError(name)


def _cfgs(cfgs: tuple, what: str) -> tuple:
    return (cfgs[0], cfgs[-1]) if what in CORNERS_ONLY else cfgs


def _ji_settings(full: bool, variants: bool):
    """(vec, jw, jlog, stage, bitmap) of a join-index group under one setting."""
    for vec in (0, 4, 8, 16) if full else (0, 8):
        for jw, jlog in ((4, 0), (2, 8), (1, 7)) if full else ((4, 0), (1, 7)):
            for stage, bitmap in ((False, False), (True, False), (False, True)):
                if variants or not (stage or bitmap):
                    yield vec, jw, jlog, stage, bitmap


def cases(group: str):
    """Yield (case key, thunk generating the kernel) of ``group``; a thunk runs inside its
    ``kernel_config.use``."""
    from hyperspace_amd.exec import jit, jit_runs, kernel_config

    def under(cfg, fn):
        def run():
            with kernel_config.use(**cfg):
                return fn()
        return run

    # (a shape's parameters are built once: they depend on no tunable, and the generators do
    # not change them)
    shape = functools.lru_cache(maxsize=None)(
        lambda kind, name: {"scan": scan_shape, "join": join_shape,
                            "mj": merge_join_variant}[kind](name))
    fam, _, name = group.partition("/")
    if fam == "scan":
        p, comp, hk = shape("scan", name)
        for cfg in _cfgs(SCAN_CFGS, group):
            for vec in (0, 8, 16):
                yield f"{cfg_key(cfg)};vec={vec}", under(
                    cfg, lambda vec=vec: jit.gen_scan_agg(p, comp, vec, hk))
                with kernel_config.use(**cfg):
                    lay = jit.scan_pack_layout(p, comp, vec, hk)
                if lay is not None:
                    yield f"{cfg_key(cfg)};vec={vec},pack", under(
                        cfg, lambda vec=vec, lay=lay: jit.gen_scan_agg(p, comp, vec, hk, lay))
    elif fam == "ji":
        j, comp = shape("join", name)
        for cfg in _cfgs(JI_CFGS, group):
            for vec, jw, jlog, stage, bitmap in _ji_settings(name in JI_FULL and not cfg, not cfg):
                yield (f"{cfg_key(cfg)};vec={vec},jw={jw},jlog={jlog},stage={int(stage)},"
                       f"bitmap={int(bitmap)}"), under(
                    cfg, lambda a=(vec, jw, jlog, stage, bitmap):
                    jit.gen_join_index_agg(j, comp, *a))
        yield "pred_bitmap", under({}, lambda: jit.gen_pred_bitmap(j, comp))
    elif group == "join_agg":
        for name in JOIN_SHAPES:
            j, comp = shape("join", name)
            for fl in (False, True) if name == "mixed" else (False,):
                jj = _float_key(j) if fl else j
                for cfg in _cfgs(JA_CFGS, f"{group}/{name}"):
                    yield f"{name},float={int(fl)};{cfg_key(cfg)}", under(
                        cfg, lambda jj=jj, comp=comp: jit.gen_join_agg(jj, comp))
    elif group == "merge_join":
        for name in MJ_VARIANTS:
            for cfg in _cfgs(MJ_CFGS, f"{group}/{name}"):
                yield f"{name};{cfg_key(cfg)}", under(
                    cfg, lambda name=name: jit.gen_merge_join_agg(*shape("mj", name)))
    elif group == "run_scan":
        G = S.gen_join_src()
        q3 = functools.lru_cache(maxsize=None)(G.q3_params)
        for ng in (1, 3, 200):
            for NI in (8, 16):
                for cfg in RS_CFGS:
                    yield f"groups={ng},NI={NI};{cfg_key(cfg)}", under(
                        cfg, lambda ng=ng, NI=NI: jit_runs.gen_run_scan(
                            q3(ng)[0], q3(ng)[1], jit_runs.tag_width(q3(ng)[0]), NI))
    else:
        raise KeyError(group)


def generate(group: str):
    """``source_manifest.generate`` over ``group``."""
    return S.generate(cases(group))


if __name__ == "__main__":
    S.main(__doc__, GROUPS, cases)
