"""Every source the streaming generators of ``exec/jit.py`` emit (``gen_scan_agg``,
``gen_join_index_agg``, ``gen_pred_bitmap``) and the consumers of their shared helpers
(``gen_join_agg``, ``gen_merge_join_agg``, ``jit_runs.gen_run_scan``) over the shapes, tunables and
generator arguments of ``scripts/dev/stream_manifest.py`` is the recorded one, byte for byte:
``tests/golden/stream_sources.json`` holds their hashes as that script wrote them on the commit
before the generators were split into stage emitters (``_Stream``).  A slip in a restructuring
would otherwise show only as a recompile on the device (the ahead-of-time set is looked up by
source hash) or as a wrong aggregate.

The manifest of any commit: ``git worktree add ../parent <commit>``, then
``python scripts/dev/stream_manifest.py --root ../parent --out FILE``.
"""
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts", "dev"))
try:
    import source_manifest as S
    import stream_manifest as M
finally:
    sys.path.pop(0)

# what the recorded sources must reach between them (searched after the shared prelude): the
# row-packed loads and their LDS transpose, the three list entry types, the join index's (row, j)
# list, staged columns with a validity byte, bitmap phase 2 and block-coded index, the pipelined
# tile loop, both list barriers, code-bound / reciprocal / exact decimal decodes, grouping, hash
# mode, a guard's ELSE constant, and the generic join's batch function and direct table
FEATURES = ("pload<", "ploadc<", "hs_pk_t<", "typedef u64 crow_t", "typedef unsigned int crow_t",
            "typedef unsigned short crow_t", "cj_s[", "st9_s", "sn9_s", "a.rbm", "a.jbase[",
            "fullP", "__syncthreads();", "__builtin_amdgcn_wave_barrier", "a.CL0", "a.R0", "a.Q",
            "group_base", "atomicCAS", "a.E0", "load_batch(", "dtab[")


def _manifest() -> dict:
    with open(os.path.join(HERE, "golden", "stream_sources.json")) as fh:
        return json.load(fh)


def test_manifest_covers_the_sweep():
    m = _manifest()
    assert tuple(m["cases"]) == M.GROUPS
    recs = [r for c in m["cases"].values() for r in c]
    assert len(recs) == 463 and len(m["sources"]) == 347
    # (cases, distinct sources) per group
    assert {g: (len(c), len({r for r in c if isinstance(r, int)}))
            for g, c in m["cases"].items()} == {
        "scan/float_inset": (24, 17), "scan/grouped_null": (24, 17), "scan/compact": (24, 17),
        "scan/q6": (30, 22), "scan/q6_wide": (7, 7), "scan/hk2": (24, 17), "scan/hk3": (6, 6),
        "scan/guard": (24, 17), "ji/mixed": (17, 10), "ji/mixed_g10": (57, 35),
        "ji/mixed_g1": (17, 10), "ji/q3c": (57, 48), "ji/q3": (17, 15), "ji/q3_nullable": (17, 15),
        "join_agg": (34, 33), "merge_join": (66, 47), "run_scan": (18, 18)}
    # every case applies; only the predicate bitmap of the three mixed shapes raises (its
    # left/right compare reads a slot the bitmap's column map drops; the engine never asks)
    assert [(g, r) for g, c in m["cases"].items() for r in c if not isinstance(r, int)] == \
        [(g, "!KeyError") for g in ("ji/mixed", "ji/mixed_g10", "ji/mixed_g1")]
    assert all(c[-1] == "!KeyError" for g, c in m["cases"].items() if g.startswith("ji/mixed"))
    assert sorted({r for r in recs if isinstance(r, int)}) == list(range(len(m["sources"])))
    assert {s[0] for s in m["sources"]} == {
        "hs_jit_scan_agg", "hs_jit_join_index_agg", "hs_jit_pred_bitmap", "hs_jit_join_agg",
        "hs_jit_merge_join_agg", "hs_jit_run_scan"}
    # no larger than the largest manifest that was in the tree before it
    assert os.path.getsize(os.path.join(HERE, "golden", "stream_sources.json")) <= 216_773


@pytest.mark.parametrize("group", M.GROUPS)
def test_sources_are_the_recorded_ones(group):
    from hyperspace_amd.exec import jit
    m = _manifest()
    assert hashlib.sha1(jit._PRELUDE.encode()).hexdigest() == m["prelude"], "jit._PRELUDE changed"
    want = m["cases"][group]
    got = list(M.generate(group))
    assert len(got) == len(want)
    bad = []
    for (key, rec, k), w in zip(got, want):
        w = m["sources"][w] if isinstance(w, int) else w
        if isinstance(rec, tuple) and isinstance(w, list):
            if list(rec[:4]) != w[:4]:
                bad.append(f"{group} [{key}]: " + S.first_difference(rec, w, k.src, jit._PRELUDE))
        elif rec != w:
            bad.append(f"{group} [{key}]: generated {rec and rec[:2]!r}, recorded {w and w[:2]!r}")
    assert not bad, f"{len(bad)} of {len(got)} cases differ; first: {bad[0]}"


def test_sources_reach_every_feature():
    """Each of ``FEATURES`` occurs in at least one generated source (with the sources equal to
    the recorded ones, above, the manifest covers them)."""
    from hyperspace_amd.exec import jit
    seen = set()
    for group in M.GROUPS:
        for _key, _rec, k in M.generate(group):
            if k is not None:
                body = k.src[len(jit._PRELUDE):]
                seen.update(f for f in FEATURES if f in body)
    assert not [f for f in FEATURES if f not in seen]
