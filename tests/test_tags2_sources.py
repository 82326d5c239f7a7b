"""Every source ``jit_runs.gen_run_tags2`` emits over the phase-1 tunables, modes and forms (and
one ``gen_match_gather`` source per shape) is the recorded one, byte for byte:
``tests/golden/tags2_sources.json`` holds their hashes as ``scripts/dev/tags2_manifest.py`` wrote
them on the commit before the generator was split into stage emitters (``_Tags2``).  A slip in a
restructuring would otherwise show only as a recompile on the device (the ahead-of-time set is
looked up by source hash) or as a wrong tag.

The manifest of any commit: ``git worktree add ../parent <commit>``, then
``python scripts/dev/tags2_manifest.py --root ../parent --out FILE``.
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
    import tags2_manifest as M
finally:
    sys.path.pop(0)

# what the recorded sources must reach between them: the pair's second bitmap, 16-bit key
# offsets, a grouped 16-bit right key, the record / recorded-match / copy / lo16 / lo16prep
# modes, the four-run form's staged column vectors, nullable right key and predicate column, both
# kinds of run bound, the W > 1 shuffle store and a right-side group key
FEATURES = ("tags_b", "a.LO16", "a.G8[", "a.MOUT", "a.MATCH", "a.HIT", "a.LL[", "NRIGHT",
            "hs_jit_key_lo16", "hs_c9x4", "a.v8", "a.v9", "a.RMX", "a.RMN", "__shfl((int)tg",
            "group_base")


def _manifest() -> dict:
    with open(os.path.join(HERE, "golden", "tags2_sources.json")) as fh:
        return json.load(fh)


def test_manifest_covers_the_sweep():
    m = _manifest()
    assert tuple(m["cases"]) == M.GROUPS
    recs = [r for c in m["cases"].values() for r in c]
    assert len(recs) == 1318 and len(m["sources"]) == 242
    assert {g: len(c) for g, c in m["cases"].items()} == {
        "q3g1": 145, "q3g3": 112, "q3g200": 112, "headline": 145, "left_grouped": 115,
        "plain_pred_col": 145, "nullable_pred_col": 133, "nullable_key": 133, "grouped_key": 133,
        "lt_pred": 145}
    # every case applies (the enumeration skips what the asserts forbid); nothing raised
    assert all(isinstance(r, int) for r in recs)
    assert sorted(set(recs)) == list(range(len(m["sources"])))
    names = {s[0] for s in m["sources"]}
    assert names == {"hs_jit_run_tags2", "hs_jit_key_lo16", "hs_jit_match_gather"}


def test_shapes_reach_the_bounds_and_forms():
    """The tenth shape exists for the ``RMN<slot>`` bound; the four-run, k16 and pair forms
    apply to the headline's shape."""
    from hyperspace_amd.exec import jit_runs, kernel_config
    p, comp, _keep = M.shape("lt_pred")
    plan = jit_runs.prune_plan(p, comp, 1)
    assert plan and not plan[0][2]
    p, comp, _keep = M.shape("headline")
    with kernel_config.use(rt2_wide=4, rt2_k16=True):
        assert jit_runs.tags2_pair(p, comp, 1, True, "", True)


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
    seen = set()
    for group in M.GROUPS:
        for _key, _rec, k in M.generate(group):
            seen.update(f for f in FEATURES if k is not None and f in k.src)
    assert not [f for f in FEATURES if f not in seen]
