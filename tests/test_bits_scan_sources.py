"""Every source ``jit_runs.gen_run_sparse_scan`` emits over the phase-2 tunables and forms (and
one ``gen_run_scan`` source) is the recorded one, byte for byte: ``tests/golden/bits_scan_sources.json``
holds their hashes as ``scripts/dev/bits_scan_manifest.py`` wrote them before the generator was
split into stage emitters.  A slip in a restructuring would otherwise show only as a recompile on
the device (the ahead-of-time set is looked up by source hash) or as a wrong sum.

The manifest of any commit: ``git worktree add ../parent <commit>``, then
``python scripts/dev/bits_scan_manifest.py --root ../parent --out FILE``.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts", "dev"))
try:
    import bits_scan_manifest as M
finally:
    sys.path.pop(0)


def _manifest() -> dict:
    with open(os.path.join(HERE, "golden", "bits_scan_sources.json")) as fh:
        return json.load(fh)


def _first_difference(got: tuple, want: list, src: str, prelude: str) -> str:
    """What differs between a generated record and the recorded one, down to the line."""
    for what, g, w in zip(("kernel name", "source sha1", "sha1 of args.slots", "lds_bytes"),
                          got, want):
        if g != w and what != "source sha1":
            return f"{what}: {g!r}, recorded {w!r}"
    a, b = got[4], want[4]
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    lines = src[len(prelude):].split("\n")
    return (f"source differs, first at line {n + 1} after the prelude ({len(a)} lines, recorded "
            f"{len(b)}): {lines[n] if n < len(lines) else '<end of source>'!r}")


def test_manifest_covers_the_sweep():
    m = _manifest()
    assert tuple(m["cases"]) == M.GROUPS
    n = 1
    for _, vs in M.SWEEP:
        n *= len(vs)
    assert n == 768 and all(len(m["cases"][g]) == n for g in M.BASE_GROUPS)
    assert all(len(m["cases"][g]) == len(M.EXTRA_CFGS) for g in M.EXTRA_GROUPS)
    recs = [r for c in m["cases"].values() for r in c if r is not None]
    assert len(recs) == 3669 and len(m["sources"]) == 423
    # the candidate forms exist where rs_pack (and, for the pair, rs_lut) is set; nothing raised
    applies = {g: sum(r is not None for r in m["cases"][g]) for g in M.BASE_GROUPS}
    assert applies == {"headline/stream": 768, "headline/cand": 384, "headline/cand2": 192,
                       "q3/stream": 768, "q3/hash": 768, "q3/topk": 768}
    assert not [r for r in recs if isinstance(r, str)]
    assert sorted({i for i in recs}) == list(range(len(m["sources"])))


@pytest.mark.parametrize("group", M.GROUPS)
def test_sources_are_the_recorded_ones(group):
    import hashlib
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
                bad.append(f"{group} [{key}]: " +
                           _first_difference(rec, w, k.src, jit._PRELUDE))
        elif rec != w:
            bad.append(f"{group} [{key}]: generated {rec and rec[:2]!r}, recorded {w and w[:2]!r}")
    assert not bad, f"{len(bad)} of {len(got)} cases differ; first: {bad[0]}"
