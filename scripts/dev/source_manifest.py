"""What the generated-source manifests (``bits_scan_manifest.py``, ``tags2_manifest.py``,
``stream_manifest.py``) share: importing the tree under test, the per-case record, the
enumeration into a manifest and its file form.

Per case the kernel name, sha1 of the source, sha1 of ``repr(args.slots)`` and ``lds_bytes`` - or
``!<exception type>`` if generation raises, or null where the form does not apply under the
setting.  A group's cases are a list in the order its ``cases(group)`` yields them, each an index
into the distinct sources, which are stored once; each of those also keeps one character per line
after the prelude (6 bits of the line's sha1), from which a mismatch names its first differing
line (a changed line goes unnoticed there with probability 1/64; the sha1 of the whole source
decides equality).
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def cfg_key(cfg: dict) -> str:
    return ",".join(f"{k}={int(v)}" for k, v in cfg.items()) or "default"


def use_tree(root: str) -> None:
    """Import ``hyperspace_amd`` and the tests' helpers from ``root``."""
    for d in (os.path.join(root, "tests"), root):
        if d in sys.path:
            sys.path.remove(d)
        sys.path.insert(0, d)


def gen_join_src():
    """``scripts/dev/gen_join_src`` of the tree ``hyperspace_amd`` comes from."""
    import hyperspace_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(hyperspace_amd.__file__)))
    sys.path.insert(0, os.path.join(root, "scripts", "dev"))
    try:
        import gen_join_src
    finally:
        sys.path.pop(0)
    return gen_join_src


def line_digest(src: str, prelude: str) -> str:
    assert src.startswith(prelude)
    return "".join(_B64[hashlib.sha1(x.encode()).digest()[0] & 63]
                   for x in src[len(prelude):].split("\n"))


def record(k, prelude: str) -> tuple:
    return (k.name, hashlib.sha1(k.src.encode()).hexdigest(),
            hashlib.sha1(repr(k.args.slots).encode()).hexdigest(), k.lds_bytes,
            line_digest(k.src, prelude))


def first_difference(got: tuple, want: list, src: str, prelude: str) -> str:
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


def generate(cases):
    """Yield (configuration key, ``record`` tuple | "!ExceptionType" | None, kernel | None) of
    the (key, thunk) pairs ``cases``; a thunk returns the kernel, or None where the form does
    not apply."""
    from hyperspace_amd.exec import jit
    for key, run in cases:
        try:
            k = run()
        except Exception as e:  # noqa: BLE001 — recorded: a case may raise on the parent too
            yield key, "!" + type(e).__name__, None
            continue
        yield key, (None if k is None else record(k, jit._PRELUDE)), k


def manifest(groups, cases) -> dict:
    from hyperspace_amd.exec import jit
    sources, index, out = [], {}, {}
    for group in groups:
        got = out[group] = []
        for _key, rec, _k in generate(cases(group)):
            if isinstance(rec, tuple):
                if rec not in index:
                    index[rec] = len(sources)
                    sources.append(list(rec))
                rec = index[rec]
            got.append(rec)
    return {"prelude": hashlib.sha1(jit._PRELUDE.encode()).hexdigest(),
            "sources": sources, "cases": out}


def write(m: dict, path: str) -> None:
    """One distinct source / one group per line."""
    dumps = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    with open(path, "w") as f:
        f.write('{"prelude":' + dumps(m["prelude"]) + ',\n"sources":[\n' +
                ",\n".join(dumps(s) for s in m["sources"]) + '],\n"cases":{\n' +
                ",\n".join(dumps(g) + ":" + dumps(c) for g, c in m["cases"].items()) + "}}\n")


def main(doc: str, groups, cases) -> None:
    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    use_tree(os.path.abspath(a.root))
    m = manifest(groups, cases)
    write(m, a.out)
    import hyperspace_amd
    assert os.path.abspath(hyperspace_amd.__file__).startswith(os.path.abspath(a.root) + os.sep)
    recs = [r for v in m["cases"].values() for r in v if r is not None]
    n, bad = len(recs), sum(isinstance(r, str) for r in recs)
    print(f"{n} cases, {len(m['sources'])} distinct sources, {bad} raised")
