"""tests/pq_ref.py (the reference the device page-decoder tests compare against) checked on the
CPU: every Snappy stream the builders and the generator make for test_pq_decode_kernels_gpu.py
decodes to its expected bytes with libsnappy (through pyarrow), with ``pq_ref.snappy_decode`` and
with the host decoder ``hs_pq_snappy_decompress`` (whose fast paths otherwise only see
pyarrow-shaped data); every malformed stream is refused by all three; the hybrid codec round-trips;
and the hand-built pages decode through ``native_parquet.decode_plan_host`` to what pq_ref
expects."""
import functools

import numpy as np
import pyarrow as pa
import pytest

import pq_ref as R
from hyperspace_amd.io import native_parquet as NP


@functools.lru_cache(maxsize=None)
def _window():
    from hyperspace_amd.ops import kernels as K
    return K.pq_snappy_window()


def _libsnappy(stream, size):
    return pa.decompress(stream, decompressed_size=size, codec="snappy", asbytes=True)


def _host(stream, cap):
    """(return value of the host decoder, its output buffer)."""
    src = np.frombuffer(bytes(stream) + b"\0", dtype=np.uint8)[:len(stream)]
    out = np.full(cap + 64, R.SENTINEL, dtype=np.uint8)
    got = NP.lib().hs_pq_snappy_decompress(src.ctypes.data, len(stream), out.ctypes.data, cap)
    return int(got), out


def _check_valid(cases):
    bad = []
    for name, stream, want in cases:
        n = len(want)
        if n and _libsnappy(stream, n) != want:
            bad.append((name, "libsnappy"))
        if R.snappy_decode(stream) != want:
            bad.append((name, "pq_ref"))
        got, out = _host(stream, n)
        # short moves may overrun by < 64 bytes into the caller's slack, never past it
        if got != n or out[:n].tobytes() != want:
            bad.append((name, "host"))
    assert not bad, bad


def test_window_accessor():
    assert _window() >= 64 and _window() % 64 == 0


def test_directed_streams_decode_everywhere():
    cases = R.inflate_streams(_window())
    assert len({c[0] for c in cases}) == len(cases)
    _check_valid(cases)


def test_empty_output_stream():
    assert R.snappy_decode(b"\x00") == b""
    assert _host(b"\x00", 0)[0] == 0


def test_random_streams_decode_everywhere():
    cases = R.random_streams()
    assert len(cases) >= 200
    _check_valid(cases)
    # the generator reaches what no common compressor emits: every copy kind, every width of
    # literal length field, and nothing else in the profiles without copy-4
    seen = {t for c in cases for t in R.tags(c[1])}
    assert seen == {(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (2, 3), (3, 5)}
    assert not any(t == (3, 5) for c in cases if "-text-" in c[0] or "-rle-" in c[0]
                   for t in R.tags(c[1]))


def test_long_literal_streams_decode_everywhere():
    rng = np.random.default_rng(5)
    cases = []
    for lead in range(4):
        for mis in range(4):
            for n in R.LONG_LITERAL_LENGTHS:
                s, want = R.long_literal_stream(n, mis, lead, rng)
                assert (lead + len(s) - n) % 4 == mis
                cases.append((f"long-literal-{n}-lead{lead}-in{mis}", s, want))
    _check_valid(cases)


def test_malformed_streams_are_refused_everywhere():
    bad = []
    for name, stream, usize in R.malformed_streams():
        ref = R.snappy_decode(stream)
        got, _ = _host(stream, usize)
        if name.startswith("preamble-"):
            # a valid stream of another size than the page header promises: the page is corrupt
            assert ref is not None and len(ref) != usize and got != usize, name
            continue
        if ref is not None:
            bad.append((name, "pq_ref", ref))
        if got >= 0:
            bad.append((name, "host", got))
        try:
            _libsnappy(stream, usize)
            bad.append((name, "libsnappy"))
        except (pa.ArrowInvalid, pa.ArrowIOError, OSError, ValueError):
            pass
    assert not bad, bad


def test_builder_rejects_what_it_cannot_expect():
    with pytest.raises(AssertionError):
        R.Snappy().literal(b"ab").copy(1, 3, 4)
    with pytest.raises(AssertionError):
        R.copy(1, 4, 12)


@pytest.mark.parametrize("bw", R.BIT_WIDTHS)
def test_hybrid_round_trip(bw):
    rng = np.random.default_rng(bw)
    top = (1 << bw) - 1
    val = lambda n: [int(x) for x in rng.integers(0, top, n, endpoint=True)]
    runs = [("rle", 3, top), ("packed", val(8)), ("rle", 0, val(1)[0]), ("rle", 1, val(1)[0], 2),
            ("packed", val(21), 1), ("rle", 200, val(1)[0]), ("packed", val(512)),
            ("rle", 20000, top)]
    want = R.expand_runs(runs, 3 + 8 + 1 + 21)
    for pad in (0, 1):
        s = R.hybrid_encode(runs, bw, pad)
        assert np.array_equal(R.hybrid_decode(s, bw, len(want)), want)
    n = 3 + 8 + 1 + 24 + 200 + 512 + 700          # the padded group counts, the last run clamped
    full = R.hybrid_decode(R.hybrid_encode(runs, bw), bw, n)
    vals = [x for r in runs[:7] for x in ([r[2]] * r[1] if r[0] == "rle"
                                          else list(r[1]) + [0] * (-len(r[1]) % 8))]
    assert list(full) == vals + [top] * 700
    # against the project's host hybrid decoder too
    host = NP._hybrid_host(np.frombuffer(R.hybrid_encode(runs, bw), np.uint8), bw, n)
    assert np.array_equal(host, full)
    assert R.hybrid_decode(R.hybrid_encode(runs, bw)[:-1], bw, n) is None or bw == 0


def test_hybrid_header_widths():
    assert R.hybrid_encode([("rle", 100, 1)], 1) == bytes([0xC8, 0x01, 0x01])
    assert len(R.varint(10000 << 1)) == 3
    assert R.hybrid_encode([("rle", 3, 1, 1)], 1) == bytes([0x86, 0x00, 0x01])
    assert R.hybrid_encode([("packed", [1, 0, 1])], 1) == bytes([0x03, 0x05])
    assert R.pack_bits([1, 2, 3], 3) == bytes([0b11010001, 0b0])


def _through_host_oracle(pages):
    """Decode ``pages`` (valid, fixed-width or BOOLEAN) with decode_plan_host; the mismatches."""
    raw = bytearray()
    flat, index = [], {}
    for p in pages:
        for q in ((p.dict, p) if p.dict is not None else (p,)):
            if id(q) not in index:
                index[id(q)] = len(flat)
                flat.append(q)
    tab = np.zeros(len(flat), dtype=NP.PAGE_DTYPE)
    outs, valids = {}, {}
    for i, q in enumerate(flat):
        for k, v in q.fields.items():
            tab[i][k] = v
        tab[i]["src"] = len(raw)
        raw += q.src
        tab[i]["out"] = tab[i]["valid"] = i
        if q.dict is not None:
            tab[i]["dict_page"] = index[id(q.dict)]
        if q.fields["kind"] != 2:
            dt = {1: np.uint8, 4: np.uint32, 8: np.uint64}[q.fields["eb"]]
            outs[i] = np.full(q.fields["nvals"], 0x5A, dtype=dt)
            valids[i] = np.full(q.fields["nvals"], 0x5A, dtype=np.uint8)
    NP.decode_plan_host(np.frombuffer(bytes(raw), np.uint8), tab, outs, None, valids)
    bad = []
    for i, q in enumerate(flat):
        if q.fields["kind"] == 2:
            continue
        if outs[i].tobytes() != q.out:
            bad.append((q.name, "values"))
        if q.valid is not None and not np.array_equal(valids[i], q.valid):
            bad.append((q.name, "validity"))
    return bad


def test_pages_through_host_oracle():
    pages = R.dictionary_cases() + R.plain_cases() + R.bool_cases() + \
        [p for p in R.null_cases() if p.fields["eb"] != 16]
    assert _through_host_oracle(pages) == []


def test_snappy_pages_through_host_oracle():
    rng = np.random.default_rng(6)
    pages = []
    for name, stream, want in R.inflate_streams(_window())[:80] + R.random_streams(3):
        for version, prefix in ((1, None), (2, 3)):
            body = want[:len(want) // 4 * 4]
            if len(body) != len(want):
                continue
            pages.append(R.assemble(f"{name}-v{version}", body, len(body) // 4, 4, 0,
                                    version=version, prefix=prefix, codec=1, stream=stream,
                                    rng=rng, out=body))
    assert len(pages) > 20
    assert _through_host_oracle(pages) == []


def test_string_pages_parse_on_the_host():
    for p in R.string_cases():
        if p.valid is not None:
            continue
        n = p.fields["nvals"]
        base = int(p.out[0]) - 4
        body = np.frombuffer(p.scratch[base:], np.uint8)
        arr = NP.plain_strings(body.ctypes.data, len(body), n)
        got = [s.as_py().encode() for s in arr]
        want = [p.scratch[int(o):int(o) + int(ln)] for o, ln in zip(p.out, p.lens)]
        assert got == want, p.name
