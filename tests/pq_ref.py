"""Plain reference for the device Parquet page decoder (csrc/kernels/parquet_decode.hip): pure
Python / numpy, no project imports.

* a Snappy *tag-stream builder* (not a compressor): ``literal`` / ``copy`` / ``preamble`` emit one
  element each, ``Snappy`` strings them together and builds the expected output alongside, byte by
  byte, so a test chooses every tag, length-field width and offset itself;
* ``snappy_decode``: the serial decoder, ``None`` for every stream libsnappy rejects;
* ``random_stream``: seeded random valid tag streams under a profile;
* ``hybrid_encode`` / ``hybrid_decode``: the RLE / bit-packed hybrid from an explicit run list;
* page builders: the bytes of one page and the fields of its page-table row;
* the directed case lists shared by test_pq_ref.py (CPU: anchors every stream to libsnappy
  through pyarrow and to the host decoder) and test_pq_decode_kernels_gpu.py.

test_pq_ref.py checks this file against pyarrow."""
import struct

import numpy as np

SENTINEL = 0xA5


# ------------------------------------------------------------------------------------------------
# varints and Snappy elements
# ------------------------------------------------------------------------------------------------
def varint(n, pad=0):
    """LEB128 of ``n``; ``pad`` extra bytes make it non-minimal (0x80 ... 0x00 continuation)."""
    assert n >= 0
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            break
    if pad:
        out[-1] |= 0x80
        out += bytes([0x80] * (pad - 1) + [0x00])
    return bytes(out)


def preamble(n, pad=0):
    return varint(n, pad)


def literal_header(length, length_bytes=None):
    """Header of a literal of ``length`` bytes; ``length_bytes`` 0 forces the inline form,
    1-4 a length field of that many bytes (non-minimal where a shorter one would do)."""
    m = length - 1
    assert m >= 0
    if length_bytes is None:
        length_bytes = 0 if m < 60 else (m.bit_length() + 7) // 8
    if length_bytes == 0:
        assert m < 60
        return bytes([m << 2])
    assert 1 <= length_bytes <= 4 and m < (1 << (8 * length_bytes))
    return bytes([(59 + length_bytes) << 2]) + m.to_bytes(length_bytes, "little")


def literal(data, length_bytes=None):
    return literal_header(len(data), length_bytes) + bytes(data)


def copy_legal(kind, offset, length):
    if kind == 1:
        return 4 <= length <= 11 and 0 <= offset < 2048
    if kind == 2:
        return 1 <= length <= 64 and 0 <= offset < 65536
    return kind == 3 and 1 <= length <= 64 and 0 <= offset < (1 << 32)


def copy(kind, offset, length):
    """One copy element; the offset is not checked against any output (0 and too-far offsets
    encode like any other, for the malformed cases)."""
    assert copy_legal(kind, offset, length), (kind, offset, length)
    if kind == 1:
        return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 0xFF])
    if kind == 2:
        return bytes([2 | ((length - 1) << 2)]) + offset.to_bytes(2, "little")
    return bytes([3 | ((length - 1) << 2)]) + offset.to_bytes(4, "little")


class Snappy:
    """A tag stream under construction with its expected output."""

    def __init__(self):
        self.body = bytearray()      # the elements after the preamble
        self.out = bytearray()

    def literal(self, data, length_bytes=None):
        self.body += literal(data, length_bytes)
        self.out += bytes(data)
        return self

    def copy(self, kind, offset, length):
        assert 0 < offset <= len(self.out), (offset, len(self.out))
        self.body += copy(kind, offset, length)
        for _ in range(length):
            self.out.append(self.out[-offset])
        return self

    def fill_to(self, target, rng):
        """Short literals until the body is exactly ``target`` bytes long."""
        while len(self.body) < target:
            rem = target - len(self.body)
            assert rem >= 2
            take = min(rem - 1, 60)
            if rem - 1 - take == 1:
                take -= 1
            self.literal(rng.bytes(take), 0)
        assert len(self.body) == target
        return self

    def stream(self, pad=0):
        return preamble(len(self.out), pad) + bytes(self.body)

    def expected(self):
        return bytes(self.out)


def snappy_decode(stream):
    """The output of a raw Snappy block, or None where libsnappy refuses the stream."""
    s = bytes(stream)
    n, ip, want, shift = len(s), 0, 0, 0
    while True:
        if ip >= n or shift > 28:
            return None
        b = s[ip]
        ip += 1
        want |= (b & 0x7F) << shift
        if not b & 0x80:
            break
        shift += 7
    if want >= 1 << 32:
        return None
    out = bytearray()
    while ip < n:
        tag = s[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                if ip + nb > n:
                    return None
                ln = int.from_bytes(s[ip:ip + nb], "little")
                ip += nb
            ln += 1
            if ip + ln > n or len(out) + ln > want:
                return None
            out += s[ip:ip + ln]
            ip += ln
            continue
        hb = (0, 1, 2, 4)[kind]
        if ip + hb > n:
            return None
        if kind == 1:
            ln, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | s[ip]
        else:
            ln, off = 1 + (tag >> 2), int.from_bytes(s[ip:ip + hb], "little")
        ip += hb
        if off == 0 or off > len(out) or len(out) + ln > want:
            return None
        for _ in range(ln):
            out.append(out[-off])
    return bytes(out) if len(out) == want else None


def tags(stream):
    """[(kind, header bytes)] of a valid stream's elements, in order."""
    s, ip, out = bytes(stream), 0, []
    while s[ip] & 0x80:
        ip += 1
    ip += 1
    while ip < len(s):
        kind, ln = s[ip] & 3, s[ip] >> 2
        hl = (1 + max(ln - 59, 0), 2, 3, 5)[kind]
        if kind == 0:
            ln = ln if ln < 60 else int.from_bytes(s[ip + 1:ip + hl], "little")
            ip += ln + 1
        ip += hl
        out.append((kind, hl))
    return out


# literal share, literal lengths (lo, hi), same-offset copy-run bias, short-offset bias, copy-4
PROFILES = {
    "text": dict(lit=0.45, litlen=(1, 12), run=0.10, short=0.20, copy4=False),
    "rle": dict(lit=0.10, litlen=(1, 4), run=0.70, short=0.80, copy4=False),
    "copy4": dict(lit=0.25, litlen=(1, 70), run=0.30, short=0.40, copy4=True),
    "literal": dict(lit=0.80, litlen=(1, 300), run=0.20, short=0.50, copy4=True),
}


def random_stream(seed, profile, nout=1500):
    """A seeded random valid stream of about ``nout`` output bytes -> (stream, expected)."""
    p = PROFILES[profile] if isinstance(profile, str) else profile
    rng = np.random.default_rng(seed)
    b = Snappy()
    b.literal(rng.bytes(int(rng.integers(1, 9))))
    last = None
    while len(b.out) < nout:
        if rng.random() < p["lit"]:
            ln = int(rng.integers(p["litlen"][0], p["litlen"][1] + 1))
            minimal = 0 if ln <= 60 else ((ln - 1).bit_length() + 7) // 8
            nb = None
            if rng.random() < 0.15:        # a wider length field than needed
                nb = int(rng.integers(max(minimal, 1), 5))
            b.literal(rng.bytes(ln), nb)
            continue
        have = len(b.out)
        if last is not None and rng.random() < p["run"]:
            off = last
        elif rng.random() < p["short"]:
            off = int(rng.integers(1, min(have, 16) + 1))
        else:
            off = int(rng.integers(1, have + 1))
        if not p["copy4"]:
            off = min(off, 65535)
        ln = int(rng.integers(1, 65))
        kinds = [k for k in ((1, 2, 3) if p["copy4"] else (1, 2)) if copy_legal(k, off, ln)]
        b.copy(kinds[int(rng.integers(0, len(kinds)))], off, ln)
        last = off
    return b.stream(), b.expected()


# ------------------------------------------------------------------------------------------------
# RLE / bit-packed hybrid
# ------------------------------------------------------------------------------------------------
def pack_bits(values, bw):
    """``values`` as consecutive ``bw``-bit fields, LSB first."""
    v = np.asarray(values, dtype=np.uint64)
    if bw == 0 or len(v) == 0:
        return b""
    bits = ((v[:, None] >> np.arange(bw, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.ravel(), bitorder="little").tobytes()


def hybrid_encode(runs, bw, pad=0):
    """The hybrid stream of an explicit run list: ``("rle", count, value)`` or
    ``("packed", values)``; a further tuple element pads that run's varint header with so many
    non-minimal continuation bytes (``pad`` does for all).  Packed values are padded with zeros
    to whole groups of 8."""
    out = bytearray()
    for r in runs:
        if r[0] == "rle":
            _, count, value = r[:3]
            extra = r[3] if len(r) > 3 else pad
            out += varint(count << 1, extra)
            out += int(value).to_bytes((bw + 7) // 8, "little")
        else:
            vals = list(r[1])
            extra = r[2] if len(r) > 2 else pad
            vals += [0] * (-len(vals) % 8)
            out += varint((len(vals) // 8) << 1 | 1, extra)
            out += pack_bits(vals, bw)
    return bytes(out)


def expand_runs(runs, nv):
    """The first ``nv`` values a run list stands for: RLE counts are clamped, and a bit-packed
    run stands for whole groups of 8 (zeros past its values), cut only at ``nv``."""
    out = []
    for r in runs:
        out += [int(r[2])] * r[1] if r[0] == "rle" else \
            [int(x) for x in r[1]] + [0] * (-len(r[1]) % 8)
        if len(out) >= nv:
            break
    assert len(out) >= nv, (len(out), nv)
    return np.array(out[:nv], dtype=np.int64)


def hybrid_decode(data, bw, nv):
    """The ``nv`` values of hybrid stream ``data`` at bit width ``bw`` (None: the stream ends
    or overruns before ``nv`` values)."""
    s = bytes(data)
    out = np.zeros(nv, dtype=np.int64)
    pos = have = 0
    mask = (1 << bw) - 1
    while have < nv:
        h = shift = 0
        while True:
            if pos >= len(s):
                return None
            b = s[pos]
            pos += 1
            h |= (b & 0x7F) << shift
            shift += 7
            if b < 0x80:
                break
        if h & 1:
            nbytes = (h >> 1) * bw
            if pos + nbytes > len(s):
                return None
            word = int.from_bytes(s[pos:pos + nbytes], "little")
            take = min((h >> 1) * 8, nv - have)
            for i in range(take):
                out[have + i] = (word >> (i * bw)) & mask
            pos += nbytes
        else:
            vb = (bw + 7) // 8
            if pos + vb > len(s):
                return None
            take = min(h >> 1, nv - have)
            out[have:have + take] = int.from_bytes(s[pos:pos + vb], "little")
            pos += vb
        have += take
    return out


# ------------------------------------------------------------------------------------------------
# pages
# ------------------------------------------------------------------------------------------------
class Page:
    """One page: ``src`` (the stored bytes), the page-table fields that do not depend on where
    the buffers live, and what the decoder must produce: ``scratch`` (the inflated page),
    ``out`` (raw bytes at the page's ``out`` address; strings: offsets relative to the page's
    ``dst``), ``lens`` (strings), ``valid`` (pages with nulls).  ``dict`` is the dictionary
    Page of a dictionary-encoded data page."""

    def __init__(self, name, src, fields, scratch, out=None, valid=None, lens=None, dict=None,
                 status=0):
        self.name, self.src, self.fields, self.scratch = name, bytes(src), dict_(fields), scratch
        self.out, self.valid, self.lens, self.dict, self.status = out, valid, lens, dict, status


dict_ = dict


def snappy_plain(data):
    """A valid stream for ``data`` of literals only (the page builders' default codec-1 body;
    the directed streams go in through ``stream=``)."""
    b = Snappy()
    for at in range(0, len(data), 1000):
        b.literal(data[at:at + 1000])
    return b.stream()


def level_stream(validity, level_runs=None):
    v = [int(x) for x in validity]
    if level_runs is None:
        level_runs = [("packed", v)]
    assert list(expand_runs(level_runs, len(v))) == v
    return hybrid_encode(level_runs, 1)


def assemble(name, body, nvals, eb, enc, version=1, prefix=None, codec=0, validity=None,
             level_runs=None, stream=None, rng=None, **kw):
    """Level bytes + ``body`` as a v1 / v2 page.  ``validity`` (0/1 per row) makes a page with
    nulls, its levels encoded from ``level_runs``; otherwise ``prefix`` bytes of unread level
    bytes shift where the values start (v1: behind a 4-byte length; v2: ``levels``).  codec 1
    stores ``stream`` (a Snappy stream that must inflate to the v1 page / the v2 body)."""
    rng = rng or np.random.default_rng(0)
    nulls = 0
    if validity is not None:
        ls = level_stream(validity, level_runs)
        nulls = 1
        lv = struct.pack("<I", len(ls)) + ls if version == 1 else ls
        levels = 1 if version == 1 else len(ls)
    elif prefix is not None:
        junk = rng.bytes(prefix)
        lv = struct.pack("<I", prefix) + junk if version == 1 else junk
        levels = 1 if version == 1 else prefix
    else:
        lv, levels = b"", 0
    body = bytes(body)
    page = lv + body
    if codec == 0:
        src = page
    elif version == 1:
        src = stream if stream is not None else snappy_plain(page)
    else:
        src = lv + (stream if stream is not None else snappy_plain(body))
    fields = dict(csize=len(src), usize=len(page), nvals=nvals, codec=codec, kind=version - 1,
                  enc=enc, levels=levels, eb=eb, dict_page=-1, nulls=nulls)
    return Page(name, src, fields, page, **kw)


def spread(dense, validity, dtype):
    """Dense non-null values at their rows, 0 at nulls -> raw bytes."""
    v = np.asarray(validity, dtype=bool)
    out = np.zeros(len(v), dtype=dtype)
    out[v] = np.asarray(dense, dtype=dtype)[:int(v.sum())]
    return out


def dict_page(name, values, codec=0):
    """A PLAIN dictionary page of ``values`` (uint32 / uint64 raw bits)."""
    v = np.ascontiguousarray(values)
    body = v.tobytes()
    src = body if codec == 0 else snappy_plain(body)
    fields = dict(csize=len(src), usize=len(body), nvals=len(v), codec=codec, kind=2, enc=0,
                  levels=0, eb=v.dtype.itemsize, dict_page=-1, nulls=0)
    return Page(name, src, fields, body)


def dict_data_page(name, runs, bw, nvals, dpage, dvalues, validity=None, status=0, **kw):
    """A dictionary-encoded data page: the bit width byte, then ``runs`` as a hybrid stream
    (``nvals`` rows; with ``validity`` the runs hold the non-null rows only).  Indices at or
    past the dictionary's size must decode as 0."""
    dvalues = np.asarray(dvalues)
    nn = nvals if validity is None else int(np.sum(validity))
    idx = expand_runs(runs, nn)
    dense = np.where(idx < len(dvalues), dvalues[np.minimum(idx, len(dvalues) - 1)],
                     dvalues.dtype.type(0)).astype(dvalues.dtype)
    out = dense if validity is None else spread(dense, validity, dvalues.dtype)
    body = bytes([bw]) + hybrid_encode(runs, bw)
    return assemble(name, body, nvals, dvalues.dtype.itemsize, 8, validity=validity,
                    out=out.tobytes(), dict=dpage, status=status,
                    valid=None if validity is None else np.asarray(validity, np.uint8), **kw)


def plain_page(name, values, validity=None, **kw):
    """A PLAIN page of fixed-width ``values`` (raw bits, uint32 / uint64)."""
    v = np.ascontiguousarray(values)
    nvals = len(v) if validity is None else len(validity)
    out = v if validity is None else spread(v, validity, v.dtype)
    return assemble(name, v.tobytes(), nvals, v.dtype.itemsize, 0, validity=validity,
                    out=out.tobytes(),
                    valid=None if validity is None else np.asarray(validity, np.uint8), **kw)


def bool_page(name, values, runs=None, validity=None, **kw):
    """A BOOLEAN page: PLAIN bits (``runs`` None) or RLE (encoding 3: a 4-byte length, then the
    hybrid stream of ``runs`` at width 1)."""
    v = np.asarray(values, dtype=np.uint8)
    nvals = len(v) if validity is None else len(validity)
    if runs is None:
        body, enc = np.packbits(v, bitorder="little").tobytes(), 0
    else:
        assert list(expand_runs(runs, len(v))) == list(v)
        hs = hybrid_encode(runs, 1)
        body, enc = struct.pack("<I", len(hs)) + hs, 3
    out = v if validity is None else spread(v, validity, np.uint8)
    return assemble(name, body, nvals, 1, enc, validity=validity, out=out.tobytes(),
                    valid=None if validity is None else np.asarray(validity, np.uint8), **kw)


def string_page(name, strings, validity=None, **kw):
    """A PLAIN BYTE_ARRAY page (4-byte length, bytes).  ``out``: per row the offset of the
    value's first byte inside the inflated page (the kernel writes page address + offset; nulls
    address 0, told apart by ``valid``), ``lens`` the lengths (0 at nulls)."""
    body = b"".join(struct.pack("<I", len(s)) + s for s in strings)
    nvals = len(strings) if validity is None else len(validity)
    page = assemble(name, body, nvals, 16, 0, validity=validity,
                    valid=None if validity is None else np.asarray(validity, np.uint8), **kw)
    base = len(page.scratch) - len(body)
    offs, at = [], base
    for s in strings:
        offs.append(at + 4)
        at += 4 + len(s)
    offs, lens = np.array(offs, np.int64), np.array([len(s) for s in strings], np.int32)
    if validity is not None:
        offs, lens = spread(offs, validity, np.int64), spread(lens, validity, np.int32)
    page.out, page.lens = offs, lens
    return page


# ------------------------------------------------------------------------------------------------
# directed Snappy streams (w: the decoder's parse window; positions are body offsets, i.e.
# relative to the first window, which starts right after the preamble)
# ------------------------------------------------------------------------------------------------
COPY_OFFSETS = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17)


def _kinds(offset, length):
    return [k for k in (1, 2, 3) if copy_legal(k, offset, length)]


def inflate_streams(w):
    """[(name, stream, expected output)]: the directed valid streams."""
    rng = np.random.default_rng(1234)
    cases = []

    def add(name, b, pad=0):
        cases.append((name, b.stream(pad), b.expected()))

    cases.append(("size0", b"\x00", b""))
    for n in (1, 2, 63, 64, 65):
        add(f"size{n}", Snappy().literal(rng.bytes(n)))
        if n > 1:
            add(f"size{n}-lit1-copy", _lit_then_copies(rng, n))
    # one large page: a 3-byte literal length, copy-4 offsets above 65535, 2-byte-offset copies
    b = Snappy().literal(rng.bytes(66000))
    assert len(literal_header(66000)) == 4
    for i in range(40):
        b.copy(3, 65536 + 7 * i, 1 + (i * 13) % 64)
        b.copy(2, 65535 - i, 64)
        b.literal(rng.bytes(1 + i % 5))
    b.literal(rng.bytes(300), 3)
    while len(b.out) < 70000:
        b.copy(3, len(b.out) - int(rng.integers(0, 100)), 64)
    add("large-70000", b)
    # 64 two-byte tags from the start of the first window (exactly the window at w == 128)
    for tail in (0, 1):
        b = Snappy()
        for _ in range(64):
            b.literal(rng.bytes(1), 0)
        if tail:
            b.literal(rng.bytes(1), 0)
        add(f"64-literals+{tail}", b)
        b = Snappy().literal(rng.bytes(1), 0)
        for i in range(63):
            b.copy(1, 1 + i % 3 if i > 3 else 1, 4 + i % 8)
        if tail:
            b.copy(1, 5, 4)
        add(f"literal-63-copy1+{tail}", b)
    # a header straddling the window end
    for hl in (2, 3, 4, 5):
        for start in range(w - hl + 1, w):
            b = Snappy().fill_to(start, rng)
            b.literal(rng.bytes(3), hl - 1)
            b.literal(rng.bytes(5))
            add(f"straddle-literal-hl{hl}-at{start}", b)
            if hl != 4:
                b = Snappy().fill_to(start, rng)
                b.copy({2: 1, 3: 2, 5: 3}[hl], 9, 6)
                b.literal(rng.bytes(5))
                add(f"straddle-copy-hl{hl}-at{start}", b)
    # a literal ending exactly at the window end, then another tag
    b = Snappy().fill_to(w, rng).copy(2, 40, 30).literal(rng.bytes(3))
    add("literal-ends-at-window-short", b)
    b = Snappy().literal(rng.bytes(w - 2), 1)
    assert len(b.body) == w
    add("literal-ends-at-window-long", b.copy(1, 7, 9))
    add("literal-is-window", Snappy().literal(rng.bytes(w - 2), 1))
    # non-minimal literal length fields
    for nb in (1, 2, 3, 4):
        b = Snappy().literal(rng.bytes(3)).literal(rng.bytes(5), nb).copy(2, 6, 10)
        add(f"nonminimal-literal-{nb}", b.literal(rng.bytes(70), nb))
    # copies
    for off in COPY_OFFSETS:
        for ln in (4, 11, 1, 64, off, off + 1, max(off - 1, 1)):
            for k in _kinds(off, ln):
                b = Snappy().literal(rng.bytes(20)).copy(k, off, ln).literal(rng.bytes(2))
                cases.append((f"copy{k}-off{off}-len{ln}", b.stream(), b.expected()))
    for k in (1, 2, 3):
        add(f"copy{k}-offset-is-produced", Snappy().literal(rng.bytes(20)).copy(k, 20, 8))
        add(f"copy{k}-source-straddles-tags",
            Snappy().literal(rng.bytes(8)).literal(rng.bytes(8)).copy(k, 12, 8))
        b = Snappy()
        for _ in range(6):
            b.literal(rng.bytes(40))
        assert len(b.body) > w
        add(f"copy{k}-earlier-batch", b.copy(k, 230, 11).copy(k, 100, 8).literal(rng.bytes(1)))
        # every copy reads the one or two copies before it: chains 12 deep in one batch
        b = Snappy().literal(rng.bytes(16))
        for i in range(12):
            b.copy(k, (7, 9)[i & 1], 8)
        add(f"copy{k}-chain12", b)
        for run in (2, 3, 63):
            for off, ln in ((3, 7), (1, 4), (5, 5), (8, 11)):
                b = Snappy().literal(rng.bytes(9))
                for _ in range(run):
                    b.copy(k, off, ln)
                add(f"copy{k}-run{run}-off{off}-len{ln}", b.literal(rng.bytes(2)))
        b = Snappy().literal(rng.bytes(12))
        for off in (3, 3, 3, 10, 3, 3, 3, 4, 4, 3):
            b.copy(k, off, 7)
        add(f"copy{k}-run-interrupted", b)
        # 70 tags: past the 64 tags of one batch (copy-4: past the window after 25 tags)
        b = Snappy().literal(rng.bytes(6))
        for _ in range(70):
            b.copy(k, 4, 9)
        add(f"copy{k}-run-crosses-batch", b.literal(rng.bytes(3)))
    seen = {}
    for c in cases:
        seen.setdefault(c[0], c)
    return list(seen.values())


def _lit_then_copies(rng, n):
    b = Snappy().literal(rng.bytes(1))
    while len(b.out) < n:
        left = n - len(b.out)
        b.copy(2, int(rng.integers(1, len(b.out) + 1)), min(left, int(rng.integers(1, 65))))
    return b


def random_streams(per_profile=52, nout=1200):
    """[(name with profile and seed, stream, expected)]: 4 profiles x ``per_profile`` seeds."""
    return [(f"random-{p}-seed{seed}",) + random_stream(seed, p, nout)
            for p in PROFILES for seed in range(per_profile)]


LONG_LITERAL_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 60, 61, 255, 256, 257, 65536, 65537)


def long_literal_stream(length, in_mis, lead, rng):
    """A stream that is one literal of ``length`` bytes whose first byte lies at input offset
    = ``in_mis`` (mod 4) of a stream stored ``lead`` bytes into a 4-byte aligned region: the
    literal's length field and, where that does not reach, the preamble are widened."""
    data = rng.bytes(length)
    minimal = len(literal_header(length)) - 1
    for pad in range(0, 5 - len(preamble(length)) + 1):
        for nb in range(max(minimal, 0), 5):
            if nb == 0 and length > 60:
                continue
            pre = preamble(length, pad)
            if (lead + len(pre) + 1 + nb) % 4 == in_mis:
                return pre + literal(data, nb), data
    raise AssertionError((length, in_mis, lead))


def malformed_streams():
    """[(name, stream, usize)]: streams (or stream / page-size pairs) the decoder must refuse.
    All but the two ``preamble-*`` ones are refused by libsnappy whatever the size."""
    rng = np.random.default_rng(99)
    good = Snappy().literal(rng.bytes(6)).copy(1, 3, 4)
    m = [("preamble-below-usize", good.stream(), 12), ("preamble-above-usize", good.stream(), 8)]

    def raw(n, *parts):
        return preamble(n) + b"".join(parts)

    m.append(("copy-before-output-start", raw(8, literal(rng.bytes(4)), copy(1, 5, 4)), 8))
    m.append(("copy-before-output-start-2nd-batch",
              raw(248, *[literal(rng.bytes(40)) for _ in range(6)], copy(2, 241, 8)), 248))
    m.append(("literal-past-input", raw(20, literal_header(20), rng.bytes(10)), 20))
    m.append(("literal-past-input-after-copy",
              raw(40, literal(rng.bytes(8)), copy(1, 8, 8), literal_header(24), rng.bytes(23)), 40))
    m.append(("literal-length-near-int-max",
              raw(40, literal(rng.bytes(8)), literal_header(0x7FFFFFFF, 4), rng.bytes(31)), 40))
    m.append(("literal-length-2-to-32",
              raw(40, literal(rng.bytes(8)), literal_header(1 << 32, 4), rng.bytes(31)), 40))
    for name, hdr in (("copy1", copy(1, 4, 4)), ("copy2", copy(2, 4, 4)), ("copy4", copy(3, 4, 4)),
                      ("literal1", literal_header(4, 1)), ("literal2", literal_header(4, 2)),
                      ("literal3", literal_header(4, 3)), ("literal4", literal_header(4, 4))):
        for keep in range(1, len(hdr)):
            m.append((f"header-cut-{name}-{keep}of{len(hdr)}",
                      raw(12, literal(rng.bytes(8)), hdr[:keep]), 12))
    m.append(("output-exceeds-usize", raw(8, literal(rng.bytes(4)), copy(1, 4, 8)), 8))
    m.append(("output-exceeds-usize-literal", raw(8, literal(rng.bytes(4)), literal(rng.bytes(5))),
              8))
    m.append(("output-ends-short", raw(20, literal(rng.bytes(10))), 20))
    m.append(("output-ends-short-empty", raw(3), 3))
    for k in (1, 2, 3):
        m.append((f"copy{k}-offset-0", raw(8, literal(b"abcd"), copy(k, 0, 4)), 8))
        m.append((f"copy{k}-offset-0-first-tag", raw(4, copy(k, 0, 4)), 4))
    for off in (0x80000000, 0xFFFFFFFF, 0x80000004):
        m.append((f"copy4-offset-{off:#x}", raw(16, literal(rng.bytes(8)), copy(3, off, 8)), 16))
    return m


# ------------------------------------------------------------------------------------------------
# directed expand pages (codec 0)
# ------------------------------------------------------------------------------------------------
BIT_WIDTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32)
NULL_NVALS = (1, 255, 256, 257, 511, 512, 513, 1025)
NULL_PATTERNS = ("all-null", "none-null", "first-valid", "last-valid", "alternating",
                 "last-chunk-valid", "random-5", "random-95")


def dictionary_values(dtype, n, rng):
    """``n`` raw-bit dictionary values: INT_MIN, -0.0, NaN patterns, then random bits."""
    dtype = np.dtype(dtype)
    if dtype.itemsize == 4:
        special = [0x80000000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF, 0, 0x7FFFFFFF]
    else:
        special = [0x8000000000000000, 0x7FF8000000000000, 0xFFF8000000000001,
                   0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0, 0x7FFFFFFFFFFFFFFF]
    v = rng.integers(0, np.iinfo(dtype).max, n, dtype=dtype, endpoint=True)
    k = min(n, len(special))
    v[:k] = np.array(special[:k], dtype=dtype)
    return v


def validity_pattern(pattern, n, rng):
    v = np.zeros(n, dtype=np.uint8)
    if pattern == "none-null":
        v[:] = 1
    elif pattern == "first-valid":
        v[0] = 1
    elif pattern == "last-valid":
        v[-1] = 1
    elif pattern == "alternating":
        v[::2] = 1
    elif pattern == "last-chunk-valid":
        v[(n - 1) // 256 * 256:] = 1
    elif pattern == "random-5":
        v[:] = rng.random(n) < 0.05
    elif pattern == "random-95":
        v[:] = rng.random(n) < 0.95
    elif pattern == "random-50":
        v[:] = rng.random(n) < 0.5
    else:
        assert pattern == "all-null"
    return v


def runs_for(values, mode):
    """A run list standing for ``values``: "rle" (one run per stretch), "packed" (one
    bit-packed run) or "mixed" (RLE for stretches of >= 8 equal values, groups of 8 between)."""
    v = [int(x) for x in values]
    if mode == "packed" or not v:
        return [("packed", v)]
    runs, i = [], 0
    while i < len(v):
        j = i
        while j < len(v) and v[j] == v[i]:
            j += 1
        if mode == "rle" or j - i >= 8:
            runs.append(("rle", j - i, v[i]))
            i = j
        else:
            take = v[i:i + 8]
            if runs and runs[-1][0] == "packed" and len(runs[-1][1]) < 64:
                runs[-1] = ("packed", runs[-1][1] + take)
            else:
                runs.append(("packed", take))
            i += 8
    return runs


def _indices(n, bw, dsize, rng):
    """``n`` random indices below ``dsize`` that use the top bit of width ``bw`` where the
    dictionary is large enough."""
    hi = min(dsize, 1 << bw)
    idx = rng.integers(0, hi, n)
    if n and hi > 1:
        idx[rng.integers(0, n)] = hi - 1
    return [int(x) for x in idx]


def dictionary_cases():
    """Valid dictionary-encoded pages (no nulls): [Page]."""
    rng = np.random.default_rng(77)
    pages = []
    for dtype in (np.uint32, np.uint64):
        eb = np.dtype(dtype).itemsize
        dicts = {}
        for bw in BIT_WIDTHS:
            dsize = 1 << bw if bw <= 9 else 300 + bw
            if dsize not in dicts:
                dv = dictionary_values(dtype, dsize, rng)
                dicts[dsize] = (dict_page(f"dict-eb{eb}-n{dsize}", dv), dv)
            dp, dv = dicts[dsize]

            def page(name, runs, nvals, **kw):
                pages.append(dict_data_page(f"dict-eb{eb}-bw{bw}-{name}", runs, bw, nvals, dp,
                                            dv, rng=rng, **kw))

            ix = lambda n: _indices(n, bw, dsize, rng)
            a, b, c, d = ix(4)
            # counts 0 (skipped), 1 and past the values left (clamped)
            page("rle", [("rle", 5, a), ("rle", 0, b), ("rle", 1, c), ("rle", 0, a),
                         ("rle", 100, d)], 46)
            page("packed-padded", [("packed", ix(19))], 19)
            page("packed-3-runs", [("packed", ix(8)), ("packed", ix(64)), ("packed", ix(13))], 85)
            page("alternating", [("rle", 3, a), ("packed", ix(8)), ("rle", 1, b),
                                 ("packed", ix(16)), ("rle", 0, c), ("rle", 9, d),
                                 ("packed", ix(5))], 3 + 8 + 1 + 16 + 9 + 5)
            # 2- and 3-byte varint headers and non-minimal ones
            page("varint-2-3", [("rle", 100, a), ("packed", ix(512)), ("rle", 3, b, 1),
                                ("packed", ix(8), 2), ("rle", 10000, c), ("rle", 7, d, 3)], 2000)
            for nruns in (127, 128, 129, 257):
                runs = []
                for i in range(nruns):
                    runs.append(("packed", ix(8)) if i % 3 == 1 else ("rle", 1 + i % 3, ix(1)[0]))
                nv = sum(r[1] if r[0] == "rle" else 8 for r in runs)
                page(f"{nruns}-runs", runs, nv)
            for nv in (1, 255, 256, 257, 1025):
                page(f"nvals{nv}-mixed", runs_for(sorted(ix(nv // 2)) + ix(nv - nv // 2), "mixed"),
                     nv)
                page(f"nvals{nv}-packed", [("packed", ix(nv))], nv)
            for prefix in range(4):
                for version in (1, 2):
                    page(f"v{version}-prefix{prefix}", [("packed", ix(8)), ("rle", 4, a), ("packed", ix(3))], 15,
                         version=version, prefix=prefix)
    return pages


def dictionary_range_cases():
    """Pages with an index at or past the dictionary's size ([Page], ``status`` 2): one in an
    RLE run, one in a bit-packed run, per element size."""
    rng = np.random.default_rng(78)
    pages = []
    for dtype in (np.uint32, np.uint64):
        eb = np.dtype(dtype).itemsize
        dv = dictionary_values(dtype, 5, rng)
        dv[dv == 0] = 1            # so that "decodes as 0" shows
        dp = dict_page(f"dict-eb{eb}-n5", dv)
        pages.append(dict_data_page(f"range-eb{eb}-rle", [("rle", 3, 4), ("rle", 2, 5),
                                                          ("packed", [0, 1, 2, 3, 4])], 3, 10,
                                    dp, dv, status=2))
        pages.append(dict_data_page(f"range-eb{eb}-packed", [("rle", 3, 4), ("packed",
                                    [0, 1, 2, 7, 4, 5, 3, 6, 1]), ("rle", 5, 2)], 3, 17, dp, dv,
                                    status=2))
        pages.append(dict_data_page(f"range-eb{eb}-bw32", [("rle", 2, 0xFFFFFFFF), ("packed",
                                    [1, 0x80000000, 2])], 32, 5, dp, dv, status=2))
    return pages


def plain_cases():
    """PLAIN fixed-width pages whose values start at every byte alignment: [Page]."""
    rng = np.random.default_rng(79)
    pages = []
    for dtype in (np.uint32, np.uint64):
        for version in (1, 2):
            for prefix in range(8):
                for n in (1, 67, 300):
                    pages.append(plain_page(f"plain-eb{np.dtype(dtype).itemsize}-v{version}"
                                            f"-prefix{prefix}-n{n}",
                                            dictionary_values(dtype, n, rng), version=version,
                                            prefix=prefix, rng=rng))
    return pages


def _strings(n, rng):
    pool = [b"", b"a", "é中\U0001f600".encode(), bytes(rng.integers(32, 127, 300,
            dtype=np.uint8)), b"xy", "ü".encode() * 7]
    return [pool[int(i)] for i in rng.integers(0, len(pool), n)]


def null_cases():
    """Pages with nulls: every element size x row count x validity pattern, the page version,
    the level run mix and the value encoding rotating over them: [Page]."""
    rng = np.random.default_rng(80)
    pages, dicts, turn = [], {}, 0
    for dtype in (np.uint32, np.uint64):
        dv = dictionary_values(dtype, 40, rng)
        dv[dv == 0] = 3
        dicts[np.dtype(dtype).itemsize] = (dict_page(f"dict-null-eb{dv.dtype.itemsize}", dv), dv)
    # beyond the listed patterns: random at 50 % is, as RLE runs, several hundred short runs with
    # no period, so a 128-run level round that resumes at the wrong place shows
    extra = [(nv, "random-50", version, mode) for nv in (513, 1025) for version in (1, 2)
             for mode in ("rle", "packed", "mixed")]
    for eb in (1, 4, 8, 16):
        listed = []
        for nv in NULL_NVALS:
            for pi, pattern in enumerate(NULL_PATTERNS):
                listed.append((nv, pattern, 1 + (turn & 1),
                               ("rle", "packed", "mixed")[(turn // 2 + pi) % 3]))
                turn += 1
        for ci, (nv, pattern, version, mode) in enumerate(listed + extra):
            enc = (ci // 6 + ci) & 1
            valid = validity_pattern(pattern, nv, rng)
            nn = int(valid.sum())
            name = f"nulls-eb{eb}-n{nv}-{pattern}-v{version}-{mode}-enc{enc}"
            kw = dict(validity=valid, level_runs=runs_for(valid, mode), version=version, rng=rng)
            if eb == 1:
                vals = rng.integers(0, 2, nn).astype(np.uint8)
                pages.append(bool_page(name, vals, runs_for(vals, "mixed") if enc else None, **kw))
            elif eb == 16:
                pages.append(string_page(name, _strings(nn, rng), **kw))
            elif enc:
                dp, dv = dicts[eb]
                pages.append(dict_data_page(name, runs_for(_indices(nn, 6, 40, rng), "mixed"), 6,
                                            nv, dp, dv, **kw))
            else:
                vals = dictionary_values(np.dtype(f"u{eb}"), nn, rng)
                vals[vals == 0] = 9
                pages.append(plain_page(name, vals, **kw))
    return pages


def bool_cases():
    rng = np.random.default_rng(81)
    pages = []
    for nv in (1, 7, 13, 257, 1025, 1031):
        for version in (1, 2):
            v = rng.integers(0, 2, nv).astype(np.uint8)
            pages.append(bool_page(f"bool-plain-n{nv}-v{version}", v, version=version))
            v[nv // 3:nv // 3 + 40] = 1
            for mode in ("mixed", "rle", "packed"):
                pages.append(bool_page(f"bool-rle-{mode}-n{nv}-v{version}", v, runs_for(v, mode),
                                       version=version))
    v = [1] * 3 + [0] * 8 + [1, 0, 1, 1, 0, 0, 0, 1] + [0] * 200
    pages.append(bool_page("bool-rle-count0-clamped", v, [("rle", 3, 1), ("rle", 0, 1),
                           ("rle", 8, 0), ("packed", v[11:19]), ("rle", 1000, 0, 1)]))
    return pages


def string_cases():
    rng = np.random.default_rng(82)
    pages = []
    for nv in (1, 5, 1023, 1024, 1025, 2049):
        for version in (1, 2):
            pages.append(string_page(f"strings-n{nv}-v{version}", _strings(nv, rng),
                                     version=version, prefix=(nv + version) % 4, rng=rng))
    pages.append(string_page("strings-all-empty", [b""] * 9))
    return pages


def malformed_pages():
    """Corrupt pages ([Page], ``status`` 1); no output is checked."""
    rng = np.random.default_rng(83)
    pages = []
    for eb in (4, 8):
        dv = dictionary_values(np.dtype(f"u{eb}"), 16, rng)
        dp = dict_page(f"dict-malformed-eb{eb}", dv)

        def bad(name, body, nvals, **kw):
            pages.append(assemble(f"malformed-eb{eb}-{name}", body, nvals, eb, 8, dict=dp,
                                  status=1, **kw))

        bad("bw33", bytes([33]) + hybrid_encode([("rle", 10, 1)], 8), 10)
        bad("run-header-past-end", bytes([4]) + hybrid_encode([("rle", 6, 1)], 4) + b"\x80\x80", 10)
        bad("stream-ends-early", bytes([4]) + hybrid_encode([("rle", 6, 1)], 4), 10)
        bad("rle-value-past-end", bytes([16]) + hybrid_encode([("rle", 6, 1)], 16)[:-1], 6)
        full = hybrid_encode([("packed", [1] * 800)], 4)
        bad("packed-longer-than-page", bytes([4]) + full[:10], 800)
        bad("packed-after-rle-longer-than-page",
            bytes([4]) + hybrid_encode([("rle", 300, 2)], 4) + full[:100], 1100)
        # the v1 level length beyond the page, with the levels unread and read
        body = bytes([4]) + hybrid_encode([("rle", 10, 1)], 4)
        for nulls in (0, 1):
            pg = struct.pack("<I", 4000) + b"\x03" * 4 + body
            f = dict(csize=len(pg), usize=len(pg), nvals=10, codec=0, kind=0, enc=8, levels=1,
                     eb=eb, dict_page=-1, nulls=nulls)
            pages.append(Page(f"malformed-eb{eb}-v1-level-length-nulls{nulls}", pg, f, pg,
                              dict=dp, status=1))
    for name, body, nv in (
            ("length-past-end", struct.pack("<I", 3) + b"abc" + struct.pack("<I", 50) + b"de", 2),
            ("length-field-cut", struct.pack("<I", 3) + b"abc" + b"\x01\x00", 2),
            ("length-huge", struct.pack("<I", 3) + b"abc" + struct.pack("<I", 0xFFFFFFF0) + b"d",
             2)):
        pages.append(assemble(f"malformed-strings-{name}", body, nv, 16, 0, status=1))
    return pages
