"""The device Parquet page decoder (csrc/kernels/parquet_decode.hip) against the plain reference
of tests/pq_ref.py (checked on the CPU in test_pq_ref.py), byte for byte, on pages built by hand:
Snappy tag streams no common compressor emits (copy-4, wide and non-minimal length fields, tags
placed against the parse window, copy chains and same-offset runs), hybrid streams with every
run mix and bit width, every value alignment, null patterns around the 256-row chunk, and the
corrupt inputs the kernels must refuse.

``hs_pq_decode_pages`` is driven as ``native_parquet.decode_batch`` drives it (no ``raw`` base,
absolute device addresses).  All pages of a launch live in one uint8 device buffer filled with
a sentinel; every region (stored page, inflated page, values, lengths, validity) starts 16-byte
aligned and is followed by >= 64 sentinel bytes, and the whole buffer is compared with the
expected image afterwards, so a byte written outside any output shows as well."""
import functools

import numpy as np
import pytest

import pq_ref as R
from hyperspace_amd.io import native_parquet as NP

gpu = pytest.mark.gpu
SLACK = 64


@functools.lru_cache(maxsize=None)
def _window():
    from hyperspace_amd.ops import kernels as K
    return K.pq_snappy_window()


class _Plan:
    """Host image of one launch: the buffer to upload, the page table, the expected buffer
    after the launch and the named regions."""

    def __init__(self, pages, base):
        flat, index = [], {}
        for p in pages:
            for q in ((p.dict, p) if p.dict is not None else (p,)):
                if id(q) not in index:
                    index[id(q)] = len(flat)
                    flat.append(q)
        self.pages = flat
        self.regions = []            # (start, end, page name, what, checked)
        at = [0]

        def alloc(n, name, what, checked):
            a = at[0]
            self.regions.append((a, a + n, name, what, checked))
            at[0] = (a + n + SLACK + 15) & ~15
            return a

        tab = np.zeros(len(flat), dtype=NP.PAGE_DTYPE)
        place = []
        for i, q in enumerate(flat):
            f = q.fields
            ok = q.status != 1
            nv, eb = f["nvals"], f["eb"]
            src = alloc(len(q.src), q.name, "stored page", True)
            dst = alloc(f["usize"], q.name, "inflated page", ok)
            out = lens = valid = None
            if f["kind"] != 2 and nv:
                out = alloc(nv * (8 if eb == 16 else eb), q.name, "values", ok)
                if eb == 16:
                    lens = alloc(nv * 4, q.name, "lengths", ok)
                if f["nulls"]:
                    valid = alloc(nv, q.name, "validity", ok)
            place.append((src, dst, out, lens, valid))
        self.size = at[0]
        self.buf = np.full(self.size, R.SENTINEL, dtype=np.uint8)
        for q, (src, *_) in zip(flat, place):
            self.buf[src:src + len(q.src)] = np.frombuffer(q.src, np.uint8)
        self.expected = self.buf.copy()
        for i, (q, (src, dst, out, lens, valid)) in enumerate(zip(flat, place)):
            for k, v in q.fields.items():
                tab[i][k] = v
            tab[i]["src"], tab[i]["dst"] = base + src, base + dst
            if q.dict is not None:
                tab[i]["dict_page"] = index[id(q.dict)]
                tab[i]["dict"] = base + place[index[id(q.dict)]][1]
            if q.status == 1:
                if out is not None:
                    tab[i]["out"] = base + out
                    tab[i]["valid"] = base + valid if valid is not None else 0
                    if lens is not None:
                        tab[i]["dict"] = base + lens
                continue
            self.expected[dst:dst + len(q.scratch)] = np.frombuffer(q.scratch, np.uint8)
            if out is None:
                continue
            tab[i]["out"] = base + out
            if q.fields["eb"] == 16:
                tab[i]["dict"] = base + lens
                rows = q.valid.astype(bool) if q.valid is not None else np.ones(len(q.out), bool)
                addr = np.where(rows, q.out + (base + dst), 0).astype(np.uint64)
                self._put(out, addr.tobytes())
                self._put(lens, q.lens.astype(np.int32).tobytes())
            else:
                self._put(out, q.out)
            if valid is not None:
                tab[i]["valid"] = base + valid
                self._put(valid, q.valid.tobytes())
        self.table = tab
        self.status = 0
        for q in flat:
            self.status |= q.status

    def _put(self, at, data):
        self.expected[at:at + len(data)] = np.frombuffer(data, np.uint8)

    def mismatches(self, got, limit=8):
        """Names of what differs from the expected image: regions, or the slack after them."""
        exp = self.expected.copy()
        for a, b, _, _, checked in self.regions:
            if not checked:
                exp[a:b] = got[a:b]
        diff = np.flatnonzero(got != exp)
        starts = np.array([r[0] for r in self.regions] + [self.size])
        names = []
        while len(diff) and len(names) < limit:
            d = int(diff[0])
            r = int(np.searchsorted(starts, d, side="right")) - 1
            a, b, name, what, _ = self.regions[r]
            if d < b:
                names.append(f"{name}: {what} @byte {d - a}")
            else:
                names.append(f"{name}: slack after {what} (+{d - b})")
            diff = diff[diff >= (b if d < b else starts[r + 1])]
        return names


def _decode(pages, device):
    """One hs_pq_decode_pages launch over ``pages`` -> (status, mismatching region names)."""
    import torch
    from hyperspace_amd.ops import _lib as NL
    size = _Plan(pages, 0).size
    dbuf = torch.empty(size, dtype=torch.uint8, device=device)
    plan = _Plan(pages, dbuf.data_ptr())
    assert dbuf.data_ptr() % 16 == 0 and plan.size == size
    dbuf.copy_(torch.from_numpy(plan.buf))
    dtab = torch.from_numpy(plan.table.view(np.uint8).copy()).to(device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    NL.check(NL.lib().hs_pq_decode_pages(None, None, dtab.data_ptr(), len(plan.table),
                                         status.data_ptr(), NL.stream_ptr()),
             "hs_pq_decode_pages")
    torch.cuda.synchronize()
    return int(status.item()), plan.mismatches(dbuf.cpu().numpy()), plan


def _check(pages, device):
    status, bad, plan = _decode(pages, device)
    assert status == plan.status and not bad, (status, bad)


def _words_page(name, want, rng, version=1, prefix=None, codec=1, stream=None):
    """The bytes ``want`` as a PLAIN INT32 page (expand copies the whole words out)."""
    return R.assemble(name, want, len(want) // 4, 4, 0, version=version, prefix=prefix,
                      codec=codec, stream=stream, rng=rng, out=want[:len(want) // 4 * 4])


def _odd(pages, rng):
    """``pages`` as a table whose length is no multiple of 4 (four wavefronts per block)."""
    while len({id(q) for p in pages for q in (p, p.dict) if q is not None}) % 4 == 0:
        pages = pages + [_words_page("filler", rng.bytes(12), rng, codec=0)]
    return pages


# ------------------------------------------------------------------------------------------------
# inflate
# ------------------------------------------------------------------------------------------------
@gpu
def test_inflate_directed_streams(device):
    rng = np.random.default_rng(11)
    pages = [_words_page(n, want, rng, stream=s) for n, s, want in R.inflate_streams(_window())]
    assert len(pages) > 200
    _check(_odd(pages, rng), device)


@gpu
def test_inflate_random_streams(device):
    rng = np.random.default_rng(12)
    cases = R.random_streams()
    assert len(cases) >= 200
    _check(_odd([_words_page(n, want, rng, stream=s) for n, s, want in cases], rng), device)


@gpu
def test_inflate_long_literal_alignments(device):
    """One literal per stream (the dword path): output misalignment through the v2 level
    prefix, which shifts the stream and the output alike, input misalignment through the
    widths of the preamble and the length field."""
    rng = np.random.default_rng(13)
    pages = []
    for lead in range(4):
        for mis in range(4):
            for n in R.LONG_LITERAL_LENGTHS:
                s, want = R.long_literal_stream(n, mis, lead, rng)
                pages.append(_words_page(f"long-literal-{n}-out{lead}-in{mis}", want, rng,
                                         version=2, prefix=lead, stream=s))
    _check(_odd(pages, rng), device)


@gpu
def test_inflate_mixed_codecs_and_v2_levels(device):
    """Stored (codec 0) and Snappy pages in one table, v1 and v2; v2 pages keep their level
    bytes uncompressed in front of the Snappy body."""
    rng = np.random.default_rng(14)
    cases = R.inflate_streams(_window())[::7] + R.random_streams(3)
    pages = []
    for i, (n, s, want) in enumerate(cases):
        pages.append(_words_page(f"{n}-stored-v1", want, rng, codec=0))
        pages.append(_words_page(f"{n}-stored-v2", want, rng, version=2, prefix=i % 9, codec=0))
        pages.append(_words_page(f"{n}-snappy-v2", want, rng, version=2, prefix=1 + i % 21,
                                 stream=s))
        pages.append(_words_page(f"{n}-snappy-v1", want, rng, stream=s))
    dv = R.dictionary_values(np.uint64, 700, rng)
    dp = R.dict_page("snappy-dictionary", dv, codec=1)
    idx = [int(x) for x in rng.integers(0, 700, 900)]
    data = R.dict_data_page("snappy-dictionary-data", R.runs_for(idx, "mixed"), 10, 900, dp, dv,
                            codec=1)
    _check(_odd(pages + [data], rng), device)


@gpu
def test_inflate_refuses_malformed_streams(device):
    """One launch per corrupt stream, next to two valid pages that must still decode."""
    rng = np.random.default_rng(15)
    wrong = []
    for name, stream, usize in R.malformed_streams():
        f = dict(csize=len(stream), usize=usize, nvals=0, codec=1, kind=0, enc=0, levels=0, eb=4,
                 dict_page=-1, nulls=0)
        bad_page = R.Page(name, stream, f, None, status=1)
        s, want = R.random_stream(3, "text", 300)
        good = [_words_page("valid-before", want, rng, stream=s), bad_page,
                _words_page("valid-after", rng.bytes(40), rng, codec=0)]
        status, bad, _ = _decode(good, device)
        if not status & 1 or bad:
            wrong.append((name, status, bad))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------
# expand
# ------------------------------------------------------------------------------------------------
@gpu
def test_expand_dictionary_pages(device):
    _check(_odd(R.dictionary_cases(), np.random.default_rng(16)), device)


@gpu
@pytest.mark.parametrize("where", ["rle", "packed", "bw32"])
def test_expand_dictionary_index_out_of_range(device, where):
    pages = [p for p in R.dictionary_range_cases() if p.name.endswith(where)]
    assert len(pages) == 2
    status, bad, _ = _decode(pages, device)
    assert status == 2 and not bad, (status, bad)


@gpu
def test_expand_plain_pages(device):
    _check(_odd(R.plain_cases(), np.random.default_rng(17)), device)


@gpu
def test_expand_pages_with_nulls(device):
    pages = R.null_cases()
    names = {p.name.rsplit("-", 3)[0] for p in pages}
    for eb in (1, 4, 8, 16):
        for nv in R.NULL_NVALS:
            for pattern in R.NULL_PATTERNS:
                assert f"nulls-eb{eb}-n{nv}-{pattern}" in names
    for eb in (1, 4, 8, 16):         # every element size sees both versions and all run mixes
        seen = {(p.fields["kind"], p.name.split("-")[-2]) for p in pages if p.fields["eb"] == eb}
        assert len(seen) == 6, seen
    _check(_odd(pages, np.random.default_rng(18)), device)


@gpu
def test_expand_boolean_pages(device):
    _check(_odd(R.bool_cases(), np.random.default_rng(19)), device)


@gpu
def test_expand_plain_string_pages(device):
    _check(_odd(R.string_cases(), np.random.default_rng(20)), device)


@gpu
def test_expand_refuses_malformed_pages(device):
    rng = np.random.default_rng(21)
    wrong = []
    for p in R.malformed_pages():
        good = [_words_page("valid-before", rng.bytes(64), rng, codec=0), p,
                R.string_page("valid-after", [b"ab", b"", b"cde"])]
        status, bad, _ = _decode(good, device)
        if not status & 1 or bad:
            wrong.append((p.name, status, bad))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------
# run-table kernels
# ------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 63, 64, 65, 1000)


class _Runs:
    """A staging buffer and run table under construction with the expected output."""

    def __init__(self, dtype, rng):
        self.rng, self.dtype = rng, np.dtype(dtype)
        self.buf = bytearray()
        self.runs, self.want = [], []

    def place(self, data, align):
        """``data`` at the next offset that is ``align`` mod 8."""
        while len(self.buf) % 8 != align:
            self.buf.append(R.SENTINEL)
        at = len(self.buf)
        self.buf += data
        return at

    def run(self, kind, count, src, bw, values):
        dst = sum(len(w) for w in self.want)
        self.runs.append((dst, count, src, kind, bw))
        # one sentinel element after every run: a run writing past its count shows
        self.want.append(np.concatenate([np.asarray(values, self.dtype),
                                         np.frombuffer(bytes([R.SENTINEL]) * self.dtype.itemsize,
                                                       self.dtype)]))

    def launch(self, device, call):
        import torch
        from hyperspace_amd.ops import _lib as NL
        if len(self.runs) % 4 == 0:
            self.run(0, 0, 0, 0, [])
        tab = np.array(self.runs, dtype=NP.RUN_DTYPE)
        want = np.concatenate(self.want)
        host = np.frombuffer(bytes(self.buf) + bytes([R.SENTINEL]) * SLACK, np.uint8)
        dbuf = torch.from_numpy(host.copy()).to(device)
        dtab = torch.from_numpy(tab.view(np.uint8).copy()).to(device)
        out = torch.from_numpy(np.full(want.nbytes, R.SENTINEL, np.uint8)).to(device)
        NL.check(call(NL.lib(), dbuf.data_ptr(), dtab.data_ptr(), len(tab), out.data_ptr(),
                      NL.stream_ptr()), "run-table decode")
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(self.dtype)
        starts = np.array([r[0] for r in self.runs])
        bad = sorted({int(np.searchsorted(starts, d, side="right")) - 1
                      for d in np.flatnonzero(got != want)})
        return [(i, self.runs[i]) for i in bad[:8]]


@gpu
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_value_run_kernel(device, dtype):
    rng = np.random.default_rng(22)
    t = _Runs(dtype, rng)
    dcount = 300
    dv = R.dictionary_values(dtype, dcount, rng)
    dv[dv == 0] = 5
    t.place(bytes([R.SENTINEL]) * 16, 0)
    dict_off = t.place(dv.tobytes(), 0)          # dictionary pages are 16-byte aligned
    assert dict_off == 16
    look = lambda idx: np.where(np.asarray(idx) < dcount,
                                dv[np.minimum(np.asarray(idx, np.int64), dcount - 1)], 0)
    turn = 0
    for bw in R.BIT_WIDTHS:
        for count in COUNTS:
            hi = min(dcount, 1 << bw)
            idx = rng.integers(0, hi, count)
            if count > 1 and (1 << bw) > dcount:      # indices past the dictionary decode as 0
                idx[rng.integers(0, count, 2)] = [dcount, (1 << bw) - 1]
            src = t.place(R.pack_bits(idx, bw), turn % 8)
            t.run(1, count, src, bw, look(idx))
            turn += 1
    for count in COUNTS:
        for v in (0, 7, dcount - 1, dcount, 1 << 40, -1):
            t.run(0, count, v, 0, look([v if 0 <= v < dcount else dcount] * count))
        for align in range(8):
            vals = R.dictionary_values(dtype, count, rng)
            t.run(2, count, t.place(vals.tobytes(), align), 0, vals)
    eb = np.dtype(dtype).itemsize
    bad = t.launch(device, lambda L, buf, tab, n, out, s: L.hs_pq_decode_values(
        buf, tab, n, dict_off, dcount, eb, out, s))
    assert not bad, bad


@gpu
def test_level_run_kernel(device):
    rng = np.random.default_rng(23)
    t = _Runs(np.uint8, rng)
    turn = 0
    for bw in (1, 2, 7, 8):
        for count in COUNTS:
            lv = rng.integers(0, 1 << bw, count) * (rng.random(count) < 0.5)
            src = t.place(R.pack_bits(lv, bw), turn % 8)
            t.run(1, count, src, bw, (lv != 0).astype(np.uint8))
            turn += 1
    for count in COUNTS:
        for v in (0, 1, 3):
            t.run(0, count, v, 1, [int(v != 0)] * count)
    bad = t.launch(device, lambda L, buf, tab, n, out, s: L.hs_pq_decode_levels(
        buf, tab, n, out, s))
    assert not bad, bad
