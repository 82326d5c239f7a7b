"""SQL LIKE over dictionary-coded string columns.

``compile_like`` turns a pattern into a flat token program over its UTF-8 bytes (the format
``csrc/kernels/dict_like.hip`` interprets); ``like_match_host`` is the same interpreter in plain
Python - the kernel's executable specification, checked against ``pyarrow.compute.match_like``
on a CPU and never used on the query path.

A LIKE leaf over a sorted-dictionary column lowers (``exec/compile.py``) to the first of

* exact   - no wildcard: the code comparison ``col = 'v'`` gives;
* prefix  - ``lit%`` alone in its clause and not negated: the code interval ``[lo, hi)`` found
  by binary search of the dictionary (``prefix_code_interval``);
* general - a bitmap over the codes (``like_bitmap``): bit i = entry i matches, built by the
  kernel, or by ``match_like`` on the host when an entry or the program exceeds the kernel's
  caps; either way the scan evaluates it as one more PK_BITMAP predicate.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Tuple

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

TK_LIT, TK_ONE, TK_RUN = 0, 1, 2
MAX_TOKENS = 256                 # csrc/kernels/dict_like.hip kMaxTok
KERNEL_MAX_ENTRY_BYTES = 4096    # longest dictionary entry the kernel takes

# route counters: how LIKE leaves were bound (tests and profiles read them)
LIKE_STATS = {"kernel": 0, "host": 0, "interval": 0, "exact": 0, "cache_hits": 0}


class LikeProgram:
    """Token list of a LIKE pattern: ``kinds[i]`` in (TK_LIT, TK_ONE, TK_RUN), ``bytes_[i]`` the
    literal byte of a TK_LIT token (0 otherwise).  ``cls``: "exact" (no wildcard), "prefix"
    (literal bytes then one ``%``) or "general"; ``literal``: the leading literal bytes."""

    __slots__ = ("pattern", "kinds", "bytes_", "cls", "literal")

    def __init__(self, pattern: str, kinds: bytes, bytes_: bytes):
        self.pattern, self.kinds, self.bytes_ = pattern, kinds, bytes_
        n = len(kinds)
        nlit = 0
        while nlit < n and kinds[nlit] == TK_LIT:
            nlit += 1
        self.literal = bytes_[:nlit]
        if nlit == n:
            self.cls = "exact"
        elif nlit == n - 1 and kinds[-1] == TK_RUN:
            self.cls = "prefix"
        else:
            self.cls = "general"

    def __len__(self):
        return len(self.kinds)

    @property
    def fits_kernel(self) -> bool:
        return len(self.kinds) <= MAX_TOKENS


def compile_like(pattern: str) -> LikeProgram:
    """The token program of ``pattern`` (Spark's LIKE syntax; ``E.check_like_pattern`` has the
    escape rules).  Consecutive ``%`` collapse into one any-run token.  A program may be longer
    than MAX_TOKENS: it then does not fit the kernel (``fits_kernel``)."""
    from ..plan.expressions import check_like_pattern
    check_like_pattern(pattern)
    kinds, lits = bytearray(), bytearray()
    i, n = 0, len(pattern)
    while i < n:
        ch = pattern[i]
        if ch == "\\":
            ch = pattern[i + 1]
            i += 2
        else:
            i += 1
            if ch == "%":
                if not kinds or kinds[-1] != TK_RUN:
                    kinds.append(TK_RUN)
                    lits.append(0)
                continue
            if ch == "_":
                kinds.append(TK_ONE)
                lits.append(0)
                continue
        for b in ch.encode("utf-8"):
            kinds.append(TK_LIT)
            lits.append(b)
    return LikeProgram(pattern, bytes(kinds), bytes(lits))


def _utf8_len(b: int) -> int:
    return 1 if b < 0x80 else 4 if b >= 0xF0 else 3 if b >= 0xE0 else 2 if b >= 0xC0 else 1


def like_match_host(program: LikeProgram, s: bytes) -> bool:
    """``program`` against the UTF-8 bytes ``s``: the single-backtrack-point wildcard loop of
    ``dict_like.hip``, statement for statement."""
    kinds, lits = program.kinds, program.bytes_
    ntok, ln = len(kinds), len(s)
    si = star_s = p = 0
    star_p = -1
    while si < ln:
        k = kinds[p] if p < ntok else -1
        c = s[si]
        if k == TK_LIT and lits[p] == c:
            si += 1
            p += 1
        elif k == TK_ONE:
            si = min(si + _utf8_len(c), ln)
            p += 1
        elif k == TK_RUN:
            star_p = p
            p += 1
            star_s = si
        elif star_p >= 0:
            star_s = min(star_s + _utf8_len(s[star_s]), ln)
            si = star_s
            p = star_p + 1
        else:
            return False
    while p < ntok and kinds[p] == TK_RUN:
        p += 1
    return p == ntok


# ------------------------------------------------------------------------------------------------
# prefix -> code interval
# ------------------------------------------------------------------------------------------------
def _entry_bytes(dictionary: pa.Array, i: int) -> bytes:
    return dictionary[i].as_buffer().to_pybytes()


def _lower_bound(dictionary: pa.Array, key: bytes) -> int:
    lo, hi = 0, len(dictionary)
    while lo < hi:
        mid = (lo + hi) >> 1
        if _entry_bytes(dictionary, mid) < key:
            lo = mid + 1
        else:
            hi = mid
    return lo


def prefix_code_interval(dictionary: pa.Array, prefix: bytes) -> Tuple[int, int]:
    """``[lo, hi)``: the codes of a dictionary sorted on UTF-8 bytes whose entries start with
    ``prefix``.  The upper key is the prefix with its last byte incremented, with carry (trailing
    0xFF bytes drop; nothing left means no upper bound).  O(log n) element reads."""
    lo = _lower_bound(dictionary, prefix)
    up = bytearray(prefix)
    while up and up[-1] == 0xFF:
        up.pop()
    if not up:
        return lo, len(dictionary)
    up[-1] += 1
    return lo, max(lo, _lower_bound(dictionary, bytes(up)))


# ------------------------------------------------------------------------------------------------
# device dictionary + bitmap cache
# ------------------------------------------------------------------------------------------------
class DeviceDictionary:
    """A string dictionary's UTF-8 bytes and int64 offsets on the device, plus what the host
    knows from the offsets (entry count, longest entry)."""

    __slots__ = ("dictionary", "offsets", "chars", "n", "max_len", "__weakref__")

    def __init__(self, dictionary, offsets, chars, n: int, max_len: int):
        self.dictionary, self.offsets, self.chars = dictionary, offsets, chars
        self.n, self.max_len = n, max_len


def dictionary_max_len(dictionary: pa.Array) -> int:
    if not len(dictionary):
        return 0
    return int(pc.max(pc.binary_length(dictionary)).as_py() or 0)


_DEV_DICTS: "OrderedDict[tuple, DeviceDictionary]" = OrderedDict()
_DEV_DICTS_CAP = 64
_BITMAPS: "OrderedDict[tuple, tuple]" = OrderedDict()
_BITMAPS_CAP = 64


def device_dictionary(dictionary: pa.Array, device, cache: bool = True) -> DeviceDictionary:
    """``dictionary`` on ``device``: uploaded once per dictionary object
    (``ops.kernels.dictionary_bytes``, shared with the device hash of dictionary columns) and
    counted against the table caches' budgets while it lives.  ``cache`` false: for a
    dictionary used once (a sketch build's file group); it is not kept and not counted."""
    from ..ops import kernels as K
    from .device_cache import track_derived
    key = (id(dictionary), str(device))
    hit = _DEV_DICTS.get(key)
    if hit is not None and hit.dictionary is dictionary:
        _DEV_DICTS.move_to_end(key)
        return hit
    if not cache:
        offs, chars = K.dictionary_bytes(dictionary, device, cache=False)
        return DeviceDictionary(dictionary, offs, chars, len(dictionary),
                                dictionary_max_len(dictionary))
    offs, chars = K.dictionary_bytes(dictionary, device)
    track_derived(offs)
    track_derived(chars)
    dd = DeviceDictionary(dictionary, offs, chars, len(dictionary), dictionary_max_len(dictionary))
    _DEV_DICTS[key] = dd
    while len(_DEV_DICTS) > _DEV_DICTS_CAP:
        _DEV_DICTS.popitem(last=False)
    return dd


def kernel_eligible(program: LikeProgram, max_len: int) -> bool:
    return program.fits_kernel and max_len <= KERNEL_MAX_ENTRY_BYTES


def host_bitmap_words(dictionary: pa.Array, pattern: str) -> np.ndarray:
    """The host route's bitmap: ``match_like`` over the dictionary, packed little-endian into
    64-bit words (bit i of word i // 64 = entry i matches)."""
    n = len(dictionary)
    m = pc.match_like(dictionary, pattern)
    bits = np.asarray(pc.fill_null(m, False).to_numpy(zero_copy_only=False), dtype=np.uint8)
    packed = np.packbits(bits, bitorder="little")
    out = np.zeros(((n + 63) // 64) * 8, dtype=np.uint8)
    out[:len(packed)] = packed
    return out.view("<u8").astype(np.uint64, copy=False).view(np.int64)


def like_bitmap(dictionary: pa.Array, program: LikeProgram, device):
    """int64 device words of "entry i of ``dictionary`` matches ``program``" (``len(dictionary)``
    bits).  A small LRU keyed by (dictionary identity, pattern, device): a repeated query
    launches nothing.  Never read back."""
    import torch
    from ..ops import kernels as K
    key = (id(dictionary), program.pattern, str(device))
    hit = _BITMAPS.get(key)
    if hit is not None and hit[0] is dictionary:
        _BITMAPS.move_to_end(key)
        LIKE_STATS["cache_hits"] += 1
        return hit[1]
    if kernel_eligible(program, dictionary_max_len(dictionary)):
        words = K.dict_like(device_dictionary(dictionary, device), program)
        LIKE_STATS["kernel"] += 1
    else:
        words = torch.from_numpy(host_bitmap_words(dictionary, program.pattern)).to(device)
        LIKE_STATS["host"] += 1
    _BITMAPS[key] = (dictionary, words)
    while len(_BITMAPS) > _BITMAPS_CAP:
        _BITMAPS.popitem(last=False)
    return words


def clear_caches() -> None:
    _DEV_DICTS.clear()
    _BITMAPS.clear()


__all__ = ["LikeProgram", "compile_like", "like_match_host", "prefix_code_interval",
           "DeviceDictionary", "device_dictionary", "like_bitmap", "host_bitmap_words",
           "kernel_eligible", "LIKE_STATS", "MAX_TOKENS", "KERNEL_MAX_ENTRY_BYTES"]
