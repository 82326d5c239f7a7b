"""Independent numpy reference of the data-skipping sketches: Spark-style Bloom filters
(Murmur3_x86_32 double hashing) and MinMax in Spark's orderings.  Written from the definitions,
sharing no code with ``hyperspace_amd``: plain Python integers for the hash, numpy only to hold
bits."""
from __future__ import annotations

import math
import struct

import numpy as np

M32 = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _mix_k1(k1):
    k1 = (k1 * 0xCC9E2D51) & M32
    k1 = _rotl(k1, 15)
    return (k1 * 0x1B873593) & M32


def _mix_h1(h1, k1):
    h1 ^= k1
    h1 = _rotl(h1, 13)
    return (h1 * 5 + 0xE6546B64) & M32


def _fmix(h1, length):
    h1 ^= length & M32
    h1 ^= h1 >> 16
    h1 = (h1 * 0x85EBCA6B) & M32
    h1 ^= h1 >> 13
    h1 = (h1 * 0xC2B2AE35) & M32
    return h1 ^ (h1 >> 16)


def hash_long(v: int, seed: int) -> int:
    u = v & 0xFFFFFFFFFFFFFFFF
    h1 = _mix_h1(seed & M32, _mix_k1(u & M32))
    h1 = _mix_h1(h1, _mix_k1(u >> 32))
    return _fmix(h1, 8)


def hash_bytes(b: bytes, seed: int) -> int:
    """hashUnsafeBytes: little-endian words, then every tail byte as its own signed int."""
    h1 = seed & M32
    aligned = len(b) - len(b) % 4
    for i in range(0, aligned, 4):
        h1 = _mix_h1(h1, _mix_k1(int.from_bytes(b[i:i + 4], "little")))
    for i in range(aligned, len(b)):
        byte = b[i] - 256 if b[i] > 127 else b[i]
        h1 = _mix_h1(h1, _mix_k1(byte & M32))
    return _fmix(h1, len(b))


def bloom_params(n: int, p: float):
    """(numWords, k)."""
    num_bits = int(-n * math.log(p) / (math.log(2) ** 2))
    num_words = max(1, (num_bits + 63) // 64)
    k = max(1, int(round(num_bits / n * math.log(2))))
    return num_words, k


def item_hashes(item):
    """(h1, h2) of an int (hashLong of the int64 value) or of bytes / str (UTF-8)."""
    if isinstance(item, str):
        item = item.encode("utf-8")
    if isinstance(item, (bytes, bytearray)):
        h1 = hash_bytes(bytes(item), 0)
        return h1, hash_bytes(bytes(item), h1)
    h1 = hash_long(int(item), 0)
    return h1, hash_long(int(item), h1)


def _signed32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def combined(h1: int, h2: int, i: int) -> int:
    """int32(h1 + i * h2) before the sign fold."""
    return _signed32(h1 + i * h2)


def positions(item, num_words: int, k: int):
    h1, h2 = item_hashes(item)
    out = []
    for i in range(1, k + 1):
        c = combined(h1, h2, i)
        if c < 0:
            c = ~c
        out.append(c % (64 * num_words))
    return out


def bloom_words(items, num_words: int, k: int) -> np.ndarray:
    words = [0] * num_words
    for it in items:
        for b in positions(it, num_words, k):
            words[b >> 6] |= 1 << (b & 63)
    return np.array(words, dtype=np.uint64)


def might_contain(words: np.ndarray, item, k: int) -> bool:
    return all((int(words[b >> 6]) >> (b & 63)) & 1 for b in positions(item, len(words), k))


def serialize(words: np.ndarray, k: int) -> bytes:
    out = struct.pack(">iii", 1, k, len(words))
    for w in words:
        out += struct.pack(">Q", int(w))
    return out


# -- the same definitions over numpy arrays (the kernel tests hash a few hundred thousand keys);
# test_sketch_ref.py checks them against the scalar functions above -------------------------------
def _np_rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def _np_mix_k1(k1):
    return _np_rotl(k1 * np.uint32(0xCC9E2D51), 15) * np.uint32(0x1B873593)


def _np_mix_h1(h1, k1):
    return _np_rotl(h1 ^ k1, 13) * np.uint32(5) + np.uint32(0xE6546B64)


def hash_long_np(values: np.ndarray, seeds: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        u = np.asarray(values, dtype=np.int64).view(np.uint64)
        h1 = _np_mix_h1(np.asarray(seeds, dtype=np.uint32),
                        _np_mix_k1((u & np.uint64(M32)).astype(np.uint32)))
        h1 = _np_mix_h1(h1, _np_mix_k1((u >> np.uint64(32)).astype(np.uint32)))
        h1 = h1 ^ np.uint32(8)
        h1 = (h1 ^ (h1 >> np.uint32(16))) * np.uint32(0x85EBCA6B)
        h1 = (h1 ^ (h1 >> np.uint32(13))) * np.uint32(0xC2B2AE35)
        return h1 ^ (h1 >> np.uint32(16))


def item_hashes_np(values: np.ndarray):
    h1 = hash_long_np(values, np.zeros(len(values), np.uint32))
    return h1, hash_long_np(values, h1)


def combined_np(h1: np.ndarray, h2: np.ndarray, i: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return (h1 + np.uint32(i) * h2).astype(np.uint32).view(np.int32)


def bloom_words_np(h1: np.ndarray, h2: np.ndarray, num_words: int, k: int) -> np.ndarray:
    """The filter words of items given by their (h1, h2) arrays."""
    bits = np.zeros(64 * num_words, dtype=np.uint8)
    for i in range(1, k + 1):
        c = combined_np(h1, h2, i).astype(np.int64)
        c = np.where(c < 0, ~c, c)
        bits[c % (64 * num_words)] = 1
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def minmax(values, valid=None):
    """(min, max, non-null count) in Spark's order; floats: NaN largest, -0.0 stored as 0.0.
    min / max are None without a non-null value.  NaN results are float('nan')."""
    vals = [v for i, v in enumerate(values) if valid is None or valid[i]]
    if not vals:
        return None, None, 0
    if isinstance(vals[0], (float, np.floating)):
        t = type(vals[0])

        def key(v):
            return (1, 0.0) if v != v else (0, float(v))
        mn, mx = min(vals, key=key), max(vals, key=key)
        mn = t(0.0) if mn == 0 else mn
        mx = t(0.0) if mx == 0 else mx
        return mn, mx, len(vals)
    return min(vals), max(vals), len(vals)
