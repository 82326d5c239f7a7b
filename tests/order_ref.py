"""Independent numpy reference of the key order the sort, merge and range-search kernels share.

Nothing here calls the package: the images are written from the types' definitions, the sort is
``np.lexsort`` and the searches are ``np.searchsorted``, so a kernel and its host mirror cannot
agree with this module by sharing a mistake.

The order: ascending, NULLS FIRST, stable.  Integers order by value; floats order by their bit
pattern as a sign-magnitude number (sign-bit NaN < -inf < ... < -0.0 < +0.0 < ... < +inf <
positive NaN), which is the IEEE total order.
"""
import numpy as np

KIND_OF_DTYPE = {np.dtype(np.int8): "I8", np.dtype(np.int16): "I16", np.dtype(np.int32): "I32",
                 np.dtype(np.int64): "I64", np.dtype(np.float32): "F32",
                 np.dtype(np.float64): "F64", np.dtype(np.uint8): "BOOL",
                 np.dtype(np.bool_): "BOOL", np.dtype(np.uint32): "U32"}
_INT_WIDTH = {"I8": 8, "I16": 16, "I32": 32, "I64": 64}


def ref_image(np_values, kind: str) -> np.ndarray:
    """Order-preserving uint64 image of every value: a < b in the key order <=> image(a) <
    image(b).  Signed integers are offset by 2^(width-1); a float's bits are complemented when
    its sign bit is set and get the sign bit set otherwise; BOOL and U32 are their value."""
    v = np.asarray(np_values)
    if kind in _INT_WIDTH:
        w = _INT_WIDTH[kind]
        v = v.astype(np.dtype(f"int{w}"))
        if w == 64:
            # value + 2^63 modulo 2^64
            return v.view(np.uint64) + np.uint64(1 << 63)
        return (v.astype(np.int64) + (1 << (w - 1))).astype(np.uint64)
    if kind == "F32":
        b = v.astype(np.float32).view(np.uint32)
        neg = (b >> np.uint32(31)).astype(bool)
        return np.where(neg, ~b, b | np.uint32(1 << 31)).astype(np.uint64)
    if kind == "F64":
        b = v.astype(np.float64).view(np.uint64)
        neg = (b >> np.uint64(63)).astype(bool)
        return np.where(neg, ~b, b | np.uint64(1 << 63)).astype(np.uint64)
    if kind in ("BOOL", "U32"):
        return v.astype(np.uint64)
    raise ValueError(kind)


def _kind(values) -> str:
    return KIND_OF_DTYPE[np.asarray(values).dtype]


def _masked_image(values, null_mask):
    img = ref_image(values, _kind(values))
    if null_mask is None:
        return img, np.ones(len(img), np.uint8)
    null_mask = np.asarray(null_mask, bool)
    return np.where(null_mask, np.uint64(0), img), (~null_mask).astype(np.uint8)


def ref_sort_perm(keys, leading=None, init=None) -> np.ndarray:
    """Stable ascending NULLS FIRST permutation over ``keys`` = [(values, null_mask or None), ...],
    most significant first, below an optional most significant integer key ``leading``.  With
    ``init`` (a permutation) the rows are taken in that order first, so ties keep ``init``'s
    order."""
    n = len(keys[0][0])
    take = np.arange(n) if init is None else np.asarray(init, np.int64)
    cols = [np.arange(n)]                           # least significant: position (stability)
    for values, null_mask in reversed(keys):
        img, valid = _masked_image(values, null_mask)
        cols += [img[take], valid[take]]
    if leading is not None:
        cols.append(np.asarray(leading)[take])
    return take[np.lexsort(tuple(cols))]


def _u64(x):
    return np.uint64(int(x) & 0xFFFFFFFFFFFFFFFF)


def ref_ranges(values, null_mask, bucket_off, buckets, lo, lo_incl, hi, hi_incl):
    """(rstart, rlen, rbucket) of the rows of each bucket whose key image lies in the interval
    ``lo``..``hi`` (uint64 images; None: unbounded on that side).  Every bucket holds its nulls
    first, then its non-null keys ascending; nulls never match.  An empty interval has length 0
    at the position of its lower bound."""
    img = ref_image(values, _kind(values))
    nulls = np.zeros(len(img), bool) if null_mask is None else np.asarray(null_mask, bool)
    bucket_off = np.asarray(bucket_off, np.int64)
    bs = np.arange(len(bucket_off) - 1) if buckets is None else np.asarray(buckets)
    rstart, rlen = np.zeros(len(bs), np.int64), np.zeros(len(bs), np.int64)
    for i, b in enumerate(bs):
        s, e = int(bucket_off[b]), int(bucket_off[b + 1])
        first = s + int(nulls[s:e].sum())
        assert not nulls[first:e].any(), "nulls must be a prefix of the bucket"
        seg = img[first:e]
        a = 0 if lo is None else int(np.searchsorted(seg, _u64(lo), "left" if lo_incl else "right"))
        z = len(seg) if hi is None else \
            int(np.searchsorted(seg, _u64(hi), "right" if hi_incl else "left"))
        rstart[i] = first + a
        rlen[i] = max(z, a) - a
    return rstart, rlen, bs.astype(np.int32)


def ref_probe(values, null_mask, bucket_off, pbucket, pkey):
    """(rstart, rlen, rbucket) per probe: the run of rows of bucket ``pbucket[i]`` whose key image
    equals ``pkey[i]``."""
    out = [ref_ranges(values, null_mask, bucket_off, [b], k, True, k, True)
           for b, k in zip(np.asarray(pbucket).tolist(), np.asarray(pkey).tolist())]
    if not out:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3))


def _from_bits(bits, utype, ftype):
    return np.array(bits, dtype=utype).view(ftype)


# ascending in the key order: NaN with both signs and two payloads, +-inf, +-max finite,
# 1.5, +-min denormal, +-0.0
SPECIAL_F64 = _from_bits(
    [0xFFF800000000BEEF, 0xFFF8000000000000, 0xFFF0000000000000, 0xFFEFFFFFFFFFFFFF,
     0x8000000000000001, 0x8000000000000000, 0x0000000000000000, 0x0000000000000001,
     0x3FF8000000000000, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000, 0x7FF8000000000000,
     0x7FF800000000BEEF], np.uint64, np.float64)
SPECIAL_F32 = _from_bits(
    [0xFFC0BEEF, 0xFFC00000, 0xFF800000, 0xFF7FFFFF, 0x80000001, 0x80000000, 0x00000000,
     0x00000001, 0x3FC00000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7FC0BEEF],
    np.uint32, np.float32)
