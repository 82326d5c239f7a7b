"""A plain numpy reference of the hash-join kernels (csrc/kernels/hash_join.hip) with the same
contracts, and the case lists the CPU and the GPU tests share.

* build: the build rows with a non-NULL key, stably sorted by key (``perm``); ``nkeys`` distinct
  keys; ``unique`` when no key repeats; ``slots`` = the power of two >= max(64, 2 * build rows).
* probe: stream rows in their order; the matches of one stream row are its key's build rows in
  ascending row order.  ``"pairs"`` gives (stream ids, build ids), ``"preserve"`` adds
  (row, -1) for an unmatched stream row in its place, ``"mark"`` gives one 0 / 1 byte per probed
  row.  A NULL key matches nothing on either side.

Sort-based (``numpy.searchsorted``), so it shares nothing with the device's hash table; it is
itself checked against ``pyarrow.Table.join`` in tests/test_hash_join_ref.py."""
import functools

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ROWS_PER_LANE = 4                  # hs_hj_rows_per_lane(); the GPU test checks it
TILE = 256 * ROWS_PER_LANE         # stream rows of one probe block
BUILD_SIZES = (0, 1, 2, 64, 65, 1000)
PROBE_SIZES = (0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
MODES = ("pairs", "preserve", "mark")


# ------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------
def ref_slots(nbuild: int) -> int:
    m = 64
    while m < 2 * nbuild:
        m *= 2
    return m


def ref_build(keys, valid=None, rows=None) -> dict:
    keys = np.asarray(keys).astype(np.int64)
    ids = np.arange(len(keys), dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    if valid is not None:
        ids = ids[np.asarray(valid)[ids] != 0]
    perm = ids[np.argsort(keys[ids], kind="stable")]
    sk = keys[perm]
    nkeys = int(len(np.unique(sk)))
    return {"perm": perm, "sorted_keys": sk, "nbuild": int(len(perm)), "nkeys": nkeys,
            "unique": nkeys == len(perm), "slots": ref_slots(len(perm))}


def ref_probe(table: dict, keys, valid=None, rows=None, how="pairs"):
    keys = np.asarray(keys).astype(np.int64)
    ids = np.arange(len(keys), dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    k = keys[ids]
    sk, perm = table["sorted_keys"], table["perm"]
    lo = np.searchsorted(sk, k, side="left")
    cnt = np.searchsorted(sk, k, side="right") - lo
    if valid is not None:
        cnt = np.where(np.asarray(valid)[ids] != 0, cnt, 0)
    if how == "mark":
        return (cnt > 0).astype(np.uint8)
    out = np.maximum(cnt, 1) if how == "preserve" else cnt
    total = int(out.sum())
    start = np.cumsum(out) - out
    sid = np.repeat(ids, out)
    within = np.arange(total, dtype=np.int64) - np.repeat(start, out)
    matched = np.repeat(cnt > 0, out)
    at = np.where(matched, np.repeat(lo, out) + within, 0)
    bid = np.where(matched, perm[at] if len(perm) else 0, -1).astype(np.int64)
    return sid.astype(np.int64), bid


def brute_probe(bkeys, bvalid, skeys, svalid, rows, how):
    """The contract as two Python loops (small inputs only)."""
    ids = range(len(skeys)) if rows is None else [int(r) for r in rows]
    sid, bid, mark = [], [], []
    for r in ids:
        m = [j for j in range(len(bkeys))
             if (svalid is None or svalid[r]) and (bvalid is None or bvalid[j]) and
             int(bkeys[j]) == int(skeys[r])]
        mark.append(1 if m else 0)
        if not m and how == "preserve":
            m = [-1]
        sid += [r] * len(m)
        bid += m
    if how == "mark":
        return np.asarray(mark, np.uint8)
    return np.asarray(sid, np.int64), np.asarray(bid, np.int64)


# ------------------------------------------------------------------------------------------------
# the device's hash (hs_hagg_probe.h), for the collision set
# ------------------------------------------------------------------------------------------------
def mix64(k: np.ndarray) -> np.ndarray:
    h = np.asarray(k).astype(np.int64).view(np.uint64).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h


@functools.lru_cache(maxsize=None)
def colliding_keys(slots: int, home: int, count: int) -> np.ndarray:
    """The first ``count`` non-negative integers whose home slot in a table of ``slots`` slots
    is ``home`` (brute force over consecutive integers)."""
    found, base = [], 0
    while sum(len(f) for f in found) < count:
        k = np.arange(base, base + (1 << 16), dtype=np.int64)
        found.append(k[(mix64(k) & np.uint64(slots - 1)) == np.uint64(home)])
        base += 1 << 16
    return np.concatenate(found)[:count]


# ------------------------------------------------------------------------------------------------
# cases: name -> (build keys, build valid or None, stream-key maker)
# ------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, bkeys, bvalid, pool, svalid_rate=0.0):
        self.name, self.bkeys, self.bvalid = name, bkeys, bvalid
        self.pool, self.svalid_rate = np.asarray(pool), svalid_rate

    def stream(self, n: int):
        """(stream keys in the pool's dtype, valid or None) of n rows: keys drawn from the pool
        (present and absent ones)."""
        rng = np.random.default_rng(77 + n)
        keys = self.pool[rng.integers(0, len(self.pool), n)] if n else self.pool[:0]
        valid = None
        if self.svalid_rate:
            valid = (rng.random(n) >= self.svalid_rate).astype(np.uint8)
        return keys, valid


def _unique_case(nb: int) -> Case:
    rng = np.random.default_rng(nb)
    b = rng.permutation(np.arange(nb, dtype=np.int64) * 3 + 1)
    return Case(f"unique{nb}", b, None, np.arange(-2, 3 * nb + 4, dtype=np.int64))


def _mixed_case(nb: int) -> Case:
    rng = np.random.default_rng(100 + nb)
    b = rng.integers(0, max(1, nb // 3), nb).astype(np.int64) * 5
    return Case(f"mixed{nb}", b, None, np.arange(-5, 5 * max(1, nb // 3) + 5, dtype=np.int64))


def _special_case(present: bool) -> Case:
    special = np.array([-1, 0, I64_MIN, I64_MAX], dtype=np.int64)
    other = np.array([5, -7, 1 << 40, -(1 << 40), 2, -2], dtype=np.int64)
    b = np.concatenate([other, special, special[:1], special[2:3]]) if present else other
    return Case("special_present" if present else "special_absent", b, None,
                np.concatenate([special, other, np.array([9, -9], np.int64)]))


def _width_case(bdt, sdt) -> Case:
    rng = np.random.default_rng(5)
    b = rng.integers(-128, 128, 300).astype(bdt)
    b[:3] = (-1, 0, -128)
    return Case(f"width_{np.dtype(bdt).name}_{np.dtype(sdt).name}", b, None,
                np.arange(-128, 128).astype(sdt))


def _null_case() -> Case:
    rng = np.random.default_rng(9)
    b = rng.integers(-3, 40, 500).astype(np.int64)
    return Case("nulls", b, (rng.random(500) >= 0.2).astype(np.uint8),
                np.arange(-6, 46, dtype=np.int64), svalid_rate=0.25)


def _same_case() -> Case:
    return Case("same1000", np.full(1000, 7, dtype=np.int64), None,
                np.array([7, 7, 7, 8, 6], dtype=np.int64))


def _collision_case() -> Case:
    """64 build keys (128 slots): 44 of them share the home slot 125, so their cluster runs
    125, 126, 127, 0, 1, ... - linear probing wraps; the stream also asks for 12 absent keys
    with that home slot, which walk the whole cluster to its end."""
    nb = 64
    slots = ref_slots(nb)
    assert slots == 128
    same = colliding_keys(slots, slots - 3, 56)
    rest = np.arange(10_000_000, 10_000_000 + nb - 44, dtype=np.int64)
    b = np.concatenate([same[:44], rest])
    b = b[np.random.default_rng(3).permutation(nb)]
    return Case("collisions", b, None, np.concatenate([same, rest, rest + 1000]))


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = [_unique_case(nb) for nb in BUILD_SIZES] + [_mixed_case(nb) for nb in BUILD_SIZES]
    out += [_special_case(True), _special_case(False), _null_case(), _same_case(),
            _collision_case()]
    out += [_width_case(b, s) for b, s in ((np.int8, np.int64), (np.int16, np.int32),
                                           (np.int32, np.int8), (np.int64, np.int16))]
    return {c.name: c for c in out}


def row_list(n_src: int, n: int) -> np.ndarray:
    """n ascending row ids out of n_src rows."""
    return np.sort(np.random.default_rng(n_src + n).choice(n_src, size=n, replace=False)) \
        .astype(np.int64)
