"""The numpy reference of the data-skipping sketches (tests/sketch_ref.py), checked where there
is no GPU: the worked parameter table and bit positions of the Bloom definition, the
serialization layout, no false negatives, a cap on its false-positive share, and MinMax's
orderings."""
import struct

import numpy as np
import pytest

import sketch_ref as R


@pytest.mark.parametrize("n,p,words,k", [(1000, 0.01, 150, 7), (1000, 0.1, 75, 3),
                                         (100, 0.01, 15, 7), (5, 0.01, 1, 7),
                                         (20000, 0.001, 4493, 10)])
def test_parameter_table(n, p, words, k):
    assert R.bloom_params(n, p) == (words, k)


@pytest.mark.parametrize("key,expected", [
    (0, [9384, 1707, 3199, 4691, 7512, 6020, 5071]),
    (1, [7969, 6017, 3291, 8504, 5482, 269, 9039]),
    (-1, [2378, 6444, 8689, 4623, 3538, 7604, 2070])])
def test_bit_positions(key, expected):
    assert R.positions(key, 150, 7) == expected


def test_bit_layout_and_serialization():
    words = R.bloom_words([0], 150, 7)
    for b in R.positions(0, 150, 7):
        assert (int(words[b >> 6]) >> (b & 63)) & 1
    assert sum(bin(int(w)).count("1") for w in words) == len(set(R.positions(0, 150, 7)))
    blob = R.serialize(words, 7)
    assert len(blob) == 12 + 8 * 150
    assert struct.unpack(">iii", blob[:12]) == (1, 7, 150)
    assert list(struct.unpack(">150q", blob[12:])) == [int(w) - (1 << 64) if int(w) >> 63
                                                       else int(w) for w in words]


def test_string_hash_tail_bytes():
    # hashUnsafeBytes of "" is fmix(seed, 0); a high tail byte mixes as a negative int
    assert R.hash_bytes(b"", 0) == 0
    assert R.hash_bytes(b"\xff", 0) != R.hash_bytes(b"\x7f", 0)
    assert R.hash_bytes(b"abcd", 0) == R._fmix(R._mix_h1(0, R._mix_k1(0x64636261)), 4)
    assert R.hash_bytes(b"abcd\x80", 0) == R._fmix(
        R._mix_h1(R._mix_h1(0, R._mix_k1(0x64636261)), R._mix_k1(0xFFFFFF80)), 5)


def test_no_false_negatives_and_false_positive_cap():
    rng = np.random.default_rng(20240611)
    keys = rng.integers(-2 ** 63, 2 ** 63 - 1, 1000, dtype=np.int64)
    nw, k = R.bloom_params(1000, 0.01)
    words = R.bloom_words(keys.tolist(), nw, k)
    assert all(R.might_contain(words, int(v), k) for v in keys)
    present = set(keys.tolist())
    absent = [int(v) for v in rng.integers(-2 ** 63, 2 ** 63 - 1, 200_100, dtype=np.int64)
              if int(v) not in present][:200_000]
    assert len(absent) == 200_000
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").tolist()
    fp = sum(all(bits[b] for b in R.positions(v, nw, k)) for v in absent)
    share = fp / len(absent)
    print(f"false-positive share {share:.4f}")
    assert share <= 0.02


def test_negative_combined_hashes_exist():
    negs = 0
    for v in range(64):
        h1, h2 = R.item_hashes(v)
        negs += sum(R.combined(h1, h2, i) < 0 for i in range(1, 8))
    assert negs > 0


def test_numpy_forms_equal_the_scalar_definitions():
    rng = np.random.default_rng(5)
    keys = np.concatenate([rng.integers(-2 ** 63, 2 ** 63 - 1, 500, dtype=np.int64),
                           np.array([0, 1, -1, 2 ** 63 - 1, -2 ** 63], dtype=np.int64)])
    h1, h2 = R.item_hashes_np(keys)
    assert [(int(a), int(b)) for a, b in zip(h1, h2)] == [R.item_hashes(int(v)) for v in keys]
    for i in (1, 7):
        assert R.combined_np(h1, h2, i).tolist() == [R.combined(int(a), int(b), i)
                                                     for a, b in zip(h1, h2)]
    for nw, k in ((1, 1), (3, 7), (150, 7)):
        assert np.array_equal(R.bloom_words_np(h1, h2, nw, k),
                              R.bloom_words(keys.tolist(), nw, k))


def test_minmax_orderings():
    nan = float("nan")
    mn, mx, cnt = R.minmax([1.0, nan, -0.0, float("inf")])
    assert mn == 0.0 and str(mn) == "0.0" and mx != mx and cnt == 4
    mn, mx, cnt = R.minmax([-0.0, -1.5], valid=[1, 1])
    assert (mn, mx, cnt) == (-1.5, 0.0, 2) and str(mx) == "0.0"
    assert R.minmax([3, 1, 2], valid=[0, 1, 1]) == (1, 2, 2)
    assert R.minmax([3, 1], valid=[0, 0]) == (None, None, 0)
    assert R.minmax([nan, nan])[0] != R.minmax([nan, nan])[0]
    assert R.minmax([b"\xc3\xa9", b"z", b"a"]) == (b"a", b"\xc3\xa9", 3)
