// The probe scheme of the grouped-aggregation hash tables (hash_agg.hip, distinct_agg.hip):
// open addressing with linear probing over M (a power of two) slots of 64-bit keys, claimed by
// atomicCAS on the key word; the key ~0 is the EMPTY pattern.  Two more slots are addressed
// directly: slot M for a key that equals the EMPTY pattern, slot M + 1 for the NULL key.  The join
// hash table (hash_join.hip) has the same layout and also looks keys up without inserting them
// (probe_find, probe_find_n).
#pragma once
#include <hip/hip_runtime.h>

namespace hs_hagg {

constexpr unsigned long long kEmpty = ~0ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// Slot of `key` (null: the NULL slot), inserting it if absent; -1 when the probe sequence
// exceeds max_probe (the caller flags overflow and re-runs with a larger table).
__device__ __forceinline__ long long probe_insert(unsigned long long* keys, long long M,
                                                  unsigned long long key, bool is_null,
                                                  int max_probe) {
  if (is_null) return M + 1;
  if (key == kEmpty) return M;
  unsigned long long h = mix64(key) & (unsigned long long)(M - 1);
  for (int p = 0; p < max_probe; ++p) {
    const unsigned long long prev = atomicCAS(&keys[h], kEmpty, key);
    if (prev == kEmpty || prev == key) return (long long)h;
    h = (h + 1) & (unsigned long long)(M - 1);
  }
  return -1;
}

// Slot of `key` in a finished table (no lane is inserting any more), or -1 when it is absent or
// NULL; reads only.  A key equal to the EMPTY pattern answers slot M whether or not it was
// inserted: the caller looks at what it keeps for slot M.  At most M probes, so a table with no
// EMPTY slot left still ends the search.
__device__ __forceinline__ long long probe_find(const unsigned long long* keys, long long M,
                                                unsigned long long key, bool is_null) {
  if (is_null) return -1;
  if (key == kEmpty) return M;
  unsigned long long h = mix64(key) & (unsigned long long)(M - 1);
  for (long long p = 0; p < M; ++p) {
    const unsigned long long k = keys[h];
    if (k == key) return (long long)h;
    if (k == kEmpty) return -1;
    h = (h + 1) & (unsigned long long)(M - 1);
  }
  return -1;
}

// probe_find for R keys of one lane at once: every step issues the R table reads before it looks
// at any of them, so the lane waits for one memory round trip per step, not per key.  slot[k]
// comes out as probe_find(keys, M, key[k], is_null[k]).
template <int R>
__device__ __forceinline__ void probe_find_n(const unsigned long long* keys, long long M,
                                             const unsigned long long (&key)[R],
                                             const bool (&is_null)[R], long long (&slot)[R]) {
  const unsigned long long mask = (unsigned long long)(M - 1);
  unsigned long long h[R];
  bool pend[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    h[k] = mix64(key[k]) & mask;
    pend[k] = !is_null[k] && key[k] != kEmpty;
    slot[k] = (!is_null[k] && key[k] == kEmpty) ? M : -1;
  }
  for (long long p = 0; p < M; ++p) {
    unsigned long long got[R];
#pragma unroll
    for (int k = 0; k < R; ++k) got[k] = pend[k] ? keys[h[k]] : kEmpty;
    bool more = false;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (!pend[k]) continue;
      if (got[k] == key[k]) {
        slot[k] = (long long)h[k];
        pend[k] = false;
      } else if (got[k] == kEmpty) {
        pend[k] = false;
      } else {
        h[k] = (h[k] + 1) & mask;
        more = true;
      }
    }
    if (!more) break;
  }
}

}  // namespace hs_hagg
