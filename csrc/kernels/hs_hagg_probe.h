// The probe scheme of the grouped-aggregation hash tables (hash_agg.hip, distinct_agg.hip):
// open addressing with linear probing over M (a power of two) slots of 64-bit keys, claimed by
// atomicCAS on the key word; the key ~0 is the EMPTY pattern.  Two more slots are addressed
// directly: slot M for a key that equals the EMPTY pattern, slot M + 1 for the NULL key.
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

}  // namespace hs_hagg
