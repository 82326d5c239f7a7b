// Broadcast hash join (exec/gpu_hash_join.py): a hash table over the small ("build") side, the
// large ("stream") side probes it in one pass.  gfx950, wave64.
//
// Keys are 64-bit integers read with load_i64 through a ColDesc (any integer width, dates,
// timestamps, booleans, dictionary codes): the column itself, no widened copy.  A row set is
// "all n rows" (rows == nullptr) or an ascending int64 row-id list.
//
// Table (the layout of hs_hagg_probe.h): M slots (a power of two, M >= 2 x build keys) of 64-bit
// keys claimed by atomicCAS, EMPTY = ~0; slot M belongs to the key that equals the EMPTY pattern
// (the integer -1).  Beside the keys, first[M + 2] and last[M + 2] (int32, -1 = unset) are
// positions into perm, the build rows with a non-NULL key stably sorted by key: the matches of a
// key are the contiguous perm[first .. last], in ascending build-row order.
//
//   hs_hj_build   one lane per position i of perm.  The lane whose key differs from position
//                 i - 1 (or i == 0) inserts the key and stores first[slot] = i; the lane whose key
//                 differs from position i + 1 (or i == nb - 1) inserts it and stores
//                 last[slot] = i.  Whichever arrives first claims the slot, the other finds it.
//                 One launch, no ordering between blocks, no atomic but the claiming CAS.  With
//                 load <= 0.5 an insert bounded by M probes always succeeds.
//   hs_hj_probe   one pass over the stream rows; a lane takes R rows (strided by the block, so
//                 loads stay coalesced) and issues their R table reads together
//                 (hs_hagg::probe_find_n).  Per row: the slot (int32, -1: no match or NULL key),
//                 the match count (int64; max(count, 1) in the preserved-side form), a 0 / 1 mark
//                 byte, and for a table of unique keys the one build row id (or -1) - each output
//                 optional.
//   hs_hj_emit    from the exclusive scan of the counts, one lane per stream row writes its
//                 (stream row id, build row id) pairs; -1 is the build id of an unmatched
//                 preserved row.  first / last are clamped into [0, nb) before perm is indexed
//                 and writes stay inside [offs[i], offs[i + 1]): a table not made by hs_hj_build
//                 cannot read or write out of range.
//
// Every load and store is guarded by its row count; stores are plain vector stores; no loop's
// exit depends on another lane or block (every probe loop ends after at most M steps).
#include "hs_common.h"
#include "hs_hagg_probe.h"

namespace {

constexpr int NT = 256;
// Rows per lane of the probe, measured on an MI355X over 2^26 int64 stream rows, ~80 % hits, with
// `benchmarks/configs.py --config broadcast_join --probe-sweep` (profiles/broadcast_join.txt;
// ms for 1 / 2 / 4 / 8 rows per lane):
//   25-key table (64 slots),  mark only      0.54  0.52  0.46  0.68
//   25-key table,             mark + row id  0.66  0.64  0.59  0.82
//   1M-key table (2 Mi slots), mark only     1.04  1.00  1.05  1.26
//   1M-key table,             mark + row id  2.58  2.66  2.92  2.87
// Four is 12-15 % ahead of one where the table sits in L1 / L2 (the common small dimension) and
// 1-13 % behind where every probe leaves L2; eight loses occupancy (102 VGPRs) everywhere.
constexpr int HJ_DEFAULT_ROWS_PER_LANE = 4;
constexpr int64_t HJ_MAX_SLOTS = (int64_t)1 << 30;   // slots are int32, probe counts are int

struct HjTable {
  const unsigned long long* keys;   // M + 2
  const int32_t* first;             // M + 2
  const int32_t* last;              // M + 2
  const int32_t* perm;              // nb
  int64_t M;
  int64_t nb;
};

// key of build position i; false when the position names no usable row
__device__ __forceinline__ bool build_key(const ColDesc& c, int64_t n_src,
                                          const int32_t* __restrict__ perm, int64_t i,
                                          unsigned long long* key) {
  const int64_t r = perm[i];
  if (r < 0 || r >= n_src || !col_valid(c, r)) return false;
  *key = (unsigned long long)load_i64(c, r);
  return true;
}

__global__ __launch_bounds__(NT) void hj_build_kernel(ColDesc c, int64_t n_src,
                                                      const int32_t* __restrict__ perm, int64_t nb,
                                                      unsigned long long* __restrict__ keys,
                                                      int32_t* __restrict__ first,
                                                      int32_t* __restrict__ last, int64_t M) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= nb) return;
  unsigned long long key, other;
  if (!build_key(c, n_src, perm, i, &key)) return;
  const bool head = i == 0 || !build_key(c, n_src, perm, i - 1, &other) || other != key;
  const bool tail = i == nb - 1 || !build_key(c, n_src, perm, i + 1, &other) || other != key;
  if (!head && !tail) return;
  const long long slot = hs_hagg::probe_insert(keys, M, key, false, (int)M);
  if (slot < 0) return;     // load > 0.5 only: the host sizes M >= 2 nb
  if (head) first[slot] = (int32_t)i;
  if (tail) last[slot] = (int32_t)i;
}

struct HjProbeOut {
  int32_t* slot;      // n or null
  int64_t* count;     // n or null
  uint8_t* mark;      // n or null
  int64_t* build;     // n or null: perm[first[slot]] or -1
  int32_t preserve;   // count = max(count, 1)
  int32_t pad;
};

template <int R>
__global__ __launch_bounds__(NT) void hj_probe_kernel(ColDesc c, int64_t n_src,
                                                      const int64_t* __restrict__ rows, int64_t n,
                                                      HjTable t, HjProbeOut o) {
  const int64_t base = (int64_t)blockIdx.x * (NT * R) + threadIdx.x;
  unsigned long long key[R];
  bool is_null[R];
  long long slot[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int64_t i = base + (int64_t)k * NT;
    key[k] = 0;
    is_null[k] = true;
    if (i < n) {
      const int64_t r = rows ? rows[i] : i;
      if (r >= 0 && r < n_src && col_valid(c, r)) {
        key[k] = (unsigned long long)load_i64(c, r);
        is_null[k] = false;
      }
    }
  }
  if (R == 1) {
    slot[0] = hs_hagg::probe_find(t.keys, t.M, key[0], is_null[0]);
  } else {
    hs_hagg::probe_find_n<R>(t.keys, t.M, key, is_null, slot);
  }
  const bool need_first = o.count != nullptr || o.build != nullptr;
  int32_t f[R], l[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const bool look = slot[k] >= 0 && (need_first || slot[k] == t.M);
    f[k] = look ? t.first[slot[k]] : 0;
    l[k] = (look && o.count != nullptr) ? t.last[slot[k]] : f[k];
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int64_t i = base + (int64_t)k * NT;
    if (i >= n) continue;
    int64_t cnt = 0;
    if (slot[k] >= 0 && f[k] >= 0 && l[k] >= f[k] && (int64_t)l[k] < t.nb)
      cnt = (int64_t)l[k] - f[k] + 1;
    if (cnt == 0) slot[k] = -1;     // absent (also: slot M never stored)
    if (o.slot) o.slot[i] = (int32_t)slot[k];
    if (o.count) o.count[i] = (o.preserve && cnt == 0) ? 1 : cnt;
    if (o.mark) o.mark[i] = cnt > 0 ? 1 : 0;
    if (o.build) o.build[i] = cnt > 0 ? (int64_t)t.perm[f[k]] : -1;
  }
}

__global__ __launch_bounds__(NT) void hj_emit_kernel(const int64_t* __restrict__ rows, int64_t n,
                                                     const int32_t* __restrict__ slots,
                                                     const int64_t* __restrict__ offs,
                                                     int64_t total, HjTable t, int preserve,
                                                     int64_t* __restrict__ out_stream,
                                                     int64_t* __restrict__ out_build) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  int64_t off = offs[i];
  int64_t end = i + 1 < n ? offs[i + 1] : total;
  if (end > total) end = total;
  if (off < 0 || off >= end) return;
  const int64_t row = rows ? rows[i] : i;
  const int64_t s = slots[i];
  int64_t f = 0, cnt = 0;
  if (s >= 0 && s <= t.M && t.nb > 0) {
    f = t.first[s];
    int64_t l = t.last[s];
    if (f >= 0 && l >= f) {      // an unset or reversed pair holds no match
      if (f > t.nb - 1) f = t.nb - 1;
      if (l > t.nb - 1) l = t.nb - 1;
      cnt = l - f + 1;
    }
  }
  if (cnt == 0) {
    if (preserve) {
      out_stream[off] = row;
      out_build[off] = -1;
    }
    return;
  }
  if (cnt > end - off) cnt = end - off;
  for (int64_t j = 0; j < cnt; ++j) {
    out_stream[off + j] = row;
    out_build[off + j] = (int64_t)t.perm[f + j];
  }
}

bool table_ok(int64_t M, int64_t nb) {
  return M >= 64 && M <= HJ_MAX_SLOTS && (M & (M - 1)) == 0 && nb >= 0 && 2 * nb <= M;
}

template <int R>
int launch_probe(const ColDesc& c, int64_t n_src, const int64_t* rows, int64_t n,
                 const HjTable& t, const HjProbeOut& o, hipStream_t s) {
  const int64_t tiles = (n + (int64_t)NT * R - 1) / ((int64_t)NT * R);
  if (tiles > 0x7fffffffll) return -2;
  hipLaunchKernelGGL(hj_probe_kernel<R>, dim3((unsigned)tiles), dim3(NT), 0, s, c, n_src, rows, n,
                     t, o);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// Stream rows one lane takes when hs_hj_probe is called with rows_per_lane = 0.
int hs_hj_rows_per_lane() { return HJ_DEFAULT_ROWS_PER_LANE; }

// keys: M + 2 words, every one EMPTY (~0); first / last: M + 2 int32, every one -1.  perm: nb row
// ids of `key` (n_src rows), sorted by key.  M: a power of two in [64, 2^30], M >= 2 nb.
int hs_hj_build(const ColDesc* key, int64_t n_src, const int32_t* perm, int64_t nb,
                unsigned long long* keys, int32_t* first, int32_t* last, int64_t M,
                void* stream) {
  if (!table_ok(M, nb)) return -1;
  if (nb == 0) return 0;
  const int64_t grid = (nb + NT - 1) / NT;
  if (grid > 0x7fffffffll) return -2;
  hipLaunchKernelGGL(hj_build_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream,
                     *key, n_src, perm, nb, keys, first, last, M);
  return (int)hipGetLastError();
}

// Probes n stream rows of `key` (n_src rows; rows: n ascending row ids or null for rows 0..n-1).
// slot_out (int32), count_out (int64), mark_out (uint8), build_out (int64): n each, any may be
// null.  rows_per_lane: 1, 2, 4 or 8; 0 = the default.
int hs_hj_probe(const ColDesc* key, int64_t n_src, const int64_t* rows, int64_t n,
                const unsigned long long* keys, const int32_t* first, const int32_t* last,
                const int32_t* perm, int64_t M, int64_t nb, int preserve, int rows_per_lane,
                int32_t* slot_out, int64_t* count_out, uint8_t* mark_out, int64_t* build_out,
                void* stream) {
  if (!table_ok(M, nb)) return -1;
  if (n <= 0) return 0;
  if (rows == nullptr && n > n_src) return -1;
  const HjTable t{keys, first, last, perm, M, nb};
  const HjProbeOut o{slot_out, count_out, mark_out, build_out, preserve ? 1 : 0, 0};
  hipStream_t s = (hipStream_t)stream;
  switch (rows_per_lane == 0 ? HJ_DEFAULT_ROWS_PER_LANE : rows_per_lane) {
    case 1: return launch_probe<1>(*key, n_src, rows, n, t, o, s);
    case 2: return launch_probe<2>(*key, n_src, rows, n, t, o, s);
    case 4: return launch_probe<4>(*key, n_src, rows, n, t, o, s);
    case 8: return launch_probe<8>(*key, n_src, rows, n, t, o, s);
    default: return -1;
  }
}

// slots: hs_hj_probe's slot_out; offs: the exclusive scan of its count_out; total: their sum.
// out_stream / out_build: total int64 each.
int hs_hj_emit(const int64_t* rows, int64_t n, const int32_t* slots, const int64_t* offs,
               int64_t total, const int32_t* first, const int32_t* last, const int32_t* perm,
               int64_t M, int64_t nb, int preserve, int64_t* out_stream, int64_t* out_build,
               void* stream) {
  if (!table_ok(M, nb)) return -1;
  if (n <= 0 || total <= 0) return 0;
  const int64_t grid = (n + NT - 1) / NT;
  if (grid > 0x7fffffffll) return -2;
  const HjTable t{(const unsigned long long*)nullptr, first, last, perm, M, nb};
  hipLaunchKernelGGL(hj_emit_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream, rows,
                     n, slots, offs, total, t, preserve ? 1 : 0, out_stream, out_build);
  return (int)hipGetLastError();
}

}  // extern "C"
