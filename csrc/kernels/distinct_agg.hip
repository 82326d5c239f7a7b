// COUNT(DISTINCT x) GROUP BY g..., level 2: regroup the dense groups of a hash aggregate on
// (g..., x) by g... alone.
//
// Level 1 is the ordinary hash-mode aggregate (hash_agg.hip, exec/jit.py) with x as the last,
// highest bit field of the packed key and the query's other functions as its A aggregate slots
// (the last of them the implicit COUNT(*)).  Its dense output holds one row per different
// (g..., x), so per outer group g... the distinct count is the number of its rows whose x is not
// NULL, and every other function is the merge of the rows' partials.
//
// Input: dense groups (SoA, row stride in_cap, n rows): keys[n], nulls[n], sums / cnts [A][in_cap],
// mins / maxs [A][in_cap] (null when the query has no MIN / MAX).  Per row
//   packed key:  outer = key & outer_mask;  nonnull = !x_nullable || (key >> x_shift) != 0
//   raw key (a single unpacked 64-bit x, no outer columns):  outer = 0;  nonnull = !nulls[row]
//
// Output: NA2 = A + 2 slots per outer group
//   slot a < A   the merged level-1 partials: sums added, counts added, min of mins, max of maxs
//   slot A       cnts: the distinct count (rows with nonnull); sums 0, min +inf, max -inf
//   slot A + 1   cnts: the rows merged (>= 1 for an outer group that exists): the occupancy
//                "star" count hs_hagg_extract wants for the two direct slots
//
// Two shapes:
//
//   hs_distinct_regroup_dense   few outer groups: the outer code is the slot index (no outer
//     columns = one slot).  One wavefront per block accumulates its contiguous rows into
//     accumulators in LDS, [slots][NA2] x (sum, count[, min, max]):
//         LDS bytes = slots * NA2 * 8 * (2 + 2 * minmax)  <=  64 KiB
//     (a CU has 160 KiB, two such blocks fit).  Rows of one outer group are combined across the
//     wavefront first: the lowest unfinished lane names its slot, the lanes of that slot reduce
//     their partials through a fixed xor butterfly (other lanes feed the identity) and the
//     leader alone updates LDS with plain loads and stores.  With one outer group that is one
//     reduction per 64 rows instead of 64 adders on one address, and nothing here is an atomic:
//     the block's accumulators depend on its rows only.  Each block stores them to a slab
//     [blocks][slots][NA2]; a second kernel adds the slab in a fixed order (per cell: thread t
//     takes blocks t, t + 256, ... in block order, then a fixed tree).  The grid is a function
//     of (n, slots, A), so the result is bitwise reproducible.  The output is one dense
//     row per slot (key = slot), also for slots no row fell in (rows merged 0; the host drops
//     them).
//
//   hs_distinct_regroup         many outer groups: each row probes a second hash table of
//     NA2 slots per group with the scheme of hs_hagg_probe.h and adds its partials with
//     memory-side atomics; a probe sequence longer than the budget sets flag[0] = 1 and skips
//     the row (the host re-runs with a 4x table); hs_hagg_extract (star = A + 1) compacts it.
//     Lanes are not combined first: level 1 emits its rows in table-slot order, hashed on
//     (g..., x), so equal outer keys are not adjacent and a wavefront seldom holds two.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hs_hagg_probe.h"

namespace {

using hs_hagg::probe_insert;
constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr long long kDenseLdsBytes = 64 * 1024;
constexpr long long kDenseMaxBlocks = 4096;

__device__ __forceinline__ void row_fields(unsigned long long key, unsigned char null_byte,
                                           unsigned long long outer_mask, int x_shift,
                                           int x_nullable, int raw, unsigned long long* outer,
                                           bool* nonnull) {
  if (raw) {
    *outer = 0ull;
    *nonnull = null_byte == 0;
  } else {
    const unsigned long long code = x_shift < 64 ? key >> x_shift : 0ull;
    *outer = key & outer_mask;
    *nonnull = !x_nullable || code != 0ull;
  }
}

template <bool MM>
__global__ __launch_bounds__(kWave) void regroup_dense_kernel(
    const unsigned long long* __restrict__ in_keys, const unsigned char* __restrict__ in_null,
    const double* __restrict__ in_sums, const long long* __restrict__ in_cnts,
    const double* __restrict__ in_mins, const double* __restrict__ in_maxs, long long n,
    long long in_cap, int A, unsigned long long outer_mask, int x_shift, int x_nullable, int raw,
    int slots, long long rows_per_block, double* __restrict__ slab_sums,
    long long* __restrict__ slab_cnts, double* __restrict__ slab_mins,
    double* __restrict__ slab_maxs) {
  extern __shared__ double lds[];
  const int NA2 = A + 2;
  const int cells = slots * NA2;
  double* a_sum = lds;
  long long* a_cnt = reinterpret_cast<long long*>(lds + cells);
  double* a_min = lds + 2 * cells;   // MM only
  double* a_max = lds + 3 * cells;
  const int lane = threadIdx.x;
  for (int c = lane; c < cells; c += kWave) {
    a_sum[c] = 0.0;
    a_cnt[c] = 0;
    if (MM) {
      a_min[c] = __builtin_inf();
      a_max[c] = -__builtin_inf();
    }
  }
  __syncthreads();
  const long long b0 = (long long)blockIdx.x * rows_per_block;
  const long long e = b0 + rows_per_block < n ? b0 + rows_per_block : n;
  for (long long base = b0; base < e; base += kWave) {
    const long long i = base + lane;
    const bool valid = i < e;
    int slot = 0;
    bool nonnull = false;
    if (valid) {
      unsigned long long outer;
      row_fields(in_keys[i], in_null[i], outer_mask, x_shift, x_nullable, raw, &outer, &nonnull);
      slot = (int)outer;   // < slots: slots = outer_mask + 1 (checked by the launcher)
    }
    // One aggregate slot at a time: its partials are loaded once per row (one load latency per
    // slot and tile), then the slots of the tile are walked in registers.
    const unsigned long long vmask = __ballot(valid);
    for (int a = 0; a < A; ++a) {
      const long long gi = (long long)a * in_cap + i;
      double v = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
      long long c = 0;
      if (valid) {
        v = in_sums[gi];
        c = in_cnts[gi];
        if (MM) {
          mn = in_mins[gi];
          mx = in_maxs[gi];
        }
      }
      unsigned long long todo = vmask;
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int s = __shfl(slot, leader, kWave);
        const bool mine = valid && slot == s;
        const unsigned long long m = __ballot(mine);
        const unsigned long long nn = a == 0 ? __ballot(mine && nonnull) : 0ull;
        double rv = mine ? v : 0.0;
        long long rc = mine ? c : 0;
        double rmn = mine ? mn : __builtin_inf(), rmx = mine ? mx : -__builtin_inf();
        if ((m & (m - 1ull)) != 0ull) {   // more than one row of this outer group in the tile
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            rv += __shfl_xor(rv, o, kWave);
            rc += __shfl_xor(rc, o, kWave);
            if (MM) {
              rmn = fmin(rmn, __shfl_xor(rmn, o, kWave));
              rmx = fmax(rmx, __shfl_xor(rmx, o, kWave));
            }
          }
        }
        if (lane == leader) {
          const int cell = s * NA2 + a;
          a_sum[cell] += rv;
          a_cnt[cell] += rc;
          if (MM) {
            a_min[cell] = fmin(a_min[cell], rmn);
            a_max[cell] = fmax(a_max[cell], rmx);
          }
          if (a == 0) {
            a_cnt[s * NA2 + A] += __popcll(nn);
            a_cnt[s * NA2 + A + 1] += __popcll(m);
          }
        }
        todo &= ~m;
      }
    }
  }
  __syncthreads();
  const long long sb = (long long)blockIdx.x * cells;
  for (int c = lane; c < cells; c += kWave) {
    slab_sums[sb + c] = a_sum[c];
    slab_cnts[sb + c] = a_cnt[c];
    if (MM) {
      slab_mins[sb + c] = a_min[c];
      slab_maxs[sb + c] = a_max[c];
    }
  }
}

// One block per (slot, aggregate) cell: thread t adds the partials of blocks t, t + 256, ... in
// block order, then a fixed tree over the 256 threads.  The order depends on nblocks alone.
__global__ __launch_bounds__(kBlock) void regroup_dense_sum_kernel(
    const double* __restrict__ slab_sums, const long long* __restrict__ slab_cnts,
    const double* __restrict__ slab_mins, const double* __restrict__ slab_maxs, int nblocks,
    int slots, int NA2, long long out_cap, unsigned long long* __restrict__ out_keys,
    unsigned char* __restrict__ out_null, double* __restrict__ out_sums,
    long long* __restrict__ out_cnts, double* __restrict__ out_mins,
    double* __restrict__ out_maxs) {
  __shared__ double p_sum[kBlock], p_min[kBlock], p_max[kBlock];
  __shared__ long long p_cnt[kBlock];
  const int cells = slots * NA2;
  const int j = blockIdx.x;   // < cells: the grid is one block per cell
  const int t = threadIdx.x;
  const int s = j / NA2, a = j % NA2;
  double sum = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  long long c = 0;
  for (int b = t; b < nblocks; b += kBlock) {
    const long long si = (long long)b * cells + j;
    sum += slab_sums[si];
    c += slab_cnts[si];
    if (slab_mins) {
      mn = fmin(mn, slab_mins[si]);
      mx = fmax(mx, slab_maxs[si]);
    }
  }
  p_sum[t] = sum;
  p_cnt[t] = c;
  p_min[t] = mn;
  p_max[t] = mx;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (t < o) {
      p_sum[t] += p_sum[t + o];
      p_cnt[t] += p_cnt[t + o];
      p_min[t] = fmin(p_min[t], p_min[t + o]);
      p_max[t] = fmax(p_max[t], p_max[t + o]);
    }
    __syncthreads();
  }
  if (t != 0) return;
  const long long oi = (long long)a * out_cap + s;
  out_sums[oi] = p_sum[0];
  out_cnts[oi] = p_cnt[0];
  if (out_mins) out_mins[oi] = p_min[0];
  if (out_maxs) out_maxs[oi] = p_max[0];
  if (a == 0) {
    out_keys[s] = (unsigned long long)s;
    out_null[s] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void regroup_hash_kernel(
    const unsigned long long* __restrict__ in_keys, const unsigned char* __restrict__ in_null,
    const double* __restrict__ in_sums, const long long* __restrict__ in_cnts,
    const double* __restrict__ in_mins, const double* __restrict__ in_maxs, long long n,
    long long in_cap, int A, unsigned long long outer_mask, int x_shift, int x_nullable, int raw,
    unsigned long long* keys, double* sums, long long* cnts, double* mins, double* maxs,
    long long M, int max_probe, long long* flag) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long st = M + 2;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) {
    unsigned long long outer;
    bool nonnull;
    row_fields(in_keys[g], in_null[g], outer_mask, x_shift, x_nullable, raw, &outer, &nonnull);
    const long long s = probe_insert(keys, M, outer, false, max_probe);
    if (s < 0) {
      flag[0] = 1;
      continue;
    }
    for (int a = 0; a < A; ++a) {
      const long long si = (long long)a * st + s, gi = (long long)a * in_cap + g;
      unsafeAtomicAdd(&sums[si], in_sums[gi]);
      if (in_cnts[gi]) atomicAdd((unsigned long long*)&cnts[si], (unsigned long long)in_cnts[gi]);
      if (mins) atomicMin(&mins[si], in_mins[gi]);
      if (maxs) atomicMax(&maxs[si], in_maxs[gi]);
    }
    if (nonnull) atomicAdd((unsigned long long*)&cnts[(long long)A * st + s], 1ull);
    atomicAdd((unsigned long long*)&cnts[(long long)(A + 1) * st + s], 1ull);
  }
}

inline long long dense_bytes(long long slots, int A, int minmax) {
  return slots * (long long)(A + 2) * 8 * (2 + (minmax ? 2 : 0));
}

}  // namespace

extern "C" {

// LDS bytes of the dense shape; it applies while they fit one block's 64 KiB.
long long hs_distinct_dense_bytes(long long slots, int A, int minmax) {
  return dense_bytes(slots, A, minmax);
}

int hs_distinct_dense_fits(long long slots, int A, int minmax) {
  return slots >= 1 && A >= 1 && slots <= (1 << 20) &&
         dense_bytes(slots, A, minmax) <= kDenseLdsBytes;
}

// Blocks (= slab rows) of the dense shape over n rows: each block takes at least 256 rows and
// at least 4 rows per accumulator cell, so the slab stays a fraction of the input.
long long hs_distinct_dense_blocks(long long n, long long slots, int A) {
  long long per = 4 * slots * (A + 2);
  if (per < 256) per = 256;
  long long b = (n + per - 1) / per;
  return b < 1 ? 1 : (b > kDenseMaxBlocks ? kDenseMaxBlocks : b);
}

// slab_*: hs_distinct_dense_blocks(n, slots, A) * slots * (A + 2) elements each (mins / maxs
// null without MIN / MAX).  out_*: dense groups of row stride out_cap >= slots, A + 2
// aggregates; all `slots` rows are written.
int hs_distinct_regroup_dense(const unsigned long long* in_keys, const unsigned char* in_null,
                              const double* in_sums, const long long* in_cnts,
                              const double* in_mins, const double* in_maxs, long long n,
                              long long in_cap, int A, unsigned long long outer_mask, int x_shift,
                              int x_nullable, int raw, long long slots, double* slab_sums,
                              long long* slab_cnts, double* slab_mins, double* slab_maxs,
                              long long out_cap, unsigned long long* out_keys,
                              unsigned char* out_null, double* out_sums, long long* out_cnts,
                              double* out_mins, double* out_maxs, void* stream) {
  const int minmax = in_mins != nullptr;
  if (n < 0 || n > in_cap || !hs_distinct_dense_fits(slots, A, minmax) || out_cap < slots ||
      x_shift < 0 || (in_mins == nullptr) != (in_maxs == nullptr) ||
      (minmax && (!slab_mins || !slab_maxs || !out_mins || !out_maxs)))
    return -1;
  if (raw ? slots != 1 : outer_mask != (unsigned long long)(slots - 1)) return -1;
  (void)hipGetLastError();
  hipStream_t s = (hipStream_t)stream;
  const long long nb = hs_distinct_dense_blocks(n, slots, A);
  long long per = (n + nb - 1) / nb;
  per = (per + kWave - 1) / kWave * kWave;
  const size_t lds = (size_t)dense_bytes(slots, A, minmax);
  if (minmax)
    hipLaunchKernelGGL(regroup_dense_kernel<true>, dim3((unsigned)nb), dim3(kWave), lds, s,
                       in_keys, in_null, in_sums, in_cnts, in_mins, in_maxs, n, in_cap, A,
                       outer_mask, x_shift, x_nullable, raw, (int)slots, per, slab_sums,
                       slab_cnts, slab_mins, slab_maxs);
  else
    hipLaunchKernelGGL(regroup_dense_kernel<false>, dim3((unsigned)nb), dim3(kWave), lds, s,
                       in_keys, in_null, in_sums, in_cnts, in_mins, in_maxs, n, in_cap, A,
                       outer_mask, x_shift, x_nullable, raw, (int)slots, per, slab_sums,
                       slab_cnts, slab_mins, slab_maxs);
  const int cells = (int)(slots * (A + 2));
  hipLaunchKernelGGL(regroup_dense_sum_kernel, dim3((unsigned)cells), dim3(kBlock), 0, s, (const double*)slab_sums, (const long long*)slab_cnts,
                     (const double*)(minmax ? slab_mins : nullptr),
                     (const double*)(minmax ? slab_maxs : nullptr), (int)nb, (int)slots, A + 2,
                     out_cap, out_keys, out_null, out_sums, out_cnts, out_mins, out_maxs);
  return (int)hipGetLastError();
}

// keys / sums / cnts / mins / maxs: a table of M slots and A + 2 aggregates (hs_hagg_init).
int hs_distinct_regroup(const unsigned long long* in_keys, const unsigned char* in_null,
                        const double* in_sums, const long long* in_cnts, const double* in_mins,
                        const double* in_maxs, long long n, long long in_cap, int A,
                        unsigned long long outer_mask, int x_shift, int x_nullable, int raw,
                        unsigned long long* keys, double* sums, long long* cnts, double* mins,
                        double* maxs, long long M, long long* flag, void* stream) {
  if (n <= 0) return n == 0 ? 0 : -1;
  if (M <= 0 || (M & (M - 1)) != 0 || A < 1 || n > in_cap || x_shift < 0 ||
      (in_mins == nullptr) != (mins == nullptr) || (in_maxs == nullptr) != (maxs == nullptr))
    return -1;
  (void)hipGetLastError();
  const long long blocks = (n + kBlock - 1) / kBlock;
  const int max_probe = (int)(M < 4096 ? M : 4096);
  hipLaunchKernelGGL(regroup_hash_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)),
                     dim3(kBlock), 0, (hipStream_t)stream, in_keys, in_null, in_sums, in_cnts,
                     in_mins, in_maxs, n, in_cap, A, outer_mask, x_shift, x_nullable, raw, keys,
                     sums, cnts, mins, maxs, M, max_probe, flag);
  return (int)hipGetLastError();
}

}  // extern "C"
