// Z-order covering indexes (index/zorder.py, exec/zorder.py): the build's Z-address kernel and
// the query side's zone maps and zone pruning.
//
// hs_zorder_keys: one thread per row.  Column j of up to 8 contributes bits[j] bits of
//   code_j = (hs_sortable(row) - mn[j]) >> shift[j]          (0 for a null row),
// interleaved from the most significant bit: level l = 0, 1, ... takes bit bits[j] - 1 - l of
// every column (declared order) with bits[j] > l.  Sum(bits) <= 63, so the key is a non-negative
// int64 the radix sort takes as it is.  The images are hs_sortable's throughout: nothing is
// canonicalised, mn[] must come from the same images (hs_zone_minmax).
//
// hs_zone_minmax: one block per (zone, column); zone z is rows [z * zone_rows, min(n, (z + 1) *
// zone_rows)).  Min / max of the hs_sortable image and the non-null count go through wave
// reductions and 3 x 4 LDS words per block.  An all-null zone keeps mn = ~0 > mx = 0.
//
// hs_zone_prune: zone z is kept iff every constrained column has cnt > 0 && mx >= lo && mn <= hi.
// Runs of adjacent kept zones become one (start, len) range each; live ranges come first in
// ascending order, the rest of the NZ entries are zero-length, the last zone is clipped to n.
// Three launches, one lane per zone, no block waits on another and no atomics, so the output is
// a function of the zone maps alone:
//   count  per 256-zone block: run starts, kept zones, the last run start in the block
//   scan   one wave over the block partials: exclusive sum of run starts, running maximum of
//          the last run start (the run still open when a block begins), the totals
//   write  the lane at a run's END owns the run: its index is the number of starts up to it,
//          its start the nearest start at or below it - found in its wave's ballot, else in the
//          block's earlier waves (LDS), else in the scanned carry.  Lane z >= total writes the
//          zero-length entry z.
#include "hs_common.h"

namespace {

constexpr int kZMaxCols = 8;
constexpr int kKeyThreads = 256;
constexpr int kZoneThreads = 256;
constexpr int kPruneThreads = 256;
constexpr int kPruneWaves = kPruneThreads / HS_WAVE;

struct ZKeyArgs {
  ColDesc cols[kZMaxCols];
  uint64_t mn[kZMaxCols];
  int32_t shift[kZMaxCols];
  int32_t bits[kZMaxCols];
  int32_t ncols;
  int32_t maxb;
};

struct ZZoneArgs {
  ColDesc cols[kZMaxCols];
  int32_t ncols;
  int32_t pad;
};

struct ZPruneArgs {
  uint64_t lo[kZMaxCols];
  uint64_t hi[kZMaxCols];
  int32_t col[kZMaxCols];     // zone-map column of constraint i
  int32_t ncons;
  int32_t pad;
};

__global__ __launch_bounds__(kKeyThreads) void zorder_keys(ZKeyArgs a, int64_t n,
                                                           int64_t* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * kKeyThreads + threadIdx.x;
  if (row >= n) return;
  uint64_t code[kZMaxCols];
#pragma unroll
  for (int j = 0; j < kZMaxCols; ++j) {
    code[j] = 0;
    if (j < a.ncols && a.bits[j] > 0 && col_valid(a.cols[j], row))
      code[j] = (hs_sortable(a.cols[j], row) - a.mn[j]) >> a.shift[j];
  }
  uint64_t key = 0;
  for (int l = 0; l < a.maxb; ++l) {
#pragma unroll
    for (int j = 0; j < kZMaxCols; ++j) {
      const int b = a.bits[j];
      if (b > l) key = (key << 1) | ((code[j] >> (b - 1 - l)) & 1ull);
    }
  }
  out[row] = (int64_t)key;
}

// -------------------------------------------------------------------------------------------
// zone maps
// -------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t zwave_min(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ uint64_t zwave_max(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

template <int TYPE>
__device__ __forceinline__ void zone_rows_minmax(const ColDesc& c, int64_t r0, int64_t r1,
                                                 uint64_t& mn, uint64_t& mx, long long& cnt) {
  ColDesc t = c;
  t.type = TYPE;      // a constant type folds hs_sortable's switch out of the row loop
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kZoneThreads) {
    if (!col_valid(t, r)) continue;
    const uint64_t im = hs_sortable(t, r);
    mn = im < mn ? im : mn;
    mx = im > mx ? im : mx;
    ++cnt;
  }
}

__global__ __launch_bounds__(kZoneThreads) void zone_minmax(ZZoneArgs a, int64_t n,
                                                            int64_t zone_rows, int64_t nz,
                                                            uint64_t* __restrict__ omn,
                                                            uint64_t* __restrict__ omx,
                                                            int64_t* __restrict__ ocnt) {
  constexpr int kWaves = kZoneThreads / HS_WAVE;
  __shared__ uint64_t s_mn[kWaves], s_mx[kWaves];
  __shared__ long long s_cnt[kWaves];
  const int64_t z = blockIdx.x;
  const int j = blockIdx.y;
  const ColDesc& c = a.cols[j];
  const int64_t r0 = z * zone_rows;
  int64_t r1 = r0 + zone_rows;
  if (r1 > n) r1 = n;
  uint64_t mn = ~0ull, mx = 0ull;
  long long cnt = 0;
  switch (c.type) {
    case HS_I8: zone_rows_minmax<HS_I8>(c, r0, r1, mn, mx, cnt); break;
    case HS_I16: zone_rows_minmax<HS_I16>(c, r0, r1, mn, mx, cnt); break;
    case HS_I32: zone_rows_minmax<HS_I32>(c, r0, r1, mn, mx, cnt); break;
    case HS_I64: zone_rows_minmax<HS_I64>(c, r0, r1, mn, mx, cnt); break;
    case HS_F32: zone_rows_minmax<HS_F32>(c, r0, r1, mn, mx, cnt); break;
    default: zone_rows_minmax<HS_F64>(c, r0, r1, mn, mx, cnt); break;
  }
  mn = zwave_min(mn);
  mx = zwave_max(mx);
  cnt = hs_wave_sum<long long>(cnt);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_mn[wave] = mn;
    s_mx[wave] = mx;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      mn = s_mn[w] < mn ? s_mn[w] : mn;
      mx = s_mx[w] > mx ? s_mx[w] : mx;
      cnt += s_cnt[w];
    }
    omn[(int64_t)j * nz + z] = mn;
    omx[(int64_t)j * nz + z] = mx;
    ocnt[(int64_t)j * nz + z] = cnt;
  }
}

// -------------------------------------------------------------------------------------------
// zone pruning
// -------------------------------------------------------------------------------------------
struct ZoneMaps {
  const uint64_t* __restrict__ mn;
  const uint64_t* __restrict__ mx;
  const int64_t* __restrict__ cnt;
  int64_t nz;
};

__device__ __forceinline__ bool zone_kept(const ZoneMaps& m, const ZPruneArgs& a, int64_t z) {
  if (z < 0 || z >= m.nz) return false;
  bool keep = true;
#pragma unroll
  for (int i = 0; i < kZMaxCols; ++i) {
    if (i < a.ncons) {
      const int64_t at = (int64_t)a.col[i] * m.nz + z;
      keep = keep && m.cnt[at] > 0 && m.mx[at] >= a.lo[i] && m.mn[at] <= a.hi[i];
    }
  }
  return keep;
}

// keep / run-start / run-end of this lane's zone and the wave's ballots of keep and start
struct LaneZone {
  bool keep, start, end;
  unsigned long long keeps, starts;
};

__device__ __forceinline__ LaneZone lane_zone(const ZoneMaps& m, const ZPruneArgs& a, int64_t z) {
  LaneZone s;
  const int lane = threadIdx.x & 63;
  s.keep = zone_kept(m, a, z);
  s.keeps = __ballot(s.keep);
  // the neighbours of lanes 0 and 63 live in other waves: evaluate those two zones here
  const bool prev = lane > 0 ? ((s.keeps >> (lane - 1)) & 1ull) != 0 : zone_kept(m, a, z - 1);
  const bool next = lane < 63 ? ((s.keeps >> (lane + 1)) & 1ull) != 0 : zone_kept(m, a, z + 1);
  s.start = s.keep && !prev;
  s.end = s.keep && !next;
  s.starts = __ballot(s.start);
  return s;
}

// per block: {run starts, kept zones, last start zone or -1}
__global__ __launch_bounds__(kPruneThreads) void zone_prune_count(ZoneMaps m, ZPruneArgs a,
                                                                  int64_t* __restrict__ part) {
  __shared__ int64_t s_part[kPruneWaves][3];
  const int64_t z = (int64_t)blockIdx.x * kPruneThreads + threadIdx.x;
  const LaneZone s = lane_zone(m, a, z);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_part[wave][0] = __popcll(s.starts);
    s_part[wave][1] = __popcll(s.keeps);
    s_part[wave][2] = s.starts ? z + 63 - __clzll((long long)s.starts) : -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t ns = 0, nk = 0, last = -1;
#pragma unroll
    for (int w = 0; w < kPruneWaves; ++w) {
      ns += s_part[w][0];
      nk += s_part[w][1];
      last = s_part[w][2] > last ? s_part[w][2] : last;
    }
    part[3 * (int64_t)blockIdx.x] = ns;
    part[3 * (int64_t)blockIdx.x + 1] = nk;
    part[3 * (int64_t)blockIdx.x + 2] = last;
  }
}

// one wave: boff[b] = run starts in blocks < b, bcarry[b] = last start zone in blocks < b (-1),
// counts = {ranges, kept zones}
__global__ __launch_bounds__(HS_WAVE) void zone_prune_scan(const int64_t* __restrict__ part,
                                                           int64_t nb, int64_t* __restrict__ boff,
                                                           int64_t* __restrict__ bcarry,
                                                           int64_t* __restrict__ counts) {
  const int lane = threadIdx.x;
  int64_t sum = 0, kept = 0, carry = -1;
  for (int64_t base = 0; base < nb; base += HS_WAVE) {
    const int64_t b = base + lane;
    const bool in = b < nb;
    int64_t ns = in ? part[3 * b] : 0;
    int64_t nk = in ? part[3 * b + 1] : 0;
    int64_t ls = in ? part[3 * b + 2] : -1;
    const int64_t own_ns = ns;
    // inclusive wave scans: sum of starts, maximum of last starts
#pragma unroll
    for (int off = 1; off < HS_WAVE; off <<= 1) {
      const int64_t os = __shfl_up((long long)ns, off, 64);
      const int64_t ol = __shfl_up((long long)ls, off, 64);
      if (lane >= off) {
        ns += os;
        ls = ol > ls ? ol : ls;
      }
    }
    // exclusive values for this block
    const int64_t ex_ns = ns - own_ns;
    int64_t ex_ls = __shfl_up((long long)ls, 1, 64);
    if (lane == 0) ex_ls = -1;
    if (in) {
      boff[b] = sum + ex_ns;
      bcarry[b] = ex_ls > carry ? ex_ls : carry;
    }
    nk = hs_wave_sum<long long>(nk);
    const int64_t tot_ns = __shfl((long long)ns, 63, 64);
    const int64_t tot_ls = __shfl((long long)ls, 63, 64);
    sum += tot_ns;
    kept += nk;
    carry = tot_ls > carry ? tot_ls : carry;
  }
  if (lane == 0) {
    counts[0] = sum;
    counts[1] = kept;
  }
}

__global__ __launch_bounds__(kPruneThreads) void zone_prune_write(
    ZoneMaps m, ZPruneArgs a, int64_t n, int64_t zone_rows, const int64_t* __restrict__ boff,
    const int64_t* __restrict__ bcarry, const int64_t* __restrict__ counts,
    int64_t* __restrict__ rstart, int64_t* __restrict__ rlen) {
  __shared__ int64_t s_ns[kPruneWaves], s_last[kPruneWaves];
  const int64_t z = (int64_t)blockIdx.x * kPruneThreads + threadIdx.x;
  const LaneZone s = lane_zone(m, a, z);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t wave_z0 = z - lane;
  if (lane == 0) {
    s_ns[wave] = __popcll(s.starts);
    s_last[wave] = s.starts ? wave_z0 + 63 - __clzll((long long)s.starts) : -1;
  }
  __syncthreads();
  const int64_t total = counts[0];
  if (z < m.nz && z >= total) {      // total <= nz: entries below it belong to the run ends
    rstart[z] = 0;
    rlen[z] = 0;
  }
  if (!s.end) return;
  const unsigned long long upto = s.starts & ((2ull << lane) - 1ull);   // starts at lanes <= lane
  int64_t idx = boff[blockIdx.x] + __popcll(upto) - 1;
  int64_t first = upto ? wave_z0 + 63 - __clzll((long long)upto) : -1;
  for (int w = 0; w < kPruneWaves; ++w) {
    if (w < wave) {
      idx += s_ns[w];
      if (upto == 0 && s_last[w] >= 0) first = s_last[w];   // ascending w: the nearest one wins
    }
  }
  if (first < 0) first = bcarry[blockIdx.x];
  // a run end always has a start at or below it, so 0 <= idx < total and first >= 0
  const int64_t r0 = first * zone_rows;
  int64_t r1 = (z + 1) * zone_rows;
  if (r1 > n) r1 = n;
  rstart[idx] = r0;
  rlen[idx] = r1 - r0;
}

}  // namespace

extern "C" {

int hs_zorder_max_cols() { return kZMaxCols; }

// cols: ncols (1..8) integer / float storage columns of n rows; mn / shift / bits per column
// (Sum(bits) <= 63, shift = need - bits); out: n int64 keys.
int hs_zorder_keys(const ColDesc* cols, int ncols, const uint64_t* mn, const int32_t* shift,
                   const int32_t* bits, int64_t n, int64_t* out, void* stream) {
  if (ncols < 1 || ncols > kZMaxCols || n < 0 || n > 0x7fffffffll * kKeyThreads) return -1;
  ZKeyArgs a{};
  int total = 0;
  for (int j = 0; j < ncols; ++j) {
    if (cols[j].type > HS_F64 || bits[j] < 0 || bits[j] > 63 || shift[j] < 0 ||
        shift[j] + bits[j] > 64)
      return -1;
    a.cols[j] = cols[j];
    a.mn[j] = mn[j];
    a.shift[j] = shift[j];
    a.bits[j] = bits[j];
    a.maxb = bits[j] > a.maxb ? bits[j] : a.maxb;
    total += bits[j];
  }
  if (total > 63) return -1;
  a.ncols = ncols;
  if (n == 0) return 0;
  hipLaunchKernelGGL(zorder_keys, dim3((unsigned)((n + kKeyThreads - 1) / kKeyThreads)),
                     dim3(kKeyThreads), 0, (hipStream_t)stream, a, n, out);
  return (int)hipGetLastError();
}

// omn / omx / ocnt: ncols x nz entries, nz = ceil(n / zone_rows), column-major ([col][zone]).
int hs_zone_minmax(const ColDesc* cols, int ncols, int64_t n, int64_t zone_rows, uint64_t* omn,
                   uint64_t* omx, int64_t* ocnt, void* stream) {
  if (ncols < 1 || ncols > kZMaxCols || n < 0 || zone_rows < 1) return -1;
  const int64_t nz = (n + zone_rows - 1) / zone_rows;
  if (nz > 0x7fffffffll) return -1;
  ZZoneArgs a{};
  for (int j = 0; j < ncols; ++j) {
    if (cols[j].type > HS_F64) return -1;
    a.cols[j] = cols[j];
  }
  a.ncols = ncols;
  if (nz == 0) return 0;
  hipLaunchKernelGGL(zone_minmax, dim3((unsigned)nz, (unsigned)ncols), dim3(kZoneThreads), 0,
                     (hipStream_t)stream, a, n, zone_rows, nz, omn, omx, ocnt);
  return (int)hipGetLastError();
}

// Workspace of hs_zone_prune in int64 words.
int64_t hs_zone_prune_workspace(int64_t nz) {
  const int64_t nb = (nz + kPruneThreads - 1) / kPruneThreads;
  return 5 * (nb > 0 ? nb : 1);
}

// mn / mx / cnt: nmaps x nz zone maps ([col][zone]) of a table of n rows in zones of zone_rows;
// constraint i keeps zones of map column col[i] that may hold an image in [lo[i], hi[i]].
// rstart / rlen: nz entries, all written; counts: {ranges, kept zones}.
int hs_zone_prune(const uint64_t* mn, const uint64_t* mx, const int64_t* cnt, int nmaps,
                  int64_t nz, int64_t n, int64_t zone_rows, const int32_t* col,
                  const uint64_t* lo, const uint64_t* hi, int ncons, int64_t* ws,
                  int64_t* rstart, int64_t* rlen, int64_t* counts, void* stream) {
  if (nmaps < 1 || nmaps > kZMaxCols || ncons < 0 || ncons > kZMaxCols || nz < 0 ||
      zone_rows < 1 || n < 0 || nz != (n + zone_rows - 1) / zone_rows)
    return -1;
  const int64_t nb = (nz + kPruneThreads - 1) / kPruneThreads;
  if (nb > 0x7fffffffll) return -1;
  ZPruneArgs a{};
  for (int i = 0; i < ncons; ++i) {
    if (col[i] < 0 || col[i] >= nmaps) return -1;
    a.col[i] = col[i];
    a.lo[i] = lo[i];
    a.hi[i] = hi[i];
  }
  a.ncons = ncons;
  hipStream_t st = (hipStream_t)stream;
  if (nz == 0) {
    HS_CHECK(hipMemsetAsync(counts, 0, 16, st));
    return 0;
  }
  const ZoneMaps m{mn, mx, cnt, nz};
  int64_t* part = ws;
  int64_t* boff = ws + 3 * nb;
  int64_t* bcarry = ws + 4 * nb;
  hipLaunchKernelGGL(zone_prune_count, dim3((unsigned)nb), dim3(kPruneThreads), 0, st, m, a,
                     part);
  hipLaunchKernelGGL(zone_prune_scan, dim3(1), dim3(HS_WAVE), 0, st, part, nb, boff, bcarry,
                     counts);
  hipLaunchKernelGGL(zone_prune_write, dim3((unsigned)nb), dim3(kPruneThreads), 0, st, m, a, n,
                     zone_rows, boff, bcarry, counts, rstart, rlen);
  return (int)hipGetLastError();
}

}  // extern "C"
