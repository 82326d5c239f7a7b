// Window functions (exec/window.py): segmented scans over rows already in (partition, order)
// order.  gfx950, wave64.
//
//   hs_win_heads        one lane per row: compares row i with row i - 1 on the partition and the
//                       order keys and writes one flag byte - bit 0 "starts a partition", bit 1
//                       "starts a peer group" (bit 0 implies bit 1; row 0 has both).  NULL equals
//                       NULL; floats compare by value (0.0 == -0.0) with every NaN equal to every
//                       NaN.
//   hs_win_rank         row_number / rank / dense_rank from the flags: ONE unsegmented scan of the
//                       triple (index of the last partition head, index of the last peer head,
//                       number of peer heads) with (max, max, +), then an elementwise pass:
//                       row_number = i - phead + 1, rank = qhead - phead + 1,
//                       dense_rank = cnt[i] - cnt[phead] + 1.
//   hs_win_frame_ends   the last row of every row's frame: a min-scan from the right over "index
//                       of the next head" (peer heads for the running frame, partition heads for
//                       the whole-partition frame), minus one.
//   hs_win_agg          a segmented inclusive scan of (value, valid-row count) restarting at bit
//                       0, then a gather: row i takes the scan at frame_end[i]; it is valid when
//                       that count is above 0.  A NULL input contributes the identity.
//
// Every scan is the same three launches over fixed tiles of 256 x ITEMS rows (hs_win_tile_rows):
//   1. win_tile_totals   each block reduces its tile to one element, tot[tile];
//   2. win_scan_totals   ONE block scans tot[] in place (inclusive), chunk by chunk;
//   3. win_downsweep     each block scans its tile again, combines tot[tile - 1] in front and
//                        stores.
// No block waits on another block: the only ordering is the stream order of the launches.  The
// decomposition depends on n alone, so results - fp64 sums included - are bitwise reproducible.
//
// Mapping: block 256 = 4 wavefronts; thread t of tile b owns the ITEMS consecutive positions
// b * TILE + t * ITEMS ... (a serial scan in registers), wavefront totals are scanned with
// __shfl_up, the 4 wavefront totals cross through LDS.  Segmentation lives in the element: the
// operator of a segmented scan is  a (+) b = b.head ? b : (a.v op b.v, a.head)  - associative, so
// the same engine runs it, and the carry from the previous tile reaches exactly the rows before
// the tile's first head.  Positions >= n load the identity; every load and store is guarded by
// pos < n.  Stores are plain vector stores.
#include "hs_common.h"

namespace {

constexpr int NT = 256;
constexpr int ITEMS = 8;
constexpr int TILE = NT * ITEMS;
constexpr int64_t I64_MAX = 0x7fffffffffffffffll;

__device__ __forceinline__ int64_t shfl_up_i64(int64_t v, int d) {
  return (int64_t)__shfl_up((long long)v, (unsigned)d, 64);
}

__device__ __forceinline__ int64_t shfl_up_val(int64_t v, int d) { return shfl_up_i64(v, d); }

__device__ __forceinline__ double shfl_up_val(double v, int d) {
  return __shfl_up(v, (unsigned)d, 64);
}

// In-place inclusive scan of the block's NT * ITEMS elements (thread-blocked layout); returns
// the block total to every thread.
template <class S>
__device__ __forceinline__ typename S::E block_scan(typename S::E (&x)[ITEMS]) {
  using E = typename S::E;
  __shared__ E s_wave[NT / 64];
#pragma unroll
  for (int k = 1; k < ITEMS; ++k) x[k] = S::combine(x[k - 1], x[k]);
  E t = x[ITEMS - 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const E o = S::shfl_up(t, d);
    if (lane >= d) t = S::combine(o, t);
  }
  if (lane == 63) s_wave[w] = t;
  E excl = S::shfl_up(t, 1);
  if (lane == 0) excl = S::identity();
  __syncthreads();
  E pre = S::identity();
  for (int j = 0; j < w; ++j) pre = S::combine(pre, s_wave[j]);   // w is wavefront-uniform
  pre = S::combine(pre, excl);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) x[k] = S::combine(pre, x[k]);
  E total = s_wave[0];
#pragma unroll
  for (int j = 1; j < NT / 64; ++j) total = S::combine(total, s_wave[j]);
  __syncthreads();   // s_wave is free again for a caller that loops
  return total;
}

template <class S>
__global__ __launch_bounds__(NT) void win_tile_totals(typename S::Args a, int64_t n,
                                                      typename S::E* __restrict__ tot) {
  typename S::E x[ITEMS];
  const int64_t base = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * ITEMS;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) x[k] = base + k < n ? S::load(a, base + k, n) : S::identity();
  const typename S::E total = block_scan<S>(x);
  if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

template <class S>
__global__ __launch_bounds__(NT) void win_scan_totals(typename S::E* __restrict__ tot,
                                                      int64_t ntiles) {
  typename S::E carry = S::identity();
  for (int64_t c0 = 0; c0 < ntiles; c0 += TILE) {   // block-uniform bound
    typename S::E x[ITEMS];
    const int64_t base = c0 + (int64_t)threadIdx.x * ITEMS;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) x[k] = base + k < ntiles ? tot[base + k] : S::identity();
    const typename S::E total = block_scan<S>(x);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k)
      if (base + k < ntiles) tot[base + k] = S::combine(carry, x[k]);
    carry = S::combine(carry, total);
  }
}

template <class S>
__global__ __launch_bounds__(NT) void win_downsweep(typename S::Args a, int64_t n,
                                                    const typename S::E* __restrict__ tot) {
  typename S::E x[ITEMS];
  const int64_t base = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * ITEMS;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) x[k] = base + k < n ? S::load(a, base + k, n) : S::identity();
  block_scan<S>(x);
  const typename S::E carry = blockIdx.x > 0 ? tot[blockIdx.x - 1] : S::identity();
#pragma unroll
  for (int k = 0; k < ITEMS; ++k)
    if (base + k < n) S::store(a, base + k, n, S::combine(carry, x[k]));
}

template <class S>
int run_scan(const typename S::Args& a, int64_t n, typename S::E* tot, hipStream_t s) {
  const int64_t ntiles = (n + TILE - 1) / TILE;
  if (ntiles <= 0) return 0;
  if (ntiles > 0x7fffffffll) return -2;
  hipLaunchKernelGGL(win_tile_totals<S>, dim3((unsigned)ntiles), dim3(NT), 0, s, a, n, tot);
  hipLaunchKernelGGL(win_scan_totals<S>, dim3(1), dim3(NT), 0, s, tot, ntiles);
  hipLaunchKernelGGL(win_downsweep<S>, dim3((unsigned)ntiles), dim3(NT), 0, s, a, n,
                     (const typename S::E*)tot);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// heads
// ------------------------------------------------------------------------------------------------
constexpr int WIN_MAX_KEYS = 8;

struct WinKeys {
  ColDesc part[WIN_MAX_KEYS];
  ColDesc order[WIN_MAX_KEYS];
  int32_t npart;
  int32_t norder;
};

__device__ __forceinline__ bool key_differs(const ColDesc& c, int64_t i) {
  const bool va = col_valid(c, i - 1), vb = col_valid(c, i);
  if (!va || !vb) return va != vb;
  if (c.type == HS_F32 || c.type == HS_F64) {
    const double a = load_f64(c, i - 1), b = load_f64(c, i);
    return !(a == b || (a != a && b != b));
  }
  return load_i64(c, i - 1) != load_i64(c, i);
}

__global__ __launch_bounds__(NT) void win_heads_kernel(WinKeys k, int64_t n,
                                                       uint8_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  bool p = i == 0, q = false;
  if (i > 0) {
    for (int c = 0; c < k.npart && !p; ++c) p = key_differs(k.part[c], i);
    for (int c = 0; c < k.norder && !p && !q; ++c) q = key_differs(k.order[c], i);
  }
  flags[i] = p ? 3 : (q ? 2 : 0);
}

// ------------------------------------------------------------------------------------------------
// ranks
// ------------------------------------------------------------------------------------------------
struct RankScan {
  struct E {
    int64_t ph, qh, cnt;
  };
  struct Args {
    const uint8_t* flags;
    int64_t* ph;
    int64_t* qh;
    int64_t* cnt;
  };
  static __device__ __forceinline__ E identity() { return E{-1, -1, 0}; }
  static __device__ __forceinline__ E combine(const E& a, const E& b) {
    return E{a.ph > b.ph ? a.ph : b.ph, a.qh > b.qh ? a.qh : b.qh, a.cnt + b.cnt};
  }
  static __device__ __forceinline__ E shfl_up(const E& v, int d) {
    return E{shfl_up_i64(v.ph, d), shfl_up_i64(v.qh, d), shfl_up_i64(v.cnt, d)};
  }
  static __device__ __forceinline__ E load(const Args& a, int64_t pos, int64_t) {
    const uint8_t f = a.flags[pos];
    return E{(f & 1) ? pos : -1, (f & 2) ? pos : -1, (int64_t)((f >> 1) & 1)};
  }
  static __device__ __forceinline__ void store(const Args& a, int64_t pos, int64_t, const E& v) {
    a.ph[pos] = v.ph;
    a.qh[pos] = v.qh;
    a.cnt[pos] = v.cnt;
  }
};

__global__ __launch_bounds__(NT) void win_rank_emit(const int64_t* __restrict__ ph,
                                                    const int64_t* __restrict__ qh,
                                                    const int64_t* __restrict__ cnt, int64_t n,
                                                    int32_t* __restrict__ row_number,
                                                    int32_t* __restrict__ rank,
                                                    int32_t* __restrict__ dense_rank) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  int64_t p = ph[i];
  if (p < 0 || p > i) p = 0;     // flags not made by hs_win_heads (row 0 unflagged): stay in range
  if (row_number) row_number[i] = (int32_t)(i - p + 1);
  if (rank) rank[i] = (int32_t)(qh[i] - p + 1);
  if (dense_rank) dense_rank[i] = (int32_t)(cnt[i] - cnt[p] + 1);
}

// ------------------------------------------------------------------------------------------------
// frame ends: positions run from the right (position p is row n - 1 - p)
// ------------------------------------------------------------------------------------------------
struct EndScan {
  struct E {
    int64_t nxt;
  };
  struct Args {
    const uint8_t* flags;
    int64_t* ends;
    int32_t bit;
    int32_t pad;
  };
  static __device__ __forceinline__ E identity() { return E{I64_MAX}; }
  static __device__ __forceinline__ E combine(const E& a, const E& b) {
    return E{a.nxt < b.nxt ? a.nxt : b.nxt};
  }
  static __device__ __forceinline__ E shfl_up(const E& v, int d) {
    return E{shfl_up_i64(v.nxt, d)};
  }
  static __device__ __forceinline__ E load(const Args& a, int64_t pos, int64_t n) {
    const int64_t r = n - 1 - pos;
    if (r + 1 >= n) return E{n};
    return E{(a.flags[r + 1] & a.bit) ? r + 1 : I64_MAX};
  }
  static __device__ __forceinline__ void store(const Args& a, int64_t pos, int64_t n,
                                               const E& v) {
    a.ends[n - 1 - pos] = v.nxt - 1;   // the scan includes the row n at position 0: nxt <= n
  }
};

// ------------------------------------------------------------------------------------------------
// aggregates
// ------------------------------------------------------------------------------------------------
enum WinAgg : int32_t {
  WA_SUM_I64 = 0, WA_SUM_F64 = 1, WA_COUNT = 2, WA_MIN_I64 = 3, WA_MAX_I64 = 4, WA_MIN_F64 = 5,
  WA_MAX_F64 = 6
};

template <int KIND>
struct AggOp;
template <>
struct AggOp<WA_SUM_I64> {
  using T = int64_t;
  static __device__ __forceinline__ T id() { return 0; }
  static __device__ __forceinline__ T op(T a, T b) { return (T)((uint64_t)a + (uint64_t)b); }
  static __device__ __forceinline__ T get(const ColDesc& c, int64_t r) { return load_i64(c, r); }
};
template <>
struct AggOp<WA_COUNT> : AggOp<WA_SUM_I64> {
  static __device__ __forceinline__ int64_t get(const ColDesc&, int64_t) { return 0; }
};
template <>
struct AggOp<WA_MIN_I64> {
  using T = int64_t;
  static __device__ __forceinline__ T id() { return I64_MAX; }
  static __device__ __forceinline__ T op(T a, T b) { return a < b ? a : b; }
  static __device__ __forceinline__ T get(const ColDesc& c, int64_t r) { return load_i64(c, r); }
};
template <>
struct AggOp<WA_MAX_I64> {
  using T = int64_t;
  static __device__ __forceinline__ T id() { return -I64_MAX - 1; }
  static __device__ __forceinline__ T op(T a, T b) { return a > b ? a : b; }
  static __device__ __forceinline__ T get(const ColDesc& c, int64_t r) { return load_i64(c, r); }
};
template <>
struct AggOp<WA_SUM_F64> {
  using T = double;
  static __device__ __forceinline__ T id() { return 0.0; }
  static __device__ __forceinline__ T op(T a, T b) { return a + b; }
  static __device__ __forceinline__ T get(const ColDesc& c, int64_t r) { return load_f64(c, r); }
};
// float min / max skip NaN like a NULL, but a frame whose non-NULL inputs are all NaN is NaN: the
// count carries the non-NaN rows in its high half (kNonNan per row) beside the valid rows
constexpr int64_t kNonNan = (int64_t)1 << 32;

template <>
struct AggOp<WA_MIN_F64> {
  using T = double;
  static __device__ __forceinline__ T id() { return __builtin_inf(); }
  static __device__ __forceinline__ T op(T a, T b) { return fmin(a, b); }   // NaN: skipped
  static __device__ __forceinline__ T get(const ColDesc& c, int64_t r) { return load_f64(c, r); }
};
template <>
struct AggOp<WA_MAX_F64> {
  using T = double;
  static __device__ __forceinline__ T id() { return -__builtin_inf(); }
  static __device__ __forceinline__ T op(T a, T b) { return fmax(a, b); }
  static __device__ __forceinline__ T get(const ColDesc& c, int64_t r) { return load_f64(c, r); }
};

struct AggArgs {
  ColDesc col;             // data == nullptr: count(*) - every row counts
  const uint8_t* flags;
  void* v;                 // n scan values (T)
  int64_t* c;              // n valid-row counts
};

template <int KIND>
struct AggScan {
  using O = AggOp<KIND>;
  using T = typename O::T;
  struct E {
    T v;
    int64_t c;
    int32_t head;
    int32_t pad;
  };
  using Args = AggArgs;
  static __device__ __forceinline__ E identity() { return E{O::id(), 0, 0, 0}; }
  static __device__ __forceinline__ E combine(const E& a, const E& b) {
    if (b.head) return b;
    return E{O::op(a.v, b.v), a.c + b.c, a.head, 0};
  }
  static __device__ __forceinline__ E shfl_up(const E& x, int d) {
    E o;
    o.v = shfl_up_val(x.v, d);
    o.c = shfl_up_i64(x.c, d);
    o.head = __shfl_up(x.head, (unsigned)d, 64);
    o.pad = 0;
    return o;
  }
  static __device__ __forceinline__ E load(const Args& a, int64_t pos, int64_t) {
    const int32_t head = a.flags[pos] & 1;
    if (a.col.data == nullptr) return E{O::id(), 1, head, 0};
    if (!col_valid(a.col, pos)) return E{O::id(), 0, head, 0};
    const T x = O::get(a.col, pos);
    if (KIND == WA_MIN_F64 || KIND == WA_MAX_F64) return E{x, x == x ? 1 + kNonNan : 1, head, 0};
    return E{x, 1, head, 0};
  }
  static __device__ __forceinline__ void store(const Args& a, int64_t pos, int64_t, const E& x) {
    ((T*)a.v)[pos] = x.v;
    a.c[pos] = x.c;
  }
};

// out[i] = scan[ends[i]] as 8 raw bytes (int64 or double); count kinds take the count itself.
// mode 0: a value; 1: the count; 2: a float min / max (the count's high half holds the non-NaN
// rows: none of them among valid rows gives NaN)
__global__ __launch_bounds__(NT) void win_agg_take(const int64_t* __restrict__ v,
                                                   const int64_t* __restrict__ c,
                                                   const int64_t* __restrict__ ends, int64_t n,
                                                   int mode, int64_t* __restrict__ out,
                                                   uint8_t* __restrict__ out_valid,
                                                   int64_t* __restrict__ out_count) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  int64_t e = ends[i];
  if (e < i || e >= n) e = i;      // ends not made by hs_win_frame_ends: stay in range
  const int64_t packed = c[e];
  const int64_t cnt = mode == 2 ? (packed & (kNonNan - 1)) : packed;
  int64_t r = cnt > 0 ? v[e] : 0;
  if (mode == 1) r = cnt;
  if (mode == 2 && cnt > 0 && (packed >> 32) == 0) r = 0x7ff8000000000000ll;   // quiet NaN
  out[i] = r;
  if (out_valid) out_valid[i] = mode == 1 || cnt > 0;
  if (out_count) out_count[i] = cnt;
}

constexpr int64_t kTotBytes = 32;   // >= sizeof of every scan element

int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

unsigned row_grid(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

template <int KIND>
int run_agg(const AggArgs& a, int64_t n, void* tot, hipStream_t s) {
  static_assert(sizeof(typename AggScan<KIND>::E) <= kTotBytes, "workspace element size");
  return run_scan<AggScan<KIND>>(a, n, (typename AggScan<KIND>::E*)tot, s);
}

}  // namespace

extern "C" {

int hs_win_tile_rows() { return TILE; }

int hs_win_keys_size() { return (int)sizeof(WinKeys); }

// Bytes of scratch hs_win_rank / hs_win_agg need for n rows: three n-element int64 arrays and
// the per-tile totals.
int64_t hs_win_workspace_bytes(int64_t n) {
  if (n < 0) n = 0;
  const int64_t ntiles = (n + TILE - 1) / TILE;
  return 3 * align256(n * 8) + align256((ntiles + 1) * kTotBytes) + 256;
}

// flags: n bytes, every one written.
int hs_win_heads(const WinKeys* keys, int64_t n, uint8_t* flags, void* stream) {
  if (keys->npart < 0 || keys->npart > WIN_MAX_KEYS || keys->norder < 0 ||
      keys->norder > WIN_MAX_KEYS)
    return -1;
  if (n <= 0) return 0;
  if ((n + NT - 1) / NT > 0x7fffffffll) return -2;
  hipLaunchKernelGGL(win_heads_kernel, dim3(row_grid(n)), dim3(NT), 0, (hipStream_t)stream,
                     *keys, n, flags);
  return (int)hipGetLastError();
}

// row_number / rank / dense_rank: n int32 each, any of them may be null.
int hs_win_rank(const uint8_t* flags, int64_t n, int32_t* row_number, int32_t* rank,
                int32_t* dense_rank, void* ws, void* stream) {
  if (n <= 0) return 0;
  if ((n + NT - 1) / NT > 0x7fffffffll) return -2;
  char* w = (char*)ws;
  const int64_t an = align256(n * 8);
  RankScan::Args a{flags, (int64_t*)w, (int64_t*)(w + an), (int64_t*)(w + 2 * an)};
  const int rc = run_scan<RankScan>(a, n, (RankScan::E*)(w + 3 * an), (hipStream_t)stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(win_rank_emit, dim3(row_grid(n)), dim3(NT), 0, (hipStream_t)stream,
                     (const int64_t*)a.ph, (const int64_t*)a.qh, (const int64_t*)a.cnt, n,
                     row_number, rank, dense_rank);
  return (int)hipGetLastError();
}

// ends: n int64, ends[i] = last row of row i's frame (whole != 0: its partition's last row,
// else its peer group's).  ws: hs_win_workspace_bytes(n).
int hs_win_frame_ends(const uint8_t* flags, int64_t n, int whole, int64_t* ends, void* ws,
                      void* stream) {
  if (n <= 0) return 0;
  EndScan::Args a{flags, ends, whole ? 1 : 2, 0};
  return run_scan<EndScan>(a, n, (EndScan::E*)ws, (hipStream_t)stream);
}

// col: the value column (null data pointer: count(*)); out: n 8-byte values (int64 for the
// integer kinds and count, double otherwise); out_valid: n bytes or null; out_count: the
// frame's non-NULL input count per row (n int64) or null - what avg divides by.
int hs_win_agg(const ColDesc* col, const uint8_t* flags, const int64_t* ends, int64_t n,
               int kind, void* out, uint8_t* out_valid, int64_t* out_count, void* ws,
               void* stream) {
  if (n <= 0) return 0;
  if ((n + NT - 1) / NT > 0x7fffffffll) return -2;
  const bool fminmax = kind == WA_MIN_F64 || kind == WA_MAX_F64;
  if (fminmax && n >= kNonNan / 2) return -2;   // two counts share one 64-bit word
  char* w = (char*)ws;
  const int64_t an = align256(n * 8);
  AggArgs a{*col, flags, (void*)w, (int64_t*)(w + an)};
  void* tot = (void*)(w + 3 * an);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  switch (kind) {
    case WA_SUM_I64: rc = run_agg<WA_SUM_I64>(a, n, tot, s); break;
    case WA_SUM_F64: rc = run_agg<WA_SUM_F64>(a, n, tot, s); break;
    case WA_COUNT: rc = run_agg<WA_COUNT>(a, n, tot, s); break;
    case WA_MIN_I64: rc = run_agg<WA_MIN_I64>(a, n, tot, s); break;
    case WA_MAX_I64: rc = run_agg<WA_MAX_I64>(a, n, tot, s); break;
    case WA_MIN_F64: rc = run_agg<WA_MIN_F64>(a, n, tot, s); break;
    case WA_MAX_F64: rc = run_agg<WA_MAX_F64>(a, n, tot, s); break;
    default: return -1;
  }
  if (rc != 0) return rc;
  hipLaunchKernelGGL(win_agg_take, dim3(row_grid(n)), dim3(NT), 0, s, (const int64_t*)a.v,
                     (const int64_t*)a.c, ends, n, kind == WA_COUNT ? 1 : (fminmax ? 2 : 0),
                     (int64_t*)out, out_valid, out_count);
  return (int)hipGetLastError();
}

}  // extern "C"
