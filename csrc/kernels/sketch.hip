// Data-skipping sketches (index/dataskipping.py, exec/device_sketch.py): per-source-file MinMax
// and Bloom-filter sketches of a decoded column, built in the pass that follows the source
// upload of a sketch build.
//
// Work unit: a (file, slab) pair from a host-built list.  The column holds the rows of several
// files back to back; file f owns rows [row0, row1) at arbitrary row numbers, cut into slabs of
// at most kSlabRows rows.  slabs[3 * s] = {file, first row, end row}; the slabs of one file are
// consecutive and file_slab_off[f] .. file_slab_off[f + 1] names them.  One block per slab, no
// block waits on another, and a second kernel folds each file's slab partials - so every result
// is a function of the data alone, never of the order blocks ran in.
//
// hs_sketch_minmax reduces on the order-preserving unsigned image of the value (hs_sortable's
// mapping, with Spark's float total order: every NaN is the one canonical NaN above +inf and
// -0.0 is +0.0), so float results are exact and order-independent and no float atomics exist.
// Rows are read with 16-byte loads: a scalar head up to the first 16-byte-aligned address of the
// slab (a slab starts at any row), a vector body, a scalar tail.  min / max / non-null count go
// through wave reductions (__shfl_xor) and 3 x 8 LDS words per block into the partial arrays.
//
// hs_sketch_bloom sets, per non-null row, the k bits of Spark's BloomFilterImpl:
//   h1 = murmur3(item, 0), h2 = murmur3(item, h1), c = int32(h1 + i * h2), c < 0 -> ~c,
//   bit c % bitSize, i = 1..k; bit b is bit (b & 31) of 32-bit word b >> 5 (the little-endian
//   halves of the 64-bit word b >> 6).
// Items are int64 values (hashLong of the widened integer) or, for dictionary-coded strings, the
// (h1, h2) pair of the row's dictionary entry, hashed once per entry by hs_sketch_hash_entries
// (hashUnsafeBytes with Spark's byte-wise tail).
//   LDS path (filter <= kBloomLdsWords 64-bit words = 64 KiB, so two 512-thread workgroups share
//   a CU's 160 KiB and keep 16 waves of row loads in flight): the block zeroes a private filter
//   in LDS, ORs its slab's bits in with LDS atomics, and writes it out as the slab's partial with
//   plain 16-byte stores; hs_sketch_bloom_fold ORs a file's partials.  A slab of 65536 rows sets
//   k * 65536 bits for at most 8192 flushed words.
//   Global path (larger filters): the file's filter is zeroed, blocks atomicOr its 32-bit words
//   in global memory and ignore the returned value.  OR commutes, so any order gives the same
//   words; it is the slower path.
#include "hs_common.h"

namespace {

constexpr int kSlabRows = 1 << 16;
constexpr int kBloomLdsWords = 8192;      // 64-bit words: 64 KiB of LDS
constexpr int kMinMaxThreads = 256;
constexpr int kBloomThreads = 512;

// ---------------------------------------------------------------------------------------------
// MinMax
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ uint64_t image_of(T v);

template <>
__device__ __forceinline__ uint64_t image_of<int8_t>(int8_t v) {
  return (uint64_t)(uint8_t)(v ^ (int8_t)0x80);
}
template <>
__device__ __forceinline__ uint64_t image_of<int16_t>(int16_t v) {
  return (uint64_t)(uint16_t)(v ^ (int16_t)0x8000);
}
template <>
__device__ __forceinline__ uint64_t image_of<int32_t>(int32_t v) {
  return (uint64_t)((uint32_t)v ^ 0x80000000u);
}
template <>
__device__ __forceinline__ uint64_t image_of<int64_t>(int64_t v) {
  return (uint64_t)v ^ 0x8000000000000000ull;
}
template <>
__device__ __forceinline__ uint64_t image_of<float>(float v) {
  uint32_t b = __float_as_uint(v);
  if (v != v) b = 0x7fc00000u;           // every NaN: the canonical one, above +inf
  else if (v == 0.0f) b = 0u;            // -0.0 == 0.0, kept as +0.0
  return (uint64_t)((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
template <>
__device__ __forceinline__ uint64_t image_of<double>(double v) {
  uint64_t b = (uint64_t)__double_as_longlong(v);
  if (v != v) b = 0x7ff8000000000000ull;
  else if (v == 0.0) b = 0ull;
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

struct MinMaxAcc {
  uint64_t mn, mx;
  int64_t cnt;
};

template <typename T>
__device__ __forceinline__ void acc_row(MinMaxAcc& a, T v, bool ok) {
  if (ok) {
    const uint64_t im = image_of<T>(v);
    a.mn = im < a.mn ? im : a.mn;
    a.mx = im > a.mx ? im : a.mx;
    ++a.cnt;
  }
}

template <typename T>
__device__ __forceinline__ void slab_minmax(const T* __restrict__ data,
                                            const uint8_t* __restrict__ valid, int64_t r0,
                                            int64_t r1, MinMaxAcc& a) {
  constexpr int V = 16 / (int)sizeof(T);
  const int64_t n = r1 - r0;
  // rows before the first 16-byte-aligned address of the slab
  const uintptr_t addr = (uintptr_t)(data + r0);
  int64_t head = (int64_t)(((16 - (addr & 15)) & 15) / sizeof(T));
  if (head > n) head = n;
  const int64_t nvec = (n - head) / V;
  const int64_t body0 = r0 + head, tail0 = body0 + nvec * V;
  for (int64_t r = r0 + threadIdx.x; r < body0; r += blockDim.x)
    acc_row<T>(a, data[r], valid == nullptr || valid[r] != 0);
  const uint4* __restrict__ vec = (const uint4*)(data + body0);
  for (int64_t i = threadIdx.x; i < nvec; i += blockDim.x) {
    const uint4 q = vec[i];
    T vals[V];
    __builtin_memcpy(vals, &q, 16);
    const int64_t r = body0 + i * V;
#pragma unroll
    for (int j = 0; j < V; ++j)
      acc_row<T>(a, vals[j], valid == nullptr || valid[r + j] != 0);
  }
  for (int64_t r = tail0 + threadIdx.x; r < r1; r += blockDim.x)
    acc_row<T>(a, data[r], valid == nullptr || valid[r] != 0);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(kMinMaxThreads) void sketch_minmax_slabs(
    ColDesc col, const int64_t* __restrict__ slabs, uint64_t* __restrict__ pmin,
    uint64_t* __restrict__ pmax, int64_t* __restrict__ pcnt) {
  constexpr int kWaves = kMinMaxThreads / HS_WAVE;
  __shared__ uint64_t s_mn[kWaves], s_mx[kWaves];
  __shared__ int64_t s_cnt[kWaves];
  const int64_t s = blockIdx.x;
  const int64_t r0 = slabs[3 * s + 1], r1 = slabs[3 * s + 2];
  MinMaxAcc a{~0ull, 0ull, 0};
  switch (col.type) {
    case HS_I8: slab_minmax<int8_t>((const int8_t*)col.data, col.valid, r0, r1, a); break;
    case HS_I16: slab_minmax<int16_t>((const int16_t*)col.data, col.valid, r0, r1, a); break;
    case HS_I32: slab_minmax<int32_t>((const int32_t*)col.data, col.valid, r0, r1, a); break;
    case HS_I64: slab_minmax<int64_t>((const int64_t*)col.data, col.valid, r0, r1, a); break;
    case HS_F32: slab_minmax<float>((const float*)col.data, col.valid, r0, r1, a); break;
    default: slab_minmax<double>((const double*)col.data, col.valid, r0, r1, a); break;
  }
  a.mn = wave_min_u64(a.mn);
  a.mx = wave_max_u64(a.mx);
  a.cnt = hs_wave_sum<long long>(a.cnt);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_mn[wave] = a.mn;
    s_mx[wave] = a.mx;
    s_cnt[wave] = a.cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t mn = s_mn[0], mx = s_mx[0];
    int64_t cnt = s_cnt[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      mn = s_mn[w] < mn ? s_mn[w] : mn;
      mx = s_mx[w] > mx ? s_mx[w] : mx;
      cnt += s_cnt[w];
    }
    pmin[s] = mn;
    pmax[s] = mx;
    pcnt[s] = cnt;
  }
}

// one wave per file over that file's slab partials
__global__ __launch_bounds__(HS_WAVE) void sketch_minmax_fold(
    const int64_t* __restrict__ file_slab_off, const uint64_t* __restrict__ pmin,
    const uint64_t* __restrict__ pmax, const int64_t* __restrict__ pcnt,
    uint64_t* __restrict__ omin, uint64_t* __restrict__ omax, int64_t* __restrict__ ocnt) {
  const int64_t f = blockIdx.x;
  const int64_t s0 = file_slab_off[f], s1 = file_slab_off[f + 1];
  uint64_t mn = ~0ull, mx = 0ull;
  long long cnt = 0;
  for (int64_t s = s0 + threadIdx.x; s < s1; s += HS_WAVE) {
    mn = pmin[s] < mn ? pmin[s] : mn;
    mx = pmax[s] > mx ? pmax[s] : mx;
    cnt += pcnt[s];
  }
  mn = wave_min_u64(mn);
  mx = wave_max_u64(mx);
  cnt = hs_wave_sum<long long>(cnt);
  if (threadIdx.x == 0) {
    omin[f] = mn;
    omax[f] = mx;
    ocnt[f] = cnt;
  }
}

// ---------------------------------------------------------------------------------------------
// Bloom
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hash_bytes(const uint8_t* __restrict__ p, int64_t len,
                                               uint32_t seed) {
  uint32_t h1 = seed;
  const int64_t aligned = len - (len & 3);
  for (int64_t i = 0; i < aligned; i += 4) {
    const uint32_t w = (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) |
                       ((uint32_t)p[i + 3] << 24);
    h1 = hs_mix_h1(h1, hs_mix_k1(w));
  }
  for (int64_t i = aligned; i < len; ++i)     // each tail byte as its own sign-extended int
    h1 = hs_mix_h1(h1, hs_mix_k1((uint32_t)(int32_t)(int8_t)p[i]));
  return hs_fmix(h1, (uint32_t)len);
}

__global__ __launch_bounds__(256) void sketch_hash_entries(
    const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets, int64_t n,
    uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t b = offsets[i], len = offsets[i + 1] - b;
  const uint32_t h1 = hash_bytes(bytes + b, len, 0u);
  out[2 * i] = h1;
  out[2 * i + 1] = hash_bytes(bytes + b, len, h1);
}

// (h1, h2) of row r, false for a null row
__device__ __forceinline__ bool row_hashes(const ColDesc& col, const uint32_t* __restrict__ entries,
                                           int64_t r, uint32_t& h1, uint32_t& h2) {
  if (!col_valid(col, r)) return false;
  if (entries != nullptr) {
    const int64_t code = ((const int32_t*)col.data)[r];
    h1 = entries[2 * code];
    h2 = entries[2 * code + 1];
  } else {
    const uint64_t v = (uint64_t)load_i64(col, r);
    h1 = hs_hash_long(v, 0u);
    h2 = hs_hash_long(v, h1);
  }
  return true;
}

__device__ __forceinline__ uint32_t bloom_bit(uint32_t h1, uint32_t h2, int i, int32_t bit_size) {
  int32_t c = (int32_t)(h1 + (uint32_t)i * h2);
  if (c < 0) c = ~c;
  return (uint32_t)(c % bit_size);
}

__global__ __launch_bounds__(kBloomThreads) void sketch_bloom_lds(
    ColDesc col, const uint32_t* __restrict__ entries, const int64_t* __restrict__ slabs,
    int num_words, int k, uint64_t* __restrict__ partials) {
  extern __shared__ uint4 s_filter4[];
  uint32_t* s_filter = (uint32_t*)s_filter4;
  const int n32 = num_words * 2;
  for (int i = threadIdx.x; i < n32; i += blockDim.x) s_filter[i] = 0u;
  __syncthreads();
  const int64_t s = blockIdx.x;
  const int64_t r0 = slabs[3 * s + 1], r1 = slabs[3 * s + 2];
  const int32_t bit_size = num_words * 64;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
    uint32_t h1, h2;
    if (!row_hashes(col, entries, r, h1, h2)) continue;
    for (int i = 1; i <= k; ++i) {
      const uint32_t b = bloom_bit(h1, h2, i, bit_size);
      atomicOr(&s_filter[b >> 5], 1u << (b & 31));
    }
  }
  __syncthreads();
  // the partial of slab s starts at a multiple of 8 * num_words bytes: 16-byte stores only when
  // the word count is even, 8-byte stores otherwise
  uint64_t* __restrict__ out = partials + s * (int64_t)num_words;
  if ((num_words & 1) == 0) {
    uint4* __restrict__ out4 = (uint4*)out;
    for (int i = threadIdx.x; i < num_words / 2; i += blockDim.x) out4[i] = s_filter4[i];
  } else {
    const uint64_t* s_filter8 = (const uint64_t*)s_filter4;
    for (int i = threadIdx.x; i < num_words; i += blockDim.x) out[i] = s_filter8[i];
  }
}

// out[f][w] = OR of the partials of file f's slabs (0 for a file without rows)
__global__ __launch_bounds__(256) void sketch_bloom_fold(
    const int64_t* __restrict__ file_slab_off, const uint64_t* __restrict__ partials,
    int num_words, uint64_t* __restrict__ out) {
  const int64_t f = blockIdx.y;
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= num_words) return;
  const int64_t s0 = file_slab_off[f], s1 = file_slab_off[f + 1];
  uint64_t acc = 0;
  for (int64_t s = s0; s < s1; ++s) acc |= partials[s * (int64_t)num_words + w];
  out[f * (int64_t)num_words + w] = acc;
}

__global__ __launch_bounds__(kBloomThreads) void sketch_bloom_global(
    ColDesc col, const uint32_t* __restrict__ entries, const int64_t* __restrict__ slabs,
    int num_words, int k, uint32_t* __restrict__ out) {
  const int64_t s = blockIdx.x;
  const int64_t f = slabs[3 * s], r0 = slabs[3 * s + 1], r1 = slabs[3 * s + 2];
  const int32_t bit_size = num_words * 64;
  uint32_t* __restrict__ filter = out + f * (int64_t)num_words * 2;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
    uint32_t h1, h2;
    if (!row_hashes(col, entries, r, h1, h2)) continue;
    for (int i = 1; i <= k; ++i) {
      const uint32_t b = bloom_bit(h1, h2, i, bit_size);
      atomicOr(&filter[b >> 5], 1u << (b & 31));
    }
  }
}

}  // namespace

extern "C" {

int hs_sketch_slab_rows() { return kSlabRows; }
int hs_sketch_bloom_lds_words() { return kBloomLdsWords; }

// col: rows of nfiles files back to back (integer or float storage); slabs: nslabs x {file,
// first row, end row}, the slabs of a file consecutive; file_slab_off: nfiles + 1 entries.
// pmin / pmax / pcnt: nslabs entries of workspace; omin / omax: nfiles order-preserving images
// (~0 / 0 for a file without a non-null value); ocnt: nfiles non-null counts.
int hs_sketch_minmax(const ColDesc* col, const int64_t* slabs, int64_t nslabs,
                     const int64_t* file_slab_off, int64_t nfiles, uint64_t* pmin, uint64_t* pmax,
                     int64_t* pcnt, uint64_t* omin, uint64_t* omax, int64_t* ocnt, void* stream) {
  if (col->type > HS_F64 || nslabs > 0x7fffffffll || nfiles > 0x7fffffffll) return -1;
  if (nslabs > 0)
    hipLaunchKernelGGL(sketch_minmax_slabs, dim3((unsigned)nslabs), dim3(kMinMaxThreads), 0,
                       (hipStream_t)stream, *col, slabs, pmin, pmax, pcnt);
  if (nfiles > 0)
    hipLaunchKernelGGL(sketch_minmax_fold, dim3((unsigned)nfiles), dim3(HS_WAVE), 0,
                       (hipStream_t)stream, file_slab_off, pmin, pmax, pcnt, omin, omax, ocnt);
  return (int)hipGetLastError();
}

// col: integer values (hashed as int64), or int32 dictionary codes when entries (2 x uint32 per
// dictionary entry from hs_sketch_hash_entries) is given.  out: nfiles x num_words 64-bit words,
// all written.  partials: nslabs x num_words words of workspace when num_words <=
// hs_sketch_bloom_lds_words(), unused (may be null) above it.
int hs_sketch_bloom(const ColDesc* col, const uint32_t* entries, const int64_t* slabs,
                    int64_t nslabs, const int64_t* file_slab_off, int64_t nfiles, int num_words,
                    int k, uint64_t* partials, uint64_t* out, void* stream) {
  if (num_words < 1 || num_words > (1 << 20) || k < 1 || nslabs > 0x7fffffffll ||
      nfiles > 65535)
    return -1;
  if (entries != nullptr ? col->type != HS_I32 : col->type > HS_I64) return -1;
  if (nfiles == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (num_words <= kBloomLdsWords) {
    if (nslabs > 0)
      hipLaunchKernelGGL(sketch_bloom_lds, dim3((unsigned)nslabs), dim3(kBloomThreads),
                         (size_t)num_words * 8, st, *col, entries, slabs, num_words, k, partials);
    hipLaunchKernelGGL(sketch_bloom_fold, dim3((unsigned)((num_words + 255) / 256),
                                               (unsigned)nfiles), dim3(256), 0, st,
                       file_slab_off, partials, num_words, out);
  } else {
    HS_CHECK(hipMemsetAsync(out, 0, (size_t)nfiles * num_words * 8, st));
    if (nslabs > 0)
      hipLaunchKernelGGL(sketch_bloom_global, dim3((unsigned)nslabs), dim3(kBloomThreads), 0, st,
                         *col, entries, slabs, num_words, k, (uint32_t*)out);
  }
  return (int)hipGetLastError();
}

// out: 2 x uint32 per entry: murmur3 hashUnsafeBytes(entry, 0) and hashUnsafeBytes(entry, h1).
int hs_sketch_hash_entries(const uint8_t* bytes, const int64_t* offsets, int64_t n, uint32_t* out,
                           void* stream) {
  if (n > 0)
    hipLaunchKernelGGL(sketch_hash_entries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, bytes, offsets, n, out);
  return (int)hipGetLastError();
}

}  // extern "C"
