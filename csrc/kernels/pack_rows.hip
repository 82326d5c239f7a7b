// Row-packed copy of up to 8 compact code columns (exec/jit.py scan_pack_layout: the packed form
// of the generated scan reads one bit-packed row stream instead of its code columns).
//
// Layout: a row is B bits (a multiple of 4, at most 64), column c's field
// ((code - off_c) mod 2^32) & (2^bits_c - 1) at bits [pos_c, pos_c + bits_c) of it; rows are laid
// back to back, little endian, so 8 rows fill exactly B bytes = B / 4 dwords and row i of the
// table starts at bit (i % 8) * B of the dword group (i / 8) * (B / 4).  Rows of [n, npad) are
// padding (npad a multiple of 2048, the scan's tile): every field reads as zero.
//
// One pass: a thread owns one 8-row group (its codes are 8 / 16 / 32 contiguous bytes per column:
// one or two vector loads when the column's base is aligned, element loads in the table's last
// group), builds the group's B / 4 dwords in registers with constant shifts (the kernel is
// instantiated per B / 4), and the wavefront's 64 groups - 64 * B contiguous bytes - go out
// through its LDS slab as whole dwordx4s, 1 KB per store instruction.
#include <hip/hip_runtime.h>

#include <cstdint>

extern "C" {
struct HsPackCol {
  const void* data;   // int8 / int16 / int32 codes
  int64_t off;        // subtracted from every code (the column's smallest code)
  int32_t width;      // bytes per code: 1, 2 or 4
  int32_t pos;        // first bit of the field in the row
  int32_t bits;       // field width, 1..32
  int32_t vec;        // base aligned to 8 * width bytes: full groups load as vectors
};
struct HsPackArgs {
  HsPackCol c[8];
  int32_t ncols;
  int32_t pad;
};
}

namespace {

constexpr int PACK_BLOCK = 256;
constexpr int PACK_TILE_ROWS = 2048;   // 8 rows per thread: one block per scan tile

template <typename T>
__device__ __forceinline__ void pack_load8(const T* __restrict__ p, int64_t i, int64_t n, bool vec,
                                           uint32_t (&v)[8]) {
  if (vec && i + 8 <= n) {
    T x[8];
    if constexpr (sizeof(T) == 1) {
      *reinterpret_cast<uint2*>(x) = *reinterpret_cast<const uint2*>(p + i);
    } else if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<uint4*>(x) = *reinterpret_cast<const uint4*>(p + i);
    } else {
      reinterpret_cast<uint4*>(x)[0] = reinterpret_cast<const uint4*>(p + i)[0];
      reinterpret_cast<uint4*>(x)[1] = reinterpret_cast<const uint4*>(p + i)[1];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (uint32_t)(int32_t)x[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = i + k < n ? (uint32_t)(int32_t)p[i + k] : 0u;
  }
}

template <int NW>
__global__ __launch_bounds__(PACK_BLOCK) void hs_pack_bits_kernel(HsPackArgs a, int64_t n,
                                                                  uint32_t* __restrict__ out) {
  constexpr int B = 4 * NW;
  __shared__ __attribute__((aligned(16))) uint32_t slab[PACK_BLOCK / 64][64 * NW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * PACK_BLOCK + threadIdx.x;   // 8-row group
  const int64_t i0 = g * 8;
  uint64_t row[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) row[k] = 0ull;
  if (i0 < n) {
    for (int c = 0; c < a.ncols; ++c) {
      const HsPackCol col = a.c[c];
      uint32_t v[8];
      if (col.width == 1) {
        pack_load8(static_cast<const int8_t*>(col.data), i0, n, col.vec != 0, v);
      } else if (col.width == 2) {
        pack_load8(static_cast<const int16_t*>(col.data), i0, n, col.vec != 0, v);
      } else {
        pack_load8(static_cast<const int32_t*>(col.data), i0, n, col.vec != 0, v);
      }
      const uint32_t mask = col.bits >= 32 ? 0xFFFFFFFFu : ((1u << col.bits) - 1u);
      const uint32_t off = (uint32_t)col.off;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t f = i0 + k < n ? ((v[k] - off) & mask) : 0u;
        row[k] |= (uint64_t)f << col.pos;
      }
    }
  }
  uint32_t w[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) w[j] = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int o = k * B, j0 = o >> 5, sh = o & 31;   // constants once unrolled
    w[j0] |= (uint32_t)(row[k] << sh);
    if (sh + B > 32) w[j0 + 1 < NW ? j0 + 1 : 0] |= (uint32_t)(row[k] >> (32 - sh));
    if (sh + B > 64) w[j0 + 2 < NW ? j0 + 2 : 0] |= (uint32_t)(row[k] >> (64 - sh));
  }
#pragma unroll
  for (int j = 0; j < NW; ++j) slab[wv][lane * NW + j] = w[j];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // the wavefront's 64 groups are 64 * NW dwords = 16 * NW dwordx4s, contiguous in the output
  const int64_t wbase = ((int64_t)blockIdx.x * PACK_BLOCK + wv * 64) * NW;   // dwords
  uint4* __restrict__ o4 = reinterpret_cast<uint4*>(out + wbase);
  const uint4* s4 = reinterpret_cast<const uint4*>(slab[wv]);
  for (int c = lane; c < 16 * NW; c += 64) o4[c] = s4[c];
}

template <int NW>
void pack_launch(const HsPackArgs& a, int64_t n, int64_t npad, uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(hs_pack_bits_kernel<NW>, dim3((unsigned)(npad / PACK_TILE_ROWS)),
                     dim3(PACK_BLOCK), 0, s, a, n, out);
}

}  // namespace

extern "C" {

int hs_pack_args_size() { return (int)sizeof(HsPackArgs); }

// out: npad / 8 * (B / 4) dwords, 16-byte aligned; npad >= n, a positive multiple of 2048
int hs_pack_rows(const HsPackArgs* a, int64_t n, int B, uint32_t* out, int64_t npad,
                 void* stream) {
  if (!a || a->ncols < 1 || a->ncols > 8 || B < 4 || B > 64 || (B & 3) || n < 0 || npad < n ||
      npad <= 0 || npad % PACK_TILE_ROWS || ((uintptr_t)out & 15))
    return (int)hipErrorInvalidValue;
  for (int c = 0; c < a->ncols; ++c) {
    const HsPackCol& k = a->c[c];
    if ((k.width != 1 && k.width != 2 && k.width != 4) || k.bits < 1 || k.bits > 32 ||
        k.pos < 0 || k.pos + k.bits > B || (!k.data && n > 0))
      return (int)hipErrorInvalidValue;
  }
  if (npad / PACK_TILE_ROWS > 0x7fffffffll) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  switch (B / 4) {
#define HS_PACK_CASE(NW) case NW: pack_launch<NW>(*a, n, npad, out, s); break;
    HS_PACK_CASE(1) HS_PACK_CASE(2) HS_PACK_CASE(3) HS_PACK_CASE(4)
    HS_PACK_CASE(5) HS_PACK_CASE(6) HS_PACK_CASE(7) HS_PACK_CASE(8)
    HS_PACK_CASE(9) HS_PACK_CASE(10) HS_PACK_CASE(11) HS_PACK_CASE(12)
    HS_PACK_CASE(13) HS_PACK_CASE(14) HS_PACK_CASE(15) HS_PACK_CASE(16)
#undef HS_PACK_CASE
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
