
typedef long long i64;
typedef unsigned long long u64;
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ i64 wsumi(i64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wmin(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ bool in_set(const i64* s, int n, i64 x) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (s[m] < x) lo = m + 1; else hi = m; }
  return lo < n && s[lo] == x;
}
__device__ __forceinline__ bool bit_test(const u64* w, i64 nbits, i64 x) {
  return x >= 0 && x < nbits && ((w[x >> 6] >> (x & 63)) & 1ull);
}
// V consecutive elements starting at an index that is a multiple of V (so the address is
// aligned to V * sizeof(T) for a 16-byte aligned base): one dwordx4 per 16 bytes
template <typename T, int V>
__device__ __forceinline__ void vload(const T* __restrict__ p, long long i, T (&x)[V]) {
  constexpr int B = (int)sizeof(T) * V;
  if constexpr (B % 16 == 0) {
    const uint4* q = reinterpret_cast<const uint4*>(p + i);
#pragma unroll
    for (int k = 0; k < B / 16; ++k) reinterpret_cast<uint4*>(x)[k] = q[k];
  } else if constexpr (B == 8) {
    *reinterpret_cast<uint2*>(x) = *reinterpret_cast<const uint2*>(p + i);
  } else if constexpr (B == 4) {
    *reinterpret_cast<unsigned*>(x) = *reinterpret_cast<const unsigned*>(p + i);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) x[k] = p[i + k];
  }
}
// NW dwords of a wavefront-uniform window through a raw buffer resource: the base is uniform
// (scalar registers), the range check of the buffer unit returns 0 for bytes at or past
// ``nbytes`` - so the table's last, partial group loads with the same dwordx4s as a full one
// instead of a per-element edge path (which doubled the kernel's register footprint)
typedef unsigned hs_v4u __attribute__((ext_vector_type(4)));
// two 16-bit codes' range test at once: per half, (x - lo) | (hi - x) with saturation (the
// sign survives clamping), so bits 15 and 31 are the two rows' fail bits
typedef short hs_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned hs_rng2(unsigned x, int lo, int hi) {
  const hs_s2 v = __builtin_bit_cast(hs_s2, x);
  const hs_s2 l = {(short)lo, (short)lo}, h = {(short)hi, (short)hi};
  return __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(v, l)) |
         __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(h, v));
}
// [lo, hi] clamped to int16 for hs_rng2: a range wholly outside int16 becomes the empty
// (32767, -32768), which every code fails (clamping it bound by bound would keep an endpoint)
__device__ __forceinline__ int hs_c16lo(long long lo, long long hi) {
  return (hi < -32768ll || lo > 32767ll) ? 32767 : (int)(lo < -32768ll ? -32768ll : lo);
}
__device__ __forceinline__ int hs_c16hi(long long lo, long long hi) {
  return (hi < -32768ll || lo > 32767ll) ? -32768 : (int)(hi > 32767ll ? 32767ll : hi);
}
// bits 0..15 of x to the even, 16..31 to the odd positions (row order of a 2-rows-per-word mask)
__device__ __forceinline__ unsigned hs_unzip16(unsigned x) {
  unsigned a = x & 0xFFFFu, b = x >> 16;
  a = (a | (a << 8)) & 0x00FF00FFu; a = (a | (a << 4)) & 0x0F0F0F0Fu;
  a = (a | (a << 2)) & 0x33333333u; a = (a | (a << 1)) & 0x55555555u;
  b = (b | (b << 8)) & 0x00FF00FFu; b = (b | (b << 4)) & 0x0F0F0F0Fu;
  b = (b | (b << 2)) & 0x33333333u; b = (b | (b << 1)) & 0x55555555u;
  return a | (b << 1);
}
// a code bound clamped to +-2^20: narrow (<= 16-bit) codes against it never overflow int32
__device__ __forceinline__ int hs_c20(long long v) {
  return (int)(v < -1048576ll ? -1048576ll : (v > 1048576ll ? 1048576ll : v));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t hs_rsrc(const void* base, long long nbytes) {
  const u64 a_ = (u64)base;
  const unsigned lo_ = __builtin_amdgcn_readfirstlane((unsigned)a_);
  const unsigned hi_ = __builtin_amdgcn_readfirstlane((unsigned)(a_ >> 32));
  const long long n_ = nbytes < 0 ? 0 : (nbytes > 0x7fffffffll ? 0x7fffffffll : nbytes);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((u64)hi_ << 32) | lo_), (short)0,
                                           __builtin_amdgcn_readfirstlane((int)n_), 0x00020000);
}
template <int NW>
__device__ __forceinline__ void bload(__amdgpu_buffer_rsrc_t r, unsigned off, unsigned (&x)[NW]) {
  static_assert(NW % 4 == 0, "bload: whole dwordx4s");
#pragma unroll
  for (int k = 0; k < NW / 4; ++k) {
    const hs_v4u v = __builtin_amdgcn_raw_buffer_load_b128(r, off + 16 * k, 0, 0);
    x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
  }
}
// the same window read lane-coalesced: instruction k of the wavefront covers 1 KB contiguous
// (lane l: 16 bytes at (64 k + l) * 16), so lane l holds 16-byte chunks of other lanes' rows;
// hs_lds_t then moves every chunk to its owner through the wavefront's LDS slab (chunk j of
// lane g at slot g * NJ + (j ^ (g % NJ)): both the stores and the loads hit distinct banks)
template <int NW>
__device__ __forceinline__ void bload_t(__amdgpu_buffer_rsrc_t r, int ln, unsigned (&x)[NW]) {
  static_assert(NW % 4 == 0, "bload_t: whole dwordx4s");
#pragma unroll
  for (int k = 0; k < NW / 4; ++k) {
    const hs_v4u v = __builtin_amdgcn_raw_buffer_load_b128(r, (unsigned)((64 * k + ln) * 16), 0, 0);
    x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
  }
}
template <int NW>
__device__ __forceinline__ void hs_lds_t(hs_v4u* slab, int ln, unsigned (&x)[NW]) {
  constexpr int NJ = NW / 4;
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const int c = 64 * k + ln, g = c / NJ, j = c % NJ;
    hs_v4u v; v.x = x[4 * k]; v.y = x[4 * k + 1]; v.z = x[4 * k + 2]; v.w = x[4 * k + 3];
    slab[g * NJ + (j ^ (g % NJ))] = v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const hs_v4u v = slab[ln * NJ + (j ^ (ln % NJ))];
    x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void lds_min(double* p, double v) {
  u64* a = (u64*)p; u64 old = *a, as;
  do { as = old; if (__longlong_as_double((i64)as) <= v) break;
       old = atomicCAS(a, as, (u64)__double_as_longlong(v)); } while (as != old);
}
__device__ __forceinline__ void lds_max(double* p, double v) {
  u64* a = (u64*)p; u64 old = *a, as;
  do { as = old; if (__longlong_as_double((i64)as) >= v) break;
       old = atomicCAS(a, as, (u64)__double_as_longlong(v)); } while (as != old);
}
// order-preserving signed image of a double (top-K thresholds published with atomicMax)
__device__ __forceinline__ long long hs_dimg(double d) {
  const long long u = __double_as_longlong(d);
  return u >= 0 ? u : u ^ 0x7fffffffffffffffll;
}
__device__ __forceinline__ double hs_dimg_inv(long long i) {
  return __longlong_as_double(i >= 0 ? i : i ^ 0x7fffffffffffffffll);
}
// hash-mode grouping (exec/hash_agg.py, csrc/kernels/hash_agg.hip): probe hash and the bit
// images of float group keys (-0.0 -> 0.0, one NaN)
__device__ __forceinline__ u64 hs_mix64(u64 h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
  return h ^ (h >> 33);
}
__device__ __forceinline__ u64 hs_f64key(double d) {
  d = d == 0.0 ? 0.0 : d;
  return d != d ? 0x7ff8000000000000ull : (u64)__double_as_longlong(d);
}
__device__ __forceinline__ u64 hs_f32key(float f) {
  f = f == 0.0f ? 0.0f : f;
  return f != f ? 0x7fc00000ull : (u64)(unsigned)__float_as_uint(f);
}
struct Args {
  const int* RK0;
  const long long* RNG;
  unsigned* tags;
  unsigned* tags_b;
  long long NRG;
  long long NRUNS;
  long long KLO;
  long long KSP;
  long long KOF;
  const unsigned short* RMX1;
  long long CL1;
  const unsigned short* LO16;
  const unsigned short* RO16;
  const int* LG16;
  const int* RG16;
  const int* c8;
  long long B8;
  const short* c9;
  long long B9;
  long long CL4;
  long long CH4;
  long long CL4_b;
  long long CH4_b;
  long long CL1_b;
};
typedef int hs_i4 __attribute__((ext_vector_type(4)));
typedef unsigned short hs_us4 __attribute__((ext_vector_type(4)));
typedef unsigned short hs_ro4 __attribute__((ext_vector_type(4), aligned(2)));
typedef int hs_rk4 __attribute__((ext_vector_type(4), aligned(4)));
typedef int hs_c8x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef short hs_c9x4 __attribute__((ext_vector_type(4), aligned(2)));
extern "C" __global__ __launch_bounds__(256) void hs_jit_run_tags2(Args a) {
  auto IMG = [&](int row_) -> unsigned { return (false ? 0u : ({ const i64 __v_ = (i64)((long long)(a.B8 + (i64)a.c8[row_])); const i64 d_ = __v_ - a.KLO; (d_ < 0) ? 0u : (d_ > a.KSP ? 0xFFFFFFFFu : (unsigned)(d_ + 1)); })); };
  auto IMGF = [&](int row_) -> unsigned { return (false ? 0u : ({ const i64 __v_ = (i64)((long long)(a.B8 + (i64)a.c8[row_])); const i64 d_ = __v_ - a.KLO; (d_ < 0) ? 0u : (d_ > a.KSP ? 0xFFFFFFFFu : (unsigned)(d_ + 1)); })); };
  auto IMGV = [&](int w_) -> unsigned { return (false ? 0u : ({ const i64 __v_ = (i64)((long long)(a.B8 + (i64)w_)); const i64 d_ = __v_ - a.KLO; (d_ < 0) ? 0u : (d_ > a.KSP ? 0xFFFFFFFFu : (unsigned)(d_ + 1)); })); };
  const int lane = (int)(threadIdx.x & 63);
  const i64 G = (a.NRUNS + 63) >> 6;
  const int NR = (int)a.NRUNS, NB = (int)((a.NRUNS + 255) >> 8);
  const int nwv = (int)gridDim.x * 4;
  const int wv = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int per = ((NB + nwv - 1) / nwv + 1) / 2 * 2;
  const int bbeg = wv * per;
  const int bend = NB < bbeg + per ? NB : bbeg + per;
  if (bbeg >= bend || a.NRG <= 0) return;
  const i64 gend = G < ((i64)bend << 2) ? G : ((i64)bend << 2);
  const i64* RG = a.RNG;
  int rg = 0;
  { int lo = 0, hi = (int)a.NRG; const i64 r0 = (i64)bbeg << 8;
    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (RG[4 * m] <= r0) lo = m; else hi = m; }
    rg = lo; }
  int lr0 = (int)RG[4 * rg], lr1 = (int)RG[4 * rg + 1], s0 = (int)RG[4 * rg + 2], s1 = (int)RG[4 * rg + 3];
  i64 nxt0 = rg + 1 < a.NRG ? RG[4 * (rg + 1)] : 0x7fffffffffffffffll;
  int gbase = -1;   // right row of the next stage's first run (-1: range-relative)
  int pbA = 0; hs_us4 LA0 = {}; hs_ro4 RA0 = {}; int LGA0 = 0, RGA0 = 0, RHA0 = 0; hs_us4 M0A0 = {}; hs_c8x4 C8A0 = {}; hs_c9x4 C9A0 = {}; hs_us4 LA1 = {}; hs_ro4 RA1 = {}; int LGA1 = 0, RGA1 = 0, RHA1 = 0; hs_us4 M0A1 = {}; hs_c8x4 C8A1 = {}; hs_c9x4 C9A1 = {};
  int pbB = 0; hs_us4 LB0 = {}; hs_ro4 RB0 = {}; int LGB0 = 0, RGB0 = 0, RHB0 = 0; hs_us4 M0B0 = {}; hs_c8x4 C8B0 = {}; hs_c9x4 C9B0 = {}; hs_us4 LB1 = {}; hs_ro4 RB1 = {}; int LGB1 = 0, RGB1 = 0, RHB1 = 0; hs_us4 M0B1 = {}; hs_c8x4 C8B1 = {}; hs_c9x4 C9B1 = {};
  int slow_ = 0;
  int nb = bbeg;
  while (nb < bend) {
    while (nxt0 <= ((i64)nb << 8)) {
      ++rg; lr0 = (int)RG[4 * rg]; lr1 = (int)RG[4 * rg + 1]; s0 = (int)RG[4 * rg + 2];
      s1 = (int)RG[4 * rg + 3]; gbase = -1;
      nxt0 = rg + 1 < a.NRG ? RG[4 * (rg + 1)] : 0x7fffffffffffffffll;
    }
    const int rb_ = (nb) << 8;
    const int base_ = gbase >= 0 ? gbase + 0 : s0 + (rb_ - lr0);
    const bool f_ = slow_ == 0 && (nb) + 2 <= bend && rb_ >= lr0 && rb_ + 512 <= lr1 && rb_ + 512 <= NR && (i64)rb_ + 512 <= nxt0 && base_ >= s0 && base_ + 512 <= s1;
    if (!f_) {   // slow block: its 64-run groups one at a time
#pragma unroll 1
      for (i64 gi = (i64)nb << 2; gi < (((i64)nb + 1) << 2) && gi < gend; ++gi) {
        while (nxt0 <= (gi << 6)) {
          ++rg; lr0 = (int)RG[4 * rg]; lr1 = (int)RG[4 * rg + 1]; s0 = (int)RG[4 * rg + 2];
          s1 = (int)RG[4 * rg + 3]; gbase = -1;
          nxt0 = rg + 1 < a.NRG ? RG[4 * (rg + 1)] : 0x7fffffffffffffffll;
        }
        const int r0 = (int)(((gi + 0) << 6) + lane);
        const bool in0 = gi + 0 < gend;
        int l0_0 = lr0, l1_0 = lr1, a0_0 = s0, a1_0 = s1; bool own0 = true;
        if (r0 >= nxt0) { own0 = false; int q_ = rg;
          while (q_ + 1 < (int)a.NRG && RG[4 * (q_ + 1)] <= r0) ++q_;
          l0_0 = (int)RG[4 * q_]; l1_0 = (int)RG[4 * q_ + 1]; a0_0 = (int)RG[4 * q_ + 2]; a1_0 = (int)RG[4 * q_ + 3]; }
        const bool act0 = in0 && r0 < a.NRUNS && r0 >= l0_0 && r0 < l1_0 && a1_0 > a0_0;
        int j0 = (own0 && gbase >= 0) ? gbase + 0 + lane : a0_0 + (r0 - l0_0);
        j0 = act0 ? (j0 < a0_0 ? a0_0 : (j0 >= a1_0 ? a1_0 - 1 : j0)) : 0;
        const unsigned key0 = (unsigned)a.RK0[act0 ? r0 : 0] + (unsigned)a.KOF;
        const unsigned k0 = IMGF(j0);
        const int bm0_0 = (int)a.RMX1[act0 ? r0 : 0];
        const int w8_g0 = a.c8[j0];
        const int r8_g0 = (int)w8_g0;
        const long long x8_g0 = (long long)(a.B8 + (i64)w8_g0);
        const short w9_g0 = a.c9[j0];
        const int r9_g0 = (int)w9_g0;
        const int x9_g0 = (int)(a.B9 + (i64)w9_g0);
        bool hit0 = act0 && k0 == key0;
        int m0 = j0;
        unsigned tg0 = ((hit0) && ((true)) && ((true)) && ((true && (r9_g0 >= (int)a.CL4 && r9_g0 <= (int)a.CH4))) ? 1u : 0u);
        unsigned tgb0 = ((hit0) && ((true)) && ((true)) && ((true && (r9_g0 >= (int)a.CL4_b && r9_g0 <= (int)a.CH4_b))) ? 1u : 0u);
        if (act0 && !hit0) {
          const unsigned key_ = key0; int lo_, hi_;
          const unsigned kj_ = IMG(j0);
          if (kj_ == key_) { lo_ = j0; hi_ = j0; }
          else if (kj_ > key_) {
            hi_ = j0; int st_ = 1; lo_ = j0 - 1;
            while (lo_ > a0_0 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
            if (lo_ < a0_0) lo_ = a0_0;
          } else {
            lo_ = j0 + 1; int st_ = 1; hi_ = j0 + 1;
            while (hi_ < a1_0 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = j0 + st_; }
            if (hi_ > a1_0) hi_ = a1_0;
          }
          while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
          m0 = lo_;
          hit0 = lo_ < a1_0 && IMG(lo_) == key_;
          const int jm0 = hit0 ? lo_ : 0;
          const int w8_h0 = a.c8[jm0];
          const int r8_h0 = (int)w8_h0;
          const long long x8_h0 = (long long)(a.B8 + (i64)w8_h0);
          const short w9_h0 = a.c9[jm0];
          const int r9_h0 = (int)w9_h0;
          const int x9_h0 = (int)(a.B9 + (i64)w9_h0);
          tg0 = ((hit0) && ((true)) && ((true)) && ((true && (r9_h0 >= (int)a.CL4 && r9_h0 <= (int)a.CH4))) ? 1u : 0u);
          tgb0 = ((hit0) && ((true)) && ((true)) && ((true && (r9_h0 >= (int)a.CL4_b && r9_h0 <= (int)a.CH4_b))) ? 1u : 0u);
        }
        tg0 = ((bm0_0 >= hs_c20(a.CL1) + 32768)) ? tg0 : 0u;
        tgb0 = ((bm0_0 >= hs_c20(a.CL1_b) + 32768)) ? tgb0 : 0u;
        { const u64 bal_ = __ballot(tg0 != 0u);
          if (in0 && lane < 2) a.tags[((gi + 0) << 1) + lane] = (unsigned)(bal_ >> (32 * lane)); }
        { const u64 bal_ = __ballot(tgb0 != 0u);
          if (in0 && lane < 2) a.tags_b[((gi + 0) << 1) + lane] = (unsigned)(bal_ >> (32 * lane)); }
        gbase = __builtin_amdgcn_readlane((hit0 && own0) ? m0 + 1 : -1, 63);
      }
      slow_ -= slow_ > 0 ? 1 : 0;
      ++nb; continue;
    }
    pbA = base_;
    LA0 = *(const hs_us4*)(a.LO16 + (rb_ + 0 + 4 * lane));
    RA0 = *(const hs_ro4*)(a.RO16 + (base_ + 0 + 4 * lane));
    LGA0 = a.LG16[(rb_ + 0 + 4 * lane) >> 5];
    RGA0 = a.RG16[(base_ + 0 + 4 * lane) >> 5]; RHA0 = a.RG16[((base_ + 0 + 4 * lane) + 3) >> 5];
    M0A0 = *(const hs_us4*)(a.RMX1 + (rb_ + 0 + 4 * lane));
    C8A0 = *(const hs_c8x4*)(a.c8 + (base_ + 0 + 4 * lane));
    C9A0 = *(const hs_c9x4*)(a.c9 + (base_ + 0 + 4 * lane));
    LA1 = *(const hs_us4*)(a.LO16 + (rb_ + 256 + 4 * lane));
    RA1 = *(const hs_ro4*)(a.RO16 + (base_ + 256 + 4 * lane));
    LGA1 = a.LG16[(rb_ + 256 + 4 * lane) >> 5];
    RGA1 = a.RG16[(base_ + 256 + 4 * lane) >> 5]; RHA1 = a.RG16[((base_ + 256 + 4 * lane) + 3) >> 5];
    M0A1 = *(const hs_us4*)(a.RMX1 + (rb_ + 256 + 4 * lane));
    C8A1 = *(const hs_c8x4*)(a.c8 + (base_ + 256 + 4 * lane));
    C9A1 = *(const hs_c9x4*)(a.c9 + (base_ + 256 + 4 * lane));
    for (;;) {
      {
        const int rb_ = (nb + 2) << 8;
        const int base_ = gbase >= 0 ? gbase + 512 : s0 + (rb_ - lr0);
        const bool f_ = slow_ == 0 && (nb + 2) + 2 <= bend && rb_ >= lr0 && rb_ + 512 <= lr1 && rb_ + 512 <= NR && (i64)rb_ + 512 <= nxt0 && base_ >= s0 && base_ + 512 <= s1;
        const int nr_ = f_ ? rb_ : (nb << 8), nj_ = f_ ? base_ : pbA;
        pbB = nj_;
        LB0 = *(const hs_us4*)(a.LO16 + (nr_ + 0 + 4 * lane));
        RB0 = *(const hs_ro4*)(a.RO16 + (nj_ + 0 + 4 * lane));
        LGB0 = a.LG16[(nr_ + 0 + 4 * lane) >> 5];
        RGB0 = a.RG16[(nj_ + 0 + 4 * lane) >> 5]; RHB0 = a.RG16[((nj_ + 0 + 4 * lane) + 3) >> 5];
        M0B0 = *(const hs_us4*)(a.RMX1 + (nr_ + 0 + 4 * lane));
        C8B0 = *(const hs_c8x4*)(a.c8 + (nj_ + 0 + 4 * lane));
        C9B0 = *(const hs_c9x4*)(a.c9 + (nj_ + 0 + 4 * lane));
        LB1 = *(const hs_us4*)(a.LO16 + (nr_ + 256 + 4 * lane));
        RB1 = *(const hs_ro4*)(a.RO16 + (nj_ + 256 + 4 * lane));
        LGB1 = a.LG16[(nr_ + 256 + 4 * lane) >> 5];
        RGB1 = a.RG16[(nj_ + 256 + 4 * lane) >> 5]; RHB1 = a.RG16[((nj_ + 256 + 4 * lane) + 3) >> 5];
        M0B1 = *(const hs_us4*)(a.RMX1 + (nr_ + 256 + 4 * lane));
        C8B1 = *(const hs_c8x4*)(a.c8 + (nj_ + 256 + 4 * lane));
        C9B1 = *(const hs_c9x4*)(a.c9 + (nj_ + 256 + 4 * lane));
        if (__ballot(LGA0 == (int)0x80000000 || RGA0 == (int)0x80000000 || RHA0 == (int)0x80000000 || LGA1 == (int)0x80000000 || RGA1 == (int)0x80000000 || RHA1 == (int)0x80000000) != 0ull) { slow_ = 2; __builtin_amdgcn_s_waitcnt(0x0F70); break; }
        int nx_ = -1;
        { unsigned pk_ = 0u; unsigned pkb_ = 0u;
          { const int jA0_0 = pbA + 0 + 4 * lane;
          const int a0_A0_0 = s0, a1_A0_0 = s1; const bool actA0_0 = true;
          const unsigned keyA0_0 = (unsigned)LGA0 + (unsigned)LA0[0] + (unsigned)a.KOF;
          const unsigned kA0_0 = IMGV((int)((unsigned)((((pbA + 0 + 4 * lane) & 31) + 0) < 32 ? RGA0 : RHA0) + (unsigned)RA0[0]));
          const int bm0_A0_0 = (int)M0A0[0];
          const int r8_gA0_0 = (int)C8A0[0];
          const long long x8_gA0_0 = (long long)(a.B8 + (i64)C8A0[0]);
          const int r9_gA0_0 = (int)C9A0[0];
          const int x9_gA0_0 = (int)(a.B9 + (i64)C9A0[0]);
          bool hitA0_0 = actA0_0 && kA0_0 == keyA0_0;
          int mA0_0 = jA0_0;
          unsigned tgA0_0 = ((hitA0_0) && ((true)) && ((true)) && ((true && (r9_gA0_0 >= (int)a.CL4 && r9_gA0_0 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbA0_0 = ((hitA0_0) && ((true)) && ((true)) && ((true && (r9_gA0_0 >= (int)a.CL4_b && r9_gA0_0 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actA0_0 && !hitA0_0) {
            const unsigned key_ = keyA0_0; int lo_, hi_;
            const unsigned kj_ = IMG(jA0_0);
            if (kj_ == key_) { lo_ = jA0_0; hi_ = jA0_0; }
            else if (kj_ > key_) {
              hi_ = jA0_0; int st_ = 1; lo_ = jA0_0 - 1;
              while (lo_ > a0_A0_0 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_A0_0) lo_ = a0_A0_0;
            } else {
              lo_ = jA0_0 + 1; int st_ = 1; hi_ = jA0_0 + 1;
              while (hi_ < a1_A0_0 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jA0_0 + st_; }
              if (hi_ > a1_A0_0) hi_ = a1_A0_0;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mA0_0 = lo_;
            hitA0_0 = lo_ < a1_A0_0 && IMG(lo_) == key_;
            const int jmA0_0 = hitA0_0 ? lo_ : 0;
            const int w8_hA0_0 = a.c8[jmA0_0];
            const int r8_hA0_0 = (int)w8_hA0_0;
            const long long x8_hA0_0 = (long long)(a.B8 + (i64)w8_hA0_0);
            const short w9_hA0_0 = a.c9[jmA0_0];
            const int r9_hA0_0 = (int)w9_hA0_0;
            const int x9_hA0_0 = (int)(a.B9 + (i64)w9_hA0_0);
            tgA0_0 = ((hitA0_0) && ((true)) && ((true)) && ((true && (r9_hA0_0 >= (int)a.CL4 && r9_hA0_0 <= (int)a.CH4))) ? 1u : 0u);
            tgbA0_0 = ((hitA0_0) && ((true)) && ((true)) && ((true && (r9_hA0_0 >= (int)a.CL4_b && r9_hA0_0 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgA0_0 = ((bm0_A0_0 >= hs_c20(a.CL1) + 32768)) ? tgA0_0 : 0u;
          tgbA0_0 = ((bm0_A0_0 >= hs_c20(a.CL1_b) + 32768)) ? tgbA0_0 : 0u;
          pk_ |= (tgA0_0 & 1u) << 0;
          pkb_ |= (tgbA0_0 & 1u) << 0;
          }
          { const int jA0_1 = pbA + 1 + 4 * lane;
          const int a0_A0_1 = s0, a1_A0_1 = s1; const bool actA0_1 = true;
          const unsigned keyA0_1 = (unsigned)LGA0 + (unsigned)LA0[1] + (unsigned)a.KOF;
          const unsigned kA0_1 = IMGV((int)((unsigned)((((pbA + 0 + 4 * lane) & 31) + 1) < 32 ? RGA0 : RHA0) + (unsigned)RA0[1]));
          const int bm0_A0_1 = (int)M0A0[1];
          const int r8_gA0_1 = (int)C8A0[1];
          const long long x8_gA0_1 = (long long)(a.B8 + (i64)C8A0[1]);
          const int r9_gA0_1 = (int)C9A0[1];
          const int x9_gA0_1 = (int)(a.B9 + (i64)C9A0[1]);
          bool hitA0_1 = actA0_1 && kA0_1 == keyA0_1;
          int mA0_1 = jA0_1;
          unsigned tgA0_1 = ((hitA0_1) && ((true)) && ((true)) && ((true && (r9_gA0_1 >= (int)a.CL4 && r9_gA0_1 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbA0_1 = ((hitA0_1) && ((true)) && ((true)) && ((true && (r9_gA0_1 >= (int)a.CL4_b && r9_gA0_1 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actA0_1 && !hitA0_1) {
            const unsigned key_ = keyA0_1; int lo_, hi_;
            const unsigned kj_ = IMG(jA0_1);
            if (kj_ == key_) { lo_ = jA0_1; hi_ = jA0_1; }
            else if (kj_ > key_) {
              hi_ = jA0_1; int st_ = 1; lo_ = jA0_1 - 1;
              while (lo_ > a0_A0_1 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_A0_1) lo_ = a0_A0_1;
            } else {
              lo_ = jA0_1 + 1; int st_ = 1; hi_ = jA0_1 + 1;
              while (hi_ < a1_A0_1 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jA0_1 + st_; }
              if (hi_ > a1_A0_1) hi_ = a1_A0_1;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mA0_1 = lo_;
            hitA0_1 = lo_ < a1_A0_1 && IMG(lo_) == key_;
            const int jmA0_1 = hitA0_1 ? lo_ : 0;
            const int w8_hA0_1 = a.c8[jmA0_1];
            const int r8_hA0_1 = (int)w8_hA0_1;
            const long long x8_hA0_1 = (long long)(a.B8 + (i64)w8_hA0_1);
            const short w9_hA0_1 = a.c9[jmA0_1];
            const int r9_hA0_1 = (int)w9_hA0_1;
            const int x9_hA0_1 = (int)(a.B9 + (i64)w9_hA0_1);
            tgA0_1 = ((hitA0_1) && ((true)) && ((true)) && ((true && (r9_hA0_1 >= (int)a.CL4 && r9_hA0_1 <= (int)a.CH4))) ? 1u : 0u);
            tgbA0_1 = ((hitA0_1) && ((true)) && ((true)) && ((true && (r9_hA0_1 >= (int)a.CL4_b && r9_hA0_1 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgA0_1 = ((bm0_A0_1 >= hs_c20(a.CL1) + 32768)) ? tgA0_1 : 0u;
          tgbA0_1 = ((bm0_A0_1 >= hs_c20(a.CL1_b) + 32768)) ? tgbA0_1 : 0u;
          pk_ |= (tgA0_1 & 1u) << 1;
          pkb_ |= (tgbA0_1 & 1u) << 1;
          }
          { const int jA0_2 = pbA + 2 + 4 * lane;
          const int a0_A0_2 = s0, a1_A0_2 = s1; const bool actA0_2 = true;
          const unsigned keyA0_2 = (unsigned)LGA0 + (unsigned)LA0[2] + (unsigned)a.KOF;
          const unsigned kA0_2 = IMGV((int)((unsigned)((((pbA + 0 + 4 * lane) & 31) + 2) < 32 ? RGA0 : RHA0) + (unsigned)RA0[2]));
          const int bm0_A0_2 = (int)M0A0[2];
          const int r8_gA0_2 = (int)C8A0[2];
          const long long x8_gA0_2 = (long long)(a.B8 + (i64)C8A0[2]);
          const int r9_gA0_2 = (int)C9A0[2];
          const int x9_gA0_2 = (int)(a.B9 + (i64)C9A0[2]);
          bool hitA0_2 = actA0_2 && kA0_2 == keyA0_2;
          int mA0_2 = jA0_2;
          unsigned tgA0_2 = ((hitA0_2) && ((true)) && ((true)) && ((true && (r9_gA0_2 >= (int)a.CL4 && r9_gA0_2 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbA0_2 = ((hitA0_2) && ((true)) && ((true)) && ((true && (r9_gA0_2 >= (int)a.CL4_b && r9_gA0_2 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actA0_2 && !hitA0_2) {
            const unsigned key_ = keyA0_2; int lo_, hi_;
            const unsigned kj_ = IMG(jA0_2);
            if (kj_ == key_) { lo_ = jA0_2; hi_ = jA0_2; }
            else if (kj_ > key_) {
              hi_ = jA0_2; int st_ = 1; lo_ = jA0_2 - 1;
              while (lo_ > a0_A0_2 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_A0_2) lo_ = a0_A0_2;
            } else {
              lo_ = jA0_2 + 1; int st_ = 1; hi_ = jA0_2 + 1;
              while (hi_ < a1_A0_2 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jA0_2 + st_; }
              if (hi_ > a1_A0_2) hi_ = a1_A0_2;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mA0_2 = lo_;
            hitA0_2 = lo_ < a1_A0_2 && IMG(lo_) == key_;
            const int jmA0_2 = hitA0_2 ? lo_ : 0;
            const int w8_hA0_2 = a.c8[jmA0_2];
            const int r8_hA0_2 = (int)w8_hA0_2;
            const long long x8_hA0_2 = (long long)(a.B8 + (i64)w8_hA0_2);
            const short w9_hA0_2 = a.c9[jmA0_2];
            const int r9_hA0_2 = (int)w9_hA0_2;
            const int x9_hA0_2 = (int)(a.B9 + (i64)w9_hA0_2);
            tgA0_2 = ((hitA0_2) && ((true)) && ((true)) && ((true && (r9_hA0_2 >= (int)a.CL4 && r9_hA0_2 <= (int)a.CH4))) ? 1u : 0u);
            tgbA0_2 = ((hitA0_2) && ((true)) && ((true)) && ((true && (r9_hA0_2 >= (int)a.CL4_b && r9_hA0_2 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgA0_2 = ((bm0_A0_2 >= hs_c20(a.CL1) + 32768)) ? tgA0_2 : 0u;
          tgbA0_2 = ((bm0_A0_2 >= hs_c20(a.CL1_b) + 32768)) ? tgbA0_2 : 0u;
          pk_ |= (tgA0_2 & 1u) << 2;
          pkb_ |= (tgbA0_2 & 1u) << 2;
          }
          { const int jA0_3 = pbA + 3 + 4 * lane;
          const int a0_A0_3 = s0, a1_A0_3 = s1; const bool actA0_3 = true;
          const unsigned keyA0_3 = (unsigned)LGA0 + (unsigned)LA0[3] + (unsigned)a.KOF;
          const unsigned kA0_3 = IMGV((int)((unsigned)((((pbA + 0 + 4 * lane) & 31) + 3) < 32 ? RGA0 : RHA0) + (unsigned)RA0[3]));
          const int bm0_A0_3 = (int)M0A0[3];
          const int r8_gA0_3 = (int)C8A0[3];
          const long long x8_gA0_3 = (long long)(a.B8 + (i64)C8A0[3]);
          const int r9_gA0_3 = (int)C9A0[3];
          const int x9_gA0_3 = (int)(a.B9 + (i64)C9A0[3]);
          bool hitA0_3 = actA0_3 && kA0_3 == keyA0_3;
          int mA0_3 = jA0_3;
          unsigned tgA0_3 = ((hitA0_3) && ((true)) && ((true)) && ((true && (r9_gA0_3 >= (int)a.CL4 && r9_gA0_3 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbA0_3 = ((hitA0_3) && ((true)) && ((true)) && ((true && (r9_gA0_3 >= (int)a.CL4_b && r9_gA0_3 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actA0_3 && !hitA0_3) {
            const unsigned key_ = keyA0_3; int lo_, hi_;
            const unsigned kj_ = IMG(jA0_3);
            if (kj_ == key_) { lo_ = jA0_3; hi_ = jA0_3; }
            else if (kj_ > key_) {
              hi_ = jA0_3; int st_ = 1; lo_ = jA0_3 - 1;
              while (lo_ > a0_A0_3 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_A0_3) lo_ = a0_A0_3;
            } else {
              lo_ = jA0_3 + 1; int st_ = 1; hi_ = jA0_3 + 1;
              while (hi_ < a1_A0_3 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jA0_3 + st_; }
              if (hi_ > a1_A0_3) hi_ = a1_A0_3;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mA0_3 = lo_;
            hitA0_3 = lo_ < a1_A0_3 && IMG(lo_) == key_;
            const int jmA0_3 = hitA0_3 ? lo_ : 0;
            const int w8_hA0_3 = a.c8[jmA0_3];
            const int r8_hA0_3 = (int)w8_hA0_3;
            const long long x8_hA0_3 = (long long)(a.B8 + (i64)w8_hA0_3);
            const short w9_hA0_3 = a.c9[jmA0_3];
            const int r9_hA0_3 = (int)w9_hA0_3;
            const int x9_hA0_3 = (int)(a.B9 + (i64)w9_hA0_3);
            tgA0_3 = ((hitA0_3) && ((true)) && ((true)) && ((true && (r9_hA0_3 >= (int)a.CL4 && r9_hA0_3 <= (int)a.CH4))) ? 1u : 0u);
            tgbA0_3 = ((hitA0_3) && ((true)) && ((true)) && ((true && (r9_hA0_3 >= (int)a.CL4_b && r9_hA0_3 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgA0_3 = ((bm0_A0_3 >= hs_c20(a.CL1) + 32768)) ? tgA0_3 : 0u;
          tgbA0_3 = ((bm0_A0_3 >= hs_c20(a.CL1_b) + 32768)) ? tgbA0_3 : 0u;
          pk_ |= (tgA0_3 & 1u) << 3;
          pkb_ |= (tgbA0_3 & 1u) << 3;
          }
          pk_ <<= (unsigned)(4 * (lane & 7));
          pk_ |= (unsigned)__shfl_xor((int)pk_, 1, 64);
          pk_ |= (unsigned)__shfl_xor((int)pk_, 2, 64);
          pk_ |= (unsigned)__shfl_xor((int)pk_, 4, 64);
          if ((lane & 7) == 0) a.tags[(nb + 0) * 8 + (lane >> 3)] = pk_;
          pkb_ <<= (unsigned)(4 * (lane & 7));
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 1, 64);
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 2, 64);
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 4, 64);
          if ((lane & 7) == 0) a.tags_b[(nb + 0) * 8 + (lane >> 3)] = pkb_;
        }
        { unsigned pk_ = 0u; unsigned pkb_ = 0u;
          { const int jA1_0 = pbA + 256 + 4 * lane;
          const int a0_A1_0 = s0, a1_A1_0 = s1; const bool actA1_0 = true;
          const unsigned keyA1_0 = (unsigned)LGA1 + (unsigned)LA1[0] + (unsigned)a.KOF;
          const unsigned kA1_0 = IMGV((int)((unsigned)((((pbA + 256 + 4 * lane) & 31) + 0) < 32 ? RGA1 : RHA1) + (unsigned)RA1[0]));
          const int bm0_A1_0 = (int)M0A1[0];
          const int r8_gA1_0 = (int)C8A1[0];
          const long long x8_gA1_0 = (long long)(a.B8 + (i64)C8A1[0]);
          const int r9_gA1_0 = (int)C9A1[0];
          const int x9_gA1_0 = (int)(a.B9 + (i64)C9A1[0]);
          bool hitA1_0 = actA1_0 && kA1_0 == keyA1_0;
          int mA1_0 = jA1_0;
          unsigned tgA1_0 = ((hitA1_0) && ((true)) && ((true)) && ((true && (r9_gA1_0 >= (int)a.CL4 && r9_gA1_0 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbA1_0 = ((hitA1_0) && ((true)) && ((true)) && ((true && (r9_gA1_0 >= (int)a.CL4_b && r9_gA1_0 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actA1_0 && !hitA1_0) {
            const unsigned key_ = keyA1_0; int lo_, hi_;
            const unsigned kj_ = IMG(jA1_0);
            if (kj_ == key_) { lo_ = jA1_0; hi_ = jA1_0; }
            else if (kj_ > key_) {
              hi_ = jA1_0; int st_ = 1; lo_ = jA1_0 - 1;
              while (lo_ > a0_A1_0 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_A1_0) lo_ = a0_A1_0;
            } else {
              lo_ = jA1_0 + 1; int st_ = 1; hi_ = jA1_0 + 1;
              while (hi_ < a1_A1_0 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jA1_0 + st_; }
              if (hi_ > a1_A1_0) hi_ = a1_A1_0;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mA1_0 = lo_;
            hitA1_0 = lo_ < a1_A1_0 && IMG(lo_) == key_;
            const int jmA1_0 = hitA1_0 ? lo_ : 0;
            const int w8_hA1_0 = a.c8[jmA1_0];
            const int r8_hA1_0 = (int)w8_hA1_0;
            const long long x8_hA1_0 = (long long)(a.B8 + (i64)w8_hA1_0);
            const short w9_hA1_0 = a.c9[jmA1_0];
            const int r9_hA1_0 = (int)w9_hA1_0;
            const int x9_hA1_0 = (int)(a.B9 + (i64)w9_hA1_0);
            tgA1_0 = ((hitA1_0) && ((true)) && ((true)) && ((true && (r9_hA1_0 >= (int)a.CL4 && r9_hA1_0 <= (int)a.CH4))) ? 1u : 0u);
            tgbA1_0 = ((hitA1_0) && ((true)) && ((true)) && ((true && (r9_hA1_0 >= (int)a.CL4_b && r9_hA1_0 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgA1_0 = ((bm0_A1_0 >= hs_c20(a.CL1) + 32768)) ? tgA1_0 : 0u;
          tgbA1_0 = ((bm0_A1_0 >= hs_c20(a.CL1_b) + 32768)) ? tgbA1_0 : 0u;
          pk_ |= (tgA1_0 & 1u) << 0;
          pkb_ |= (tgbA1_0 & 1u) << 0;
          }
          { const int jA1_1 = pbA + 257 + 4 * lane;
          const int a0_A1_1 = s0, a1_A1_1 = s1; const bool actA1_1 = true;
          const unsigned keyA1_1 = (unsigned)LGA1 + (unsigned)LA1[1] + (unsigned)a.KOF;
          const unsigned kA1_1 = IMGV((int)((unsigned)((((pbA + 256 + 4 * lane) & 31) + 1) < 32 ? RGA1 : RHA1) + (unsigned)RA1[1]));
          const int bm0_A1_1 = (int)M0A1[1];
          const int r8_gA1_1 = (int)C8A1[1];
          const long long x8_gA1_1 = (long long)(a.B8 + (i64)C8A1[1]);
          const int r9_gA1_1 = (int)C9A1[1];
          const int x9_gA1_1 = (int)(a.B9 + (i64)C9A1[1]);
          bool hitA1_1 = actA1_1 && kA1_1 == keyA1_1;
          int mA1_1 = jA1_1;
          unsigned tgA1_1 = ((hitA1_1) && ((true)) && ((true)) && ((true && (r9_gA1_1 >= (int)a.CL4 && r9_gA1_1 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbA1_1 = ((hitA1_1) && ((true)) && ((true)) && ((true && (r9_gA1_1 >= (int)a.CL4_b && r9_gA1_1 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actA1_1 && !hitA1_1) {
            const unsigned key_ = keyA1_1; int lo_, hi_;
            const unsigned kj_ = IMG(jA1_1);
            if (kj_ == key_) { lo_ = jA1_1; hi_ = jA1_1; }
            else if (kj_ > key_) {
              hi_ = jA1_1; int st_ = 1; lo_ = jA1_1 - 1;
              while (lo_ > a0_A1_1 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_A1_1) lo_ = a0_A1_1;
            } else {
              lo_ = jA1_1 + 1; int st_ = 1; hi_ = jA1_1 + 1;
              while (hi_ < a1_A1_1 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jA1_1 + st_; }
              if (hi_ > a1_A1_1) hi_ = a1_A1_1;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mA1_1 = lo_;
            hitA1_1 = lo_ < a1_A1_1 && IMG(lo_) == key_;
            const int jmA1_1 = hitA1_1 ? lo_ : 0;
            const int w8_hA1_1 = a.c8[jmA1_1];
            const int r8_hA1_1 = (int)w8_hA1_1;
            const long long x8_hA1_1 = (long long)(a.B8 + (i64)w8_hA1_1);
            const short w9_hA1_1 = a.c9[jmA1_1];
            const int r9_hA1_1 = (int)w9_hA1_1;
            const int x9_hA1_1 = (int)(a.B9 + (i64)w9_hA1_1);
            tgA1_1 = ((hitA1_1) && ((true)) && ((true)) && ((true && (r9_hA1_1 >= (int)a.CL4 && r9_hA1_1 <= (int)a.CH4))) ? 1u : 0u);
            tgbA1_1 = ((hitA1_1) && ((true)) && ((true)) && ((true && (r9_hA1_1 >= (int)a.CL4_b && r9_hA1_1 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgA1_1 = ((bm0_A1_1 >= hs_c20(a.CL1) + 32768)) ? tgA1_1 : 0u;
          tgbA1_1 = ((bm0_A1_1 >= hs_c20(a.CL1_b) + 32768)) ? tgbA1_1 : 0u;
          pk_ |= (tgA1_1 & 1u) << 1;
          pkb_ |= (tgbA1_1 & 1u) << 1;
          }
          { const int jA1_2 = pbA + 258 + 4 * lane;
          const int a0_A1_2 = s0, a1_A1_2 = s1; const bool actA1_2 = true;
          const unsigned keyA1_2 = (unsigned)LGA1 + (unsigned)LA1[2] + (unsigned)a.KOF;
          const unsigned kA1_2 = IMGV((int)((unsigned)((((pbA + 256 + 4 * lane) & 31) + 2) < 32 ? RGA1 : RHA1) + (unsigned)RA1[2]));
          const int bm0_A1_2 = (int)M0A1[2];
          const int r8_gA1_2 = (int)C8A1[2];
          const long long x8_gA1_2 = (long long)(a.B8 + (i64)C8A1[2]);
          const int r9_gA1_2 = (int)C9A1[2];
          const int x9_gA1_2 = (int)(a.B9 + (i64)C9A1[2]);
          bool hitA1_2 = actA1_2 && kA1_2 == keyA1_2;
          int mA1_2 = jA1_2;
          unsigned tgA1_2 = ((hitA1_2) && ((true)) && ((true)) && ((true && (r9_gA1_2 >= (int)a.CL4 && r9_gA1_2 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbA1_2 = ((hitA1_2) && ((true)) && ((true)) && ((true && (r9_gA1_2 >= (int)a.CL4_b && r9_gA1_2 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actA1_2 && !hitA1_2) {
            const unsigned key_ = keyA1_2; int lo_, hi_;
            const unsigned kj_ = IMG(jA1_2);
            if (kj_ == key_) { lo_ = jA1_2; hi_ = jA1_2; }
            else if (kj_ > key_) {
              hi_ = jA1_2; int st_ = 1; lo_ = jA1_2 - 1;
              while (lo_ > a0_A1_2 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_A1_2) lo_ = a0_A1_2;
            } else {
              lo_ = jA1_2 + 1; int st_ = 1; hi_ = jA1_2 + 1;
              while (hi_ < a1_A1_2 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jA1_2 + st_; }
              if (hi_ > a1_A1_2) hi_ = a1_A1_2;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mA1_2 = lo_;
            hitA1_2 = lo_ < a1_A1_2 && IMG(lo_) == key_;
            const int jmA1_2 = hitA1_2 ? lo_ : 0;
            const int w8_hA1_2 = a.c8[jmA1_2];
            const int r8_hA1_2 = (int)w8_hA1_2;
            const long long x8_hA1_2 = (long long)(a.B8 + (i64)w8_hA1_2);
            const short w9_hA1_2 = a.c9[jmA1_2];
            const int r9_hA1_2 = (int)w9_hA1_2;
            const int x9_hA1_2 = (int)(a.B9 + (i64)w9_hA1_2);
            tgA1_2 = ((hitA1_2) && ((true)) && ((true)) && ((true && (r9_hA1_2 >= (int)a.CL4 && r9_hA1_2 <= (int)a.CH4))) ? 1u : 0u);
            tgbA1_2 = ((hitA1_2) && ((true)) && ((true)) && ((true && (r9_hA1_2 >= (int)a.CL4_b && r9_hA1_2 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgA1_2 = ((bm0_A1_2 >= hs_c20(a.CL1) + 32768)) ? tgA1_2 : 0u;
          tgbA1_2 = ((bm0_A1_2 >= hs_c20(a.CL1_b) + 32768)) ? tgbA1_2 : 0u;
          pk_ |= (tgA1_2 & 1u) << 2;
          pkb_ |= (tgbA1_2 & 1u) << 2;
          }
          { const int jA1_3 = pbA + 259 + 4 * lane;
          const int a0_A1_3 = s0, a1_A1_3 = s1; const bool actA1_3 = true;
          const unsigned keyA1_3 = (unsigned)LGA1 + (unsigned)LA1[3] + (unsigned)a.KOF;
          const unsigned kA1_3 = IMGV((int)((unsigned)((((pbA + 256 + 4 * lane) & 31) + 3) < 32 ? RGA1 : RHA1) + (unsigned)RA1[3]));
          const int bm0_A1_3 = (int)M0A1[3];
          const int r8_gA1_3 = (int)C8A1[3];
          const long long x8_gA1_3 = (long long)(a.B8 + (i64)C8A1[3]);
          const int r9_gA1_3 = (int)C9A1[3];
          const int x9_gA1_3 = (int)(a.B9 + (i64)C9A1[3]);
          bool hitA1_3 = actA1_3 && kA1_3 == keyA1_3;
          int mA1_3 = jA1_3;
          unsigned tgA1_3 = ((hitA1_3) && ((true)) && ((true)) && ((true && (r9_gA1_3 >= (int)a.CL4 && r9_gA1_3 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbA1_3 = ((hitA1_3) && ((true)) && ((true)) && ((true && (r9_gA1_3 >= (int)a.CL4_b && r9_gA1_3 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actA1_3 && !hitA1_3) {
            const unsigned key_ = keyA1_3; int lo_, hi_;
            const unsigned kj_ = IMG(jA1_3);
            if (kj_ == key_) { lo_ = jA1_3; hi_ = jA1_3; }
            else if (kj_ > key_) {
              hi_ = jA1_3; int st_ = 1; lo_ = jA1_3 - 1;
              while (lo_ > a0_A1_3 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_A1_3) lo_ = a0_A1_3;
            } else {
              lo_ = jA1_3 + 1; int st_ = 1; hi_ = jA1_3 + 1;
              while (hi_ < a1_A1_3 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jA1_3 + st_; }
              if (hi_ > a1_A1_3) hi_ = a1_A1_3;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mA1_3 = lo_;
            hitA1_3 = lo_ < a1_A1_3 && IMG(lo_) == key_;
            const int jmA1_3 = hitA1_3 ? lo_ : 0;
            const int w8_hA1_3 = a.c8[jmA1_3];
            const int r8_hA1_3 = (int)w8_hA1_3;
            const long long x8_hA1_3 = (long long)(a.B8 + (i64)w8_hA1_3);
            const short w9_hA1_3 = a.c9[jmA1_3];
            const int r9_hA1_3 = (int)w9_hA1_3;
            const int x9_hA1_3 = (int)(a.B9 + (i64)w9_hA1_3);
            tgA1_3 = ((hitA1_3) && ((true)) && ((true)) && ((true && (r9_hA1_3 >= (int)a.CL4 && r9_hA1_3 <= (int)a.CH4))) ? 1u : 0u);
            tgbA1_3 = ((hitA1_3) && ((true)) && ((true)) && ((true && (r9_hA1_3 >= (int)a.CL4_b && r9_hA1_3 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgA1_3 = ((bm0_A1_3 >= hs_c20(a.CL1) + 32768)) ? tgA1_3 : 0u;
          tgbA1_3 = ((bm0_A1_3 >= hs_c20(a.CL1_b) + 32768)) ? tgbA1_3 : 0u;
          pk_ |= (tgA1_3 & 1u) << 3;
          pkb_ |= (tgbA1_3 & 1u) << 3;
          nx_ = hitA1_3 ? mA1_3 + 1 : -1;
          }
          pk_ <<= (unsigned)(4 * (lane & 7));
          pk_ |= (unsigned)__shfl_xor((int)pk_, 1, 64);
          pk_ |= (unsigned)__shfl_xor((int)pk_, 2, 64);
          pk_ |= (unsigned)__shfl_xor((int)pk_, 4, 64);
          if ((lane & 7) == 0) a.tags[(nb + 1) * 8 + (lane >> 3)] = pk_;
          pkb_ <<= (unsigned)(4 * (lane & 7));
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 1, 64);
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 2, 64);
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 4, 64);
          if ((lane & 7) == 0) a.tags_b[(nb + 1) * 8 + (lane >> 3)] = pkb_;
        }
        gbase = __builtin_amdgcn_readlane(nx_, 63);
        nb += 2;
        if (!f_) { __builtin_amdgcn_s_waitcnt(0x0F70); break; }
      }
      {
        const int rb_ = (nb + 2) << 8;
        const int base_ = gbase >= 0 ? gbase + 512 : s0 + (rb_ - lr0);
        const bool f_ = slow_ == 0 && (nb + 2) + 2 <= bend && rb_ >= lr0 && rb_ + 512 <= lr1 && rb_ + 512 <= NR && (i64)rb_ + 512 <= nxt0 && base_ >= s0 && base_ + 512 <= s1;
        const int nr_ = f_ ? rb_ : (nb << 8), nj_ = f_ ? base_ : pbB;
        pbA = nj_;
        LA0 = *(const hs_us4*)(a.LO16 + (nr_ + 0 + 4 * lane));
        RA0 = *(const hs_ro4*)(a.RO16 + (nj_ + 0 + 4 * lane));
        LGA0 = a.LG16[(nr_ + 0 + 4 * lane) >> 5];
        RGA0 = a.RG16[(nj_ + 0 + 4 * lane) >> 5]; RHA0 = a.RG16[((nj_ + 0 + 4 * lane) + 3) >> 5];
        M0A0 = *(const hs_us4*)(a.RMX1 + (nr_ + 0 + 4 * lane));
        C8A0 = *(const hs_c8x4*)(a.c8 + (nj_ + 0 + 4 * lane));
        C9A0 = *(const hs_c9x4*)(a.c9 + (nj_ + 0 + 4 * lane));
        LA1 = *(const hs_us4*)(a.LO16 + (nr_ + 256 + 4 * lane));
        RA1 = *(const hs_ro4*)(a.RO16 + (nj_ + 256 + 4 * lane));
        LGA1 = a.LG16[(nr_ + 256 + 4 * lane) >> 5];
        RGA1 = a.RG16[(nj_ + 256 + 4 * lane) >> 5]; RHA1 = a.RG16[((nj_ + 256 + 4 * lane) + 3) >> 5];
        M0A1 = *(const hs_us4*)(a.RMX1 + (nr_ + 256 + 4 * lane));
        C8A1 = *(const hs_c8x4*)(a.c8 + (nj_ + 256 + 4 * lane));
        C9A1 = *(const hs_c9x4*)(a.c9 + (nj_ + 256 + 4 * lane));
        if (__ballot(LGB0 == (int)0x80000000 || RGB0 == (int)0x80000000 || RHB0 == (int)0x80000000 || LGB1 == (int)0x80000000 || RGB1 == (int)0x80000000 || RHB1 == (int)0x80000000) != 0ull) { slow_ = 2; __builtin_amdgcn_s_waitcnt(0x0F70); break; }
        int nx_ = -1;
        { unsigned pk_ = 0u; unsigned pkb_ = 0u;
          { const int jB0_0 = pbB + 0 + 4 * lane;
          const int a0_B0_0 = s0, a1_B0_0 = s1; const bool actB0_0 = true;
          const unsigned keyB0_0 = (unsigned)LGB0 + (unsigned)LB0[0] + (unsigned)a.KOF;
          const unsigned kB0_0 = IMGV((int)((unsigned)((((pbB + 0 + 4 * lane) & 31) + 0) < 32 ? RGB0 : RHB0) + (unsigned)RB0[0]));
          const int bm0_B0_0 = (int)M0B0[0];
          const int r8_gB0_0 = (int)C8B0[0];
          const long long x8_gB0_0 = (long long)(a.B8 + (i64)C8B0[0]);
          const int r9_gB0_0 = (int)C9B0[0];
          const int x9_gB0_0 = (int)(a.B9 + (i64)C9B0[0]);
          bool hitB0_0 = actB0_0 && kB0_0 == keyB0_0;
          int mB0_0 = jB0_0;
          unsigned tgB0_0 = ((hitB0_0) && ((true)) && ((true)) && ((true && (r9_gB0_0 >= (int)a.CL4 && r9_gB0_0 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbB0_0 = ((hitB0_0) && ((true)) && ((true)) && ((true && (r9_gB0_0 >= (int)a.CL4_b && r9_gB0_0 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actB0_0 && !hitB0_0) {
            const unsigned key_ = keyB0_0; int lo_, hi_;
            const unsigned kj_ = IMG(jB0_0);
            if (kj_ == key_) { lo_ = jB0_0; hi_ = jB0_0; }
            else if (kj_ > key_) {
              hi_ = jB0_0; int st_ = 1; lo_ = jB0_0 - 1;
              while (lo_ > a0_B0_0 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_B0_0) lo_ = a0_B0_0;
            } else {
              lo_ = jB0_0 + 1; int st_ = 1; hi_ = jB0_0 + 1;
              while (hi_ < a1_B0_0 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jB0_0 + st_; }
              if (hi_ > a1_B0_0) hi_ = a1_B0_0;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mB0_0 = lo_;
            hitB0_0 = lo_ < a1_B0_0 && IMG(lo_) == key_;
            const int jmB0_0 = hitB0_0 ? lo_ : 0;
            const int w8_hB0_0 = a.c8[jmB0_0];
            const int r8_hB0_0 = (int)w8_hB0_0;
            const long long x8_hB0_0 = (long long)(a.B8 + (i64)w8_hB0_0);
            const short w9_hB0_0 = a.c9[jmB0_0];
            const int r9_hB0_0 = (int)w9_hB0_0;
            const int x9_hB0_0 = (int)(a.B9 + (i64)w9_hB0_0);
            tgB0_0 = ((hitB0_0) && ((true)) && ((true)) && ((true && (r9_hB0_0 >= (int)a.CL4 && r9_hB0_0 <= (int)a.CH4))) ? 1u : 0u);
            tgbB0_0 = ((hitB0_0) && ((true)) && ((true)) && ((true && (r9_hB0_0 >= (int)a.CL4_b && r9_hB0_0 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgB0_0 = ((bm0_B0_0 >= hs_c20(a.CL1) + 32768)) ? tgB0_0 : 0u;
          tgbB0_0 = ((bm0_B0_0 >= hs_c20(a.CL1_b) + 32768)) ? tgbB0_0 : 0u;
          pk_ |= (tgB0_0 & 1u) << 0;
          pkb_ |= (tgbB0_0 & 1u) << 0;
          }
          { const int jB0_1 = pbB + 1 + 4 * lane;
          const int a0_B0_1 = s0, a1_B0_1 = s1; const bool actB0_1 = true;
          const unsigned keyB0_1 = (unsigned)LGB0 + (unsigned)LB0[1] + (unsigned)a.KOF;
          const unsigned kB0_1 = IMGV((int)((unsigned)((((pbB + 0 + 4 * lane) & 31) + 1) < 32 ? RGB0 : RHB0) + (unsigned)RB0[1]));
          const int bm0_B0_1 = (int)M0B0[1];
          const int r8_gB0_1 = (int)C8B0[1];
          const long long x8_gB0_1 = (long long)(a.B8 + (i64)C8B0[1]);
          const int r9_gB0_1 = (int)C9B0[1];
          const int x9_gB0_1 = (int)(a.B9 + (i64)C9B0[1]);
          bool hitB0_1 = actB0_1 && kB0_1 == keyB0_1;
          int mB0_1 = jB0_1;
          unsigned tgB0_1 = ((hitB0_1) && ((true)) && ((true)) && ((true && (r9_gB0_1 >= (int)a.CL4 && r9_gB0_1 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbB0_1 = ((hitB0_1) && ((true)) && ((true)) && ((true && (r9_gB0_1 >= (int)a.CL4_b && r9_gB0_1 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actB0_1 && !hitB0_1) {
            const unsigned key_ = keyB0_1; int lo_, hi_;
            const unsigned kj_ = IMG(jB0_1);
            if (kj_ == key_) { lo_ = jB0_1; hi_ = jB0_1; }
            else if (kj_ > key_) {
              hi_ = jB0_1; int st_ = 1; lo_ = jB0_1 - 1;
              while (lo_ > a0_B0_1 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_B0_1) lo_ = a0_B0_1;
            } else {
              lo_ = jB0_1 + 1; int st_ = 1; hi_ = jB0_1 + 1;
              while (hi_ < a1_B0_1 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jB0_1 + st_; }
              if (hi_ > a1_B0_1) hi_ = a1_B0_1;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mB0_1 = lo_;
            hitB0_1 = lo_ < a1_B0_1 && IMG(lo_) == key_;
            const int jmB0_1 = hitB0_1 ? lo_ : 0;
            const int w8_hB0_1 = a.c8[jmB0_1];
            const int r8_hB0_1 = (int)w8_hB0_1;
            const long long x8_hB0_1 = (long long)(a.B8 + (i64)w8_hB0_1);
            const short w9_hB0_1 = a.c9[jmB0_1];
            const int r9_hB0_1 = (int)w9_hB0_1;
            const int x9_hB0_1 = (int)(a.B9 + (i64)w9_hB0_1);
            tgB0_1 = ((hitB0_1) && ((true)) && ((true)) && ((true && (r9_hB0_1 >= (int)a.CL4 && r9_hB0_1 <= (int)a.CH4))) ? 1u : 0u);
            tgbB0_1 = ((hitB0_1) && ((true)) && ((true)) && ((true && (r9_hB0_1 >= (int)a.CL4_b && r9_hB0_1 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgB0_1 = ((bm0_B0_1 >= hs_c20(a.CL1) + 32768)) ? tgB0_1 : 0u;
          tgbB0_1 = ((bm0_B0_1 >= hs_c20(a.CL1_b) + 32768)) ? tgbB0_1 : 0u;
          pk_ |= (tgB0_1 & 1u) << 1;
          pkb_ |= (tgbB0_1 & 1u) << 1;
          }
          { const int jB0_2 = pbB + 2 + 4 * lane;
          const int a0_B0_2 = s0, a1_B0_2 = s1; const bool actB0_2 = true;
          const unsigned keyB0_2 = (unsigned)LGB0 + (unsigned)LB0[2] + (unsigned)a.KOF;
          const unsigned kB0_2 = IMGV((int)((unsigned)((((pbB + 0 + 4 * lane) & 31) + 2) < 32 ? RGB0 : RHB0) + (unsigned)RB0[2]));
          const int bm0_B0_2 = (int)M0B0[2];
          const int r8_gB0_2 = (int)C8B0[2];
          const long long x8_gB0_2 = (long long)(a.B8 + (i64)C8B0[2]);
          const int r9_gB0_2 = (int)C9B0[2];
          const int x9_gB0_2 = (int)(a.B9 + (i64)C9B0[2]);
          bool hitB0_2 = actB0_2 && kB0_2 == keyB0_2;
          int mB0_2 = jB0_2;
          unsigned tgB0_2 = ((hitB0_2) && ((true)) && ((true)) && ((true && (r9_gB0_2 >= (int)a.CL4 && r9_gB0_2 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbB0_2 = ((hitB0_2) && ((true)) && ((true)) && ((true && (r9_gB0_2 >= (int)a.CL4_b && r9_gB0_2 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actB0_2 && !hitB0_2) {
            const unsigned key_ = keyB0_2; int lo_, hi_;
            const unsigned kj_ = IMG(jB0_2);
            if (kj_ == key_) { lo_ = jB0_2; hi_ = jB0_2; }
            else if (kj_ > key_) {
              hi_ = jB0_2; int st_ = 1; lo_ = jB0_2 - 1;
              while (lo_ > a0_B0_2 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_B0_2) lo_ = a0_B0_2;
            } else {
              lo_ = jB0_2 + 1; int st_ = 1; hi_ = jB0_2 + 1;
              while (hi_ < a1_B0_2 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jB0_2 + st_; }
              if (hi_ > a1_B0_2) hi_ = a1_B0_2;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mB0_2 = lo_;
            hitB0_2 = lo_ < a1_B0_2 && IMG(lo_) == key_;
            const int jmB0_2 = hitB0_2 ? lo_ : 0;
            const int w8_hB0_2 = a.c8[jmB0_2];
            const int r8_hB0_2 = (int)w8_hB0_2;
            const long long x8_hB0_2 = (long long)(a.B8 + (i64)w8_hB0_2);
            const short w9_hB0_2 = a.c9[jmB0_2];
            const int r9_hB0_2 = (int)w9_hB0_2;
            const int x9_hB0_2 = (int)(a.B9 + (i64)w9_hB0_2);
            tgB0_2 = ((hitB0_2) && ((true)) && ((true)) && ((true && (r9_hB0_2 >= (int)a.CL4 && r9_hB0_2 <= (int)a.CH4))) ? 1u : 0u);
            tgbB0_2 = ((hitB0_2) && ((true)) && ((true)) && ((true && (r9_hB0_2 >= (int)a.CL4_b && r9_hB0_2 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgB0_2 = ((bm0_B0_2 >= hs_c20(a.CL1) + 32768)) ? tgB0_2 : 0u;
          tgbB0_2 = ((bm0_B0_2 >= hs_c20(a.CL1_b) + 32768)) ? tgbB0_2 : 0u;
          pk_ |= (tgB0_2 & 1u) << 2;
          pkb_ |= (tgbB0_2 & 1u) << 2;
          }
          { const int jB0_3 = pbB + 3 + 4 * lane;
          const int a0_B0_3 = s0, a1_B0_3 = s1; const bool actB0_3 = true;
          const unsigned keyB0_3 = (unsigned)LGB0 + (unsigned)LB0[3] + (unsigned)a.KOF;
          const unsigned kB0_3 = IMGV((int)((unsigned)((((pbB + 0 + 4 * lane) & 31) + 3) < 32 ? RGB0 : RHB0) + (unsigned)RB0[3]));
          const int bm0_B0_3 = (int)M0B0[3];
          const int r8_gB0_3 = (int)C8B0[3];
          const long long x8_gB0_3 = (long long)(a.B8 + (i64)C8B0[3]);
          const int r9_gB0_3 = (int)C9B0[3];
          const int x9_gB0_3 = (int)(a.B9 + (i64)C9B0[3]);
          bool hitB0_3 = actB0_3 && kB0_3 == keyB0_3;
          int mB0_3 = jB0_3;
          unsigned tgB0_3 = ((hitB0_3) && ((true)) && ((true)) && ((true && (r9_gB0_3 >= (int)a.CL4 && r9_gB0_3 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbB0_3 = ((hitB0_3) && ((true)) && ((true)) && ((true && (r9_gB0_3 >= (int)a.CL4_b && r9_gB0_3 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actB0_3 && !hitB0_3) {
            const unsigned key_ = keyB0_3; int lo_, hi_;
            const unsigned kj_ = IMG(jB0_3);
            if (kj_ == key_) { lo_ = jB0_3; hi_ = jB0_3; }
            else if (kj_ > key_) {
              hi_ = jB0_3; int st_ = 1; lo_ = jB0_3 - 1;
              while (lo_ > a0_B0_3 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_B0_3) lo_ = a0_B0_3;
            } else {
              lo_ = jB0_3 + 1; int st_ = 1; hi_ = jB0_3 + 1;
              while (hi_ < a1_B0_3 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jB0_3 + st_; }
              if (hi_ > a1_B0_3) hi_ = a1_B0_3;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mB0_3 = lo_;
            hitB0_3 = lo_ < a1_B0_3 && IMG(lo_) == key_;
            const int jmB0_3 = hitB0_3 ? lo_ : 0;
            const int w8_hB0_3 = a.c8[jmB0_3];
            const int r8_hB0_3 = (int)w8_hB0_3;
            const long long x8_hB0_3 = (long long)(a.B8 + (i64)w8_hB0_3);
            const short w9_hB0_3 = a.c9[jmB0_3];
            const int r9_hB0_3 = (int)w9_hB0_3;
            const int x9_hB0_3 = (int)(a.B9 + (i64)w9_hB0_3);
            tgB0_3 = ((hitB0_3) && ((true)) && ((true)) && ((true && (r9_hB0_3 >= (int)a.CL4 && r9_hB0_3 <= (int)a.CH4))) ? 1u : 0u);
            tgbB0_3 = ((hitB0_3) && ((true)) && ((true)) && ((true && (r9_hB0_3 >= (int)a.CL4_b && r9_hB0_3 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgB0_3 = ((bm0_B0_3 >= hs_c20(a.CL1) + 32768)) ? tgB0_3 : 0u;
          tgbB0_3 = ((bm0_B0_3 >= hs_c20(a.CL1_b) + 32768)) ? tgbB0_3 : 0u;
          pk_ |= (tgB0_3 & 1u) << 3;
          pkb_ |= (tgbB0_3 & 1u) << 3;
          }
          pk_ <<= (unsigned)(4 * (lane & 7));
          pk_ |= (unsigned)__shfl_xor((int)pk_, 1, 64);
          pk_ |= (unsigned)__shfl_xor((int)pk_, 2, 64);
          pk_ |= (unsigned)__shfl_xor((int)pk_, 4, 64);
          if ((lane & 7) == 0) a.tags[(nb + 0) * 8 + (lane >> 3)] = pk_;
          pkb_ <<= (unsigned)(4 * (lane & 7));
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 1, 64);
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 2, 64);
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 4, 64);
          if ((lane & 7) == 0) a.tags_b[(nb + 0) * 8 + (lane >> 3)] = pkb_;
        }
        { unsigned pk_ = 0u; unsigned pkb_ = 0u;
          { const int jB1_0 = pbB + 256 + 4 * lane;
          const int a0_B1_0 = s0, a1_B1_0 = s1; const bool actB1_0 = true;
          const unsigned keyB1_0 = (unsigned)LGB1 + (unsigned)LB1[0] + (unsigned)a.KOF;
          const unsigned kB1_0 = IMGV((int)((unsigned)((((pbB + 256 + 4 * lane) & 31) + 0) < 32 ? RGB1 : RHB1) + (unsigned)RB1[0]));
          const int bm0_B1_0 = (int)M0B1[0];
          const int r8_gB1_0 = (int)C8B1[0];
          const long long x8_gB1_0 = (long long)(a.B8 + (i64)C8B1[0]);
          const int r9_gB1_0 = (int)C9B1[0];
          const int x9_gB1_0 = (int)(a.B9 + (i64)C9B1[0]);
          bool hitB1_0 = actB1_0 && kB1_0 == keyB1_0;
          int mB1_0 = jB1_0;
          unsigned tgB1_0 = ((hitB1_0) && ((true)) && ((true)) && ((true && (r9_gB1_0 >= (int)a.CL4 && r9_gB1_0 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbB1_0 = ((hitB1_0) && ((true)) && ((true)) && ((true && (r9_gB1_0 >= (int)a.CL4_b && r9_gB1_0 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actB1_0 && !hitB1_0) {
            const unsigned key_ = keyB1_0; int lo_, hi_;
            const unsigned kj_ = IMG(jB1_0);
            if (kj_ == key_) { lo_ = jB1_0; hi_ = jB1_0; }
            else if (kj_ > key_) {
              hi_ = jB1_0; int st_ = 1; lo_ = jB1_0 - 1;
              while (lo_ > a0_B1_0 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_B1_0) lo_ = a0_B1_0;
            } else {
              lo_ = jB1_0 + 1; int st_ = 1; hi_ = jB1_0 + 1;
              while (hi_ < a1_B1_0 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jB1_0 + st_; }
              if (hi_ > a1_B1_0) hi_ = a1_B1_0;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mB1_0 = lo_;
            hitB1_0 = lo_ < a1_B1_0 && IMG(lo_) == key_;
            const int jmB1_0 = hitB1_0 ? lo_ : 0;
            const int w8_hB1_0 = a.c8[jmB1_0];
            const int r8_hB1_0 = (int)w8_hB1_0;
            const long long x8_hB1_0 = (long long)(a.B8 + (i64)w8_hB1_0);
            const short w9_hB1_0 = a.c9[jmB1_0];
            const int r9_hB1_0 = (int)w9_hB1_0;
            const int x9_hB1_0 = (int)(a.B9 + (i64)w9_hB1_0);
            tgB1_0 = ((hitB1_0) && ((true)) && ((true)) && ((true && (r9_hB1_0 >= (int)a.CL4 && r9_hB1_0 <= (int)a.CH4))) ? 1u : 0u);
            tgbB1_0 = ((hitB1_0) && ((true)) && ((true)) && ((true && (r9_hB1_0 >= (int)a.CL4_b && r9_hB1_0 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgB1_0 = ((bm0_B1_0 >= hs_c20(a.CL1) + 32768)) ? tgB1_0 : 0u;
          tgbB1_0 = ((bm0_B1_0 >= hs_c20(a.CL1_b) + 32768)) ? tgbB1_0 : 0u;
          pk_ |= (tgB1_0 & 1u) << 0;
          pkb_ |= (tgbB1_0 & 1u) << 0;
          }
          { const int jB1_1 = pbB + 257 + 4 * lane;
          const int a0_B1_1 = s0, a1_B1_1 = s1; const bool actB1_1 = true;
          const unsigned keyB1_1 = (unsigned)LGB1 + (unsigned)LB1[1] + (unsigned)a.KOF;
          const unsigned kB1_1 = IMGV((int)((unsigned)((((pbB + 256 + 4 * lane) & 31) + 1) < 32 ? RGB1 : RHB1) + (unsigned)RB1[1]));
          const int bm0_B1_1 = (int)M0B1[1];
          const int r8_gB1_1 = (int)C8B1[1];
          const long long x8_gB1_1 = (long long)(a.B8 + (i64)C8B1[1]);
          const int r9_gB1_1 = (int)C9B1[1];
          const int x9_gB1_1 = (int)(a.B9 + (i64)C9B1[1]);
          bool hitB1_1 = actB1_1 && kB1_1 == keyB1_1;
          int mB1_1 = jB1_1;
          unsigned tgB1_1 = ((hitB1_1) && ((true)) && ((true)) && ((true && (r9_gB1_1 >= (int)a.CL4 && r9_gB1_1 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbB1_1 = ((hitB1_1) && ((true)) && ((true)) && ((true && (r9_gB1_1 >= (int)a.CL4_b && r9_gB1_1 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actB1_1 && !hitB1_1) {
            const unsigned key_ = keyB1_1; int lo_, hi_;
            const unsigned kj_ = IMG(jB1_1);
            if (kj_ == key_) { lo_ = jB1_1; hi_ = jB1_1; }
            else if (kj_ > key_) {
              hi_ = jB1_1; int st_ = 1; lo_ = jB1_1 - 1;
              while (lo_ > a0_B1_1 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_B1_1) lo_ = a0_B1_1;
            } else {
              lo_ = jB1_1 + 1; int st_ = 1; hi_ = jB1_1 + 1;
              while (hi_ < a1_B1_1 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jB1_1 + st_; }
              if (hi_ > a1_B1_1) hi_ = a1_B1_1;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mB1_1 = lo_;
            hitB1_1 = lo_ < a1_B1_1 && IMG(lo_) == key_;
            const int jmB1_1 = hitB1_1 ? lo_ : 0;
            const int w8_hB1_1 = a.c8[jmB1_1];
            const int r8_hB1_1 = (int)w8_hB1_1;
            const long long x8_hB1_1 = (long long)(a.B8 + (i64)w8_hB1_1);
            const short w9_hB1_1 = a.c9[jmB1_1];
            const int r9_hB1_1 = (int)w9_hB1_1;
            const int x9_hB1_1 = (int)(a.B9 + (i64)w9_hB1_1);
            tgB1_1 = ((hitB1_1) && ((true)) && ((true)) && ((true && (r9_hB1_1 >= (int)a.CL4 && r9_hB1_1 <= (int)a.CH4))) ? 1u : 0u);
            tgbB1_1 = ((hitB1_1) && ((true)) && ((true)) && ((true && (r9_hB1_1 >= (int)a.CL4_b && r9_hB1_1 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgB1_1 = ((bm0_B1_1 >= hs_c20(a.CL1) + 32768)) ? tgB1_1 : 0u;
          tgbB1_1 = ((bm0_B1_1 >= hs_c20(a.CL1_b) + 32768)) ? tgbB1_1 : 0u;
          pk_ |= (tgB1_1 & 1u) << 1;
          pkb_ |= (tgbB1_1 & 1u) << 1;
          }
          { const int jB1_2 = pbB + 258 + 4 * lane;
          const int a0_B1_2 = s0, a1_B1_2 = s1; const bool actB1_2 = true;
          const unsigned keyB1_2 = (unsigned)LGB1 + (unsigned)LB1[2] + (unsigned)a.KOF;
          const unsigned kB1_2 = IMGV((int)((unsigned)((((pbB + 256 + 4 * lane) & 31) + 2) < 32 ? RGB1 : RHB1) + (unsigned)RB1[2]));
          const int bm0_B1_2 = (int)M0B1[2];
          const int r8_gB1_2 = (int)C8B1[2];
          const long long x8_gB1_2 = (long long)(a.B8 + (i64)C8B1[2]);
          const int r9_gB1_2 = (int)C9B1[2];
          const int x9_gB1_2 = (int)(a.B9 + (i64)C9B1[2]);
          bool hitB1_2 = actB1_2 && kB1_2 == keyB1_2;
          int mB1_2 = jB1_2;
          unsigned tgB1_2 = ((hitB1_2) && ((true)) && ((true)) && ((true && (r9_gB1_2 >= (int)a.CL4 && r9_gB1_2 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbB1_2 = ((hitB1_2) && ((true)) && ((true)) && ((true && (r9_gB1_2 >= (int)a.CL4_b && r9_gB1_2 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actB1_2 && !hitB1_2) {
            const unsigned key_ = keyB1_2; int lo_, hi_;
            const unsigned kj_ = IMG(jB1_2);
            if (kj_ == key_) { lo_ = jB1_2; hi_ = jB1_2; }
            else if (kj_ > key_) {
              hi_ = jB1_2; int st_ = 1; lo_ = jB1_2 - 1;
              while (lo_ > a0_B1_2 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_B1_2) lo_ = a0_B1_2;
            } else {
              lo_ = jB1_2 + 1; int st_ = 1; hi_ = jB1_2 + 1;
              while (hi_ < a1_B1_2 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jB1_2 + st_; }
              if (hi_ > a1_B1_2) hi_ = a1_B1_2;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mB1_2 = lo_;
            hitB1_2 = lo_ < a1_B1_2 && IMG(lo_) == key_;
            const int jmB1_2 = hitB1_2 ? lo_ : 0;
            const int w8_hB1_2 = a.c8[jmB1_2];
            const int r8_hB1_2 = (int)w8_hB1_2;
            const long long x8_hB1_2 = (long long)(a.B8 + (i64)w8_hB1_2);
            const short w9_hB1_2 = a.c9[jmB1_2];
            const int r9_hB1_2 = (int)w9_hB1_2;
            const int x9_hB1_2 = (int)(a.B9 + (i64)w9_hB1_2);
            tgB1_2 = ((hitB1_2) && ((true)) && ((true)) && ((true && (r9_hB1_2 >= (int)a.CL4 && r9_hB1_2 <= (int)a.CH4))) ? 1u : 0u);
            tgbB1_2 = ((hitB1_2) && ((true)) && ((true)) && ((true && (r9_hB1_2 >= (int)a.CL4_b && r9_hB1_2 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgB1_2 = ((bm0_B1_2 >= hs_c20(a.CL1) + 32768)) ? tgB1_2 : 0u;
          tgbB1_2 = ((bm0_B1_2 >= hs_c20(a.CL1_b) + 32768)) ? tgbB1_2 : 0u;
          pk_ |= (tgB1_2 & 1u) << 2;
          pkb_ |= (tgbB1_2 & 1u) << 2;
          }
          { const int jB1_3 = pbB + 259 + 4 * lane;
          const int a0_B1_3 = s0, a1_B1_3 = s1; const bool actB1_3 = true;
          const unsigned keyB1_3 = (unsigned)LGB1 + (unsigned)LB1[3] + (unsigned)a.KOF;
          const unsigned kB1_3 = IMGV((int)((unsigned)((((pbB + 256 + 4 * lane) & 31) + 3) < 32 ? RGB1 : RHB1) + (unsigned)RB1[3]));
          const int bm0_B1_3 = (int)M0B1[3];
          const int r8_gB1_3 = (int)C8B1[3];
          const long long x8_gB1_3 = (long long)(a.B8 + (i64)C8B1[3]);
          const int r9_gB1_3 = (int)C9B1[3];
          const int x9_gB1_3 = (int)(a.B9 + (i64)C9B1[3]);
          bool hitB1_3 = actB1_3 && kB1_3 == keyB1_3;
          int mB1_3 = jB1_3;
          unsigned tgB1_3 = ((hitB1_3) && ((true)) && ((true)) && ((true && (r9_gB1_3 >= (int)a.CL4 && r9_gB1_3 <= (int)a.CH4))) ? 1u : 0u);
          unsigned tgbB1_3 = ((hitB1_3) && ((true)) && ((true)) && ((true && (r9_gB1_3 >= (int)a.CL4_b && r9_gB1_3 <= (int)a.CH4_b))) ? 1u : 0u);
          if (actB1_3 && !hitB1_3) {
            const unsigned key_ = keyB1_3; int lo_, hi_;
            const unsigned kj_ = IMG(jB1_3);
            if (kj_ == key_) { lo_ = jB1_3; hi_ = jB1_3; }
            else if (kj_ > key_) {
              hi_ = jB1_3; int st_ = 1; lo_ = jB1_3 - 1;
              while (lo_ > a0_B1_3 && IMG(lo_) >= key_) { hi_ = lo_; st_ <<= 1; lo_ = hi_ - st_; }
              if (lo_ < a0_B1_3) lo_ = a0_B1_3;
            } else {
              lo_ = jB1_3 + 1; int st_ = 1; hi_ = jB1_3 + 1;
              while (hi_ < a1_B1_3 && IMG(hi_) < key_) { lo_ = hi_ + 1; st_ <<= 1; hi_ = jB1_3 + st_; }
              if (hi_ > a1_B1_3) hi_ = a1_B1_3;
            }
            while (lo_ < hi_) { const int md_ = (lo_ + hi_) >> 1; if (IMG(md_) < key_) lo_ = md_ + 1; else hi_ = md_; }
            mB1_3 = lo_;
            hitB1_3 = lo_ < a1_B1_3 && IMG(lo_) == key_;
            const int jmB1_3 = hitB1_3 ? lo_ : 0;
            const int w8_hB1_3 = a.c8[jmB1_3];
            const int r8_hB1_3 = (int)w8_hB1_3;
            const long long x8_hB1_3 = (long long)(a.B8 + (i64)w8_hB1_3);
            const short w9_hB1_3 = a.c9[jmB1_3];
            const int r9_hB1_3 = (int)w9_hB1_3;
            const int x9_hB1_3 = (int)(a.B9 + (i64)w9_hB1_3);
            tgB1_3 = ((hitB1_3) && ((true)) && ((true)) && ((true && (r9_hB1_3 >= (int)a.CL4 && r9_hB1_3 <= (int)a.CH4))) ? 1u : 0u);
            tgbB1_3 = ((hitB1_3) && ((true)) && ((true)) && ((true && (r9_hB1_3 >= (int)a.CL4_b && r9_hB1_3 <= (int)a.CH4_b))) ? 1u : 0u);
          }
          tgB1_3 = ((bm0_B1_3 >= hs_c20(a.CL1) + 32768)) ? tgB1_3 : 0u;
          tgbB1_3 = ((bm0_B1_3 >= hs_c20(a.CL1_b) + 32768)) ? tgbB1_3 : 0u;
          pk_ |= (tgB1_3 & 1u) << 3;
          pkb_ |= (tgbB1_3 & 1u) << 3;
          nx_ = hitB1_3 ? mB1_3 + 1 : -1;
          }
          pk_ <<= (unsigned)(4 * (lane & 7));
          pk_ |= (unsigned)__shfl_xor((int)pk_, 1, 64);
          pk_ |= (unsigned)__shfl_xor((int)pk_, 2, 64);
          pk_ |= (unsigned)__shfl_xor((int)pk_, 4, 64);
          if ((lane & 7) == 0) a.tags[(nb + 1) * 8 + (lane >> 3)] = pk_;
          pkb_ <<= (unsigned)(4 * (lane & 7));
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 1, 64);
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 2, 64);
          pkb_ |= (unsigned)__shfl_xor((int)pkb_, 4, 64);
          if ((lane & 7) == 0) a.tags_b[(nb + 1) * 8 + (lane >> 3)] = pkb_;
        }
        gbase = __builtin_amdgcn_readlane(nx_, 63);
        nb += 2;
        if (!f_) { __builtin_amdgcn_s_waitcnt(0x0F70); break; }
      }
    }
  }
}
