// SQL LIKE over a string dictionary (exec/like.py, exec/compile.py "like" leaves).
//
// String columns live on the device as int32 codes into a sorted dictionary, so `col LIKE p` is
// "bit code of a bitmap over the dictionary" - the PK_BITMAP predicate the generated scans already
// evaluate.  hs_dict_like builds that bitmap: it matches the compiled pattern against every
// dictionary entry once, one lane per entry.  Nothing is read back; the scan consumes the words
// on the same stream.
//
// Mapping: block 256 = 4 waves; wave w of the grid owns bitmap word w, then w + nwaves, ... (the
// stride is in whole waves, so a word never straddles two waves).  Lane l of the wave matches
// entry 64 * word + l; lanes past n vote 0.  The word loop's bound is wave-uniform and every lane
// reaches the __ballot (no early exit before it), so the tail word is right for any n.  Lane 0
// stores the ballot with a plain 64-bit store: every word is written exactly once, no atomics,
// no zero-fill needed.
//
// Pattern tokens (kind: 0 literal byte, 1 any one character, 2 any run; exec/like.py
// LikeProgram) are staged in LDS once per block: up to 256 tokens, 512 bytes.  The matcher's
// token index is uniform until lanes first disagree and diverges after that, so the tokens are
// read from LDS (a broadcast while uniform) rather than from global memory on every step.
//
// Matcher: the single-backtrack-point wildcard loop.  `_` and the backtrack both advance by one
// UTF-8 code point (lead byte + its 10xxxxxx continuation bytes), never past the entry's end.
// Worst case per lane is len * ntok steps; the host keeps len <= 4096 and ntok <= 256
// (exec/like.py KERNEL_MAX_ENTRY_BYTES / MAX_TOKENS), so no pattern makes a long-running kernel.
// Input is assumed valid UTF-8.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kMaxTok = 256;
constexpr int TK_LIT = 0, TK_ONE = 1, TK_RUN = 2;

__device__ __forceinline__ int64_t utf8_len(uint8_t b) {
  return b < 0x80 ? 1 : (b >= 0xF0 ? 4 : (b >= 0xE0 ? 3 : (b >= 0xC0 ? 2 : 1)));
}

__device__ __forceinline__ bool like_match(const uint8_t* __restrict__ s, int64_t len,
                                           const uint8_t* kind, const uint8_t* byte, int ntok) {
  int64_t si = 0, star_s = 0;
  int p = 0, star_p = -1;
  while (si < len) {
    const int k = p < ntok ? kind[p] : -1;
    const uint8_t c = s[si];
    if (k == TK_LIT && byte[p] == c) {
      ++si;
      ++p;
    } else if (k == TK_ONE) {
      si += utf8_len(c);
      if (si > len) si = len;
      ++p;
    } else if (k == TK_RUN) {
      star_p = p++;
      star_s = si;
    } else if (star_p >= 0) {
      // retry with the last run one character longer
      star_s += utf8_len(s[star_s]);
      if (star_s > len) star_s = len;
      si = star_s;
      p = star_p + 1;
    } else {
      return false;
    }
  }
  while (p < ntok && kind[p] == TK_RUN) ++p;
  return p == ntok;
}

__global__ __launch_bounds__(256) void hs_dict_like_kernel(
    const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets, int64_t n,
    const uint8_t* __restrict__ tok_kind, const uint8_t* __restrict__ tok_byte, int ntok,
    unsigned long long* __restrict__ words, int64_t nwords) {
  __shared__ uint8_t s_kind[kMaxTok];
  __shared__ uint8_t s_byte[kMaxTok];
  for (int i = threadIdx.x; i < ntok; i += blockDim.x) {
    s_kind[i] = tok_kind[i];
    s_byte[i] = tok_byte[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t w = wave; w < nwords; w += nwaves) {   // wave-uniform bound
    const int64_t i = w * 64 + lane;
    bool m = false;
    if (i < n) {
      const int64_t b = offsets[i];
      m = like_match(bytes + b, offsets[i + 1] - b, s_kind, s_byte, ntok);
    }
    const unsigned long long vote = __ballot(m);
    if (lane == 0) words[w] = vote;
  }
}

// key_bitmap.hip's cap, over the threads the words need
unsigned grid_for(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

extern "C" {

// bytes / offsets: the dictionary's UTF-8 bytes and n + 1 int64 offsets into them; tok_kind /
// tok_byte: ntok (<= 256) tokens; words: ceil(n / 64) entries, every one written (bit i = entry
// i matches).  Returns a HIP error code, or -1 for a program over the token cap.
int hs_dict_like(const uint8_t* bytes, const int64_t* offsets, int64_t n,
                 const uint8_t* tok_kind, const uint8_t* tok_byte, int ntok,
                 unsigned long long* words, void* stream) {
  if (ntok < 0 || ntok > kMaxTok) return -1;
  if (n > 0) {
    const int64_t nwords = (n + 63) / 64;
    hipLaunchKernelGGL(hs_dict_like_kernel, dim3(grid_for(nwords * 64)), dim3(256), 0,
                       (hipStream_t)stream, bytes, offsets, n, tok_kind, tok_byte, ntok, words,
                       nwords);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
