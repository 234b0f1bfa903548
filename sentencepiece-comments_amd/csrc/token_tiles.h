// Token-tile layout shared by the passes that walk the tokens of a batch
// (decode_kernels.hip, byte_epilogue_kernels.hip): every pass runs
// kDecodeBlocks blocks, block b owns one contiguous token range whose length
// is a multiple of kDecodeTile, and walks it one sub-tile (one token per
// thread) at a time.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "decode.h"

namespace spm_amd {
namespace {

struct TokView {
  const int32_t *ids;
  const uint64_t *tok_off;
  uint64_t n;
  uint64_t base;  // tok_off[0], read by each kernel (the id CSR need not start at 0)
  uint32_t extras;
};

__device__ __forceinline__ uint64_t SentStart(const TokView &v, uint64_t i) {
  return v.tok_off[i] - v.base + i * v.extras;
}

// Largest a in [lo, hi) with S(a) <= g; the caller guarantees S(lo) <= g and
// (hi == limit or S(hi) > g).  Gallops from lo, so a thread that walks
// ascending tokens pays for the distance moved.
__device__ __forceinline__ uint64_t FindSentence(const TokView &v, uint64_t lo, uint64_t limit, uint64_t g) {
  uint64_t a = lo, b, step = 1;
  for (;;) {
    b = a + step;
    if (b >= limit) {
      b = limit;
      break;
    }
    if (SentStart(v, b) > g) break;
    a = b;
    step <<= 1;
  }
  while (b - a > 1) {
    const uint64_t mid = a + (b - a) / 2;
    if (SentStart(v, mid) <= g) a = mid;
    else b = mid;
  }
  return a;
}

struct Range {
  uint64_t begin, end;
};

__device__ __forceinline__ Range BlockRange(const TokView &v) {
  const uint64_t total = SentStart(v, v.n);
  uint64_t chunk = (total + gridDim.x - 1) / gridDim.x;
  chunk = (chunk + kDecodeTile - 1) / kDecodeTile * kDecodeTile;
  Range r;
  r.begin = static_cast<uint64_t>(blockIdx.x) * chunk;
  r.end = r.begin + chunk;
  if (r.begin > total) r.begin = total;
  if (r.end > total) r.end = total;
  return r;
}

__device__ __forceinline__ uint64_t BlockSum64(uint64_t v, uint64_t *s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), o);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), o);
    v += (static_cast<uint64_t>(hi) << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint64_t r = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  __syncthreads();
  return r;
}

// Exclusive scan of one value per thread over the block; *total = the sum.
__device__ __forceinline__ uint32_t BlockExclusiveScan(uint32_t v, uint32_t *s_w, uint32_t *total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t wv = s_w[k];
    if (k < w) before += wv;
    tot += wv;
  }
  __syncthreads();
  *total = tot;
  return before + inc - v;
}

}  // namespace
}  // namespace spm_amd
