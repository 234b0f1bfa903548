// Vocabulary restriction and piece counting on the device.
//
// Re-tag: SetVocabulary / ResetVocabulary change piece types on a loaded
// model (sentencepiece_processor.cc:203-245).  The per-unit tables of the
// unigram trie (kind bits in the value, the byte pass's usable-node score)
// and the BPE pair entries (the unused bit of the merged piece) are rewritten
// in place from an uploaded per-piece kind array (0 other, 1 user-defined,
// 2 unused): one byte per piece goes up, the tables never come down.
//
// Count: occurrences of every id of a token stream, added to 64-bit counters.
// Piece frequencies are Zipfian, so both kernels sum equal ids before they
// touch global memory: per-workgroup 32-bit bins in LDS where the vocabulary
// fits (one global add per non-zero bin and workgroup), else a few rounds of
// a wave-level combine of equal ids and one global add per group.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_types.h"
#include "kernels.h"

namespace spm_amd {
namespace {

constexpr uint32_t kQuietNaN = 0x7FC00000u;  // std::numeric_limits<float>::quiet_NaN()
constexpr int kRetagThreads = 256;

// One thread per trie unit.  A leaf of a NORMAL / UNUSED piece gets its new
// kind bits and, in the (unit, score) table, the piece's score or NaN;
// USER_DEFINED leaves never change.
__global__ __launch_bounds__(kRetagThreads) void vocab_retag_unigram_kernel(
    const uint32_t *__restrict__ units, int32_t *__restrict__ values, uint32_t *__restrict__ uvs,
    const float *__restrict__ scores, const uint8_t *__restrict__ kind, uint32_t num_units, uint32_t num_pieces) {
  const uint32_t u = blockIdx.x * kRetagThreads + threadIdx.x;
  if (u >= num_units) return;
  if (((units[u] >> 8) & 1u) == 0) return;  // DoubleArray::Leaf
  const int32_t v = values[u];
  if (v < 0) return;
  const uint32_t id = static_cast<uint32_t>(v & kIdMask);
  if ((v >> kKindShift) == kKindUserDefined || id >= num_pieces) return;
  const uint32_t k = kind[id];
  if (k == static_cast<uint32_t>(kKindUserDefined)) return;
  values[u] = static_cast<int32_t>(id | (k << kKindShift));
  if (uvs) uvs[2 * static_cast<uint64_t>(u) + 1] = k == 0 ? __float_as_uint(scores[id]) : kQuietNaN;
}

// One thread per pair slot: the unused bit of the merged piece.
__global__ __launch_bounds__(kRetagThreads) void vocab_retag_bpe_kernel(uint4 *__restrict__ ent, uint64_t slots,
                                                                        const uint8_t *__restrict__ kind,
                                                                        uint32_t num_pieces) {
  const uint64_t h = static_cast<uint64_t>(blockIdx.x) * kRetagThreads + threadIdx.x;
  if (h >= slots) return;
  const uint4 e = ent[h];
  if (e.x == 0xFFFFFFFFu && e.y == 0xFFFFFFFFu) return;  // empty slot
  const uint32_t id = e.z & 0x7FFFFFFFu;
  if (id >= num_pieces) return;
  reinterpret_cast<uint32_t *>(ent + h)[2] = id | (kind[id] == kKindUnused ? 0x80000000u : 0u);
}

constexpr int kCountThreads = 1024;
constexpr int kCountPerThread = kCountTile / kCountThreads;
static_assert(kCountTile % kCountThreads == 0, "a tile is a whole number of block passes");

// LDS bins.  A wave whose valid lanes all hold one id adds their number once
// (a stream of one id would otherwise serialize 64 LDS adds per instruction).
__global__ __launch_bounds__(kCountThreads) void vocab_count_lds_kernel(const int32_t *__restrict__ ids, uint64_t n,
                                                                        unsigned long long *__restrict__ counts,
                                                                        uint32_t num_pieces,
                                                                        uint32_t *__restrict__ status) {
  extern __shared__ uint32_t bins[];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  for (uint32_t b = tid; b < num_pieces; b += kCountThreads) bins[b] = 0;
  __syncthreads();
  bool bad = false;
  const uint64_t tiles = (n + kCountTile - 1) / kCountTile;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t base = t * kCountTile;
#pragma unroll
    for (int k = 0; k < kCountPerThread; ++k) {
      const uint64_t i = base + static_cast<uint64_t>(k) * kCountThreads + tid;
      const int32_t id = i < n ? ids[i] : -1;
      const bool valid = static_cast<uint32_t>(id) < num_pieces;
      bad |= i < n && !valid;
      const uint64_t vm = __ballot(valid);
      if (vm == 0) continue;
      const int src = __ffsll(static_cast<long long>(vm)) - 1;
      const int32_t lead = __shfl(id, src);
      const uint64_t same = __ballot(valid && id == lead);
      if (same == vm) {
        if (lane == static_cast<uint32_t>(src)) atomicAdd(&bins[lead], static_cast<uint32_t>(__popcll(same)));
      } else if (valid) {
        atomicAdd(&bins[id], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t b = tid; b < num_pieces; b += kCountThreads) {
    const uint32_t c = bins[b];
    if (c) atomicAdd(&counts[b], static_cast<unsigned long long>(c));
  }
  if (bad) atomicOr(status, 1u);
}

// No bins: kCombineRounds times the first live lane's id is summed over the
// wave and added once (the few hot ids of a Zipfian stream), then every lane
// still live adds its own.
constexpr int kCombineRounds = 4;
__global__ __launch_bounds__(256) void vocab_count_wave_kernel(const int32_t *__restrict__ ids, uint64_t n,
                                                               unsigned long long *__restrict__ counts,
                                                               uint32_t num_pieces, uint32_t *__restrict__ status) {
  const uint32_t lane = threadIdx.x & 63u;
  bool bad = false;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  const uint64_t rounds = (n + stride - 1) / stride;  // the same trip count in every lane
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t i = r * stride + static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int32_t id = i < n ? ids[i] : -1;
    bool live = static_cast<uint32_t>(id) < num_pieces;
    bad |= i < n && !live;
    for (int c = 0; c < kCombineRounds; ++c) {
      const uint64_t lm = __ballot(live);
      if (lm == 0) break;
      const int src = __ffsll(static_cast<long long>(lm)) - 1;
      const int32_t lead = __shfl(id, src);
      const bool mine = live && id == lead;
      const uint64_t same = __ballot(mine);
      if (lane == static_cast<uint32_t>(src))
        atomicAdd(&counts[lead], static_cast<unsigned long long>(__popcll(same)));
      if (mine) live = false;
    }
    if (live) atomicAdd(&counts[id], 1ull);
  }
  if (bad) atomicOr(status, 1u);
}

}  // namespace

hipError_t LaunchVocabRetagUnigram(const uint32_t *units, int32_t *values, uint32_t *uvs, const float *scores,
                                   const uint8_t *kind, uint32_t num_units, uint32_t num_pieces, hipStream_t st) {
  if (num_units == 0) return hipSuccess;
  const unsigned grid = (num_units + kRetagThreads - 1) / kRetagThreads;
  hipLaunchKernelGGL(vocab_retag_unigram_kernel, dim3(grid), dim3(kRetagThreads), 0, st, units, values, uvs, scores,
                     kind, num_units, num_pieces);
  return hipGetLastError();
}

hipError_t LaunchVocabRetagBpe(void *pair_ent, uint64_t slots, const uint8_t *kind, uint32_t num_pieces,
                               hipStream_t st) {
  if (slots == 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((slots + kRetagThreads - 1) / kRetagThreads);
  hipLaunchKernelGGL(vocab_retag_bpe_kernel, dim3(grid), dim3(kRetagThreads), 0, st, static_cast<uint4 *>(pair_ent),
                     slots, kind, num_pieces);
  return hipGetLastError();
}

hipError_t LaunchVocabCount(const int32_t *ids, uint64_t n, uint64_t *counts, uint32_t num_pieces, uint32_t *status,
                            hipStream_t st) {
  if (n == 0 || num_pieces == 0) return hipSuccess;
  static const int kCus = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    return cus;
  }();
  auto *c = reinterpret_cast<unsigned long long *>(counts);
  if (num_pieces <= kCountLdsMaxPieces) {
    // 4 B per bin: up to 128 KiB of the CU's 160 KiB, so one workgroup of 16
    // waves per CU at the largest vocabulary and two from 64 KiB down.
    const size_t lds = static_cast<size_t>(num_pieces) * 4;
    static const hipError_t kAttr =
        hipFuncSetAttribute(reinterpret_cast<const void *>(vocab_count_lds_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kCountLdsMaxPieces * 4);
    if (kAttr != hipSuccess) return kAttr;
    const uint64_t tiles = (n + kCountTile - 1) / kCountTile;
    const uint64_t per_cu = lds <= (64u << 10) ? 2 : 1;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(tiles, per_cu * kCus));
    hipLaunchKernelGGL(vocab_count_lds_kernel, dim3(grid), dim3(kCountThreads), lds, st, ids, n, c, num_pieces,
                       status);
  } else {
    const uint64_t blocks = (n + 255) / 256;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(blocks, 8ull * kCus));
    hipLaunchKernelGGL(vocab_count_wave_kernel, dim3(grid), dim3(256), 0, st, ids, n, c, num_pieces, status);
  }
  return hipGetLastError();
}

}  // namespace spm_amd
