// Device-side pieces the BPE encode kernels share (bpe_kernels.hip: the batch
// tiers, bpe_line.hip: one wave per line): the kernels' model tables, the
// exact-match walk of the symbol trie, the fused pair probe and the wave
// maximum over score keys.  Every definition is local to the including file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sample_rng.h"

namespace spm_amd {
namespace {

__device__ __forceinline__ uint32_t OneCharLenB(uint32_t lead) {
  return (0x4322111111111111ull >> ((lead >> 4) * 4)) & 0xFu;
}

// Hash of a (left id << 32 | right id) pair key: 32-bit multiplies only (the
// fast kernel computes it once per merge; 64-bit multiplies cost ~4x the VALU
// issue).  Linear probing at load factor <= 0.5.
__host__ __device__ __forceinline__ uint32_t PairHash(uint64_t k) {
  uint32_t h = static_cast<uint32_t>(k >> 32) * 0x9E3779B1u ^ static_cast<uint32_t>(k) * 0x85EBCA77u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}

struct BpeArgs {
  const uint8_t *__restrict__ bytes;
  const uint64_t *__restrict__ off;
  uint64_t n;
  const uint32_t *__restrict__ units;
  const int32_t *__restrict__ values;     // entry index
  const int32_t *__restrict__ entry_piece;
  const int32_t *__restrict__ entry_out;
  const float *__restrict__ scores;       // per piece id
  const uint8_t *__restrict__ piece_kind;
  const int32_t *__restrict__ piece_out;
  const uint64_t *__restrict__ pair_keys;
  const int32_t *__restrict__ pair_vals;
  const uint4 *__restrict__ pair_ent;     // fused: key, merged id | unused bit, score
  uint64_t pair_mask;
  uint32_t root_base;
  int32_t unk_id;
  int32_t irregular;
  int32_t *__restrict__ slot_ids;
  uint32_t *__restrict__ slot_len;
  uint32_t *__restrict__ ntok;
  uint32_t *__restrict__ flagged;
  uint32_t *__restrict__ status;
  uint64_t capacity;                      // caller's bound on off[n]
  const uint32_t *__restrict__ chain;     // asynchronous chain status (nullable)
  const int16_t *__restrict__ rank_piece; // unique score ranks: rank -> merged piece (lane kernel)
  int32_t rank_base;                      // >= 0: merged piece = rank_base - rank (BpeDevice::rank_base)
  int32_t pipe_probes;                    // lane kernel: new pairs' probes in flight across the next scan
  // bpe_lane_kernel's tile-dense output (lane_ids[off[tile base] + k] for
  // the tile's k-th token in sentence order; lane_len alongside, nullable).
  int32_t *__restrict__ lane_ids;
  uint32_t *__restrict__ lane_len;
};

// Exact-match walk of s[0:len) in the string trie; returns entry or -1.
__device__ __forceinline__ int32_t ExactEntry(const BpeArgs &a, const uint8_t *s, uint32_t len) {
  uint32_t base = a.root_base, node = 0, u = 0;
  for (uint32_t j = 0; j < len; ++j) {
    const uint32_t c = s[j];
    if (c == 0) return -1;
    node = base ^ c;
    u = a.units[node];
    if ((u & 0xFFu) != c) return -1;
    base = u >> 9;
  }
  return (len && (u & 0x100u)) ? a.values[node] : -1;
}

// Hands sentence i (nb bytes) to the general kernel: status[0] counts the
// flagged sentences, status[1] keeps the longest.
__device__ __forceinline__ void FlagSentence(const BpeArgs &a, uint64_t i, uint32_t nb) {
  a.ntok[i] = 0xFFFFFFFFu;
  const uint32_t k = atomicAdd(&a.status[0], 1u);
  a.flagged[k] = static_cast<uint32_t>(i);
  atomicMax(&a.status[1], nb);
}

// One 16-byte load per probe returns the merged id, its score and whether it
// is UNUSED (the fast kernel's per-merge dependent chain is this load alone).
__device__ __forceinline__ int32_t PairLookupFused(const BpeArgs &a, int32_t l, int32_t r, uint32_t *rank,
                                                   bool *unused) {
  if (l < 0 || r < 0) return -1;
  const uint64_t key = (static_cast<uint64_t>(static_cast<uint32_t>(l)) << 32) | static_cast<uint32_t>(r);
  const uint32_t mask = static_cast<uint32_t>(a.pair_mask);  // table < 2^32 entries
  uint32_t h = PairHash(key) & mask;
  for (;;) {
    const uint4 e = a.pair_ent[h];
    if (e.x == static_cast<uint32_t>(r) && e.y == static_cast<uint32_t>(l)) {
      *rank = e.w;
      *unused = (e.z >> 31) != 0;
      return static_cast<int32_t>(e.z & 0x7FFFFFFFu);
    }
    if (e.x == 0xFFFFFFFFu && e.y == 0xFFFFFFFFu) return -1;
    h = (h + 1) & mask;
  }
}

// BPE-dropout of one sentence: its key in the sampler's counter-based stream
// (SampleKey(seed, global index)) and the integer threshold ceil(alpha * 2^53).
struct BpeDropKey {
  uint64_t key, threshold;
};

// The pair named (start, end) is dropped: SampleDraw(key, start << 32 | end)
// < alpha, as an integer compare (the draw is (mix >> 11) * 2^-53).
__device__ __forceinline__ bool BpeDropped(const BpeDropKey &d, uint32_t start, uint32_t end) {
  const uint64_t k = (static_cast<uint64_t>(start) << 32) | end;
  return (SampleMix(d.key + kSampleGolden * (k + 1)) >> 11) < d.threshold;
}

// Pair keys: the entry's w word is the merged piece's score as a dense rank
// (BpeScoreRanks, host side): equal scores share a rank, a higher score has a
// higher rank, 0 = no pair — the same order as the scores themselves, in 16
// bits for vocabularies under 32768 pieces.
// Wave-wide max of a key (all 64 lanes active): DPP within each 16-lane row
// (quad perms, half-row and row mirrors — VALU, no LDS round trip), then the
// four row maxima through v_readlane.
__device__ __forceinline__ uint32_t WaveMaxU(uint32_t v) {
  v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(v), static_cast<int>(v), 0xB1, 0xF, 0xF, false)));
  v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(v), static_cast<int>(v), 0x4E, 0xF, 0xF, false)));
  v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(v), static_cast<int>(v), 0x141, 0xF, 0xF, false)));
  v = max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(v), static_cast<int>(v), 0x140, 0xF, 0xF, false)));
  const uint32_t r0 = __builtin_amdgcn_readlane(static_cast<int>(v), 0);
  const uint32_t r1 = __builtin_amdgcn_readlane(static_cast<int>(v), 16);
  const uint32_t r2 = __builtin_amdgcn_readlane(static_cast<int>(v), 32);
  const uint32_t r3 = __builtin_amdgcn_readlane(static_cast<int>(v), 48);
  return max(max(r0, r1), max(r2, r3));
}

}  // namespace
}  // namespace spm_amd
