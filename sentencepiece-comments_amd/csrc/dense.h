// Dense id batches: a final id CSR (ids, offsets[n+1]; the offsets index ids
// and need not start at 0) as a rectangle of row_len int32 per row.  Internal;
// the public entries are spm_hip_pad_ids / spm_hip_pack_ids and their _host
// siblings.  The rule of one output slot is stated once here and runs in the
// kernels of dense_kernels.hip and in the host loops below alike.
//
//   pad : one sentence per row; a sentence longer than the row is cut.
//   pack: the sentences' ids run on as one stream, row_len slots per row (the
//         LM-pretraining layout); a sentence may cross a row edge.  Packing
//         whole sentences into rows without splitting them (bin packing) is
//         out of scope.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/spm_hip.h"

namespace spm_amd {

constexpr uint32_t kDenseFlagMask = SPM_DENSE_PAD_LEFT | SPM_DENSE_TRUNCATE_LEFT | SPM_DENSE_KEEP_END;

// Pad: the token of a sentence of `len` tokens that column c of its row holds,
// or -1 for a pad slot.  k = min(len, L) tokens are kept: [0, k), or
// [len - k, len) with TRUNCATE_LEFT; they stand in columns [0, k), or
// [L - k, L) with PAD_LEFT.  KEEP_END, on a sentence that is cut: the outermost
// kept slot on the cut side holds the sentence's outermost token (cut on the
// right: the last kept slot holds token len - 1; cut on the left: the first
// kept slot holds token 0), so a bos / eos of the extra options survives.
__host__ __device__ inline int64_t PadSlotSource(uint64_t len, uint32_t L, uint32_t flags, uint32_t c) {
  const uint64_t k = len < L ? len : L;
  const uint64_t first = (flags & SPM_DENSE_PAD_LEFT) ? L - k : 0;
  if (c < first || c >= first + k) return -1;
  const uint64_t j = c - first;  // kept slot, [0, k)
  const bool left = (flags & SPM_DENSE_TRUNCATE_LEFT) != 0;
  if (len > L && (flags & SPM_DENSE_KEEP_END)) {
    if (left && j == 0) return 0;
    if (!left && j == k - 1) return static_cast<int64_t>(len - 1);
  }
  return static_cast<int64_t>(left ? len - k + j : j);
}

// Pack: what slot t of the stream holds besides its id (ids[offsets[0] + t]):
// the sentence it belongs to and its position there, given that sentence and
// where it starts in the stream.  A slot past the `tokens` of the stream is
// padding: seq -1, pos 0.
struct PackedSlot {
  int32_t seq, pos;
};
__host__ __device__ inline PackedSlot PackSlot(uint64_t t, uint64_t tokens, uint64_t sent, uint64_t sent_start) {
  if (t >= tokens) return PackedSlot{-1, 0};
  return PackedSlot{static_cast<int32_t>(sent), static_cast<int32_t>(t - sent_start)};
}

// Blocks of either kernel and slots a block covers per step (256 threads, 4
// consecutive slots each).
constexpr uint32_t kDenseBlocks = 1024;
constexpr uint32_t kDenseTile = 1024;
// The pack kernel waits on the dependent offset loads of its sentence search:
// twice the blocks, all 8 waves of a SIMD, hide more of them.
constexpr uint32_t kDensePackBlocks = 2048;

// Enqueue on st; every nullable output may be null.  stats (2 words) must be
// zero when the pad kernel starts; the pack kernel stores into it.
hipError_t LaunchDensePad(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                          uint32_t flags, int32_t *out, int32_t *lengths, uint8_t *mask, uint64_t *stats,
                          hipStream_t st);
hipError_t LaunchDensePack(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                           uint64_t rows_cap, int32_t *out, int32_t *seq, int32_t *pos, uint64_t *stats,
                           hipStream_t st);

// The same results as plain loops over host buffers.
inline void DensePadHostLoop(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                             uint32_t flags, int32_t *out, int32_t *lengths, uint8_t *mask, uint64_t *stats) {
  uint64_t cut = 0, dropped = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = off[i + 1] - off[i];
    if (lengths) lengths[i] = static_cast<int32_t>(len < L ? len : L);
    if (len > L) {
      ++cut;
      dropped += len - L;
    }
    for (uint32_t c = 0; c < L; ++c) {
      const int64_t src = PadSlotSource(len, L, flags, c);
      out[i * L + c] = src >= 0 ? ids[off[i] + src] : pad_id;
      if (mask) mask[i * L + c] = src >= 0;
    }
  }
  if (stats) {
    stats[0] = cut;
    stats[1] = dropped;
  }
}

inline void DensePackHostLoop(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                              uint64_t rows_cap, int32_t *out, int32_t *seq, int32_t *pos, uint64_t *stats) {
  const uint64_t base = n ? off[0] : 0, tokens = n ? off[n] - base : 0;
  const uint64_t need = (tokens + L - 1) / L, rows = need < rows_cap ? need : rows_cap;
  uint64_t sent = 0;
  for (uint64_t t = 0; t < rows * L; ++t) {
    while (t < tokens && off[sent + 1] - base <= t) ++sent;  // skips the empty sentences too
    const PackedSlot s = PackSlot(t, tokens, sent, t < tokens ? off[sent] - base : 0);
    out[t] = t < tokens ? ids[base + t] : pad_id;
    if (seq) seq[t] = s.seq;
    if (pos) pos[t] = s.pos;
  }
  if (stats) {
    stats[0] = need;
    stats[1] = tokens;
  }
}

}  // namespace spm_amd
