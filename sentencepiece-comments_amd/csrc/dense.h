// Dense id batches: a final id CSR (ids, offsets[n+1]; the offsets index ids
// and need not start at 0) as a rectangle of row_len int32 per row.  Internal;
// the public entries are spm_hip_pad_ids / spm_hip_pack_ids / spm_hip_fit_ids
// and their _host siblings.  The rule of one output slot is stated once here
// and runs in the kernels of dense_kernels.hip / dense_fit.hip and in the host
// loops below alike.
//
//   pad : one sentence per row; a sentence longer than the row is cut.
//   pack: the sentences' ids run on as one stream, row_len slots per row (the
//         LM-pretraining layout); a sentence may cross a row edge.
//   fit : whole sentences share a row and none is split (in-order next-fit):
//         a sentence that does not fit into what is left of the row opens the
//         next row; one longer than a row is cut to the row.
// The fourth layout, window (a long sentence as rows that overlap by a
// stride), has its rule in dense_window.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
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

// Fit (in-order next-fit).  Sentence i keeps k_i = min(len_i, L) tokens.  With
// (row, used) = (0, 0), the sentences in order: k_i = 0 is skipped and takes
// nothing; else if used + k_i > L then ++row, used = 0; the sentence takes
// columns [used, used + k_i) of row, used += k_i.  Its kept slot j holds the
// token below: the cut rule of pad over the sentence's own k_i columns, no
// PAD_LEFT.  Every other slot of rows [0, R) is padding (seq -1, pos 0);
// R = row + 1 if a token was placed, else 0.
__host__ __device__ inline uint64_t FitSlotSource(uint64_t len, uint32_t L, uint32_t flags, uint32_t j) {
  const uint32_t k = len < L ? static_cast<uint32_t>(len) : L;
  return static_cast<uint64_t>(PadSlotSource(len, k, flags & ~SPM_DENSE_PAD_LEFT, j));
}

// A thread's 4 consecutive output slots at flat index t (a multiple of 4): one
// 16-byte store when the base is 16-byte aligned (vec) and the quad is whole.
__device__ __forceinline__ void StoreQuad(int32_t *__restrict__ p, uint64_t t, const int32_t v[4], uint32_t cnt,
                                          bool vec) {
  if (vec && cnt == 4) {
    *reinterpret_cast<int4 *>(p + t) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
    for (uint32_t j = 0; j < cnt; ++j) p[t + j] = v[j];
  }
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

// ---- fit: the placement passes of dense_fit.hip ----
//
// kFitTile sentences are one level-0 tile (its jump tables live in LDS: 96 KiB
// in fit_tile_kernel, 108 KiB with the row marks in fit_mark_kernel);
// `branch` tiles of a level are one tile of the next; tables are built up to
// the first level with at most `top_walk` tiles, which one thread walks.
constexpr uint32_t kFitTile = 4096;
constexpr uint32_t kFitLift = 12;  // log2(kFitTile): binary-lifting tables of a tile
constexpr uint32_t kFitBranch = 16;
constexpr uint32_t kFitTopWalk = 256;
constexpr uint32_t kFitScanTiles = 1024;  // chunks of the prefix scan
constexpr uint32_t kFitMaxLevels = 20;    // branch >= 2 and n < 2^31
constexpr uint32_t kFitCtlWords = 8;

struct FitGeometry {
  uint32_t branch, top_walk;
};

// Where the passes keep their state in the caller's scratch (byte offsets,
// all multiples of 16), for n >= 1.
struct FitPlan {
  uint32_t levels;                  // jump-table levels, >= 1
  uint64_t tiles[kFitMaxLevels];    // tiles of level l
  uint64_t span[kFitMaxLevels];     // sentences of one tile of level l
  size_t ctl, desc, prefix, next, row_first, jump[kFitMaxLevels], rec[kFitMaxLevels], bytes;
};

inline FitPlan FitPlanFor(uint64_t n, uint64_t rows_cap, FitGeometry g) {
  FitPlan p{};
  auto take = [&p](uint64_t bytes) {
    const size_t at = p.bytes;
    p.bytes += static_cast<size_t>((bytes + 15) / 16 * 16);
    return at;
  };
  p.ctl = take(kFitCtlWords * 8);
  p.desc = take(kFitScanTiles * 8);
  p.prefix = take((n + 1) * 8);
  p.next = take(n * 4);
  p.row_first = take((rows_cap < n ? rows_cap : n) * 4);
  uint64_t span = kFitTile, tiles = (n + span - 1) / span;
  for (;;) {
    const uint32_t l = p.levels++;
    p.tiles[l] = tiles;
    p.span[l] = span;
    p.jump[l] = take(n * 16);
    p.rec[l] = take(tiles * 16);
    if (tiles <= g.top_walk || p.levels == kFitMaxLevels) break;
    span *= g.branch;
    tiles = (n + span - 1) / span;
  }
  return p;
}

// Enqueue on st; n >= 1, scratch as FitPlanFor lays it out (16-byte aligned).
// Every output but out may be null.
hipError_t LaunchDenseFit(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                          uint32_t flags, uint64_t rows_cap, int32_t *out, int32_t *seq, int32_t *pos,
                          int32_t *row_lengths, uint64_t *place, uint64_t *stats, void *scratch, const FitPlan &plan,
                          FitGeometry g, hipStream_t st);
// stats[0..4) = 0 (the n == 0 call).
hipError_t LaunchDenseFitEmpty(uint64_t *stats, hipStream_t st);

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

inline void DenseFitHostLoop(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                             uint32_t flags, uint64_t rows_cap, int32_t *out, int32_t *seq, int32_t *pos,
                             int32_t *row_lengths, uint64_t *place, uint64_t *stats) {
  uint64_t row = 0, used = 0, placed = 0, cut = 0, dropped = 0;
  bool any = false;
  auto close_row = [&]() {  // the pads of the row in progress
    if (row >= rows_cap) return;
    for (uint64_t c = used; c < L; ++c) {
      out[row * L + c] = pad_id;
      if (seq) seq[row * L + c] = -1;
      if (pos) pos[row * L + c] = 0;
    }
    if (row_lengths) row_lengths[row] = static_cast<int32_t>(used);
  };
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = off[i + 1] - off[i], k = len < L ? len : L;
    if (len > L) {
      ++cut;
      dropped += len - L;
    }
    if (k == 0) {
      if (place) place[i] = UINT64_MAX;
      continue;
    }
    if (used + k > L) {
      close_row();
      ++row;
      used = 0;
    }
    any = true;
    if (place) place[i] = row * L + used;
    if (row < rows_cap) {
      for (uint32_t j = 0; j < k; ++j) {
        const uint64_t t = row * L + used + j;
        out[t] = ids[off[i] + FitSlotSource(len, L, flags, j)];
        if (seq) seq[t] = static_cast<int32_t>(i);
        if (pos) pos[t] = static_cast<int32_t>(j);
      }
    }
    used += k;
    placed += k;
  }
  if (any) close_row();
  if (stats) {
    stats[0] = any ? row + 1 : 0;
    stats[1] = placed;
    stats[2] = cut;
    stats[3] = dropped;
  }
}

}  // namespace spm_amd
