// Dense id batches, window: a sentence longer than a row as several rows of
// row_len that overlap by a stride (sliding-window perplexity, embedding or QA
// over long passages).  Internal; the public entries are spm_hip_window_ids
// and spm_hip_window_ids_host.  The rule of one sentence and of one output
// slot is stated once here and runs in the kernels of dense_window.hip and in
// the host loop below alike.
//
//   h, t = 1 with SPM_WINDOW_KEEP_FIRST / SPM_WINDOW_KEEP_LAST, else 0.
//   C = L - h - t is the payload of a row, step = C - S; C >= 1, 0 <= S < C.
//   A sentence of len <= h + t tokens is one row that holds them as they are.
//   Otherwise its body is tokens [h, len - t), m = len - h - t of them: one
//   row if m <= C, else 1 + ceil((m - C) / step).  Row w holds token 0 if h,
//   body tokens [w * step, min(w * step + C, m)), token len - 1 if t, then
//   pads.  The rows of sentence i follow those of sentence i - 1.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/spm_hip.h"

namespace spm_amd {

constexpr uint32_t kWindowFlagMask = SPM_WINDOW_KEEP_FIRST | SPM_WINDOW_KEEP_LAST;

struct WindowGeom {
  uint32_t L, h, t, C, S, step;
};

// C >= 1 and 0 <= S < C, else false.
inline bool WindowGeomFor(uint32_t L, uint32_t S, uint32_t flags, WindowGeom *g) {
  g->L = L;
  g->h = (flags & SPM_WINDOW_KEEP_FIRST) ? 1 : 0;
  g->t = (flags & SPM_WINDOW_KEEP_LAST) ? 1 : 0;
  if (L < g->h + g->t + 1) return false;
  g->C = L - g->h - g->t;
  if (S >= g->C) return false;
  g->S = S;
  g->step = g->C - S;
  return true;
}

// Rows of a sentence of len tokens, >= 1.
__host__ __device__ inline uint64_t WindowRows(uint64_t len, const WindowGeom &g) {
  if (len <= g.h + g.t + g.C) return 1;
  const uint64_t over = len - g.h - g.t - g.C + g.step - 1;  // (m - C) rounded up to a step
  // Sentences of 2^32 tokens are rare: the 32-bit quotient is the cheap one on the device.
  return 1 + ((over >> 32) ? over / g.step : static_cast<uint32_t>(over) / g.step);
}

// Whether row w is the last row of its sentence.
__host__ __device__ inline bool WindowLastRow(uint64_t len, uint64_t w, const WindowGeom &g) {
  return len <= g.h + g.t + g.C || w * g.step + g.C >= len - g.h - g.t;
}

// Column c of row w of a sentence of len tokens: the token it holds (-1: a
// pad) and whether no earlier row carries that token.  A later row repeats the
// head and tail tokens and the S body tokens it shares with the row before.
struct WindowSlot {
  int64_t src;
  bool fresh;
};
__host__ __device__ inline WindowSlot WindowSlotSource(uint64_t len, uint64_t w, uint32_t c, const WindowGeom &g) {
  if (len <= g.h + g.t) return WindowSlot{c < len ? static_cast<int64_t>(c) : -1, c < len};
  if (c < g.h) return WindowSlot{0, w == 0};
  const uint64_t m = len - g.h - g.t, b0 = w * g.step;
  const uint64_t cnt = m - b0 < g.C ? m - b0 : g.C;  // body tokens of the row, >= S + 1
  const uint32_t j = c - g.h;
  if (j < cnt) return WindowSlot{static_cast<int64_t>(g.h + b0 + j), w == 0 || j >= g.S};
  if (g.t && j == cnt) return WindowSlot{static_cast<int64_t>(len - 1), w == 0};
  return WindowSlot{-1, false};
}

// Count-and-scan: sentences of one tile (256 threads, 8 rounds) and the
// scratch of a call: {ticket, -} | one look-back word per tile | n + 1 words
// that stand in for a null d_first_row.
constexpr uint32_t kWindowScanTile = 2048;
// Fill: output slots a block fills at a time (a multiple of kDenseTile) and
// the sentences of such a chunk whose first rows fit into LDS.
constexpr uint32_t kWindowChunk = 8192;
constexpr uint32_t kWindowSeg = 2048;
constexpr uint32_t kWindowMaxBlocks = 1u << 18;

struct WindowPlan {
  uint64_t tiles;
  size_t desc, first_row, bytes;
};
inline WindowPlan WindowPlanFor(uint64_t n) {
  WindowPlan p{};
  if (n == 0) return p;
  p.tiles = (n + kWindowScanTile - 1) / kWindowScanTile;
  p.desc = 16;
  p.first_row = p.desc + static_cast<size_t>((p.tiles * 8 + 15) / 16 * 16);
  p.bytes = p.first_row + static_cast<size_t>(((n + 1) * 8 + 15) / 16 * 16);
  return p;
}

// Enqueue on st; every output but out may be null.  scratch as WindowPlanFor
// lays it out (16-byte aligned; null for n == 0).
hipError_t LaunchDenseWindow(const int32_t *ids, const uint64_t *off, uint64_t n, const WindowGeom &g, int32_t pad_id,
                             uint64_t rows_cap, int32_t *out, int32_t *pos, uint8_t *fresh, int32_t *lengths,
                             int32_t *row_sentence, uint64_t *first_row, uint64_t *stats, void *scratch,
                             hipStream_t st);

// The same results as a plain loop over host buffers.
inline void DenseWindowHostLoop(const int32_t *ids, const uint64_t *off, uint64_t n, const WindowGeom &g,
                                int32_t pad_id, uint64_t rows_cap, int32_t *out, int32_t *pos, uint8_t *fresh,
                                int32_t *lengths, int32_t *row_sentence, uint64_t *first_row, uint64_t *stats) {
  uint64_t row = 0, multi = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t len = off[i + 1] - off[i], r = WindowRows(len, g);
    if (first_row) first_row[i] = row;
    multi += r > 1;
    for (uint64_t w = 0; w < r && row + w < rows_cap; ++w) {
      int32_t used = 0;
      for (uint32_t c = 0; c < g.L; ++c) {
        const WindowSlot s = WindowSlotSource(len, w, c, g);
        const uint64_t t = (row + w) * g.L + c;
        out[t] = s.src >= 0 ? ids[off[i] + s.src] : pad_id;
        if (pos) pos[t] = s.src >= 0 ? static_cast<int32_t>(s.src) : 0;
        if (fresh) fresh[t] = s.fresh;
        used += s.src >= 0;
      }
      if (lengths) lengths[row + w] = used;
      if (row_sentence) row_sentence[row + w] = static_cast<int32_t>(i);
    }
    row += r;
  }
  if (first_row) first_row[n] = row;
  if (stats) {
    stats[0] = row;
    stats[1] = multi;
  }
}

}  // namespace spm_amd
