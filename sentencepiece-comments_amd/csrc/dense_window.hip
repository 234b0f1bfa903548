// Dense id batches, window: long sentences as overlapping rows of [rows, L]
// int32 (the rule of dense_window.h).  Where a sentence's rows start depends on
// the rows of every sentence before it, so the call is a count-and-scan over
// the sentences and a fill over the output slots.  State lives in the caller's
// scratch (WindowPlan); no result depends on the launch geometry.
//
//   init : the scratch is the caller's and undefined: a small kernel clears
//          the ticket, the look-back words and the second stats word.
//   scan : one launch over tiles of kWindowScanTile sentences.  A thread takes
//          8 sentences, 256 apart (coalesced offset loads), computes their row
//          counts r_i and scans each round in its wave; the 32 wave totals
//          meet in LDS behind one barrier.  The tile's exclusive prefix comes
//          from a decoupled look-back (lookback.h, tiles in ticket order), and
//          first_row[i + 1] is stored from registers: the offsets are read
//          once.  The tile that holds the last sentence stores R; the
//          sentences with more than one row are summed per block and added
//          with one atomic.
//   fill : laid out over the output slots as dense_pad_kernel is: a thread
//          owns 4 consecutive slots, a block a chunk of kWindowChunk
//          consecutive slots, that is a contiguous run of rows (the first and
//          last possibly shared with its neighbours).  Wave 0 finds the
//          sentences of the chunk's first and last row in first_row with a
//          64-way search: one pivot per lane, a ballot, and the range narrows
//          to one 64th per round of dependent loads.  If those sentences
//          number at most kWindowSeg, their first rows, relative to the
//          chunk's first row, are staged in LDS (8 KiB) and a thread resolves
//          the row of its quad there; else (L < 4 with one-row sentences) it
//          searches first_row between the two sentences in global memory.  A
//          thread searches once per quad: where the column wraps it steps to
//          the sentence's next row or to the next sentence, which the rule
//          tells apart without a division.  One document that fills many
//          blocks is a segment of one sentence.  The slot at column 0 writes
//          the row's length and sentence.  Source ids are read by dword at
//          any alignment; the S / C of them that two rows share come from L2.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense.h"
#include "dense_window.h"
#include "lookback.h"
#include "token_tiles.h"

namespace spm_amd {
namespace {

constexpr uint32_t kScanRounds = kWindowScanTile / 256;

__global__ __launch_bounds__(256) void window_init_kernel(uint32_t *__restrict__ ctl, uint64_t *__restrict__ desc,
                                                          uint64_t tiles, uint64_t *__restrict__ first_row,
                                                          uint64_t *__restrict__ stats) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (uint64_t i = tid; i < tiles; i += stride) desc[i] = 0;
  if (tid == 0) {
    if (ctl) ctl[0] = 0;
    if (first_row) first_row[0] = 0;
    if (stats) stats[0] = stats[1] = 0;
  }
}

__global__ __launch_bounds__(256) void window_scan_kernel(const uint64_t *__restrict__ off, uint64_t n, WindowGeom g,
                                                          uint32_t *__restrict__ ctl, uint64_t *__restrict__ desc,
                                                          uint64_t *__restrict__ first_row,
                                                          uint64_t *__restrict__ stats) {
  __shared__ uint32_t s_tile;
  __shared__ uint64_t s_tot[kScanRounds][4];
  __shared__ uint64_t s_w[4];
  __shared__ uint64_t s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_tile = atomicAdd(ctl, 1u);
  __syncthreads();
  const uint64_t tile = s_tile, lo = tile * kWindowScanTile;
  uint64_t inc[kScanRounds];  // inclusive over the wave's 64 sentences of round k
  uint64_t multi = 0;
#pragma unroll
  for (uint32_t k = 0; k < kScanRounds; ++k) {
    const uint64_t i = lo + k * 256u + tid;
    uint64_t x = 0;
    if (i < n) {
      x = WindowRows(off[i + 1] - off[i], g);
      multi += x > 1;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t ylo = __shfl_up(static_cast<uint32_t>(x), o);
      const uint32_t yhi = __shfl_up(static_cast<uint32_t>(x >> 32), o);
      if (lane >= o) x += (static_cast<uint64_t>(yhi) << 32) | ylo;
    }
    inc[k] = x;
    if (lane == 63) s_tot[k][wave] = x;
  }
  __syncthreads();
  uint64_t base[kScanRounds], total = 0;  // rows of the tile before the wave's sentences of round k
#pragma unroll
  for (uint32_t k = 0; k < kScanRounds; ++k) {
    base[k] = total;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint64_t v = s_tot[k][w];
      if (w < wave) base[k] += v;
      total += v;
    }
  }
  if (stats) {  // uniform
    multi = BlockSum64(multi, s_w);
    if (tid == 0 && multi)
      atomicAdd(reinterpret_cast<unsigned long long *>(stats + 1), static_cast<unsigned long long>(multi));
  }
  if (wave == 0) {
    const uint64_t pre = LookbackExclusive(desc, tile, total, lane);
    if (lane == 0) s_carry = pre;
  }
  __syncthreads();
  const uint64_t carry = s_carry;
#pragma unroll
  for (uint32_t k = 0; k < kScanRounds; ++k) {
    const uint64_t i = lo + k * 256u + tid;
    if (i < n) first_row[i + 1] = carry + base[k] + inc[k];
  }
  if (stats && tid == 0 && lo + kWindowScanTile >= n) stats[0] = carry + total;
}

// The largest i in [a, b) with fr[i] <= row, given fr[a] <= row and fr
// ascending.  All 64 lanes of one wave; the result is uniform.
__device__ __forceinline__ uint64_t WaveFindSentence(const uint64_t *__restrict__ fr, uint64_t a, uint64_t b,
                                                     uint64_t row, int lane) {
  for (;;) {
    const uint64_t step = (b - a + 63) / 64;
    const uint64_t p = a + lane * step;
    const bool le = p < b && fr[p] <= row;  // true on lane 0, and on a prefix of the lanes
    a += (__popcll(__builtin_amdgcn_ballot_w64(le)) - 1) * step;
    if (step == 1) return a;
    if (a + step < b) b = a + step;
  }
}

struct WindowOut {
  int32_t *out, *pos;
  uint8_t *fresh;
  int32_t *lengths, *row_sentence;
  bool vec_out, vec_pos, vec_fresh;
};

__global__ __launch_bounds__(256) void window_fill_kernel(const int32_t *__restrict__ ids,
                                                          const uint64_t *__restrict__ off, uint64_t n, WindowGeom g,
                                                          int32_t pad_id, uint64_t rows_cap,
                                                          const uint64_t *__restrict__ fr, WindowOut o,
                                                          uint32_t stride_rows, uint32_t stride_cols) {
  __shared__ uint32_t s_seg[kWindowSeg];  // first_row[s_lo + k] - row_lo; s_seg[0] stands for 0
  __shared__ uint64_t s_edge[3];          // the chunk's first and last sentence, first_row of the first
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t L = g.L;
  const uint64_t need = fr[n];
  const uint64_t total = (need < rows_cap ? need : rows_cap) * L;
  for (uint64_t chunk = blockIdx.x;; chunk += gridDim.x) {
    const uint64_t begin = chunk * kWindowChunk;
    if (begin >= total) break;  // uniform
    const uint64_t end = total - begin < kWindowChunk ? total : begin + kWindowChunk;
    const uint64_t row_lo = begin / L, row_hi = (end - 1) / L;
    __syncthreads();  // the previous chunk's segment is consumed
    if (tid < 64) {
      const uint64_t a = WaveFindSentence(fr, 0, n, row_lo, lane);
      const uint64_t b = WaveFindSentence(fr, a, n, row_hi, lane);
      if (lane == 0) {
        s_edge[0] = a;
        s_edge[1] = b;
        s_edge[2] = fr[a];
      }
    }
    __syncthreads();
    const uint64_t s_lo = s_edge[0], s_hi = s_edge[1], fr_lo = s_edge[2];
    const uint32_t nseg = s_hi - s_lo < kWindowSeg ? static_cast<uint32_t>(s_hi - s_lo) + 1 : 0;  // 0: not staged
    if (nseg) {  // uniform
      for (uint32_t k = tid; k < nseg; k += 256) s_seg[k] = k ? static_cast<uint32_t>(fr[s_lo + k] - row_lo) : 0u;
      __syncthreads();
    }
    uint64_t row = row_lo + (tid * 4u) / L;  // begin = row_lo * L + col0, col0 < L
    uint64_t col64 = begin - row_lo * L + (tid * 4u) % L;
    if (col64 >= L) {
      col64 -= L;
      ++row;
    }
    uint32_t col = static_cast<uint32_t>(col64);
    for (uint64_t t = begin + tid * 4u; t < end; t += kDenseTile) {
      const uint32_t cnt = end - t < 4 ? static_cast<uint32_t>(end - t) : 4u;
      // The sentence of `row` and the row's index in it.
      uint64_t s, first;
      if (nseg) {
        const uint32_t rel = static_cast<uint32_t>(row - row_lo);
        uint32_t a = 0, b = nseg;
        while (b - a > 1) {
          const uint32_t mid = (a + b) / 2;
          if (s_seg[mid] <= rel) a = mid;
          else b = mid;
        }
        s = s_lo + a;
        first = a ? row_lo + s_seg[a] : fr_lo;
      } else {
        uint64_t a = s_lo, b = s_hi + 1;
        while (b - a > 1) {
          const uint64_t mid = a + (b - a) / 2;
          if (fr[mid] <= row) a = mid;
          else b = mid;
        }
        s = a;
        first = fr[a];
      }
      uint64_t r = row, w = row - first;
      uint32_t c = col;
      uint64_t base = off[s], len = off[s + 1] - base;
      int32_t id[4] = {pad_id, pad_id, pad_id, pad_id}, ps[4] = {0, 0, 0, 0};
      uint32_t fm = 0;
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        if (j < cnt) {
          const WindowSlot sl = WindowSlotSource(len, w, c, g);
          if (sl.src >= 0) {
            id[j] = ids[base + sl.src];
            ps[j] = static_cast<int32_t>(sl.src);
            if (sl.fresh) fm |= 1u << (8 * j);
          }
          if (c == 0) {
            if (o.row_sentence) o.row_sentence[r] = static_cast<int32_t>(s);
            if (o.lengths) {
              const uint64_t m = len > g.h + g.t ? len - g.h - g.t - w * g.step : 0;  // body tokens from this row on
              o.lengths[r] = static_cast<int32_t>(len <= g.h + g.t ? len : g.h + g.t + (m < g.C ? m : g.C));
            }
          }
          if (++c == L && j + 1 < cnt) {
            c = 0;
            ++r;
            if (WindowLastRow(len, w, g)) {  // every sentence has a row: the next one follows
              ++s;
              w = 0;
              base = off[s];
              len = off[s + 1] - base;
            } else {
              ++w;
            }
          }
        }
      }
      StoreQuad(o.out, t, id, cnt, o.vec_out);
      if (o.pos) StoreQuad(o.pos, t, ps, cnt, o.vec_pos);
      if (o.fresh) {
        if (o.vec_fresh && cnt == 4) {
          *reinterpret_cast<uint32_t *>(o.fresh + t) = fm;
        } else {
          for (uint32_t j = 0; j < cnt; ++j) o.fresh[t + j] = static_cast<uint8_t>(fm >> (8 * j));
        }
      }
      row += stride_rows;
      col += stride_cols;  // < 2 * L
      if (col >= L) {
        col -= L;
        ++row;
      }
    }
  }
}

bool Aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

hipError_t LaunchDenseWindow(const int32_t *ids, const uint64_t *off, uint64_t n, const WindowGeom &g, int32_t pad_id,
                             uint64_t rows_cap, int32_t *out, int32_t *pos, uint8_t *fresh, int32_t *lengths,
                             int32_t *row_sentence, uint64_t *first_row, uint64_t *stats, void *scratch,
                             hipStream_t st) {
  const WindowPlan plan = WindowPlanFor(n);
  char *base = static_cast<char *>(scratch);
  uint32_t *ctl = n ? reinterpret_cast<uint32_t *>(base) : nullptr;
  uint64_t *desc = n ? reinterpret_cast<uint64_t *>(base + plan.desc) : nullptr;
  if (!first_row && n) first_row = reinterpret_cast<uint64_t *>(base + plan.first_row);
  const uint64_t init_blocks = (plan.tiles + 255) / 256;
  hipLaunchKernelGGL(window_init_kernel, dim3(static_cast<unsigned>(init_blocks ? init_blocks : 1)), dim3(256), 0, st,
                     ctl, desc, plan.tiles, first_row, stats);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n == 0) return e;
  hipLaunchKernelGGL(window_scan_kernel, dim3(static_cast<unsigned>(plan.tiles)), dim3(256), 0, st, off, n, g, ctl,
                     desc, first_row, stats);
  if ((e = hipGetLastError()) != hipSuccess || rows_cap == 0) return e;
  // The row count is on the device only: the grid covers the capacity, and a
  // block whose chunks lie past the rows needed does nothing.
  const uint64_t chunks = rows_cap * g.L / kWindowChunk + 1;  // rows_cap * L fits: the entry clamps
  const WindowOut o{out, pos, fresh, lengths, row_sentence, Aligned(out, 16), Aligned(pos, 16), Aligned(fresh, 4)};
  hipLaunchKernelGGL(window_fill_kernel, dim3(static_cast<unsigned>(chunks < kWindowMaxBlocks ? chunks : kWindowMaxBlocks)),
                     dim3(256), 0, st, ids, off, n, g, pad_id, rows_cap, first_row, o, kDenseTile / g.L,
                     kDenseTile % g.L);
  return hipGetLastError();
}

}  // namespace spm_amd
