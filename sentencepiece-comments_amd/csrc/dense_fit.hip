// Dense id batches, fit: whole sentences share the rows of [rows, L] int32 and
// none is split (the in-order next-fit rule of dense.h).  Unlike pad and pack
// this is no per-slot rule: where row r starts depends on every sentence
// before it.  The placement runs as four passes over the sentences, the fill
// as one pass over the output slots.  State lives in the caller's scratch
// (FitPlan); no atomics but the tile ticket of the scan and the two sums of
// the stats, and no result depends on the launch geometry.
//
//   1 prefix  : P[i] = sum of k_j = min(len_j, L), j < i.  One contiguous
//               chunk per block, chunk offsets by a decoupled look-back
//               (lookback.h); the cut and dropped counts fall out.
//   2 next    : next(i) = the first j > i with P[j + 1] - P[i] > L (else n):
//               the sentence that opens the row after a row that i opens.
//               A gallop and binary search on P per sentence (FindSentence).
//               next is monotone and > i; the row starts are the orbit of the
//               first non-empty sentence.
//     tile    : a block takes kFitTile consecutive sentences, holds next as
//               16-bit tile-local indices in LDS and squares it kFitLift - 1
//               times (binary lifting: 12 tables of 4096 x 2 bytes, 96 KiB of
//               the 160 KiB a gfx950 workgroup has; fit_mark_kernel adds the
//               row marks: 110608 bytes, 108 KiB).  For every sentence as a
//               possible entry a descent through the tables gives the jump
//               {first orbit element past the tile, row starts on the way,
//               last row start in the tile}.
//   3 compose : a tile of level l is `branch` tiles of level l - 1.  One
//               launch per sub-tile index, from the last to the first, over
//               all tiles at once: the jump of a sentence out of its sub-tile
//               either leaves the tile or lands in a later sub-tile whose
//               level-l jumps are final, so every sentence costs one hop per
//               level.  Levels are built until at most top_walk tiles are
//               left.
//     resolve : downwards.  One thread walks the top tiles from the first
//               non-empty sentence; then one thread per tile of level l walks
//               its sub-tiles through the table of level l - 1.  Every tile
//               gets {its entry or none, the rows before it, the sentence
//               that opened the row in progress}.  A tile inside one long row
//               has no entry.
//   4 mark    : the tile rebuilds its lifting tables; thread h finds the
//               h-th row start from the entry by the bits of h, writes the
//               row's first sentence and length; the starts are counted per
//               sentence with BlockExclusiveScan, which numbers the rows and
//               gives every sentence its place.
//   5 fill    : laid out over the output slots exactly as dense_pack_kernel;
//               a slot finds its sentence between its row's first sentence
//               and the next row's, galloping from the previous slot's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense.h"
#include "lookback.h"
#include "token_tiles.h"

namespace spm_amd {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint16_t kOut = 0xFFFFu;
// ctl words.
constexpr int kCtlTicket = 0, kCtlCut = 1, kCtlDropped = 2, kCtlRows = 3;

// Jump of a sentence out of its tile: x = first orbit element past the tile
// (n: none), y = row starts on the way (the sentence itself included), z =
// the last of them.  Record of a tile: x = entry (kNone: no row starts
// here), y = rows before the tile, z = the sentence that opened the row in
// progress at the tile's first sentence (kNone: none).
using Quad = uint4;

// The scratch is the caller's: no memset in the stream, a kernel clears it.
__global__ __launch_bounds__(256) void fit_init_kernel(uint64_t *__restrict__ ctl, uint64_t *__restrict__ desc,
                                                       uint64_t *__restrict__ stats) {
  for (uint32_t i = threadIdx.x; i < kFitScanTiles; i += 256) desc[i] = 0;
  if (threadIdx.x < kFitCtlWords) ctl[threadIdx.x] = 0;
  if (stats && threadIdx.x < 4) stats[threadIdx.x] = 0;
}

__global__ void fit_empty_kernel(uint64_t *__restrict__ stats) {
  if (threadIdx.x < 4) stats[threadIdx.x] = 0;
}

// Pass 1.  The shape of fixup_scan_kernel (compact.hip).
__global__ __launch_bounds__(256) void fit_prefix_kernel(const uint64_t *__restrict__ off, uint64_t n, uint32_t L,
                                                         uint64_t chunk, uint64_t *__restrict__ ctl,
                                                         uint64_t *__restrict__ desc, uint64_t *__restrict__ P) {
  __shared__ uint32_t s_tile;
  __shared__ uint64_t s_w[4];
  __shared__ uint64_t s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_tile = atomicAdd(reinterpret_cast<uint32_t *>(ctl + kCtlTicket), 1u);
  __syncthreads();
  const uint64_t tile = s_tile;
  const uint64_t lo = tile * chunk;
  const uint64_t hi = lo + chunk < n ? lo + chunk : n;
  uint64_t sum = 0, cut = 0, dropped = 0;
  for (uint64_t i = lo + tid; i < hi; i += 256) {
    const uint64_t len = off[i + 1] - off[i];
    sum += len < L ? len : L;
    if (len > L) {
      ++cut;
      dropped += len - L;
    }
  }
  sum = BlockSum64(sum, s_w);
  cut = BlockSum64(cut, s_w);
  dropped = BlockSum64(dropped, s_w);
  if (tid == 0 && cut) {
    atomicAdd(reinterpret_cast<unsigned long long *>(ctl + kCtlCut), static_cast<unsigned long long>(cut));
    atomicAdd(reinterpret_cast<unsigned long long *>(ctl + kCtlDropped), static_cast<unsigned long long>(dropped));
  }
  if (wave == 0) {
    const uint64_t pre = LookbackExclusive(desc, tile, sum, lane);
    if (lane == 0) s_carry = pre;
  }
  __syncthreads();
  uint64_t carry = s_carry;
  if (tile == 0 && tid == 0) P[0] = 0;
  for (uint64_t r = lo; r < hi; r += 256) {
    const uint64_t i = r + tid;
    uint64_t x = 0;
    if (i < hi) {
      const uint64_t len = off[i + 1] - off[i];
      x = len < L ? len : L;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t ylo = __shfl_up(static_cast<uint32_t>(x), o);
      const uint32_t yhi = __shfl_up(static_cast<uint32_t>(x >> 32), o);
      if (lane >= o) x += (static_cast<uint64_t>(yhi) << 32) | ylo;
    }
    __syncthreads();  // s_w of the previous round consumed
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint64_t wpre = 0;
    for (int w = 0; w < wave; ++w) wpre += s_w[w];
    if (i < hi) P[i + 1] = carry + wpre + x;
    carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
  }
}

// Pass 2a.  The largest a in [i + 1, n] with P[a] <= P[i] + L has
// P[a + 1] > P[i] + L (or a == n): a is next(i).  P[i + 1] <= P[i] + L holds
// because k_i <= L.
__global__ __launch_bounds__(256) void fit_next_kernel(const uint64_t *__restrict__ P, uint64_t n, uint32_t L,
                                                       uint32_t *__restrict__ next) {
  const TokView v{nullptr, P, n, 0, 0};  // SentStart(v, a) == P[a]
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride)
    next[i] = static_cast<uint32_t>(FindSentence(v, i + 1, n + 1, P[i] + L));
}

// up[r][x] = the 2^r-th successor of tile-local sentence x, kOut once the
// orbit has left the tile's cnt sentences.  256 threads; ends with a barrier.
__device__ __forceinline__ void BuildLift(uint16_t (*up)[kFitTile], const uint32_t *__restrict__ next, uint64_t t0,
                                          uint32_t cnt) {
  for (uint32_t x = threadIdx.x; x < kFitTile; x += 256) {
    uint16_t v = kOut;
    if (x < cnt) {
      const uint64_t d = next[t0 + x] - t0;
      if (d < cnt) v = static_cast<uint16_t>(d);
    }
    up[0][x] = v;
  }
  for (uint32_t r = 0; r + 1 < kFitLift; ++r) {
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < kFitTile; x += 256) {
      const uint16_t v = up[r][x];
      up[r + 1][x] = v == kOut ? kOut : up[r][v];
    }
  }
  __syncthreads();
}

// Pass 2b.  One block per level-0 tile.
__global__ __launch_bounds__(256) void fit_tile_kernel(const uint32_t *__restrict__ next, uint64_t n,
                                                       Quad *__restrict__ jump) {
  __shared__ uint16_t up[kFitLift][kFitTile];
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kFitTile;
  const uint32_t cnt = n - t0 < kFitTile ? static_cast<uint32_t>(n - t0) : kFitTile;
  BuildLift(up, next, t0, cnt);
  for (uint32_t x = threadIdx.x; x < cnt; x += 256) {
    uint32_t y = x, hops = 0;
#pragma unroll
    for (int r = kFitLift - 1; r >= 0; --r) {
      const uint16_t v = up[r][y];
      if (v != kOut) {
        y = v;
        hops += 1u << r;
      }
    }
    jump[t0 + x] = make_uint4(next[t0 + y], hops + 1, static_cast<uint32_t>(t0 + y), 0u);
  }
}

// Pass 3a, one launch per sub-tile index s of the level being built, from the
// last to the first, each over that sub-tile of every tile at once: the
// jumps of the later sub-tiles are final when this one reads them.  sub =
// sentences of a tile of the level below.  (One block per tile walking its
// sub-tiles between barriers was 2.4 of 3.7 ms on 10 M sentences: a level has
// too few tiles to fill the device.)
__global__ __launch_bounds__(256) void fit_compose_kernel(const Quad *__restrict__ below, Quad *above, uint64_t n,
                                                           uint64_t sub, uint32_t branch, uint32_t s,
                                                           uint64_t tiles) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; k < tiles * sub; k += stride) {
    const uint64_t g = k / sub, g0 = g * sub * branch;
    const uint64_t g1 = g0 + sub * branch < n ? g0 + sub * branch : n;
    const uint64_t i = g0 + s * sub + (k - g * sub);
    if (i >= g1) continue;
    Quad a = below[i];
    if (a.x < g1) {  // lands in a later sub-tile of this tile
      const Quad b = above[a.x];
      a = make_uint4(b.x, a.y + b.y, b.z, 0u);
    }
    above[i] = a;
  }
}

// Pass 3b.  Thread g takes parent tile g and walks its `per` children through
// the children's jump table.  parent == nullptr: the one walk at the top,
// from the first non-empty sentence; it also finishes the stats.
__global__ __launch_bounds__(64) void fit_resolve_kernel(const Quad *__restrict__ jump,
                                                         const Quad *__restrict__ parent, uint64_t parents,
                                                         Quad *__restrict__ child, uint64_t children, uint64_t per,
                                                         uint64_t span, uint64_t n, const uint64_t *__restrict__ P,
                                                         uint64_t *__restrict__ ctl, uint64_t *__restrict__ stats) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * 64 + threadIdx.x;
  if (g >= parents) return;
  Quad r;
  if (parent) {
    r = parent[g];
  } else {
    // The first i with P[i + 1] > 0.
    uint64_t a = 0, b = n;  // P[a] == 0; answer in [a, b]
    while (a < b) {
      const uint64_t mid = a + (b - a) / 2;
      if (P[mid + 1] > 0) b = mid;
      else a = mid + 1;
    }
    r = make_uint4(a < n ? static_cast<uint32_t>(a) : kNone, 0u, kNone, 0u);
  }
  uint64_t e = r.x;
  uint32_t base = r.y, prev = r.z;
  const uint64_t first = g * per, last = first + per < children ? first + per : children;
  for (uint64_t t = first; t < last; ++t) {
    const uint64_t end = (t + 1) * span < n ? (t + 1) * span : n;
    if (e < end) {
      child[t] = make_uint4(static_cast<uint32_t>(e), base, prev, 0u);
      const Quad j = jump[e];
      e = j.x;
      base += j.y;
      prev = j.z;
    } else {
      child[t] = make_uint4(kNone, base, prev, 0u);
    }
  }
  if (!parent) {
    ctl[kCtlRows] = base;
    if (stats) {
      stats[0] = base;
      stats[1] = P[n];
      stats[2] = ctl[kCtlCut];
      stats[3] = ctl[kCtlDropped];
    }
  }
}

// Pass 4.  One block per level-0 tile.
__global__ __launch_bounds__(256) void fit_mark_kernel(const uint64_t *__restrict__ P,
                                                       const uint32_t *__restrict__ next, uint64_t n, uint32_t L,
                                                       const Quad *__restrict__ jump, const Quad *__restrict__ rec,
                                                       uint64_t rows_cap, uint32_t *__restrict__ row_first,
                                                       int32_t *__restrict__ row_lengths,
                                                       uint64_t *__restrict__ place) {
  __shared__ uint16_t up[kFitLift][kFitTile];
  __shared__ uint16_t s_start[kFitTile];  // the h-th row start of the tile
  __shared__ uint8_t s_flag[kFitTile];
  __shared__ uint32_t s_w[4];
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kFitTile;
  const uint32_t cnt = n - t0 < kFitTile ? static_cast<uint32_t>(n - t0) : kFitTile;
  const Quad me = rec[blockIdx.x];
  for (uint32_t x = threadIdx.x; x < kFitTile; x += 256) s_flag[x] = 0;
  BuildLift(up, next, t0, cnt);
  if (me.x != kNone) {
    const uint32_t entry = static_cast<uint32_t>(me.x - t0), starts = jump[me.x].y;  // <= cnt
    for (uint32_t h = threadIdx.x; h < starts; h += 256) {
      uint32_t y = entry;
#pragma unroll
      for (uint32_t r = 0; r < kFitLift; ++r)
        if (h >> r & 1u) y = up[r][y];
      s_start[h] = static_cast<uint16_t>(y);
      s_flag[y] = 1;
      const uint64_t row = static_cast<uint64_t>(me.y) + h;
      if (row < rows_cap) {
        row_first[row] = static_cast<uint32_t>(t0 + y);
        if (row_lengths) row_lengths[row] = static_cast<int32_t>(P[next[t0 + y]] - P[t0 + y]);
      }
    }
  }
  __syncthreads();
  // Thread t numbers sentences [16 t, 16 t + 16).
  constexpr uint32_t kPer = kFitTile / 256;
  const uint32_t x0 = threadIdx.x * kPer;
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) mine += s_flag[x0 + j];
  uint32_t total;
  uint32_t seen = BlockExclusiveScan(mine, s_w, &total);  // row starts of the tile before x0
  if (!place) return;
  uint64_t start = seen ? t0 + s_start[seen - 1] : me.z;  // kNone only in front of the first non-empty sentence
  uint64_t p_start = start != kNone ? P[start] : 0;
  for (uint32_t j = 0; j < kPer && x0 + j < cnt; ++j) {
    const uint64_t i = t0 + x0 + j;
    if (s_flag[x0 + j]) {
      ++seen;
      start = i;
      p_start = P[i];
    }
    const uint64_t p = P[i];
    place[i] = P[i + 1] == p ? UINT64_MAX : (static_cast<uint64_t>(me.y) + seen - 1) * L + (p - p_start);
  }
}

// Pass 5.  dense_pack_kernel's layout; the rows to write come from ctl.
__global__ __launch_bounds__(256) void fit_fill_kernel(const int32_t *__restrict__ ids,
                                                       const uint64_t *__restrict__ off, uint64_t n, uint32_t L,
                                                       int32_t pad_id, uint32_t flags, uint64_t rows_cap,
                                                       const uint64_t *__restrict__ P,
                                                       const uint32_t *__restrict__ next,
                                                       const uint32_t *__restrict__ row_first,
                                                       const uint64_t *__restrict__ ctl, int32_t *__restrict__ out,
                                                       int32_t *__restrict__ seq, int32_t *__restrict__ pos,
                                                       bool vec_out, bool vec_seq, bool vec_pos) {
  const TokView v{nullptr, P, n, 0, 0};
  const uint64_t need = ctl[kCtlRows];
  const uint64_t total = (need < rows_cap ? need : rows_cap) * L;
  uint64_t chunk = (total + gridDim.x - 1) / gridDim.x;
  chunk = (chunk + kDenseTile - 1) / kDenseTile * kDenseTile;
  uint64_t begin = static_cast<uint64_t>(blockIdx.x) * chunk, end = begin + chunk;
  if (begin > total) begin = total;
  if (end > total) end = total;
  for (uint64_t t = begin + threadIdx.x * 4u; t < end; t += kDenseTile) {
    const uint32_t cnt = end - t < 4 ? static_cast<uint32_t>(end - t) : 4u;
    uint64_t row = t / L;
    uint32_t col = static_cast<uint32_t>(t - row * L);
    // The row's sentences [f, stop) and their tokens [pf, pe).
    uint64_t f = row_first[row], stop = next[f], pf = P[f], pe = P[stop], sent = f;
    int32_t id[4] = {pad_id, pad_id, pad_id, pad_id}, sq[4] = {-1, -1, -1, -1}, ps[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (j < cnt) {
        const uint64_t g = pf + col;
        if (g < pe) {
          sent = FindSentence(v, sent, stop, g);
          const uint64_t b = off[sent], len = off[sent + 1] - b;
          const uint32_t k = static_cast<uint32_t>(g - P[sent]);
          id[j] = ids[b + FitSlotSource(len, L, flags, k)];
          sq[j] = static_cast<int32_t>(sent);
          ps[j] = static_cast<int32_t>(k);
        }
        if (++col == L && j + 1 < cnt) {
          col = 0;
          ++row;
          f = row_first[row];
          stop = next[f];
          pf = P[f];
          pe = P[stop];
          sent = f;
        }
      }
    }
    StoreQuad(out, t, id, cnt, vec_out);
    if (seq) StoreQuad(seq, t, sq, cnt, vec_seq);
    if (pos) StoreQuad(pos, t, ps, cnt, vec_pos);
  }
}

bool Aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

hipError_t LaunchDenseFitEmpty(uint64_t *stats, hipStream_t st) {
  if (!stats) return hipSuccess;
  hipLaunchKernelGGL(fit_empty_kernel, dim3(1), dim3(64), 0, st, stats);
  return hipGetLastError();
}

hipError_t LaunchDenseFit(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                          uint32_t flags, uint64_t rows_cap, int32_t *out, int32_t *seq, int32_t *pos,
                          int32_t *row_lengths, uint64_t *place, uint64_t *stats, void *scratch, const FitPlan &plan,
                          FitGeometry g, hipStream_t st) {
  char *base = static_cast<char *>(scratch);
  uint64_t *ctl = reinterpret_cast<uint64_t *>(base + plan.ctl);
  uint64_t *desc = reinterpret_cast<uint64_t *>(base + plan.desc);
  uint64_t *P = reinterpret_cast<uint64_t *>(base + plan.prefix);
  uint32_t *next = reinterpret_cast<uint32_t *>(base + plan.next);
  uint32_t *row_first = reinterpret_cast<uint32_t *>(base + plan.row_first);
  auto jump = [&](uint32_t l) { return reinterpret_cast<Quad *>(base + plan.jump[l]); };
  auto rec = [&](uint32_t l) { return reinterpret_cast<Quad *>(base + plan.rec[l]); };
  auto grid = [](uint64_t items, uint64_t per, uint64_t most) {
    const uint64_t b = (items + per - 1) / per;
    return dim3(static_cast<unsigned>(b < most ? (b ? b : 1) : most));
  };
#define SPM_FIT_LAUNCHED()                 \
  do {                                     \
    const hipError_t e = hipGetLastError(); \
    if (e != hipSuccess) return e;         \
  } while (0)
  hipLaunchKernelGGL(fit_init_kernel, dim3(1), dim3(256), 0, st, ctl, desc, stats);
  SPM_FIT_LAUNCHED();
  uint64_t chunks = (n + 1023) / 1024;
  if (chunks > kFitScanTiles) chunks = kFitScanTiles;
  const uint64_t chunk = (n + chunks - 1) / chunks;
  chunks = (n + chunk - 1) / chunk;
  hipLaunchKernelGGL(fit_prefix_kernel, dim3(static_cast<unsigned>(chunks)), dim3(256), 0, st, off, n, L, chunk, ctl,
                     desc, P);
  SPM_FIT_LAUNCHED();
  hipLaunchKernelGGL(fit_next_kernel, grid(n, 256, 8192), dim3(256), 0, st, P, n, L, next);
  SPM_FIT_LAUNCHED();
  hipLaunchKernelGGL(fit_tile_kernel, dim3(static_cast<unsigned>(plan.tiles[0])), dim3(256), 0, st, next, n, jump(0));
  SPM_FIT_LAUNCHED();
  for (uint32_t l = 1; l < plan.levels; ++l) {
    for (uint32_t s = g.branch; s-- > 0;) {
      hipLaunchKernelGGL(fit_compose_kernel, grid(plan.tiles[l] * plan.span[l - 1], 256, 8192), dim3(256), 0, st,
                         jump(l - 1), jump(l), n, plan.span[l - 1], g.branch, s, plan.tiles[l]);
      SPM_FIT_LAUNCHED();
    }
  }
  const uint32_t top = plan.levels - 1;
  hipLaunchKernelGGL(fit_resolve_kernel, dim3(1), dim3(64), 0, st, jump(top), static_cast<const Quad *>(nullptr),
                     uint64_t{1}, rec(top), plan.tiles[top], plan.tiles[top], plan.span[top], n, P, ctl, stats);
  SPM_FIT_LAUNCHED();
  for (uint32_t l = top; l > 0; --l) {
    hipLaunchKernelGGL(fit_resolve_kernel, grid(plan.tiles[l], 64, ~0u), dim3(64), 0, st, jump(l - 1), rec(l),
                       plan.tiles[l], rec(l - 1), plan.tiles[l - 1], uint64_t{g.branch}, plan.span[l - 1], n, P, ctl,
                       static_cast<uint64_t *>(nullptr));
    SPM_FIT_LAUNCHED();
  }
  hipLaunchKernelGGL(fit_mark_kernel, dim3(static_cast<unsigned>(plan.tiles[0])), dim3(256), 0, st, P, next, n, L,
                     jump(0), rec(0), rows_cap, row_first, row_lengths, place);
  SPM_FIT_LAUNCHED();
  // The row count is on the device only: a full grid, and a block whose range
  // is empty does nothing.
  hipLaunchKernelGGL(fit_fill_kernel, dim3(kDensePackBlocks), dim3(256), 0, st, ids, off, n, L, pad_id, flags,
                     rows_cap, P, next, row_first, ctl, out, seq, pos, Aligned(out, 16), Aligned(seq, 16),
                     Aligned(pos, 16));
#undef SPM_FIT_LAUNCHED
  return hipGetLastError();
}

}  // namespace spm_amd
