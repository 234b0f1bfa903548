// WORD / CHAR encode (word_model.cc:33-46, char_model.cc:42-58): the batch's
// tokens are views into the input, in order, so an encode is (1) a mark on
// every byte that starts a token, (2) a count of the marks before every
// position and (3) PieceToId of each marked span.
//
// Work is split over tiles of kWcTile bytes of the whole batch, never over
// sentences: a token (and a sentence) belongs to the tile of its first byte.
//
//   wc_sent_kernel    the first sentence that starts in or after each tile
//                     (one thread per sentence; saves every tile a search).
//   wc_mark_kernel    tile tier: marks token starts by the shortcut (CHAR:
//                     every non-continuation byte; WORD: sentence starts and
//                     every "▁") and checks, per lead byte, that the shortcut
//                     equals the reference's OneCharLen walk.  A sentence
//                     where it does not is flagged.
//   wc_general_kernel general tier: one sentence per lane, the reference's
//                     sequential loop (PrefixMatch over the user-defined
//                     symbols, SplitIntoWords), re-marking the flagged
//                     sentences (or every sentence).
//   wc_count_kernel   marks per tile and the first mark of each tile.
//   wc_scan_kernel    exclusive scan of the tile counts and, per tile, the
//                     first mark of any later tile (one block).
//   wc_write_kernel   per tile: the list of its token starts, one lookup per
//                     thread over that list with consecutive stores, and the
//                     token offsets of the sentences that start in the tile.
//
// Every kernel idles when the caller's chain status is already set or the
// batch exceeds the caller's capacity; the last kernel then publishes
// RESOURCE_EXHAUSTED (first error wins).
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.h"
#include "normalize_prefix.h"
#include "wordchar_table.h"

namespace spm_amd {
namespace {

constexpr uint32_t kT = kWcTile;
constexpr uint32_t kThreads = 256;
constexpr uint32_t kPer = kT / kThreads;  // bytes per thread
static_assert(kPer == 8, "a thread owns one 8-byte word of the tile");
constexpr uint32_t kStatusResourceExhausted = 8;  // SPM_RESOURCE_EXHAUSTED

__device__ __forceinline__ bool WcIdle(const WordCharLaunch &l) {
  return (l.chain && *l.chain != 0) || l.off[l.n] > l.capacity;
}

// tile_sent[t] = the first i in [0, n] with off[i] >= t * kT, for every tile
// up to the one that holds off[n] (the later tiles hold nothing and never
// read theirs).  Sentence i owns the tiles whose first byte lies in
// (off[i - 1], off[i]].  A lane writes a span of up to 8 tiles itself; the
// wave writes a longer one together, 64 tiles a step, so a line of any
// length costs its tiles / 64 steps of one wave.
__global__ __launch_bounds__(256) void wc_sent_kernel(WordCharLaunch l) {
  if (WcIdle(l)) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
  for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); w * 64 <= l.n;
       w += waves) {
    const uint64_t i = w * 64 + lane;
    uint64_t lo = 1, hi = 0;  // an empty span
    if (i <= l.n) {
      lo = i ? l.off[i - 1] / kT + 1 : 0;
      hi = l.off[i] / kT;
      if (hi >= l.tiles) hi = l.tiles - 1;
    }
    const bool wide = hi >= lo && hi - lo >= 8;
    if (!wide)
      for (uint64_t t = lo; t <= hi && hi >= lo; ++t) l.tile_sent[t] = static_cast<uint32_t>(i);
    unsigned long long m = __ballot(wide);
    while (m) {
      const int src = __ffsll(static_cast<long long>(m)) - 1;
      m &= m - 1;
      const uint64_t slo = __shfl(static_cast<unsigned long long>(lo), src, 64);
      const uint64_t shi = __shfl(static_cast<unsigned long long>(hi), src, 64);
      for (uint64_t t = slo + lane; t <= shi; t += 64) l.tile_sent[t] = static_cast<uint32_t>(w * 64 + src);
    }
  }
}

// The sentence that holds byte p (off[0] <= p < off[n]): the last i with
// off[i] <= p (empty sentences at the same offset come before it).
__device__ uint64_t WcSentenceOf(const uint64_t *__restrict__ off, uint64_t n, uint64_t p) {
  uint64_t lo = 0, hi = n;  // first index in [0, n] with off[idx] > p
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= p) lo = mid + 1;
    else hi = mid;
  }
  return lo ? lo - 1 : 0;
}

__device__ __forceinline__ uint32_t ByteOf(uint64_t lo, uint64_t hi, uint32_t j) {
  return static_cast<uint32_t>((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFFu);
}

// The tile's 8-byte word of thread `tid` (bytes at or past `total` read as 0).
__device__ __forceinline__ uint64_t LoadWord(const uint8_t *__restrict__ base, uint64_t p, uint64_t total) {
  if (p + 8 <= total && (reinterpret_cast<uintptr_t>(base + p) & 7u) == 0)
    return *reinterpret_cast<const uint64_t *>(base + p);
  uint64_t v = 0;
  for (uint32_t j = 0; j < 8; ++j)
    if (p + j < total) v |= static_cast<uint64_t>(base[p + j]) << (8 * j);
  return v;
}

__global__ __launch_bounds__(256) void wc_mark_kernel(WordCharLaunch l) {
  if (WcIdle(l)) return;
  // One word more than the tile: a lead byte looks up to 4 bytes ahead.
  __shared__ uint64_t s_b[kThreads + 1];
  __shared__ uint64_t s_bnd64[kThreads + 1];
  uint8_t *s_bnd = reinterpret_cast<uint8_t *>(s_bnd64);
  const uint64_t total = l.off[l.n], off0 = l.off[0];
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kT;
  if (t0 >= total) return;
  const uint32_t tid = threadIdx.x;
  s_b[tid] = LoadWord(l.bytes, t0 + 8ull * tid, total);
  s_bnd64[tid] = 0;
  if (tid == 0) {
    s_b[kThreads] = LoadWord(l.bytes, t0 + kT, total);
    s_bnd64[kThreads] = 0;
  }
  __syncthreads();
  // Boundaries: 1 where a sentence starts or ends (offsets in the tile and
  // its look-ahead word; off[n] = the end of the batch among them).
  const uint64_t first = l.tile_sent[blockIdx.x];
  for (uint64_t i = first + tid; i <= l.n; i += kThreads) {
    const uint64_t o = l.off[i];
    if (o >= t0 + kT + 8) break;
    if (o >= t0) s_bnd[o - t0] = 1;
  }
  __syncthreads();
  const uint64_t blo = s_b[tid], bhi = s_b[tid + 1];
  const uint64_t nlo = s_bnd64[tid], nhi = s_bnd64[tid + 1];
  uint64_t marks = 0;
  for (uint32_t j = 0; j < kPer; ++j) {
    const uint64_t p = t0 + 8ull * tid + j;
    if (p >= total || p < off0) continue;
    const uint32_t b = ByteOf(blo, bhi, j);
    const bool start = ByteOf(nlo, nhi, j) != 0;
    bool bad = false, mark;
    if ((b & 0xC0u) == 0x80u) {
      bad = start;  // the sentence begins with a continuation byte
      mark = l.word ? start : false;
    } else {
      // OneCharLen(b) must equal 1 + the run of continuation bytes that
      // follows; a run cut by the sentence end may be shorter.
      const uint32_t len = OneCharLenDev(b);
      bool cut = false;
      for (uint32_t q = 1; q < len && !bad && !cut; ++q) {
        if (ByteOf(nlo, nhi, j + q)) cut = true;
        else if ((ByteOf(blo, bhi, j + q) & 0xC0u) != 0x80u) bad = true;
      }
      if (!bad && !cut && !ByteOf(nlo, nhi, j + len) && (ByteOf(blo, bhi, j + len) & 0xC0u) == 0x80u) bad = true;
      if (l.word) {
        mark = start || (b == 0xE2u && ByteOf(blo, bhi, j + 1) == 0x96u && ByteOf(blo, bhi, j + 2) == 0x81u &&
                         !ByteOf(nlo, nhi, j + 1) && !ByteOf(nlo, nhi, j + 2));
      } else {
        mark = true;
      }
    }
    if (mark) marks |= 1ull << (8 * j);
    if (bad) {
      const uint64_t i = WcSentenceOf(l.off, l.n, p);
      if (atomicExch(&l.sflag[i], 1u) == 0u) l.flagged[atomicAdd(&l.status[kStFlagged], 1u)] = static_cast<uint32_t>(i);
    }
  }
  // The mark buffer is the workspace's own (8-byte aligned, whole tiles).
  *reinterpret_cast<uint64_t *>(l.mark + t0 + 8ull * tid) = marks;
}

__global__ __launch_bounds__(256) void wc_general_kernel(WordCharLaunch l, int all) {
  if (WcIdle(l)) return;
  const uint64_t total = l.off[l.n];
  const uint64_t count = all ? l.n : l.status[kStFlagged];
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < count; g += stride) {
    const uint64_t i = all ? g : l.flagged[g];
    const uint64_t s = l.off[i];
    uint64_t e = l.off[i + 1];
    if (e > total) e = total;
    uint64_t p = s;
    while (p < e) {
      const uint64_t left = e - p;
      uint32_t mblen;
      bool mark;
      if (l.word) {
        // SplitIntoWords (model_interface.cc:178-188), whitespace as prefix.
        mblen = OneCharLenDev(l.bytes[p]);
        if (mblen > left) mblen = static_cast<uint32_t>(left);
        mark = p == s || (mblen == 3 && l.bytes[p] == 0xE2u && l.bytes[p + 1] == 0x96u && l.bytes[p + 2] == 0x81u);
      } else {
        // PrefixMatcher::PrefixMatch (normalizer.cc): the longest
        // user-defined symbol here, else one char.
        mblen = l.ud_units ? TrieLongest(l.ud_units, l.ud_num_units, l.bytes + p, left) : 0u;
        if (mblen == 0) {
          mblen = OneCharLenDev(l.bytes[p]);
          if (mblen > left) mblen = static_cast<uint32_t>(left);
        }
        mark = true;
      }
      l.mark[p] = mark ? 1 : 0;
      for (uint32_t q = 1; q < mblen; ++q) l.mark[p + q] = 0;
      p += mblen;
    }
  }
  if (all && blockIdx.x == 0 && threadIdx.x == 0) l.status[kStFlagged] = static_cast<uint32_t>(l.n);
}

// The tile's marks of thread tid: bytes outside [off0, total) carry none.
__device__ __forceinline__ uint64_t LoadMarks(const WordCharLaunch &l, uint64_t t0, uint32_t tid, uint64_t off0,
                                              uint64_t total) {
  const uint64_t p = t0 + 8ull * tid;
  if (p >= total || p + 8 <= off0) return 0;
  uint64_t v = *reinterpret_cast<const uint64_t *>(l.mark + p) & 0x0101010101010101ull;
  for (uint32_t j = 0; j < 8; ++j)
    if (p + j >= total || p + j < off0) v &= ~(0xFFull << (8 * j));
  return v;
}

__global__ __launch_bounds__(256) void wc_count_kernel(WordCharLaunch l) {
  if (WcIdle(l)) return;
  __shared__ uint32_t s_cnt[kThreads / 64], s_first[kThreads / 64];
  const uint64_t total = l.off[l.n], off0 = l.off[0];
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kT;
  const uint32_t tid = threadIdx.x;
  const uint64_t v = LoadMarks(l, t0, tid, off0, total);
  uint32_t cnt = __popcll(v);
  uint32_t first = v ? 8u * tid + (static_cast<uint32_t>(__ffsll(static_cast<long long>(v))) - 1u) / 8u : kT;
  for (int d = 32; d > 0; d >>= 1) {
    cnt += __shfl_down(cnt, d, 64);
    const uint32_t o = __shfl_down(first, d, 64);
    first = o < first ? o : first;
  }
  if ((tid & 63u) == 0) {
    s_cnt[tid >> 6] = cnt;
    s_first[tid >> 6] = first;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0, f = kT;
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
      c += s_cnt[w];
      f = s_first[w] < f ? s_first[w] : f;
    }
    l.tile_count[blockIdx.x] = c;
    l.tile_first[blockIdx.x] = f;
  }
}

// Over the tiles up to the one that holds off[n] (one block of 1024, a
// contiguous chunk of tiles per thread): tile_prefix = exclusive scan of
// tile_count, and tile_next[t] = the position of the first mark in a later
// tile (kNoMark when none), a suffix minimum over tile_first, so no tile
// walks forward to find where its last token ends.
constexpr uint64_t kNoMark = ~0ull;
__global__ __launch_bounds__(1024) void wc_scan_kernel(WordCharLaunch l) {
  if (WcIdle(l)) return;
  __shared__ uint64_t s_sum[1024];
  __shared__ uint64_t s_pos[1024];
  const uint32_t tid = threadIdx.x;
  uint64_t used = l.off[l.n] / kT + 1;
  if (used > l.tiles) used = l.tiles;
  const uint64_t chunk = (used + 1023) / 1024;
  const uint64_t b = chunk * tid < used ? chunk * tid : used, e = b + chunk < used ? b + chunk : used;
  uint64_t sum = 0, pos = kNoMark;
  for (uint64_t t = b; t < e; ++t) {
    sum += l.tile_count[t];
    const uint32_t f = l.tile_first[t];
    if (pos == kNoMark && f < kT) pos = t * kT + f;
  }
  s_sum[tid] = sum;
  s_pos[tid] = pos;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint64_t add = tid >= d ? s_sum[tid - d] : 0;
    const uint64_t nxt = tid + d < 1024 ? s_pos[tid + d] : kNoMark;
    __syncthreads();
    s_sum[tid] += add;
    if (nxt < s_pos[tid]) s_pos[tid] = nxt;
    __syncthreads();
  }
  uint64_t run = s_sum[tid] - sum;
  for (uint64_t t = b; t < e; ++t) {
    l.tile_prefix[t] = run;
    run += l.tile_count[t];
  }
  uint64_t cur = tid + 1 < 1024 ? s_pos[tid + 1] : kNoMark;  // the first mark after this chunk
  for (uint64_t t = e; t-- > b;) {
    l.tile_next[t] = cur;
    const uint32_t f = l.tile_first[t];
    if (f < kT) cur = t * kT + f;
  }
}

__global__ __launch_bounds__(256) void wc_write_kernel(WordCharLaunch l) {
  if (WcIdle(l)) return;
  __shared__ uint16_t s_excl[kT];   // marks of the tile before each byte
  __shared__ uint16_t s_list[kT];   // the tile's token starts, in order
  __shared__ uint32_t s_wave[kThreads / 64];
  __shared__ uint64_t s_next;       // the first token start after the tile
  const uint64_t total = l.off[l.n], off0 = l.off[0];
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kT;
  if (t0 > total) return;  // the tile of `total` itself places the sentences that end the batch
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t v = LoadMarks(l, t0, tid, off0, total);
  const uint32_t own = __popcll(v);
  uint32_t incl = own;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= static_cast<uint32_t>(d)) incl += o;
  }
  if (lane == 63u) s_wave[tid >> 6] = incl;
  if (tid == 0) {
    const uint64_t nm = l.tile_next[blockIdx.x];
    s_next = nm < total ? nm : total;
  }
  __syncthreads();
  uint32_t run = incl - own;
  for (uint32_t w = 0; w < (tid >> 6); ++w) run += s_wave[w];
  for (uint32_t j = 0; j < kPer; ++j) {
    s_excl[8u * tid + j] = static_cast<uint16_t>(run);
    if ((v >> (8 * j)) & 1ull) s_list[run++] = static_cast<uint16_t>(8u * tid + j);
  }
  __syncthreads();
  const uint32_t cnt = l.tile_count[blockIdx.x];
  const uint64_t gbase = l.tile_prefix[blockIdx.x];
  const WordCharEntry *tab = reinterpret_cast<const WordCharEntry *>(l.tab);
  for (uint32_t k = tid; k < cnt; k += kThreads) {
    const uint64_t p = t0 + s_list[k];
    const uint64_t e = k + 1 < cnt ? t0 + s_list[k + 1] : s_next;
    const uint64_t len = e - p;
    // A token longer than the longest piece is unknown without a lookup.
    const int32_t id = len > l.max_piece_bytes
                           ? l.unk_id
                           : WordCharFind(tab, l.tab_mask, l.keys, l.bytes + p, static_cast<uint32_t>(len), l.unk_id);
    l.ids[gbase + k] = id;
    if (l.len) l.len[gbase + k] = static_cast<uint32_t>(len);
  }
  // Token offsets of the sentences that start in this tile (i = n: the total).
  const uint64_t first = l.tile_sent[blockIdx.x];
  for (uint64_t i = first + tid; i <= l.n; i += kThreads) {
    const uint64_t o = l.off[i];
    if (o >= t0 + kT) break;
    if (o >= t0) l.tok_off[i] = gbase + s_excl[o - t0];
  }
}

// n == 0: the only output is tok_off[0] = 0, unless the chain already failed.
__global__ void wc_empty_kernel(uint64_t *tok_off, const uint32_t *chain) {
  if (!(chain && *chain != 0)) tok_off[0] = 0;
}

__global__ void wc_status_kernel(WordCharLaunch l) {
  if (l.out_status && l.off[l.n] > l.capacity) atomicCAS(l.out_status, 0u, kStatusResourceExhausted);
}

}  // namespace

hipError_t LaunchWordCharEmpty(uint64_t *tok_off, const uint32_t *chain, hipStream_t st) {
  hipLaunchKernelGGL(wc_empty_kernel, dim3(1), dim3(1), 0, st, tok_off, chain);
  return hipGetLastError();
}

hipError_t LaunchWordCharSentences(const WordCharLaunch &l, hipStream_t st) {
  const uint64_t want = (l.n + 1 + kThreads - 1) / kThreads;  // a lane per sentence, i = n included
  hipLaunchKernelGGL(wc_sent_kernel, dim3(static_cast<uint32_t>(want > 65536 ? 65536 : want)), dim3(kThreads), 0, st, l);
  return hipGetLastError();
}

hipError_t LaunchWordCharTile(const WordCharLaunch &l, hipStream_t st) {
  hipLaunchKernelGGL(wc_mark_kernel, dim3(static_cast<uint32_t>(l.tiles)), dim3(kThreads), 0, st, l);
  return hipGetLastError();
}

hipError_t LaunchWordCharGeneral(const WordCharLaunch &l, bool all, hipStream_t st) {
  const uint64_t want = (l.n + kThreads - 1) / kThreads;
  const uint32_t blocks = static_cast<uint32_t>(want < 1 ? 1 : want > 4096 ? 4096 : want);
  hipLaunchKernelGGL(wc_general_kernel, dim3(blocks), dim3(kThreads), 0, st, l, all ? 1 : 0);
  return hipGetLastError();
}

hipError_t LaunchWordCharOutput(const WordCharLaunch &l, hipStream_t st) {
  const dim3 grid(static_cast<uint32_t>(l.tiles));
  hipLaunchKernelGGL(wc_count_kernel, grid, dim3(kThreads), 0, st, l);
  hipLaunchKernelGGL(wc_scan_kernel, dim3(1), dim3(1024), 0, st, l);
  hipLaunchKernelGGL(wc_write_kernel, grid, dim3(kThreads), 0, st, l);
  hipLaunchKernelGGL(wc_status_kernel, dim3(1), dim3(1), 0, st, l);
  return hipGetLastError();
}

}  // namespace spm_amd
