// Decode on the device: batched ids -> text.
//
// Reference: SentencePieceProcessor::Decode (sentencepiece_processor.cc:670-733)
// after ApplyExtraOptions (:945-979).  The surface of an id comes from the
// model's decode table (decode.h); the only state is "the text built so far is
// empty", under which a piece that starts with U+2581 loses that char.
//
// Work is laid out over the tokens of the batch in final order (extra options
// applied): token g of the call belongs to sentence i with S(i) <= g < S(i+1),
// S(i) = tok_off[i] - tok_off[0] + i * (bos/eos pieces per sentence).  Every
// token pass runs kDecodeBlocks blocks; block b owns the contiguous range
// [b * chunk, (b + 1) * chunk), chunk a multiple of kDecodeTile computed on the
// device from S(n), so no pass needs the token count on the host and the
// scratch is n words + kDecodeBlocks sums.  A block walks its range one
// sub-tile (one token per thread) at a time.
//
//   first pass : range-checks every id, then first[i] = min position whose
//                stripped surface is non-empty (one atomicMin per wave and
//                sentence) -- the sentence's bos state, resolved once.
//   count pass : block_sum[b] = bytes of the block's tokens.  A token before
//                first[i] gives 0 bytes, the token at first[i] its stripped
//                surface, every later one its whole surface.
//   write pass : block prefix = sum of block_sum[0, b); per sub-tile a block
//                scan gives each token its offset, the running offset carries
//                to the next sub-tile, and the sub-tile's bytes are copied
//                with one output byte per lane, so a wave stores 64
//                consecutive bytes.  Writes out_off[i] of every non-empty
//                sentence and the low word of each token's offset.
//   begin pass : piece_begin[g] -= out_off[i] (sentence-relative begins).
//   fill pass  : out_off of empty sentences and out_off[n]; sets
//                RESOURCE_EXHAUSTED.
//
// No pass reads the table or writes once the call's status word is non-zero.
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

struct Tok {
  uint64_t sent;
  uint64_t pos;  // position in the sentence, final order
  int32_t id;
  uint64_t src;  // index into ids, ~0 for a bos/eos piece
};

__device__ __forceinline__ Tok TokenAt(const TokView &v, const EpilogueExtras &x, uint64_t sent, uint64_t g) {
  Tok t;
  t.sent = sent;
  const uint64_t s0 = SentStart(v, sent);
  const uint64_t m = SentStart(v, sent + 1) - s0 - v.extras;
  t.pos = g - s0;
  if (t.pos < x.num_pre) {
    t.id = x.ids[t.pos];
    t.src = ~0ull;
  } else if (t.pos < x.num_pre + m) {
    const uint64_t q = t.pos - x.num_pre;
    t.src = v.tok_off[sent] + (x.reversed ? m - 1 - q : q);
    t.id = v.ids[t.src];
  } else {
    t.id = x.ids[kMaxExtras + (t.pos - x.num_pre - m)];
    t.src = ~0ull;
  }
  return t;
}

__device__ __forceinline__ uint32_t MetaOf(const uint32_t *meta, int32_t num_pieces, int32_t id) {
  return (id >= 0 && id < num_pieces) ? meta[id] : 0u;
}

// Bytes token (pos, meta) adds to its sentence, given the sentence's first
// non-empty position.
__device__ __forceinline__ uint32_t EffLen(uint32_t meta, uint64_t pos, uint32_t first) {
  if (pos < first) return 0;
  return (meta >> 1) - (pos == first ? (meta & 1u) : 0u);
}

__global__ __launch_bounds__(256) void decode_first_kernel(TokView v, EpilogueExtras x,
                                                           const uint32_t *__restrict__ meta, int32_t num_pieces,
                                                           uint32_t *__restrict__ first, uint64_t *__restrict__ ctl,
                                                           uint32_t *__restrict__ chain) {
  if (*chain) return;
  v.base = v.tok_off[0];
  const Range r = BlockRange(v);
  const int lane = threadIdx.x & 63;
  uint64_t sent = 0;
  bool have = false;
  for (uint64_t s = r.begin; s < r.end; s += kDecodeSubTile) {
    const uint64_t g = s + threadIdx.x;
    const bool valid = g < r.end;
    bool ne = false;
    uint32_t pos = 0;
    if (valid) {
      sent = FindSentence(v, have ? sent : 0, v.n, g);
      have = true;
      const Tok t = TokenAt(v, x, sent, g);
      pos = static_cast<uint32_t>(t.pos);
      if (t.id < 0 || t.id >= num_pieces) {  // checked before any table read
        atomicCAS(chain, 0u, static_cast<uint32_t>(SPM_OUT_OF_RANGE));
        atomicMin(reinterpret_cast<unsigned long long *>(ctl + kDcBadKey), static_cast<unsigned long long>(t.src));
      } else {
        const uint32_t mt = meta[t.id];
        ne = (mt >> 1) > (mt & 1u);
      }
    }
    // One atomic per (wave, sentence): the lowest lane of the sentence with a
    // non-empty stripped surface.  Lanes ascend with tokens, so the nearest
    // lower such lane decides.
    const uint64_t mask = __builtin_amdgcn_ballot_w64(ne);
    const uint64_t lower = mask & ((1ull << lane) - 1);
    const int near = lower ? 63 - __builtin_clzll(lower) : 0;
    const uint32_t near_lo = __shfl(static_cast<uint32_t>(sent), near);
    const uint32_t near_hi = __shfl(static_cast<uint32_t>(sent >> 32), near);
    const bool covered = lower && ((static_cast<uint64_t>(near_hi) << 32) | near_lo) == sent;
    if (ne && !covered) atomicMin(first + sent, pos);
  }
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

__global__ __launch_bounds__(256) void decode_count_kernel(TokView v, EpilogueExtras x,
                                                           const uint32_t *__restrict__ meta, int32_t num_pieces,
                                                           const uint32_t *__restrict__ first,
                                                           uint64_t *__restrict__ block_sum,
                                                           const uint32_t *__restrict__ chain) {
  __shared__ uint64_t s_w[4];
  if (*chain) return;
  v.base = v.tok_off[0];
  const Range r = BlockRange(v);
  uint64_t sent = 0, sum = 0;
  bool have = false;
  for (uint64_t g = r.begin + threadIdx.x; g < r.end; g += kDecodeSubTile) {
    sent = FindSentence(v, have ? sent : 0, v.n, g);
    have = true;
    const Tok t = TokenAt(v, x, sent, g);
    sum += EffLen(MetaOf(meta, num_pieces, t.id), t.pos, first[sent]);
  }
  sum = BlockSum64(sum, s_w);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = sum;
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

__global__ __launch_bounds__(256) void decode_write_kernel(TokView v, EpilogueExtras x,
                                                           const uint32_t *__restrict__ meta,
                                                           const uint32_t *__restrict__ off,
                                                           const uint8_t *__restrict__ bytes, int32_t num_pieces,
                                                           const uint32_t *__restrict__ first,
                                                           const uint64_t *__restrict__ block_sum,
                                                           uint64_t *__restrict__ ctl, uint8_t *__restrict__ out,
                                                           uint64_t capacity, uint64_t *__restrict__ out_off,
                                                           uint32_t *__restrict__ piece_begin,
                                                           const uint32_t *__restrict__ chain) {
  __shared__ uint64_t s_w64[4];
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_start[kDecodeSubTile];
  __shared__ uint32_t s_src[kDecodeSubTile];
  if (*chain) return;
  v.base = v.tok_off[0];
  uint64_t before = 0, all = 0;
  for (uint32_t k = threadIdx.x; k < gridDim.x; k += blockDim.x) {
    const uint64_t bs = block_sum[k];
    all += bs;
    if (k < blockIdx.x) before += bs;
  }
  uint64_t run = BlockSum64(before, s_w64);
  const uint64_t total = BlockSum64(all, s_w64);
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl[kDcTotal] = total;
  const bool write = out != nullptr && total <= capacity;
  if (out != nullptr && !write) piece_begin = nullptr;  // exhausted: offsets only
  const Range r = BlockRange(v);
  uint64_t sent = 0;
  bool have = false;
  for (uint64_t s = r.begin; s < r.end; s += kDecodeSubTile) {
    const uint64_t g = s + threadIdx.x;
    const bool valid = g < r.end;
    uint32_t len = 0, src = 0;
    uint64_t pos = 1;
    if (valid) {
      sent = FindSentence(v, have ? sent : 0, v.n, g);
      have = true;
      const Tok t = TokenAt(v, x, sent, g);
      const uint32_t mt = MetaOf(meta, num_pieces, t.id);
      const uint32_t f = first[sent];
      pos = t.pos;
      len = EffLen(mt, pos, f);
      if (len) src = off[t.id] + (pos == f ? (mt & 1u) : 0u);
    }
    uint32_t sub_total;
    const uint32_t excl = BlockExclusiveScan(len, s_w, &sub_total);
    if (valid) {
      const uint64_t at = run + excl;
      if (pos == 0) out_off[sent] = at;
      if (piece_begin) piece_begin[g] = static_cast<uint32_t>(at);
    }
    if (write) {
      s_start[threadIdx.x] = excl;
      s_src[threadIdx.x] = src;
      __syncthreads();
      for (uint32_t o = threadIdx.x; o < sub_total; o += kDecodeSubTile) {
        // The token holding byte o: the last one that starts at or before o
        // (tokens of no bytes share a start with their successor).
        uint32_t a = 0, b = kDecodeSubTile;
        while (b - a > 1) {
          const uint32_t mid = (a + b) >> 1;
          if (s_start[mid] <= o) a = mid;
          else b = mid;
        }
        out[run + o] = bytes[s_src[a] + (o - s_start[a])];
      }
      __syncthreads();
    }
    run += sub_total;
  }
}

// piece_begin holds the low word of each token's offset in the batch; make it
// relative to the token's sentence.
__global__ __launch_bounds__(256) void decode_begin_kernel(TokView v, const uint64_t *__restrict__ ctl,
                                                           uint64_t capacity,
                                                           const uint64_t *__restrict__ out_off,
                                                           uint32_t *__restrict__ piece_begin,
                                                           const uint32_t *__restrict__ chain) {
  if (*chain || ctl[kDcTotal] > capacity) return;
  v.base = v.tok_off[0];
  const Range r = BlockRange(v);
  uint64_t sent = 0;
  bool have = false;
  for (uint64_t g = r.begin + threadIdx.x; g < r.end; g += kDecodeSubTile) {
    sent = FindSentence(v, have ? sent : 0, v.n, g);
    have = true;
    piece_begin[g] -= static_cast<uint32_t>(out_off[sent]);
  }
}

// out_off of the sentences without tokens (the write pass sets the others):
// that of the next sentence with tokens, or the total.
__global__ __launch_bounds__(256) void decode_fill_kernel(TokView v, const uint64_t *__restrict__ ctl,
                                                          bool has_out, uint64_t capacity,
                                                          uint64_t *__restrict__ out_off,
                                                          uint32_t *__restrict__ chain) {
  if (*chain) return;
  v.base = v.tok_off[0];
  const uint64_t total = ctl[kDcTotal];
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= v.n; i += stride) {
    if (i == v.n) {
      out_off[i] = total;
      continue;
    }
    const uint64_t s0 = SentStart(v, i);
    if (SentStart(v, i + 1) != s0) continue;
    // Last index (n included) that starts at the same token.
    const uint64_t a = FindSentence(v, i, v.n + 1, s0);
    out_off[i] = a == v.n ? total : out_off[a];
  }
  // Last, so that the passes above ran: the text did not fit.
  if (has_out && total > capacity && blockIdx.x == 0 && threadIdx.x == 0)
    atomicCAS(chain, 0u, static_cast<uint32_t>(SPM_RESOURCE_EXHAUSTED));
}

// The first out-of-range id (lowest index into ids) as sentence and id.
__global__ void decode_bad_kernel(TokView v, uint64_t *__restrict__ ctl) {
  const uint64_t k = ctl[kDcBadKey];
  if (k == ~0ull) return;
  uint64_t a = 0, b = v.n;  // largest a with tok_off[a] <= k
  while (b - a > 1) {
    const uint64_t mid = a + (b - a) / 2;
    if (v.tok_off[mid] <= k) a = mid;
    else b = mid;
  }
  ctl[kDcBadSentence] = a;
  ctl[kDcBadId] = static_cast<uint64_t>(static_cast<int64_t>(v.ids[k]));
}

}  // namespace

hipError_t LaunchDecode(const DecodeLaunch &a, bool resolve_bad, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  TokView v{a.ids, a.tok_off, a.n, 0, a.x.num_pre + a.x.num_post};
  const dim3 grid(kDecodeBlocks), block(kDecodeSubTile);
  hipLaunchKernelGGL(decode_first_kernel, grid, block, 0, st, v, a.x, a.meta, a.num_pieces, a.first, a.ctl, a.chain);
  hipLaunchKernelGGL(decode_count_kernel, grid, block, 0, st, v, a.x, a.meta, a.num_pieces, a.first, a.block_sum,
                     a.chain);
  hipLaunchKernelGGL(decode_write_kernel, grid, block, 0, st, v, a.x, a.meta, a.off, a.bytes, a.num_pieces, a.first,
                     a.block_sum, a.ctl, a.out, a.capacity, a.out_off, a.out ? a.piece_begin : nullptr, a.chain);
  if (a.out && a.piece_begin)
    hipLaunchKernelGGL(decode_begin_kernel, grid, block, 0, st, v, a.ctl, a.capacity, a.out_off, a.piece_begin,
                       a.chain);
  const uint64_t fb = (a.n + 1 + 255) / 256;
  hipLaunchKernelGGL(decode_fill_kernel, dim3(static_cast<unsigned>(fb < 65536 ? fb : 65536)), block, 0, st, v, a.ctl,
                     a.out != nullptr, a.capacity, a.out_off, a.chain);
  if (resolve_bad) hipLaunchKernelGGL(decode_bad_kernel, dim3(1), dim3(1), 0, st, v, a.ctl);
  return hipGetLastError();
}

}  // namespace spm_amd
