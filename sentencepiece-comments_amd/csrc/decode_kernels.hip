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
// A BYTE token (byte fallback) has no table surface: every pass computes it
// from the token's byte and up to 3 neighbours on each side of its run
// (ByteTokSurface; the rule and why 3 suffice: decode.h, ByteRunSurface).  Its
// surface is never stripped, and a non-empty one ends the bos state.
//
// No pass reads the table or writes once the call's status word is non-zero.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "decode.h"
#include "token_tiles.h"

namespace spm_amd {
namespace {

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

// Surface of the BYTE token t (meta mt) at token g: its length, the bytes
// packed little-endian in *lit.  Reads up to 3 tokens on each side, inside the
// sentence and the run (decode.h, ByteRunSurface).
__device__ __forceinline__ uint32_t ByteTokSurface(const TokView &v, const EpilogueExtras &x,
                                                   const uint32_t *__restrict__ meta, int32_t num_pieces,
                                                   const Tok &t, uint64_t g, uint32_t mt, uint32_t *lit) {
  const uint64_t count = SentStart(v, t.sent + 1) - SentStart(v, t.sent);
  uint8_t w[7] = {0, 0, 0, static_cast<uint8_t>(mt), 0, 0, 0};
  uint32_t lo = 0, hi = 0;
  while (lo < 3 && t.pos > lo) {
    const uint32_t nm = MetaOf(meta, num_pieces, TokenAt(v, x, t.sent, g - lo - 1).id);
    if (!(nm & kDecodeByteFlag)) break;
    ++lo;
    w[3 - lo] = static_cast<uint8_t>(nm);
  }
  while (hi < 3 && t.pos + hi + 1 < count) {
    const uint32_t nm = MetaOf(meta, num_pieces, TokenAt(v, x, t.sent, g + hi + 1).id);
    if (!(nm & kDecodeByteFlag)) break;
    ++hi;
    w[3 + hi] = static_cast<uint8_t>(nm);
  }
  uint8_t o[4] = {0, 0, 0, 0};
  const uint32_t len = ByteRunSurface(w, lo, hi, o);
  *lit = o[0] | (static_cast<uint32_t>(o[1]) << 8) | (static_cast<uint32_t>(o[2]) << 16) |
         (static_cast<uint32_t>(o[3]) << 24);
  return len;
}

// kB: the model has BYTE pieces (byte fallback).  Without them every pass is
// the table lookup alone.
template <bool kB>
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
        if (kB && (mt & kDecodeByteFlag)) {
          uint32_t lit;
          ne = ByteTokSurface(v, x, meta, num_pieces, t, g, mt, &lit) != 0;
        } else {
          ne = (mt >> 1) > (mt & 1u);
        }
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

template <bool kB>
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
    const uint32_t mt = MetaOf(meta, num_pieces, t.id);
    if (kB && (mt & kDecodeByteFlag)) {
      uint32_t lit;
      sum += ByteTokSurface(v, x, meta, num_pieces, t, g, mt, &lit);
    } else {
      sum += EffLen(mt, t.pos, first[sent]);
    }
  }
  sum = BlockSum64(sum, s_w);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = sum;
}

template <bool kB>
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
  __shared__ uint32_t s_lit[kB ? kDecodeSubTile : 1];  // a BYTE token's surface, s_src = kDecodeByteFlag
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
    uint32_t len = 0, src = 0, lit = 0;
    uint64_t pos = 1;
    if (valid) {
      sent = FindSentence(v, have ? sent : 0, v.n, g);
      have = true;
      const Tok t = TokenAt(v, x, sent, g);
      const uint32_t mt = MetaOf(meta, num_pieces, t.id);
      const uint32_t f = first[sent];
      pos = t.pos;
      if (kB && (mt & kDecodeByteFlag)) {
        len = ByteTokSurface(v, x, meta, num_pieces, t, g, mt, &lit);
        src = kDecodeByteFlag;
      } else {
        len = EffLen(mt, pos, f);
        if (len) src = off[t.id] + (pos == f ? (mt & 1u) : 0u);
      }
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
      if (kB) s_lit[threadIdx.x] = lit;
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
        const uint32_t from = s_src[a], at = o - s_start[a];
        if (kB && (from & kDecodeByteFlag)) out[run + o] = static_cast<uint8_t>(s_lit[a] >> (8 * at));
        else out[run + o] = bytes[from + at];
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
  if (a.has_bytes) {
    hipLaunchKernelGGL(decode_first_kernel<true>, grid, block, 0, st, v, a.x, a.meta, a.num_pieces, a.first, a.ctl,
                       a.chain);
    hipLaunchKernelGGL(decode_count_kernel<true>, grid, block, 0, st, v, a.x, a.meta, a.num_pieces, a.first,
                       a.block_sum, a.chain);
    hipLaunchKernelGGL(decode_write_kernel<true>, grid, block, 0, st, v, a.x, a.meta, a.off, a.bytes, a.num_pieces,
                       a.first, a.block_sum, a.ctl, a.out, a.capacity, a.out_off, a.out ? a.piece_begin : nullptr,
                       a.chain);
  } else {
    hipLaunchKernelGGL(decode_first_kernel<false>, grid, block, 0, st, v, a.x, a.meta, a.num_pieces, a.first, a.ctl,
                       a.chain);
    hipLaunchKernelGGL(decode_count_kernel<false>, grid, block, 0, st, v, a.x, a.meta, a.num_pieces, a.first,
                       a.block_sum, a.chain);
    hipLaunchKernelGGL(decode_write_kernel<false>, grid, block, 0, st, v, a.x, a.meta, a.off, a.bytes, a.num_pieces,
                       a.first, a.block_sum, a.ctl, a.out, a.capacity, a.out_off, a.out ? a.piece_begin : nullptr,
                       a.chain);
  }
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
