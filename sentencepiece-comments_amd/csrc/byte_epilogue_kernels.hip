// Id epilogue of Encode under byte fallback (TrainerSpec.byte_fallback) on the
// device.
//
// PopulateSentencePieceText with byte fallback: an UNKNOWN token is not merged
// with its neighbours; it is replaced by one BYTE piece per byte of its
// normalized text, id = the piece named after the byte.  Every other token
// gives one output.  In the SentencePieceText form every byte piece but the
// last of its token has an empty surface at the token's begin, the last one
// carries the token's whole surface.  Then ApplyExtraOptions, folded as for
// the plain epilogue: out = pre . (expanded tokens, reversed if flagged) . post.
//
// A token's output count is its byte length, which one lane per sentence
// cannot balance (one line of unknown chars is tens of thousands of outputs),
// so the work is laid out over the model tokens of the batch as in
// decode_kernels.hip (token_tiles.h): every pass runs kDecodeBlocks blocks
// over contiguous token ranges, one token per thread and sub-tile.
//
//   count pass  : per block, the sum of the output counts (len for an UNKNOWN
//                 token, 1 otherwise) and of the normalized bytes consumed.
//   offset pass : block prefix + sub-tile scans; the first token of every
//                 sentence writes out_off[sentence].
//   fill pass   : out_off of the sentences without tokens and out_off[n]; sets
//                 RESOURCE_EXHAUSTED when the ids do not fit.
//   write pass  : the same scans; a sub-tile's outputs are written with one
//                 output per lane (the token of output o by binary search over
//                 the sub-tile's scanned counts), so a wave stores 64
//                 consecutive ids.  A byte output reads its byte from the
//                 normalized text and maps it through byte_ids.
//   extras pass : the bos/eos ids of every sentence.
//
// A token's bytes start at norm_off[0] + (bytes consumed by the tokens before
// it): the tokens of a sentence consume exactly its normalized bytes.  Reads
// of the text are clamped to the token's sentence, so token lengths that break
// that contract cannot lead a read outside the buffers.
//
// No pass writes once the call's status word is non-zero.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "epilogue.h"
#include "token_tiles.h"

namespace spm_amd {
namespace {

struct TokCount {
  uint32_t out;  // outputs of the token
  uint32_t adv;  // normalized bytes it consumes
  bool unk;
};

__device__ __forceinline__ TokCount CountOf(const ByteEpilogueLaunch &a, uint64_t k) {
  const int32_t id = a.ids[k];
  const uint32_t len = a.len[k];
  const uint8_t t = (id >= 0 && id < a.num_types) ? a.types[id] : 0;
  TokCount c;
  c.unk = (t & kPieceUnknown) != 0;
  c.out = c.unk ? len : 1u;
  c.adv = (t & kPieceControl) ? 0u : len;
  return c;
}

__global__ __launch_bounds__(256) void bf_count_kernel(ByteEpilogueLaunch a) {
  __shared__ uint64_t s_w[4];
  if (*a.chain) return;
  TokView v{a.ids, a.tok_off, a.n, a.tok_off[0], 0};
  const Range r = BlockRange(v);
  uint64_t out = 0, adv = 0;
  for (uint64_t g = r.begin + threadIdx.x; g < r.end; g += kDecodeSubTile) {
    const TokCount c = CountOf(a, v.base + g);
    out += c.out;
    adv += c.adv;
  }
  out = BlockSum64(out, s_w);
  adv = BlockSum64(adv, s_w);
  if (threadIdx.x == 0) {
    a.block_sum[blockIdx.x] = out;
    a.block_sum[kDecodeBlocks + blockIdx.x] = adv;
  }
}

// Sums of block_sum[0, blockIdx.x) and of all of it, for both halves.
__device__ __forceinline__ void BlockPrefix(const ByteEpilogueLaunch &a, uint64_t *s_w, uint64_t *out_before,
                                            uint64_t *adv_before, uint64_t *out_all) {
  uint64_t ob = 0, ab = 0, oa = 0;
  for (uint32_t k = threadIdx.x; k < gridDim.x; k += blockDim.x) {
    const uint64_t o = a.block_sum[k];
    oa += o;
    if (k < blockIdx.x) {
      ob += o;
      ab += a.block_sum[kDecodeBlocks + k];
    }
  }
  *out_before = BlockSum64(ob, s_w);
  *adv_before = BlockSum64(ab, s_w);
  *out_all = BlockSum64(oa, s_w);
}

__global__ __launch_bounds__(256) void bf_offset_kernel(ByteEpilogueLaunch a) {
  __shared__ uint64_t s_w64[4];
  __shared__ uint32_t s_w[4];
  if (*a.chain) return;
  TokView v{a.ids, a.tok_off, a.n, a.tok_off[0], 0};
  const uint32_t extras = a.x.num_pre + a.x.num_post;
  uint64_t run, adv_unused, all;
  BlockPrefix(a, s_w64, &run, &adv_unused, &all);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[0] = all + a.n * extras;
  const Range r = BlockRange(v);
  uint64_t sent = 0;
  bool have = false;
  for (uint64_t s = r.begin; s < r.end; s += kDecodeSubTile) {
    const uint64_t g = s + threadIdx.x;
    const bool valid = g < r.end;
    uint32_t c = 0;
    if (valid) {
      sent = FindSentence(v, have ? sent : 0, v.n, g);
      have = true;
      c = CountOf(a, v.base + g).out;
    }
    uint32_t sub_total;
    const uint32_t excl = BlockExclusiveScan(c, s_w, &sub_total);
    if (valid && g == SentStart(v, sent)) a.out_off[sent] = run + excl + sent * extras;
    run += sub_total;
  }
}

__global__ __launch_bounds__(256) void bf_fill_kernel(ByteEpilogueLaunch a) {
  if (*a.chain) return;
  TokView v{a.ids, a.tok_off, a.n, a.tok_off[0], 0};
  const uint32_t extras = a.x.num_pre + a.x.num_post;
  const uint64_t total = a.ctl[0];
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= v.n; i += stride) {
    if (i == v.n) {
      a.out_off[i] = total;
      continue;
    }
    const uint64_t s0 = SentStart(v, i);
    if (SentStart(v, i + 1) != s0) continue;
    // Last index (n included) that starts at the same token: the next sentence
    // with tokens, whose offset the offset pass wrote, or the end.
    const uint64_t b = FindSentence(v, i, v.n + 1, s0);
    const uint64_t ids_before = b == v.n ? total - v.n * extras : a.out_off[b] - b * extras;
    a.out_off[i] = ids_before + i * extras;
  }
  // Last, so that the offsets above are there: the ids do not fit.
  if (a.check_capacity && total > a.capacity && blockIdx.x == 0 && threadIdx.x == 0)
    atomicCAS(a.chain, 0u, static_cast<uint32_t>(SPM_RESOURCE_EXHAUSTED));
}

__device__ __forceinline__ void Store(int32_t *out, uint64_t at, const spm_hip_piece &p) { out[at] = p.id; }
__device__ __forceinline__ void Store(spm_hip_piece *out, uint64_t at, const spm_hip_piece &p) { out[at] = p; }

// Out = int32_t: the ids.  Out = spm_hip_piece: SentencePieceText pieces with
// begin / end through norm_to_orig.
template <typename Out>
__global__ __launch_bounds__(256) void bf_write_kernel(ByteEpilogueLaunch a, Out *__restrict__ out) {
  constexpr bool kSpt = sizeof(Out) == sizeof(spm_hip_piece);
  __shared__ uint64_t s_w64[4];
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_start[kDecodeSubTile];
  __shared__ int32_t s_id[kDecodeSubTile];    // the token's id, ~byte count for an UNKNOWN token
  __shared__ uint64_t s_dst[kDecodeSubTile];  // where the token's first output goes
  __shared__ uint64_t s_byte[kDecodeSubTile];  // its first byte in norm
  __shared__ uint64_t s_sent[kDecodeSubTile];
  if (*a.chain) return;
  TokView v{a.ids, a.tok_off, a.n, a.tok_off[0], 0};
  const uint32_t extras = a.x.num_pre + a.x.num_post;
  const bool rev = a.x.reversed != 0;
  uint64_t run, byte_run, all;
  BlockPrefix(a, s_w64, &run, &byte_run, &all);
  byte_run += a.norm_off[0];
  const Range r = BlockRange(v);
  uint64_t sent = 0;
  bool have = false;
  for (uint64_t s = r.begin; s < r.end; s += kDecodeSubTile) {
    const uint64_t g = s + threadIdx.x;
    const bool valid = g < r.end;
    TokCount c{0, 0, false};
    if (valid) {
      sent = FindSentence(v, have ? sent : 0, v.n, g);
      have = true;
      c = CountOf(a, v.base + g);
    }
    uint32_t sub_total, sub_adv;
    const uint32_t excl = BlockExclusiveScan(c.out, s_w, &sub_total);
    const uint32_t excl_adv = BlockExclusiveScan(c.adv, s_w, &sub_adv);
    s_start[threadIdx.x] = excl;
    if (valid) {
      // Outputs of the tokens before this one, bos/eos ids not counted.
      const uint64_t before = run + excl;
      const uint64_t o0 = a.out_off[sent], o1 = a.out_off[sent + 1];
      // Forward: first output at o0 + num_pre + (before - ids before the
      // sentence).  Reversed: output j of the token goes to s_dst - j.
      const uint64_t local = before - (o0 - sent * extras);
      s_dst[threadIdx.x] = rev ? o1 - a.x.num_post - 1 - local : o0 + a.x.num_pre + local;
      s_id[threadIdx.x] = c.unk ? ~static_cast<int32_t>(c.out) : a.ids[v.base + g];
      s_byte[threadIdx.x] = byte_run + excl_adv;
      s_sent[threadIdx.x] = sent;
    }
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < sub_total; o += kDecodeSubTile) {
      // The token holding output o: the last one that starts at or before o.
      uint32_t lo = 0, hi = kDecodeSubTile;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_start[mid] <= o) lo = mid;
        else hi = mid;
      }
      const uint32_t j = o - s_start[lo];
      const uint64_t at = rev ? s_dst[lo] - j : s_dst[lo] + j;
      const int32_t tid = s_id[lo];
      const uint64_t i = s_sent[lo];
      const uint64_t n0 = a.norm_off[i], n1 = a.norm_off[i + 1];
      spm_hip_piece p{};
      if (tid < 0) {  // byte j of an UNKNOWN token of ~tid bytes
        uint64_t b = s_byte[lo] + j;
        if (b >= n1) b = n1 - 1;
        p.id = n1 > n0 ? a.byte_ids[a.norm[b]] : 0;
      } else {
        p.id = tid;
      }
      if (kSpt) {
        const uint32_t slen = static_cast<uint32_t>(n1 - n0);
        const uint32_t *n2o = a.n2o + n0 + i;
        uint32_t c0 = static_cast<uint32_t>(s_byte[lo] - n0);
        if (c0 > slen) c0 = slen;
        const bool is_unk = tid < 0;
        const bool control = !is_unk && tid < a.num_types && (a.types[tid] & kPieceControl) != 0;
        uint32_t tl = is_unk ? static_cast<uint32_t>(~tid) : a.len[v.base + s + lo];
        uint32_t c1 = c0 + tl;
        if (c1 > slen) c1 = slen;
        p.begin = n2o[c0];
        if (is_unk) {
          p.end = j + 1 == tl ? n2o[c1] : n2o[c0];
          p.norm_begin = p.norm_end = c0;  // piece = IdToPiece(id)
        } else {
          p.end = control ? n2o[c0] : n2o[c1];
          p.norm_begin = c0;
          p.norm_end = c1;
        }
      }
      Store(out, at, p);
    }
    __syncthreads();
    run += sub_total;
    byte_run += sub_adv;
  }
}

template <typename Out>
__global__ __launch_bounds__(256) void bf_extras_kernel(ByteEpilogueLaunch a, Out *__restrict__ out) {
  if (*a.chain) return;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const uint64_t o0 = a.out_off[i], o1 = a.out_off[i + 1];
    for (uint32_t k = 0; k < a.x.num_pre; ++k) Store(out, o0 + k, spm_hip_piece{a.x.ids[k], 0, 0, 0, 0});
    for (uint32_t k = 0; k < a.x.num_post; ++k)
      Store(out, o1 - a.x.num_post + k, spm_hip_piece{a.x.ids[kMaxExtras + k], 0, 0, 0, 0});
  }
}

}  // namespace

hipError_t LaunchByteEpilogueCount(const ByteEpilogueLaunch &a, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  const dim3 grid(kDecodeBlocks), block(kDecodeSubTile);
  hipLaunchKernelGGL(bf_count_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(bf_offset_kernel, grid, block, 0, st, a);
  const uint64_t fb = (a.n + 1 + 255) / 256;
  hipLaunchKernelGGL(bf_fill_kernel, dim3(static_cast<unsigned>(fb < 65536 ? fb : 65536)), block, 0, st, a);
  return hipGetLastError();
}

hipError_t LaunchByteEpilogueWrite(const ByteEpilogueLaunch &a, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  const dim3 grid(kDecodeBlocks), block(kDecodeSubTile);
  const uint64_t fb = (a.n + 255) / 256;
  const dim3 sgrid(static_cast<unsigned>(fb < 65536 ? fb : 65536));
  const bool extras = a.x.num_pre + a.x.num_post != 0;
  if (a.out_spt) {
    hipLaunchKernelGGL(bf_write_kernel<spm_hip_piece>, grid, block, 0, st, a, a.out_spt);
    if (extras) hipLaunchKernelGGL(bf_extras_kernel<spm_hip_piece>, sgrid, block, 0, st, a, a.out_spt);
  } else {
    hipLaunchKernelGGL(bf_write_kernel<int32_t>, grid, block, 0, st, a, a.out);
    if (extras) hipLaunchKernelGGL(bf_extras_kernel<int32_t>, sgrid, block, 0, st, a, a.out);
  }
  return hipGetLastError();
}

}  // namespace spm_amd
