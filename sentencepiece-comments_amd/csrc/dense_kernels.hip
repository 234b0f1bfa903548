// Dense id batches on the device: final id CSR -> [rows, L] int32 (dense.h).
//
// Both kernels are laid out over the output slots, not over the sentences: a
// thread owns 4 consecutive slots of the flat output and a wave stores 1 KiB
// of consecutive ids whatever the sentence lengths are (the c2 batch has 4.4
// tokens per sentence; a thread or a wave per sentence would idle).  A quad
// is stored with one 16-byte store when the output base is 16-byte aligned
// (the quad's flat index is a multiple of 4 by construction, so L plays no
// part), else with scalar stores; the last quad of the output may be short.
// All indices are 64 bit.  No scratch, no atomics but the two of `stats`, LDS:
// the four words of the stats sum (pad), one word (pack).
//
//   pad : kDenseBlocks blocks stride over the n * L slots.  A thread divides
//         once (32 bit) for the row and column of its first quad and moves
//         from step to step by the stride's quotient and remainder, which the
//         host computed.  Walking its quad it reloads the sentence's bounds
//         when the column wraps.  The slot at column 0 writes the row's length
//         and counts the cut.
//   pack: the slot space is min(ceil(T / L), rows_capacity) * L, T read from
//         the offsets on the device; block b owns one contiguous range of it
//         (a multiple of kDenseTile).  Slot t < T holds ids[offsets[0] + t].
//         For seq / pos one thread finds the sentence of the range's first
//         slot (FindSentence from 0), every thread starts there and gallops
//         forward from the sentence of its previous slot, so a slot in the
//         same sentence costs one offset load.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense.h"
#include "token_tiles.h"

namespace spm_amd {
namespace {

__device__ __forceinline__ void StoreQuad(int32_t *__restrict__ p, uint64_t t, const int32_t v[4], uint32_t cnt,
                                          bool vec) {
  if (vec && cnt == 4) {
    *reinterpret_cast<int4 *>(p + t) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
    for (uint32_t j = 0; j < cnt; ++j) p[t + j] = v[j];
  }
}

__global__ __launch_bounds__(256) void dense_pad_kernel(const int32_t *__restrict__ ids,
                                                        const uint64_t *__restrict__ off, uint64_t n, uint32_t L,
                                                        int32_t pad_id, uint32_t flags, int32_t *__restrict__ out,
                                                        int32_t *__restrict__ lengths, uint8_t *__restrict__ mask,
                                                        uint64_t *__restrict__ stats, uint64_t stride_rows,
                                                        uint32_t stride_cols, bool vec_out, bool vec_mask) {
  __shared__ uint64_t s_w[4];
  const uint64_t total = n * L;
  const uint32_t first = (blockIdx.x * 256u + threadIdx.x) * 4u;  // < kDenseBlocks * kDenseTile
  uint64_t row = first / L;
  uint32_t col = first - static_cast<uint32_t>(row) * L;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDenseTile;
  uint64_t cut = 0, dropped = 0;
  for (uint64_t t = first; t < total; t += stride) {
    const uint32_t cnt = total - t < 4 ? static_cast<uint32_t>(total - t) : 4u;
    uint64_t r = row;
    uint32_t c = col;
    uint64_t b = off[r], len = off[r + 1] - b;
    int32_t v[4] = {pad_id, pad_id, pad_id, pad_id};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (j < cnt) {
        if (c == 0) {
          if (lengths) lengths[r] = static_cast<int32_t>(len < L ? len : L);
          if (len > L) {
            ++cut;
            dropped += len - L;
          }
        }
        const int64_t src = PadSlotSource(len, L, flags, c);
        if (src >= 0) {
          v[j] = ids[b + src];
          m |= 1u << (8 * j);
        }
        if (++c == L) {
          c = 0;
          if (++r < n) {
            b = off[r];
            len = off[r + 1] - b;
          }
        }
      }
    }
    StoreQuad(out, t, v, cnt, vec_out);
    if (mask) {
      if (vec_mask && cnt == 4) {
        *reinterpret_cast<uint32_t *>(mask + t) = m;
      } else {
        for (uint32_t j = 0; j < cnt; ++j) mask[t + j] = static_cast<uint8_t>(m >> (8 * j));
      }
    }
    row += stride_rows;
    col += stride_cols;  // < 2 * L <= 2^32 - 2
    if (col >= L) {
      col -= L;
      ++row;
    }
  }
  if (stats) {  // uniform: every thread of the block arrives
    cut = BlockSum64(cut, s_w);
    dropped = BlockSum64(dropped, s_w);
    if (threadIdx.x == 0 && cut) {
      atomicAdd(reinterpret_cast<unsigned long long *>(stats), static_cast<unsigned long long>(cut));
      atomicAdd(reinterpret_cast<unsigned long long *>(stats + 1), static_cast<unsigned long long>(dropped));
    }
  }
}

__global__ __launch_bounds__(256) void dense_pack_kernel(const int32_t *__restrict__ ids,
                                                         const uint64_t *__restrict__ off, uint64_t n, uint32_t L,
                                                         int32_t pad_id, uint64_t rows_cap, int32_t *__restrict__ out,
                                                         int32_t *__restrict__ seq, int32_t *__restrict__ pos,
                                                         uint64_t *__restrict__ stats, bool vec_out, bool vec_seq,
                                                         bool vec_pos) {
  __shared__ uint64_t s_edge;
  TokView v{ids, off, n, off[0], 0};
  const uint64_t tokens = SentStart(v, n);
  const uint64_t need = (tokens + L - 1) / L;
  const uint64_t total = (need < rows_cap ? need : rows_cap) * L;
  if (stats && blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = need;
    stats[1] = tokens;
  }
  uint64_t chunk = (total + gridDim.x - 1) / gridDim.x;
  chunk = (chunk + kDenseTile - 1) / kDenseTile * kDenseTile;
  uint64_t begin = static_cast<uint64_t>(blockIdx.x) * chunk, end = begin + chunk;
  if (begin > total) begin = total;
  if (end > total) end = total;
  if (begin >= end) return;  // uniform
  const bool walk = seq != nullptr || pos != nullptr;
  uint64_t sent = 0;
  if (walk) {
    if (threadIdx.x == 0) s_edge = begin < tokens ? FindSentence(v, 0, n, begin) : 0;
    __syncthreads();
    sent = s_edge;
  }
  for (uint64_t t = begin + threadIdx.x * 4u; t < end; t += kDenseTile) {
    const uint32_t cnt = end - t < 4 ? static_cast<uint32_t>(end - t) : 4u;
    int32_t id[4] = {pad_id, pad_id, pad_id, pad_id}, sq[4] = {-1, -1, -1, -1}, ps[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint64_t u = t + j;
      if (j < cnt && u < tokens) {
        id[j] = ids[v.base + u];
        if (walk) {
          sent = FindSentence(v, sent, n, u);
          const PackedSlot s = PackSlot(u, tokens, sent, SentStart(v, sent));
          sq[j] = s.seq;
          ps[j] = s.pos;
        }
      }
    }
    StoreQuad(out, t, id, cnt, vec_out);
    if (seq) StoreQuad(seq, t, sq, cnt, vec_seq);
    if (pos) StoreQuad(pos, t, ps, cnt, vec_pos);
  }
}

bool Aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

uint32_t GridFor(uint64_t slots) {
  const uint64_t tiles = (slots + kDenseTile - 1) / kDenseTile;
  return static_cast<uint32_t>(tiles < kDenseBlocks ? (tiles ? tiles : 1) : kDenseBlocks);
}

}  // namespace

hipError_t LaunchDensePad(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                          uint32_t flags, int32_t *out, int32_t *lengths, uint8_t *mask, uint64_t *stats,
                          hipStream_t st) {
  if (n == 0) return hipSuccess;
  const uint32_t grid = GridFor(n * L);
  const uint64_t stride = static_cast<uint64_t>(grid) * kDenseTile;
  hipLaunchKernelGGL(dense_pad_kernel, dim3(grid), dim3(256), 0, st, ids, off, n, L, pad_id, flags, out, lengths,
                     mask, stats, stride / L, static_cast<uint32_t>(stride % L), Aligned(out, 16), Aligned(mask, 4));
  return hipGetLastError();
}

hipError_t LaunchDensePack(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t L, int32_t pad_id,
                           uint64_t rows_cap, int32_t *out, int32_t *seq, int32_t *pos, uint64_t *stats,
                           hipStream_t st) {
  if (n == 0) return hipSuccess;
  // The token count is on the device only: a full grid, and a block whose
  // range is empty returns at once.
  hipLaunchKernelGGL(dense_pack_kernel, dim3(kDensePackBlocks), dim3(256), 0, st, ids, off, n, L, pad_id, rows_cap, out,
                     seq, pos, stats, Aligned(out, 16), Aligned(seq, 16), Aligned(pos, 16));
  return hipGetLastError();
}

}  // namespace spm_amd
