// Unigram NBestEncode kernels for gfx950 (MI355X): the n best segmentations
// of every sentence of a batch.
//
// Reference path: unigram::Model::NBestEncode (unigram_model.cc:729-753) =
// Lattice::SetSentence + Model::PopulateNodes (:535-604) + Lattice::NBest
// (:339-478): Viterbi fills every node's backtrace_score (strict >, the first
// left node wins), then A* runs from EOS.  A hypothesis is (node, next, fx,
// gx); a popped hypothesis pushes one child per node l ending at its node's
// position, in end_nodes_ order, with gx = fl(score[l] + gx_top) and fx =
// fl(backtrace_score[l] + gx_top); a popped BOS hypothesis is a result.  The
// agenda is the heap of nbest_heap.h, which moves its keys as libstdc++'s
// std::priority_queue does, so ties pop in the reference's order.  A path's
// score is the float sum of its node scores in sentence order from 0.0f, not
// fx.  nbest_size 1 is the Viterbi path itself (:347-349).
//
// unigram_nbest_kernel: one sentence per lane over all sentences or a device
// list, grid-strided.  The lane's slab holds the heap (8 bytes per entry),
// the hypothesis arena (node, next, gx: 12 bytes per entry) and the literal
// lattice of unigram_general_kernel (UnigramGeneralSlabBytes' layout: five
// per-position and seven per-node arrays).  A sentence longer than max_nb, a
// search that needs more than max_hyps hypotheses, or an agenda that reaches
// the reference's shrink threshold (kMaxAgendaSize) goes to the overflow
// list and leaves no output; the next tier (more scratch per lane, or the
// host implementation of host_nbest.h) runs it again from the start.
//
// Output: results wait as hypothesis indices (at the top of the heap array:
// live heap entries + results <= hypotheses) until the search is over, so a
// sentence that overflows half way has written nothing.  Then the lane counts
// its paths' tokens, claims that many staging entries with one atomic add,
// and writes the paths one after the other in result order: stage[i] = its
// first staging entry, npaths[i], and ntok / score of path k at [i * nbest +
// k].  LaunchNBestPathOffsets and LaunchNBestTokOffsets scan the counts into
// the two-level CSR offsets and LaunchNBestGather copies every sentence's
// block (its paths are contiguous in staging and in the output) to its place:
// the output is in sentence order whatever lane or tier ran a sentence.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

#include "device_common.h"
#include "kernels.h"
#include "nbest_heap.h"

namespace spm_amd {
namespace {

__global__ __launch_bounds__(64) void unigram_nbest_kernel(NBestLaunch a) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= a.lanes) return;
  const uint64_t nthreads = a.lanes;
  const uint64_t total = a.list ? *a.count : a.list_n;
  const int K = a.p.trie_results_size + 1;
  const uint32_t N = static_cast<uint32_t>(a.nbest);
  const uint32_t H = a.max_hyps;
  for (uint64_t j = tid; j < total; j += nthreads) {
    const uint32_t i = a.list ? a.list[j] : static_cast<uint32_t>(j);
    const uint64_t b0 = a.off[i];
    const uint32_t nb = static_cast<uint32_t>(a.off[i + 1] - b0);
    if (nb == 0) {  // one empty path of score 0 (:731-733)
      a.npaths[i] = 1;
      a.stage[i] = 0;
      a.path_ntok[static_cast<uint64_t>(i) * N] = 0;
      a.path_score[static_cast<uint64_t>(i) * N] = 0.f;
      continue;
    }
    if (nb > a.max_nb) {
      a.ovf_list[atomicAdd(a.ovf_count, 1u)] = i;
      continue;
    }
    const uint8_t *__restrict__ s = a.bytes + b0;
    uint8_t *slab = a.scratch + tid * a.slab_bytes;
    const uint32_t cap = nb * K + 2;
    // Slab carve: the search's arrays (sized by max_hyps), then the lattice.
    NBestKey *heap = reinterpret_cast<NBestKey *>(slab);
    int32_t *hnode = reinterpret_cast<int32_t *>(heap + H);
    int32_t *hnext = hnode + H;
    float *hgx = reinterpret_cast<float *>(hnext + H);
    uint32_t *cs = reinterpret_cast<uint32_t *>(hgx + H);  // nb + 1
    int32_t *end_head = reinterpret_cast<int32_t *>(cs + nb + 1);
    int32_t *end_tail = end_head + nb + 1;
    int32_t *bfirst = end_tail + nb + 1;
    int32_t *bcount = bfirst + nb + 1;
    float *nscore = reinterpret_cast<float *>(bcount + nb + 1);
    float *nbt = nscore + cap;
    int32_t *nid = reinterpret_cast<int32_t *>(nbt + cap);
    int32_t *nprev = nid + cap;
    int32_t *nnext = nprev + cap;  // next in its end list
    uint32_t *npos = reinterpret_cast<uint32_t *>(nnext + cap);
    uint32_t *nlen = npos + cap;

    // SetSentence (:147-187)
    uint32_t nc = 0;
    for (uint32_t q = 0; q < nb;) {
      cs[nc++] = q;
      const uint32_t cl = OneCharLenDev(s[q]);
      q += cl < nb - q ? cl : nb - q;
    }
    cs[nc] = nb;
    for (uint32_t p = 0; p <= nc; ++p) {
      end_head[p] = end_tail[p] = -1;
      bfirst[p] = bcount[p] = 0;
    }
    auto push_end = [&](uint32_t q, int32_t nd) {
      nnext[nd] = -1;
      if (end_tail[q] < 0) end_head[q] = nd;
      else nnext[end_tail[q]] = nd;
      end_tail[q] = nd;
    };
    auto init_node = [&](int32_t nd, uint32_t p, uint32_t len, int32_t id, float sc) {
      nscore[nd] = sc;
      nbt[nd] = 0.f;
      nid[nd] = id;
      nprev[nd] = -1;
      npos[nd] = p;
      nlen[nd] = len;
    };
    init_node(0, 0, 0, -1, 0.f);  // BOS: ends at 0
    push_end(0, 0);
    init_node(1, nc, 0, -1, 0.f);  // EOS: begins at nc
    int32_t nn = 2;
    bfirst[nc] = 1;
    bcount[nc] = 1;
    // PopulateNodes (:535-604)
    for (uint32_t p = 0; p < nc; ++p) {
      bfirst[p] = nn;
      bool single = false;
      uint32_t base = a.p.root_base, cpos = p;
      for (uint32_t q = cs[p]; q < nb; ++q) {
        const uint32_t c = s[q];
        if (c == 0) break;
        const uint32_t node = base ^ c;
        if (node >= a.num_units) break;
        const uint32_t u = a.units[node];
        if ((u & 0xFFu) != c) break;
        base = u >> 9;
        if (u & 0x100u) {
          while (cs[cpos] < q + 1) ++cpos;  // get_chars_length
          const uint32_t length = cpos - p;
          const int32_t v = a.values[node];
          const int32_t kind = v >> kKindShift;
          if (kind == kKindUnused) continue;
          if (nn >= static_cast<int32_t>(cap)) break;  // (the slab's bound; never reached)
          const int32_t nd = nn++;
          init_node(nd, p, length, v & kIdMask,
                    kind == kKindUserDefined ? UserDefinedScore(static_cast<int>(length), a.p.max_score)
                                             : a.scores[v & kIdMask]);
          push_end(p + length, nd);
          if (length == 1) single = true;
        }
      }
      if (!single && nn < static_cast<int32_t>(cap)) {
        const int32_t nd = nn++;
        init_node(nd, p, 1, a.p.unk_id, a.p.unk_score);
        push_end(p + 1, nd);
      }
      bcount[p] = nn - bfirst[p];
    }
    // Viterbi (:222-261)
    for (uint32_t p = 0; p <= nc; ++p)
      for (int32_t k = 0; k < bcount[p]; ++k) {
        const int32_t r = bfirst[p] + k;
        const float rs = nscore[r];
        int32_t best = -1;
        float best_score = 0.f;
        for (int32_t l = end_head[p]; l >= 0; l = nnext[l]) {
          const float sc = __fadd_rn(nbt[l], rs);
          if (best < 0 || sc > best_score) {
            best = l;
            best_score = sc;
          }
        }
        nprev[r] = best;
        nbt[r] = best_score;
      }

    const uint64_t row = static_cast<uint64_t>(i) * N;
    auto piece_bytes = [&](int32_t nd) { return cs[npos[nd] + nlen[nd]] - cs[npos[nd]]; };
    // Staging entries for `count` tokens; kNone64 when they do not fit (the
    // host sees the cursor beyond the capacity and runs the call again).
    auto claim = [&](uint64_t count) -> uint64_t {
      const uint64_t at = atomicAdd(a.stage_cursor, static_cast<unsigned long long>(count));
      a.stage[i] = at;
      return at + count <= a.stage_cap ? at : ~0ull;
    };

    if (N == 1) {  // {Viterbi()} (:347-349)
      // The path's forward links in nnext (the end lists are done with).
      uint32_t k = 0;
      int32_t first = 1;
      for (int32_t nd = nprev[1]; nd > 0 && k < nb; nd = nprev[nd]) {
        nnext[nd] = first;
        first = nd;
        ++k;
      }
      const uint64_t at = claim(k);
      float score = 0.f;
      uint32_t w = 0;
      for (int32_t nd = first; nd != 1 && w < k; nd = nnext[nd], ++w) {
        score = __fadd_rn(score, nscore[nd]);
        if (at != ~0ull) {
          a.stage_ids[at + w] = nid[nd];
          if (a.stage_len) a.stage_len[at + w] = piece_bytes(nd);
        }
      }
      a.path_ntok[row] = k;
      a.path_score[row] = score;
      a.npaths[i] = 1;
      continue;
    }

    // A* from EOS (:398-475).
    uint32_t hn = 0, hs = 0, results = 0;
    bool overflow = false;
    hnode[0] = 1;
    hnext[0] = -1;
    hgx[0] = nscore[1];
    hn = 1;
    NBestPush(heap, &hs, NBestKey{nscore[1], 0});
    while (hs > 0) {
      const int32_t top = NBestPop(heap, &hs).hyp;
      const int32_t tn = hnode[top];
      if (tn == 0) {  // BOS: a result, kept above the live heap
        heap[H - 1 - results].hyp = top;
        if (++results == N) break;
        continue;
      }
      const float gx = hgx[top];
      for (int32_t l = end_head[npos[tn]]; l >= 0; l = nnext[l]) {
        if (hn >= H) {
          overflow = true;
          break;
        }
        hnode[hn] = l;
        hnext[hn] = top;
        hgx[hn] = __fadd_rn(nscore[l], gx);
        NBestPush(heap, &hs, NBestKey{__fadd_rn(nbt[l], gx), static_cast<int32_t>(hn)});
        ++hn;
      }
      // The reference shrinks its agenda here (:464-474): the host's case.
      if (overflow || hs >= kNBestMaxAgenda) {
        overflow = true;
        break;
      }
    }
    if (overflow) {
      a.ovf_list[atomicAdd(a.ovf_count, 1u)] = i;
      continue;
    }
    // Results (:430-439): the chain from a BOS hypothesis runs in sentence
    // order; its last hypothesis (EOS, next = -1) is not part of the path.
    uint64_t tokens = 0;
    for (uint32_t r = 0; r < results; ++r) {
      uint32_t k = 0;
      for (int32_t h = hnext[heap[H - 1 - r].hyp]; hnext[h] != -1; h = hnext[h]) ++k;
      a.path_ntok[row + r] = k;
      tokens += k;
    }
    uint64_t at = claim(tokens);
    for (uint32_t r = 0; r < results; ++r) {
      float score = 0.f;
      for (int32_t h = hnext[heap[H - 1 - r].hyp]; hnext[h] != -1; h = hnext[h]) {
        const int32_t nd = hnode[h];
        score = __fadd_rn(score, nscore[nd]);
        if (at != ~0ull) {
          a.stage_ids[at] = nid[nd];
          if (a.stage_len) a.stage_len[at] = piece_bytes(nd);
          ++at;
        }
      }
      a.path_score[row + r] = score;
    }
    a.npaths[i] = results;
  }
}

struct NBestToU64 {
  __host__ __device__ uint64_t operator()(uint32_t x) const { return x; }
};

// ptok[path_off[i] + k] = path_ntok[i * nbest + k]: the per-path token counts
// in output order.
__global__ __launch_bounds__(256) void nbest_flatten_kernel(uint64_t n, uint32_t nbest, const uint32_t *npaths,
                                                            const uint64_t *path_off, const uint32_t *path_ntok,
                                                            uint32_t *ptok) {
  const uint64_t slots = n * nbest;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < slots;
       t += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
    const uint64_t i = t / nbest;
    const uint32_t k = static_cast<uint32_t>(t - i * nbest);
    if (k < npaths[i]) ptok[path_off[i] + k] = path_ntok[t];
  }
}

// One wavefront per sentence: its staged block to ids / piece_len at
// tok_off[path_off[i]], its scores to scores[path_off[i] ..].
__global__ __launch_bounds__(256) void nbest_gather_kernel(NBestGather g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (blockDim.x / 64);
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * (blockDim.x / 64) + threadIdx.x / 64; i < g.n; i += waves) {
    const uint64_t p0 = g.path_off[i], p1 = g.path_off[i + 1];
    const uint64_t t0 = g.tok_off[p0], t1 = g.tok_off[p1];
    const uint64_t st = g.stage[i];
    const bool from_host = (st & kNBestHostStage) != 0;
    const int32_t *src_ids = (from_host ? g.host_ids : g.stage_ids) + (st & ~kNBestHostStage);
    for (uint64_t t = lane; t < t1 - t0; t += 64) g.ids[t0 + t] = src_ids[t];
    if (g.piece_len) {
      const uint32_t *src_len = (from_host ? g.host_len : g.stage_len) + (st & ~kNBestHostStage);
      for (uint64_t t = lane; t < t1 - t0; t += 64) g.piece_len[t0 + t] = src_len[t];
    }
    for (uint64_t k = lane; k < p1 - p0; k += 64) g.scores[p0 + k] = g.path_score[i * g.nbest + k];
  }
}

}  // namespace

uint64_t UnigramNBestSlabBytes(uint32_t max_nb, int trie_results_size, uint32_t max_hyps) {
  const uint64_t b = static_cast<uint64_t>(max_hyps) * 20 + UnigramGeneralSlabBytes(max_nb, trie_results_size);
  return (b + 15) & ~15ull;
}

hipError_t LaunchUnigramNBest(const NBestLaunch &a, hipStream_t st) {
  const unsigned blocks = (a.lanes + 63) / 64;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(unigram_nbest_kernel, dim3(blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t LaunchNBestPathOffsets(const uint32_t *npaths, uint64_t n, uint64_t *path_off, void *tmp,
                                  size_t *tmp_bytes, hipStream_t st) {
  hipcub::TransformInputIterator<uint64_t, NBestToU64, const uint32_t *> in(npaths, NBestToU64());
  if (tmp == nullptr)
    return hipcub::DeviceScan::InclusiveSum(nullptr, *tmp_bytes, in, path_off + 1, static_cast<int>(n > 0 ? n : 1), st);
  hipError_t e = hipMemsetAsync(path_off, 0, sizeof(uint64_t), st);
  if (e != hipSuccess || n == 0) return e;
  return hipcub::DeviceScan::InclusiveSum(tmp, *tmp_bytes, in, path_off + 1, static_cast<int>(n), st);
}

hipError_t LaunchNBestTokOffsets(uint64_t n, uint32_t nbest, const uint32_t *npaths, const uint64_t *path_off,
                                 const uint32_t *path_ntok, uint64_t total_paths, uint32_t *ptok, uint64_t *tok_off,
                                 void *tmp, size_t *tmp_bytes, hipStream_t st) {
  hipcub::TransformInputIterator<uint64_t, NBestToU64, const uint32_t *> in(ptok, NBestToU64());
  if (tmp == nullptr)
    return hipcub::DeviceScan::InclusiveSum(nullptr, *tmp_bytes, in, tok_off + 1,
                                            static_cast<int>(total_paths > 0 ? total_paths : 1), st);
  hipError_t e = hipMemsetAsync(tok_off, 0, sizeof(uint64_t), st);
  if (e != hipSuccess || total_paths == 0) return e;
  const uint64_t g64 = (n * nbest + 255) / 256;
  hipLaunchKernelGGL(nbest_flatten_kernel, dim3(static_cast<unsigned>(g64 < 8192 ? g64 : 8192)), dim3(256), 0, st, n,
                     nbest, npaths, path_off, path_ntok, ptok);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipcub::DeviceScan::InclusiveSum(tmp, *tmp_bytes, in, tok_off + 1, static_cast<int>(total_paths), st);
}

hipError_t LaunchNBestGather(const NBestGather &g, hipStream_t st) {
  if (g.n == 0) return hipSuccess;
  const uint64_t g64 = (g.n + 3) / 4;
  hipLaunchKernelGGL(nbest_gather_kernel, dim3(static_cast<unsigned>(g64 < 16384 ? g64 : 16384)), dim3(256), 0, st, g);
  return hipGetLastError();
}

}  // namespace spm_amd
