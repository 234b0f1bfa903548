// Unigram SampleEncode kernels for gfx950 (MI355X): one segmentation per
// sentence drawn from the unigram lattice.
//
// Reference path: SentencePieceProcessor::SampleEncode with nbest_size < 0
// (sentencepiece_processor.cc:622-659) = Lattice::SetSentence + Model::
// PopulateNodes (unigram_model.cc:535-604) + Lattice::Sample (:488-526).
//
// Forward pass.  Lattice::Sample's alpha of a node is the LogSumExp, over the
// nodes l ending at the node's begin position in end_nodes_ order, of
// fl(theta * score(l)) + alpha(l).  It depends on the node's begin position
// alone, so one value A[p] per char position carries it: A[0] = 0 and
//   A[p] = LogSumExp over nodes (b, p), ascending b, of fl(theta * s) + A[b],
// the first term initialising A[p] (init mode).  end_nodes_[p] is filled in
// ascending begin order, so the orders agree.
//
// Backward pass.  From e = len: the candidates are the nodes ending at e in
// that same order, with weights
//   w_i = (float) exp((double) fl(fl(A[b_i] + fl(theta * s_i)) - A[e])),
// S = sum of the w_i in double; draw u picks the first i with
// u < (w_0 + .. + w_i) / S, else the last candidate (std::discrete_
// distribution over probs); the node becomes a token, e = b_i, until e = 0.
// Draw k of sentence g comes from the counter-based stream of sample_rng.h.
//
// Two tiers, the same float operations in the same order (bit-identical):
//   unigram_sample_fast_kernel — one sentence per lane, no node lists.  The
//     forward pass walks the trie from every char start in ascending order
//     and folds each node into A[e] as it is met (ascending begin order at
//     every e); besides A[e] it keeps a 64-bit mask of the byte distances
//     e - b that have a node, so the backward pass walks the trie again only
//     for the begins that do have a node ending at e.  Candidate weights and
//     ids wait in LDS (kCand per lane) between the sum and the pick.  A
//     sentence with a node of more than 64 bytes, a trie leaf inside a UTF-8
//     char, more than kCand nodes ending at one position or an inconsistent
//     mask is flagged for the exact tier.
//   unigram_sample_exact_kernel — the literal lattice of
//     unigram_general_kernel (node lists, end_nodes_ chains), alpha stored
//     per node, the same draw.
// Every backward step checks begin < end: a violation flags the sentence
// (fast tier) or sets the error word (exact tier), so a bad value can never
// spin a wave.
//
// Output: tokens right-aligned in the sentence's own byte range of slot_ids /
// slot_len and the count in ntok[i], the contract of unigram_general_kernel;
// LaunchCompact (compact.hip) scans the counts and packs them.  The walk is
// not run twice to count first (the Viterbi kernel's tile-dense slots need
// that): a second backward pass would repeat every fp64 exp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_common.h"
#include "kernels.h"
#include "sample_rng.h"

namespace spm_amd {
namespace {

constexpr int kSampleBlock = 256;
constexpr int kCand = 16;           // fast tier: nodes ending at one position
constexpr uint32_t kMaxNodeBytes = 64;  // fast tier: the distance mask's width

// w_i of the header comment.
__device__ __forceinline__ float SampleWeight(float a_begin, float theta, float score, float a_end) {
  const float x = __fsub_rn(__fadd_rn(a_begin, __fmul_rn(theta, score)), a_end);
  return static_cast<float>(exp(static_cast<double>(x)));
}

// Index of the candidate draw u picks among weights w(0..nc-1) of sum S.
template <typename WeightAt>
__device__ __forceinline__ uint32_t SamplePick(uint32_t nc, double S, double u, WeightAt w) {
  double cum = 0.0;
  for (uint32_t i = 0; i + 1 < nc; ++i) {
    cum = __dadd_rn(cum, static_cast<double>(w(i)));
    if (u < cum / S) return i;
  }
  return nc - 1;
}

__global__ __launch_bounds__(kSampleBlock) void unigram_sample_fast_kernel(SampleFastArgs a) {
  __shared__ float lds_w[kCand * kSampleBlock];
  __shared__ int32_t lds_id[kCand * kSampleBlock];
  const int tid = threadIdx.x;
  const uint64_t total_bytes = a.off[a.n];
  // A batch larger than the caller's capacity (the workspace is sized by it).
  if (total_bytes > a.capacity) {
    if (blockIdx.x == 0 && tid == 0) atomicOr(&a.status[kStError], 2u);
    return;
  }
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSampleBlock + tid;
  if (i >= a.n) return;
  const uint64_t b0 = a.off[i];
  const uint32_t nb = static_cast<uint32_t>(a.off[i + 1] - b0);
  if (nb == 0) {
    a.ntok[i] = 0;
    return;
  }
  const uint8_t *__restrict__ s = a.bytes + b0;
  // Position q of sentence i: entry b0 + i + q (nb + 1 entries per sentence).
  float *__restrict__ A = a.A + b0 + i;
  uint64_t *__restrict__ M = a.M + b0 + i;  // zeroed by the launcher
  const float theta = a.theta;
  bool bad = false;

  auto fold = [&](uint32_t p, uint32_t e, float A0, float score) {
    const uint64_t m = M[e];
    const float t = __fadd_rn(__fmul_rn(theta, score), A0);
    const uint64_t m2 = m | (1ull << (e - p - 1));
    A[e] = LogSumExpDev(A[e], t, m == 0);
    M[e] = m2;
    // More nodes end here than the backward pass can hold: exact tier
    // (decided here, so it does not depend on the path that is drawn).
    if (__popcll(m2) > kCand) bad = true;
  };

  // ---- Forward pass: char starts by the lead-byte chain (OneCharLen clamped
  // to the sentence, unigram_model.cc:155-160).
  A[0] = 0.f;
  for (uint32_t p = 0; p < nb && !bad;) {
    const float A0 = A[p];
    uint32_t cl = OneCharLenDev(s[p]);
    if (cl > nb - p) cl = nb - p;
    uint32_t base = a.p.root_base, rem = 0, chars = 0;
    bool single = false;
    // The position's first eight bytes with independent loads (zero past the
    // sentence: a NUL ends the walk as the sentence's end does), so most
    // walks wait for one trie gather per step, not for a byte load as well.
    uint64_t win = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t)
      if (p + t < nb) win |= static_cast<uint64_t>(s[p + t]) << (8 * t);
    for (uint32_t q = p; q < nb; ++q) {
      const uint32_t c = q - p < 8 ? static_cast<uint32_t>(win >> (8 * (q - p))) & 0xFFu : s[q];
      if (c == 0) break;
      if (rem == 0) {
        rem = OneCharLenDev(c);
        if (rem > nb - q) rem = nb - q;
      }
      const uint32_t node = base ^ c;
      if (node >= a.num_units) break;
      const uint32_t u = a.units[node];
      if ((u & 0xFFu) != c) break;
      // A walk that is still alive past the mask's width: exact tier.
      if (q - p >= kMaxNodeBytes) {
        bad = true;
        break;
      }
      base = u >> 9;
      if (--rem == 0) ++chars;
      if (u & 0x100u) {
        if (rem != 0) {  // a leaf inside a UTF-8 char: exact tier
          bad = true;
          break;
        }
        const int32_t v = a.values[node];
        const int32_t kind = v >> kKindShift;
        if (kind == kKindUnused) continue;
        const float sc = kind == kKindUserDefined ? UserDefinedScore(static_cast<int>(chars), a.p.max_score)
                                                  : a.scores[v & kIdMask];
        fold(p, q + 1, A0, sc);
        if (chars == 1) single = true;
      }
    }
    // UNK node (unigram_model.cc:597-601) after this position's trie nodes.
    if (!single && !bad) fold(p, p + cl, A0, a.p.unk_score);
    p += cl;
  }

  // Node (b, e): the usable trie leaf of exactly these bytes, else UNK.
  auto node_of = [&](uint32_t b, uint32_t e, int32_t *id_out, float *sc_out) {
    uint32_t base = a.p.root_base, rem = 0, chars = 0, node = 0, u = 0;
    bool found = true;
    for (uint32_t q = b; q < e; ++q) {
      const uint32_t c = s[q];
      if (rem == 0) {
        rem = OneCharLenDev(c);
        if (rem > nb - q) rem = nb - q;
      }
      node = base ^ c;
      if (c == 0 || node >= a.num_units) {
        found = false;
        break;
      }
      u = a.units[node];
      if ((u & 0xFFu) != c) {
        found = false;
        break;
      }
      base = u >> 9;
      if (--rem == 0) ++chars;
    }
    int32_t id = a.p.unk_id;
    float sc = a.p.unk_score;
    if (found && (u & 0x100u)) {
      const int32_t v = a.values[node];
      const int32_t kind = v >> kKindShift;
      if (kind != kKindUnused) {
        id = v & kIdMask;
        sc = kind == kKindUserDefined ? UserDefinedScore(static_cast<int>(chars), a.p.max_score) : a.scores[id];
      }
    }
    *id_out = id;
    *sc_out = sc;
  };

  // ---- Backward pass.
  int32_t *__restrict__ out_id = a.slot_ids + b0 + nb;
  uint32_t *__restrict__ out_len = a.slot_len ? a.slot_len + b0 + nb : nullptr;
  const uint64_t key = SampleKey(a.seed, a.index_base + i);
  uint32_t e = nb, ntok = 0;
  uint64_t draw = 0;
  while (e > 0 && !bad) {
    const uint64_t m = M[e];
    const float Ae = A[e];
    // A distance beyond e, no node at all, or more tokens than bytes.
    if (m == 0 || (e < 64 && (m >> e) != 0) || ntok >= nb) {
      bad = true;
      break;
    }
    // Candidates in ascending begin = descending distance.
    uint32_t nc = 0;
    double S = 0.0;
    for (uint64_t mm = m; mm != 0;) {
      const uint32_t d = 64u - static_cast<uint32_t>(__clzll(static_cast<long long>(mm)));
      mm &= ~(1ull << (d - 1));
      if (nc >= kCand) {
        bad = true;
        break;
      }
      const uint32_t b = e - d;
      int32_t id;
      float sc;
      node_of(b, e, &id, &sc);
      const float w = SampleWeight(A[b], theta, sc, Ae);
      lds_w[nc * kSampleBlock + tid] = w;
      lds_id[nc * kSampleBlock + tid] = id;
      S = __dadd_rn(S, static_cast<double>(w));
      ++nc;
    }
    if (bad) break;
    const double u = SampleDraw(key, draw++);
    const uint32_t pick = SamplePick(nc, S, u, [&](uint32_t k) { return lds_w[k * kSampleBlock + tid]; });
    // The pick's distance: the (pick + 1)-th set bit of m from the top.
    uint64_t mm = m;
    uint32_t d = 0;
    for (uint32_t k = 0; k <= pick; ++k) {
      d = 64u - static_cast<uint32_t>(__clzll(static_cast<long long>(mm)));
      mm &= ~(1ull << (d - 1));
    }
    if (d == 0 || d > e) {  // begin < end at every step
      bad = true;
      break;
    }
    ++ntok;
    out_id[-static_cast<int64_t>(ntok)] = lds_id[pick * kSampleBlock + tid];
    if (out_len) out_len[-static_cast<int64_t>(ntok)] = d;
    e -= d;
  }
  if (bad) {
    const uint32_t fk = atomicAdd(&a.status[kStFlagged], 1u);
    a.flagged[fk] = static_cast<uint32_t>(i);
    atomicMax(&a.status[kStMaxNb], nb);
    a.ntok[i] = 0;
  } else {
    a.ntok[i] = ntok;
  }
}

// ---------------------------------------------------------------------------
// Exact tier: the reference Lattice literally (unigram_general_kernel's node
// lists and slab), alpha per node, the draw over end_nodes_ chains.
// One listed sentence per lane, scratch slab per lane.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void unigram_sample_exact_kernel(SampleExactArgs a) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= a.lanes) return;
  const uint64_t nthreads = a.lanes;
  const uint64_t total = a.list ? *a.count : a.list_n;
  const int K = a.p.trie_results_size + 1;
  const float theta = a.theta;
  for (uint64_t j = tid; j < total; j += nthreads) {
    const uint32_t i = a.list ? a.list[j] : static_cast<uint32_t>(j);
    const uint64_t b0 = a.off[i];
    const uint32_t nb = static_cast<uint32_t>(a.off[i + 1] - b0);
    if (nb == 0) {
      a.ntok[i] = 0;
      continue;
    }
    if (nb > a.max_nb) {
      if (a.ovf_list) {
        a.ovf_list[atomicAdd(a.ovf_count, 1u)] = i;
      } else {
        atomicOr(a.error, 1u);
        a.ntok[i] = 0;
      }
      continue;
    }
    const uint8_t *__restrict__ s = a.bytes + b0;
    uint8_t *slab = a.scratch + tid * a.slab_bytes;
    const uint32_t cap_nodes = nb * K + 2;
    // Slab carve (all 4-byte arrays; UnigramGeneralSlabBytes sizes it: five
    // per-position arrays and seven per-node arrays, of which six are used).
    uint32_t *cs = reinterpret_cast<uint32_t *>(slab);  // nb + 1
    int32_t *end_head = reinterpret_cast<int32_t *>(cs + nb + 1);
    int32_t *end_tail = end_head + nb + 1;
    float *nscore = reinterpret_cast<float *>(end_tail + 3 * (nb + 1));
    float *nalpha = nscore + cap_nodes;
    int32_t *nid = reinterpret_cast<int32_t *>(nalpha + cap_nodes);
    float *nw = reinterpret_cast<float *>(nid + cap_nodes);
    int32_t *nnext = reinterpret_cast<int32_t *>(nw + cap_nodes);  // next in end list
    uint32_t *npos = reinterpret_cast<uint32_t *>(nnext + cap_nodes);
    uint32_t *nlen = npos + cap_nodes;

    // SetSentence (:147-187)
    uint32_t nc = 0;
    for (uint32_t q = 0; q < nb;) {
      cs[nc++] = q;
      uint32_t cl = OneCharLenDev(s[q]);
      q += cl < nb - q ? cl : nb - q;
    }
    cs[nc] = nb;
    for (uint32_t p = 0; p <= nc; ++p) {
      end_head[p] = -1;
      end_tail[p] = -1;
    }
    auto push_end = [&](uint32_t q, int32_t nd) {
      nnext[nd] = -1;
      if (end_tail[q] < 0) end_head[q] = nd;
      else nnext[end_tail[q]] = nd;
      end_tail[q] = nd;
    };
    // BOS (node 0, ends at 0) and EOS (node 1, begins at nc).
    nscore[0] = 0.f; nalpha[0] = 0.f; nid[0] = -1; npos[0] = 0; nlen[0] = 0;
    push_end(0, 0);
    nscore[1] = 0.f; nalpha[1] = 0.f; nid[1] = -1; npos[1] = nc; nlen[1] = 0;
    int32_t nn = 2;
    // PopulateNodes (:535-604) with Lattice::Sample's alpha (:499-508): the
    // nodes ending at p are complete when position p is reached, so alpha of
    // the nodes beginning at p is taken first and stored with each of them.
    for (uint32_t p = 0; p <= nc; ++p) {
      float Ap = 0.f;  // BOS
      if (p > 0) {
        bool init = true;
        for (int32_t l = end_head[p]; l >= 0; l = nnext[l]) {
          Ap = LogSumExpDev(Ap, __fadd_rn(__fmul_rn(theta, nscore[l]), nalpha[l]), init);
          init = false;
        }
      }
      if (p == nc) {
        nalpha[1] = Ap;
        break;
      }
      bool single = false;
      uint32_t base = a.p.root_base;
      uint32_t cpos = p;  // char index reached by the walk
      for (uint32_t q = cs[p]; q < nb; ++q) {
        const uint32_t c = s[q];
        if (c == 0) break;
        const uint32_t node = base ^ c;
        if (node >= a.num_units) break;
        const uint32_t u = a.units[node];
        if ((u & 0xFFu) != c) break;
        base = u >> 9;
        if (u & 0x100u) {
          const uint32_t e = q + 1;
          while (cs[cpos] < e) ++cpos;  // get_chars_length
          const uint32_t length = cpos - p;
          const int32_t v = a.values[node];
          const int32_t kind = v >> kKindShift;
          if (kind == kKindUnused) continue;
          if (nn >= static_cast<int32_t>(cap_nodes)) break;  // (the slab's bound; never reached)
          const int32_t nd = nn++;
          nid[nd] = v & kIdMask;
          nscore[nd] = kind == kKindUserDefined ? UserDefinedScore(length, a.p.max_score)
                                                : a.scores[v & kIdMask];
          nalpha[nd] = Ap;
          npos[nd] = p;
          nlen[nd] = length;
          push_end(p + length, nd);
          if (length == 1) single = true;
        }
      }
      if (!single && nn < static_cast<int32_t>(cap_nodes)) {
        const int32_t nd = nn++;
        nid[nd] = a.p.unk_id;
        nscore[nd] = a.p.unk_score;
        nalpha[nd] = Ap;
        npos[nd] = p;
        nlen[nd] = 1;
        push_end(p + 1, nd);
      }
    }
    // Lattice::Sample's backward walk (:510-524).
    int32_t *__restrict__ out_id = a.slot_ids + b0 + nb;
    uint32_t *__restrict__ out_len = a.slot_len ? a.slot_len + b0 + nb : nullptr;
    const uint64_t key = SampleKey(a.seed, a.index_base + i);
    uint32_t e = nc, k = 0;
    float Ae = nalpha[1];
    uint64_t draw = 0;
    bool fail = false;
    while (e > 0) {
      uint32_t cands = 0;
      double S = 0.0;
      for (int32_t l = end_head[e]; l >= 0; l = nnext[l]) {
        const float w = SampleWeight(nalpha[l], theta, nscore[l], Ae);
        nw[l] = w;
        S = __dadd_rn(S, static_cast<double>(w));
        ++cands;
      }
      if (cands == 0 || k >= nb) {
        fail = true;
        break;
      }
      const double u = SampleDraw(key, draw++);
      int32_t cur = end_head[e];
      double cum = 0.0;
      while (nnext[cur] >= 0) {
        cum = __dadd_rn(cum, static_cast<double>(nw[cur]));
        if (u < cum / S) break;
        cur = nnext[cur];
      }
      if (npos[cur] >= e) {  // begin < end at every step
        fail = true;
        break;
      }
      ++k;
      out_id[-static_cast<int64_t>(k)] = nid[cur];
      if (out_len) out_len[-static_cast<int64_t>(k)] = cs[npos[cur] + nlen[cur]] - cs[npos[cur]];
      e = npos[cur];
      Ae = nalpha[cur];
    }
    if (fail) {
      atomicOr(a.error, 4u);
      k = 0;
    }
    a.ntok[i] = k;
  }
}

}  // namespace

hipError_t LaunchUnigramSampleFast(const SampleFastArgs &a, hipStream_t st) {
  const uint64_t blocks64 = FastTiles(a.n);
  if (blocks64 == 0) return hipSuccess;
  if (blocks64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
  // The distance masks start empty (an empty mask is also the init mode of
  // its position's LogSumExp).
  hipError_t e = hipMemsetAsync(a.M, 0, (a.capacity + a.n + 1) * sizeof(uint64_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(unigram_sample_fast_kernel, dim3(static_cast<unsigned>(blocks64)), dim3(kSampleBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t LaunchUnigramSampleExact(const SampleExactArgs &a, hipStream_t st) {
  const unsigned blocks = (a.lanes + 63) / 64;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(unigram_sample_exact_kernel, dim3(blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace spm_amd
