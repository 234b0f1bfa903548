// Unigram lattice scores for gfx950 (MI355X): the entropy of a sentence's
// segmentation distribution, and several drawn segmentations per sentence
// with their log-probabilities.
//
// Both stand on the sampler's forward pass (unigram_sample.hip): A[0] = 0 and
//   A[p] = LogSumExp over nodes (b, p), ascending b, of fl(theta * s) + A[b].
//
// Entropy.  One float H[p] per char position, H[0] = 0, accumulated over the
// nodes (b, p) in that same order:
//   lp   = fl(fl(fl(theta * s) + A[b]) - A[p])
//   H[p] = fl(H[p] + fl((float) exp((double) lp) * fl(H[b] + lp)));
// the entropy is -H[len] and the log partition A[len].
//
// Sample and score.  The forward pass once per sentence, then num_samples
// backward walks, each the sampler's walk under the key of its own sample
// (SampleSeedAt, sample_rng.h; sample 0 is SampleEncode's draw).  A walk's
// score is fl(T - A[len]) with T = 0, T = fl(T + fl(theta * s)) over its
// nodes from the first to the last, so the walk notes the node it chose at
// every begin position and the sum follows those notes forward.
//
// Two tiers each, the same float operations in the same order:
//   fast  — one sentence per lane, no node lists: trie walks from every char
//     start in ascending order fold each node into its end position as it is
//     met.  The entropy takes two such passes (A, then H: when begin b is
//     reached every node ending at b has been seen, so H[b] is final) and
//     needs no masks and no LDS; it flags only a trie leaf inside a UTF-8
//     char (two nodes of one span).  Sample and score keeps the sampler's
//     distance masks, holds the candidates' weights in LDS, and flags what
//     the sampler flags.
//   exact — the literal lattice of unigram_general_kernel (node lists,
//     end_nodes_ chains, UnigramGeneralSlabBytes' slab), alpha per node.
// Every backward step checks begin < end, as in the sampler.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

#include "device_common.h"
#include "kernels.h"
#include "sample_rng.h"

namespace spm_amd {
namespace {

constexpr int kScoreBlock = 256;
constexpr int kCand = 16;               // fast tier: nodes ending at one position
constexpr uint32_t kMaxNodeBytes = 64;  // fast tier: the distance mask's width
constexpr uint32_t kNoLimit = 0xFFFFFFFFu;
constexpr uint32_t kNoNode = 0xFFFFFFFFu;  // bits of an A entry no node has reached

struct Trie {
  const uint32_t *__restrict__ units;
  const int32_t *__restrict__ values;
  const float *__restrict__ scores;
  uint32_t num_units;
  UnigramParams p;
};

// w_i of the sampler.
__device__ __forceinline__ float SampleWeight(float a_begin, float theta, float score, float a_end) {
  const float x = __fsub_rn(__fadd_rn(a_begin, __fmul_rn(theta, score)), a_end);
  return static_cast<float>(exp(static_cast<double>(x)));
}

// One node's share of H at its end position.
__device__ __forceinline__ float EntropyFold(float h_end, float h_begin, float a_begin, float theta, float score,
                                             float a_end) {
  const float lp = __fsub_rn(__fadd_rn(__fmul_rn(theta, score), a_begin), a_end);
  const float w = static_cast<float>(exp(static_cast<double>(lp)));
  return __fadd_rn(h_end, __fmul_rn(w, __fadd_rn(h_begin, lp)));
}

// The nodes that begin at char start p (cl = the char's bytes), in
// PopulateNodes' order: node(e, score, id) for every usable trie leaf in
// ascending end e, then the UNK node when no leaf spans exactly one char.
// False: the fast tier cannot take the sentence (a leaf inside a UTF-8 char,
// or a walk still alive after max_bytes bytes).
template <typename F>
__device__ __forceinline__ bool NodesFrom(const Trie &t, const uint8_t *__restrict__ s, uint32_t nb, uint32_t p,
                                          uint32_t cl, uint32_t max_bytes, F &&node) {
  uint32_t base = t.p.root_base, rem = 0, chars = 0;
  bool single = false;
  // The position's first eight bytes with independent loads (zero past the
  // sentence: a NUL ends the walk as the sentence's end does).
  uint64_t win = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k)
    if (p + k < nb) win |= static_cast<uint64_t>(s[p + k]) << (8 * k);
  for (uint32_t q = p; q < nb; ++q) {
    const uint32_t c = q - p < 8 ? static_cast<uint32_t>(win >> (8 * (q - p))) & 0xFFu : s[q];
    if (c == 0) break;
    if (rem == 0) {
      rem = OneCharLenDev(c);
      if (rem > nb - q) rem = nb - q;
    }
    const uint32_t n = base ^ c;
    if (n >= t.num_units) break;
    const uint32_t u = t.units[n];
    if ((u & 0xFFu) != c) break;
    if (q - p >= max_bytes) return false;
    base = u >> 9;
    if (--rem == 0) ++chars;
    if (u & 0x100u) {
      if (rem != 0) return false;
      const int32_t v = t.values[n];
      const int32_t kind = v >> kKindShift;
      if (kind == kKindUnused) continue;
      const float sc = kind == kKindUserDefined ? UserDefinedScore(static_cast<int>(chars), t.p.max_score)
                                                : t.scores[v & kIdMask];
      node(q + 1, sc, v & kIdMask);
      if (chars == 1) single = true;
    }
  }
  if (!single) node(p + cl, t.p.unk_score, t.p.unk_id);
  return true;
}

__device__ __forceinline__ uint32_t CharLenAt(const uint8_t *__restrict__ s, uint32_t nb, uint32_t p) {
  const uint32_t cl = OneCharLenDev(s[p]);
  return cl > nb - p ? nb - p : cl;
}

__device__ __forceinline__ void FlagSentence(uint32_t *status, uint32_t *flagged, uint64_t i, uint32_t nb) {
  const uint32_t fk = atomicAdd(&status[kStFlagged], 1u);
  flagged[fk] = static_cast<uint32_t>(i);
  atomicMax(&status[kStMaxNb], nb);
}

// ---------------------------------------------------------------------------
// Entropy, fast tier.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kScoreBlock) void unigram_entropy_fast_kernel(EntropyFastArgs a) {
  const int tid = threadIdx.x;
  const uint64_t total_bytes = a.off[a.n];
  // A batch larger than the caller's capacity (the workspace is sized by it).
  if (total_bytes > a.capacity) {
    if (blockIdx.x == 0 && tid == 0) atomicOr(&a.status[kStError], 2u);
    return;
  }
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScoreBlock + tid;
  if (i >= a.n) return;
  const uint64_t b0 = a.off[i];
  const uint32_t nb = static_cast<uint32_t>(a.off[i + 1] - b0);
  if (nb == 0) {
    a.entropy[i] = -0.f;
    if (a.log_z) a.log_z[i] = 0.f;
    return;
  }
  const uint8_t *__restrict__ s = a.bytes + b0;
  // Position q of sentence i: entry b0 + i + q (nb + 1 entries per sentence).
  float *__restrict__ A = a.A + b0 + i;  // kNoNode everywhere (the launcher)
  float *__restrict__ H = a.H + b0 + i;  // zero everywhere
  const Trie t{a.units, a.values, a.scores, a.num_units, a.p};
  const float theta = a.theta;
  bool ok = true;

  // ---- Pass 1: A (the sampler's forward pass).
  A[0] = 0.f;
  for (uint32_t p = 0; p < nb && ok;) {
    const float A0 = A[p];
    const uint32_t cl = CharLenAt(s, nb, p);
    ok = NodesFrom(t, s, nb, p, cl, kNoLimit, [&](uint32_t e, float sc, int32_t) {
      const float cur = A[e];
      A[e] = LogSumExpDev(cur, __fadd_rn(__fmul_rn(theta, sc), A0), __float_as_uint(cur) == kNoNode);
    });
    p += cl;
  }
  // ---- Pass 2: H.
  for (uint32_t p = 0; p < nb && ok;) {
    const float A0 = A[p], H0 = H[p];
    const uint32_t cl = CharLenAt(s, nb, p);
    ok = NodesFrom(t, s, nb, p, cl, kNoLimit,
                   [&](uint32_t e, float sc, int32_t) { H[e] = EntropyFold(H[e], H0, A0, theta, sc, A[e]); });
    p += cl;
  }
  if (!ok) {
    FlagSentence(a.status, a.flagged, i, nb);
    return;
  }
  a.entropy[i] = -H[nb];
  if (a.log_z) a.log_z[i] = A[nb];
}

// ---------------------------------------------------------------------------
// The literal lattice (the sampler's exact tier): SetSentence + PopulateNodes
// with Lattice::Sample's alpha stored per node.
// ---------------------------------------------------------------------------
struct Slab {
  uint32_t *cs;        // nb + 1: byte offset of every char position
  int32_t *end_head;   // nb + 1
  int32_t *end_tail;   // nb + 1
  int32_t *pick;       // nb + 1: the node a walk chose at each begin position
  float *nscore;
  float *nalpha;       // A at the node's begin position
  int32_t *nid;
  float *nw;           // sampling: the step's weight; entropy: H at the node's begin position
  int32_t *nnext;      // next in the end list
  uint32_t *npos;
  uint32_t *nlen;
  uint32_t cap_nodes;
};

// UnigramGeneralSlabBytes' layout: five per-position and seven per-node arrays.
__device__ __forceinline__ Slab CarveSlab(uint8_t *slab, uint32_t nb, int K) {
  Slab l;
  l.cap_nodes = nb * K + 2;
  l.cs = reinterpret_cast<uint32_t *>(slab);
  l.end_head = reinterpret_cast<int32_t *>(l.cs + nb + 1);
  l.end_tail = l.end_head + nb + 1;
  l.pick = l.end_tail + nb + 1;
  l.nscore = reinterpret_cast<float *>(l.end_tail + 3 * (nb + 1));
  l.nalpha = l.nscore + l.cap_nodes;
  l.nid = reinterpret_cast<int32_t *>(l.nalpha + l.cap_nodes);
  l.nw = reinterpret_cast<float *>(l.nid + l.cap_nodes);
  l.nnext = reinterpret_cast<int32_t *>(l.nw + l.cap_nodes);
  l.npos = reinterpret_cast<uint32_t *>(l.nnext + l.cap_nodes);
  l.nlen = l.npos + l.cap_nodes;
  return l;
}

// Builds the lattice of s in l; returns the char count.  *a_len = A[len];
// kEntropy: H rides along (nw = H at the node's begin), *h_len = H[len].
template <bool kEntropy>
__device__ uint32_t BuildLattice(const Trie &t, const uint8_t *__restrict__ s, uint32_t nb, float theta, const Slab &l,
                                 float *a_len, float *h_len) {
  // SetSentence
  uint32_t nc = 0;
  for (uint32_t q = 0; q < nb;) {
    l.cs[nc++] = q;
    q += CharLenAt(s, nb, q);
  }
  l.cs[nc] = nb;
  for (uint32_t p = 0; p <= nc; ++p) {
    l.end_head[p] = -1;
    l.end_tail[p] = -1;
  }
  auto push_end = [&](uint32_t q, int32_t nd) {
    l.nnext[nd] = -1;
    if (l.end_tail[q] < 0) l.end_head[q] = nd;
    else l.nnext[l.end_tail[q]] = nd;
    l.end_tail[q] = nd;
  };
  // BOS (node 0, ends at 0) and EOS (node 1, begins at nc).
  l.nscore[0] = 0.f; l.nalpha[0] = 0.f; l.nid[0] = -1; l.npos[0] = 0; l.nlen[0] = 0; l.nw[0] = 0.f;
  push_end(0, 0);
  l.nscore[1] = 0.f; l.nalpha[1] = 0.f; l.nid[1] = -1; l.npos[1] = nc; l.nlen[1] = 0; l.nw[1] = 0.f;
  int32_t nn = 2;
  const int32_t cap = static_cast<int32_t>(l.cap_nodes);
  // PopulateNodes: the nodes ending at p are complete when position p is
  // reached, so A (and H) of p are taken first and stored with every node
  // that begins there.
  for (uint32_t p = 0; p <= nc; ++p) {
    float Ap = 0.f, Hp = 0.f;  // BOS
    if (p > 0) {
      bool init = true;
      for (int32_t n = l.end_head[p]; n >= 0; n = l.nnext[n]) {
        Ap = LogSumExpDev(Ap, __fadd_rn(__fmul_rn(theta, l.nscore[n]), l.nalpha[n]), init);
        init = false;
      }
      if constexpr (kEntropy) {
        for (int32_t n = l.end_head[p]; n >= 0; n = l.nnext[n])
          Hp = EntropyFold(Hp, l.nw[n], l.nalpha[n], theta, l.nscore[n], Ap);
      }
    }
    if (p == nc) {
      l.nalpha[1] = Ap;
      *a_len = Ap;
      *h_len = Hp;
      break;
    }
    bool single = false;
    uint32_t base = t.p.root_base;
    uint32_t cpos = p;  // char index reached by the walk
    for (uint32_t q = l.cs[p]; q < nb; ++q) {
      const uint32_t c = s[q];
      if (c == 0) break;
      const uint32_t n = base ^ c;
      if (n >= t.num_units) break;
      const uint32_t u = t.units[n];
      if ((u & 0xFFu) != c) break;
      base = u >> 9;
      if (u & 0x100u) {
        const uint32_t e = q + 1;
        while (l.cs[cpos] < e) ++cpos;  // get_chars_length
        const uint32_t length = cpos - p;
        const int32_t v = t.values[n];
        const int32_t kind = v >> kKindShift;
        if (kind == kKindUnused) continue;
        if (nn >= cap) break;  // (the slab's bound; never reached)
        const int32_t nd = nn++;
        l.nid[nd] = v & kIdMask;
        l.nscore[nd] = kind == kKindUserDefined ? UserDefinedScore(length, t.p.max_score) : t.scores[v & kIdMask];
        l.nalpha[nd] = Ap;
        l.nw[nd] = Hp;
        l.npos[nd] = p;
        l.nlen[nd] = length;
        push_end(p + length, nd);
        if (length == 1) single = true;
      }
    }
    if (!single && nn < cap) {
      const int32_t nd = nn++;
      l.nid[nd] = t.p.unk_id;
      l.nscore[nd] = t.p.unk_score;
      l.nalpha[nd] = Ap;
      l.nw[nd] = Hp;
      l.npos[nd] = p;
      l.nlen[nd] = 1;
      push_end(p + 1, nd);
    }
  }
  return nc;
}

// Entropy, exact tier: one listed sentence per lane, scratch slab per lane.
__global__ __launch_bounds__(64) void unigram_entropy_exact_kernel(EntropyExactArgs a) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= a.lanes) return;
  const uint64_t total = a.list ? *a.count : a.list_n;
  const Trie t{a.units, a.values, a.scores, a.num_units, a.p};
  for (uint64_t j = tid; j < total; j += a.lanes) {
    const uint32_t i = a.list ? a.list[j] : static_cast<uint32_t>(j);
    const uint64_t b0 = a.off[i];
    const uint32_t nb = static_cast<uint32_t>(a.off[i + 1] - b0);
    float A = 0.f, H = 0.f;
    if (nb > a.max_nb) {
      if (a.ovf_list) {
        a.ovf_list[atomicAdd(a.ovf_count, 1u)] = i;
        continue;
      }
      atomicOr(a.error, 1u);
    } else if (nb > 0) {
      const Slab l = CarveSlab(a.scratch + tid * a.slab_bytes, nb, a.p.trie_results_size + 1);
      BuildLattice<true>(t, a.bytes + b0, nb, a.theta, l, &A, &H);
    }
    a.entropy[i] = -H;
    if (a.log_z) a.log_z[i] = A;
  }
}

// ---------------------------------------------------------------------------
// Sample and score, fast tier: the sampler's fast kernel with num_samples
// backward walks.
// ---------------------------------------------------------------------------
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

__global__ __launch_bounds__(kScoreBlock) void unigram_score_fast_kernel(ScoreFastArgs sa) {
  __shared__ float lds_w[kCand * kScoreBlock];
  const SampleFastArgs &a = sa.s;
  const int tid = threadIdx.x;
  const uint64_t total_bytes = a.off[a.n];
  if (total_bytes > a.capacity) {
    if (blockIdx.x == 0 && tid == 0) atomicOr(&a.status[kStError], 2u);
    return;
  }
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScoreBlock + tid;
  if (i >= a.n) return;
  const uint64_t b0 = a.off[i];
  const uint32_t nb = static_cast<uint32_t>(a.off[i + 1] - b0);
  const uint32_t ns = sa.num_samples;
  const uint64_t row0 = i * ns;
  if (nb == 0) {
    for (uint32_t j = 0; j < ns; ++j) {
      a.ntok[row0 + j] = 0;
      sa.score[row0 + j] = 0.f;
    }
    return;
  }
  const uint8_t *__restrict__ s = a.bytes + b0;
  float *__restrict__ A = a.A + b0 + i;
  uint64_t *__restrict__ M = a.M + b0 + i;  // zeroed by the launcher
  uint64_t *__restrict__ X = sa.X + b0 + i;
  const Trie t{a.units, a.values, a.scores, a.num_units, a.p};
  const float theta = a.theta;
  bool bad = false;

  // ---- Forward pass (once).
  A[0] = 0.f;
  for (uint32_t p = 0; p < nb && !bad;) {
    const float A0 = A[p];
    const uint32_t cl = CharLenAt(s, nb, p);
    const bool ok = NodesFrom(t, s, nb, p, cl, kMaxNodeBytes, [&](uint32_t e, float sc, int32_t) {
      const uint64_t m = M[e];
      const uint64_t m2 = m | (1ull << (e - p - 1));
      A[e] = LogSumExpDev(A[e], __fadd_rn(__fmul_rn(theta, sc), A0), m == 0);
      M[e] = m2;
      // More nodes end here than the backward pass can hold: exact tier.
      if (__popcll(m2) > kCand) bad = true;
    });
    if (!ok) bad = true;
    p += cl;
  }

  // Node (b, e): the usable trie leaf of exactly these bytes, else UNK.
  auto node_of = [&](uint32_t b, uint32_t e, int32_t *id_out, float *sc_out) {
    uint32_t base = a.p.root_base, rem = 0, chars = 0, n = 0, u = 0;
    bool found = true;
    for (uint32_t q = b; q < e; ++q) {
      const uint32_t c = s[q];
      if (rem == 0) {
        rem = OneCharLenDev(c);
        if (rem > nb - q) rem = nb - q;
      }
      n = base ^ c;
      if (c == 0 || n >= a.num_units) {
        found = false;
        break;
      }
      u = a.units[n];
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
      const int32_t v = a.values[n];
      const int32_t kind = v >> kKindShift;
      if (kind != kKindUnused) {
        id = v & kIdMask;
        sc = kind == kKindUserDefined ? UserDefinedScore(static_cast<int>(chars), a.p.max_score) : a.scores[id];
      }
    }
    *id_out = id;
    *sc_out = sc;
  };

  // ---- Backward walks.
  const float Alen = A[nb];
  for (uint32_t j = 0; j < ns && !bad; ++j) {
    const uint64_t slot_end = static_cast<uint64_t>(ns) * b0 + static_cast<uint64_t>(j + 1) * nb;
    int32_t *__restrict__ out_id = a.slot_ids + slot_end;
    uint32_t *__restrict__ out_len = a.slot_len ? a.slot_len + slot_end : nullptr;
    const uint64_t key = SampleKey(SampleSeedAt(a.seed, j), a.index_base + i);
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
        lds_w[nc * kScoreBlock + tid] = w;
        S = __dadd_rn(S, static_cast<double>(w));
        ++nc;
      }
      if (bad) break;
      const double u = SampleDraw(key, draw++);
      const uint32_t pick = SamplePick(nc, S, u, [&](uint32_t k) { return lds_w[k * kScoreBlock + tid]; });
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
      // Only the weights wait in LDS: the chosen node is walked once more
      // for its id and score, which keeps the kernel's LDS at a third.
      int32_t id;
      float sc;
      node_of(e - d, e, &id, &sc);
      ++ntok;
      out_id[-static_cast<int64_t>(ntok)] = id;
      if (out_len) out_len[-static_cast<int64_t>(ntok)] = d;
      // The chosen node at its begin position: (its end, fl(theta * s)).
      X[e - d] = static_cast<uint64_t>(e) << 32 | __float_as_uint(__fmul_rn(theta, sc));
      e -= d;
    }
    if (bad) break;
    // The score, first node to last (at most ntok steps, each moving right).
    float T = 0.f;
    uint32_t p = 0;
    for (uint32_t k = 0; k < ntok && p < nb; ++k) {
      const uint64_t x = X[p];
      T = __fadd_rn(T, __uint_as_float(static_cast<uint32_t>(x)));
      const uint32_t nx = static_cast<uint32_t>(x >> 32);
      if (nx <= p || nx > nb) {
        bad = true;
        break;
      }
      p = nx;
    }
    if (bad) break;
    a.ntok[row0 + j] = ntok;
    sa.score[row0 + j] = __fsub_rn(T, Alen);
  }
  if (bad) {
    FlagSentence(a.status, a.flagged, i, nb);
    for (uint32_t j = 0; j < ns; ++j) a.ntok[row0 + j] = 0;
  }
}

// Sample and score, exact tier.
__global__ __launch_bounds__(64) void unigram_score_exact_kernel(ScoreExactArgs sa) {
  const SampleExactArgs &a = sa.s;
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= a.lanes) return;
  const uint64_t total = a.list ? *a.count : a.list_n;
  const Trie t{a.units, a.values, a.scores, a.num_units, a.p};
  const float theta = a.theta;
  const uint32_t ns = sa.num_samples;
  for (uint64_t jj = tid; jj < total; jj += a.lanes) {
    const uint32_t i = a.list ? a.list[jj] : static_cast<uint32_t>(jj);
    const uint64_t b0 = a.off[i];
    const uint32_t nb = static_cast<uint32_t>(a.off[i + 1] - b0);
    const uint64_t row0 = static_cast<uint64_t>(i) * ns;
    if (nb == 0 || (nb > a.max_nb && !a.ovf_list)) {
      if (nb) atomicOr(a.error, 1u);
      for (uint32_t j = 0; j < ns; ++j) {
        a.ntok[row0 + j] = 0;
        sa.score[row0 + j] = 0.f;
      }
      continue;
    }
    if (nb > a.max_nb) {
      a.ovf_list[atomicAdd(a.ovf_count, 1u)] = i;
      continue;
    }
    const uint8_t *__restrict__ s = a.bytes + b0;
    const Slab l = CarveSlab(a.scratch + tid * a.slab_bytes, nb, a.p.trie_results_size + 1);
    float Alen = 0.f, unused = 0.f;
    const uint32_t nc = BuildLattice<false>(t, s, nb, theta, l, &Alen, &unused);
    bool fail = false;
    for (uint32_t j = 0; j < ns && !fail; ++j) {
      // Lattice::Sample's backward walk.
      const uint64_t slot_end = static_cast<uint64_t>(ns) * b0 + static_cast<uint64_t>(j + 1) * nb;
      int32_t *__restrict__ out_id = a.slot_ids + slot_end;
      uint32_t *__restrict__ out_len = a.slot_len ? a.slot_len + slot_end : nullptr;
      const uint64_t key = SampleKey(SampleSeedAt(a.seed, j), a.index_base + i);
      uint32_t e = nc, k = 0;
      float Ae = Alen;
      uint64_t draw = 0;
      while (e > 0) {
        uint32_t cands = 0;
        double S = 0.0;
        for (int32_t n = l.end_head[e]; n >= 0; n = l.nnext[n]) {
          const float w = SampleWeight(l.nalpha[n], theta, l.nscore[n], Ae);
          l.nw[n] = w;
          S = __dadd_rn(S, static_cast<double>(w));
          ++cands;
        }
        if (cands == 0 || k >= nb) {
          fail = true;
          break;
        }
        const double u = SampleDraw(key, draw++);
        int32_t cur = l.end_head[e];
        double cum = 0.0;
        while (l.nnext[cur] >= 0) {
          cum = __dadd_rn(cum, static_cast<double>(l.nw[cur]));
          if (u < cum / S) break;
          cur = l.nnext[cur];
        }
        if (l.npos[cur] >= e) {  // begin < end at every step
          fail = true;
          break;
        }
        ++k;
        out_id[-static_cast<int64_t>(k)] = l.nid[cur];
        if (out_len) out_len[-static_cast<int64_t>(k)] = l.cs[l.npos[cur] + l.nlen[cur]] - l.cs[l.npos[cur]];
        e = l.npos[cur];
        l.pick[e] = cur;
        Ae = l.nalpha[cur];
      }
      if (fail) break;
      // The score, first node to last (k steps, each moving right).
      float T = 0.f;
      uint32_t p = 0;
      for (uint32_t q = 0; q < k && p < nc; ++q) {
        const int32_t nd = l.pick[p];
        T = __fadd_rn(T, __fmul_rn(theta, l.nscore[nd]));
        p = l.npos[nd] + l.nlen[nd];
      }
      a.ntok[row0 + j] = k;
      sa.score[row0 + j] = __fsub_rn(T, Alen);
    }
    if (fail) {
      atomicOr(a.error, 4u);
      for (uint32_t j = 0; j < ns; ++j) {
        a.ntok[row0 + j] = 0;
        sa.score[row0 + j] = 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Rows to dense CSR: row r = i * num_samples + j holds tok_off[r + 1] -
// tok_off[r] tokens, right-aligned before slot entry num_samples * off[i] +
// (j + 1) * nb.  One wave per 64 rows, as compact_kernel (compact.hip).
// ---------------------------------------------------------------------------
struct ToU64 {
  __host__ __device__ uint64_t operator()(uint32_t x) const { return x; }
};

__device__ __forceinline__ uint64_t ReadLane64(uint64_t v, uint32_t lane) {
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(lane)));
  const uint32_t hi =
      static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v >> 32), static_cast<int>(lane)));
  return static_cast<uint64_t>(hi) << 32 | lo;
}

__global__ __launch_bounds__(256) void score_gather_kernel(const uint64_t *__restrict__ off, uint64_t rows,
                                                           uint32_t ns, const int32_t *__restrict__ slot_ids,
                                                           const uint32_t *__restrict__ slot_len,
                                                           const uint64_t *__restrict__ tok_off,
                                                           int32_t *__restrict__ ids,
                                                           uint32_t *__restrict__ piece_len) {
  const int lane = threadIdx.x & 63;
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); g * 64 < rows;
       g += waves) {
    const uint64_t r = g * 64 + static_cast<uint64_t>(lane);
    uint64_t d0 = 0, k = 0, src = 0;
    if (r < rows) {
      const uint64_t i = r / ns, j = r % ns;
      const uint64_t b0 = off[i], nb = off[i + 1] - b0;
      d0 = tok_off[r];
      k = tok_off[r + 1] - d0;
      if (k > nb) k = nb;  // (a row never holds more tokens than bytes)
      src = ns * b0 + (j + 1) * nb - k;
    }
    const uint32_t m = rows - g * 64 < 64 ? static_cast<uint32_t>(rows - g * 64) : 64u;
    for (uint32_t q = 0; q < m; ++q) {
      const uint64_t sd0 = ReadLane64(d0, q), sk = ReadLane64(k, q), ssrc = ReadLane64(src, q);
      for (uint64_t x = static_cast<uint64_t>(lane); x < sk; x += 64) ids[sd0 + x] = slot_ids[ssrc + x];
      if (piece_len)
        for (uint64_t x = static_cast<uint64_t>(lane); x < sk; x += 64) piece_len[sd0 + x] = slot_len[ssrc + x];
    }
  }
}

}  // namespace

hipError_t LaunchUnigramEntropyFast(const EntropyFastArgs &a, hipStream_t st) {
  const uint64_t blocks64 = FastTiles(a.n);
  if (blocks64 == 0) return hipSuccess;
  if (blocks64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const size_t entries = a.capacity + a.n + 1;
  hipError_t e = hipMemsetAsync(a.A, 0xFF, entries * sizeof(float), st);  // kNoNode
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.H, 0, entries * sizeof(float), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(unigram_entropy_fast_kernel, dim3(static_cast<unsigned>(blocks64)), dim3(kScoreBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t LaunchUnigramEntropyExact(const EntropyExactArgs &a, hipStream_t st) {
  const unsigned blocks = (a.lanes + 63) / 64;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(unigram_entropy_exact_kernel, dim3(blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t LaunchUnigramScoreFast(const ScoreFastArgs &a, hipStream_t st) {
  const uint64_t blocks64 = FastTiles(a.s.n);
  if (blocks64 == 0) return hipSuccess;
  if (blocks64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
  // The distance masks start empty (an empty mask is also the init mode of
  // its position's LogSumExp).
  hipError_t e = hipMemsetAsync(a.s.M, 0, (a.s.capacity + a.s.n + 1) * sizeof(uint64_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(unigram_score_fast_kernel, dim3(static_cast<unsigned>(blocks64)), dim3(kScoreBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t LaunchUnigramScoreExact(const ScoreExactArgs &a, hipStream_t st) {
  const unsigned blocks = (a.s.lanes + 63) / 64;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(unigram_score_exact_kernel, dim3(blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t LaunchScoreScan(const uint32_t *ntok, uint64_t rows, uint64_t *tok_off, void *tmp, size_t *tmp_bytes,
                           hipStream_t st) {
  hipcub::TransformInputIterator<uint64_t, ToU64, const uint32_t *> in(ntok, ToU64());
  if (tmp == nullptr)
    return hipcub::DeviceScan::InclusiveSum(nullptr, *tmp_bytes, in, tok_off + 1, static_cast<int>(rows > 0 ? rows : 1),
                                            st);
  hipError_t e = hipMemsetAsync(tok_off, 0, sizeof(uint64_t), st);
  if (e != hipSuccess || rows == 0) return e;
  return hipcub::DeviceScan::InclusiveSum(tmp, *tmp_bytes, in, tok_off + 1, static_cast<int>(rows), st);
}

hipError_t LaunchScoreGather(const uint64_t *off, uint64_t n, uint32_t num_samples, const int32_t *slot_ids,
                             const uint32_t *slot_len, const uint64_t *tok_off, int32_t *ids, uint32_t *piece_len,
                             hipStream_t st) {
  const uint64_t rows = n * num_samples;
  if (rows == 0) return hipSuccess;
  const uint64_t g64 = (rows + 255) / 256;
  const unsigned grid = static_cast<unsigned>(g64 < 8192 ? g64 : 8192);
  hipLaunchKernelGGL(score_gather_kernel, dim3(grid), dim3(256), 0, st, off, rows, num_samples, slot_ids, slot_len,
                     tok_off, ids, piece_len);
  return hipGetLastError();
}

}  // namespace spm_amd
