// Host implementation of unigram::Model::NBestEncode (unigram_model.cc:729-753
// over Lattice::NBest :339-478) on a loaded model's host tables: the third
// tier of spm_hip_nbest_encode_batch (sentences whose search outgrows the
// device arenas, the agenda shrink included) and the checker behind
// nbest_selftest.  Same lattice, same float operations and same heap moves
// (nbest_heap.h) as unigram_nbest_kernel.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_types.h"
#include "double_array.h"
#include "nbest_heap.h"
#include "normalizer.h"

namespace spm_amd {

struct HostNBestTables {
  const uint32_t *units;
  uint32_t num_units;
  const int32_t *values;  // id | kind << kKindShift at the leaves
  const float *scores;    // by piece id
  UnigramParams p;
};

struct HostNBestPath {
  std::vector<int32_t> ids;
  std::vector<uint32_t> lens;  // piece byte lengths
  float score = 0.f;           // left-to-right float sum of the node scores
};

struct HostNBestStats {
  uint64_t hyps = 0;        // hypotheses allocated
  uint64_t max_agenda = 0;  // largest agenda seen
  uint64_t shrinks = 0;
};

// The n best paths of normalized bytes s[0, nb).  shrink_at = kMaxAgendaSize
// of the reference (a parameter so tests reach the shrink on small inputs).
inline void HostNBest(const HostNBestTables &t, const uint8_t *s, uint32_t nb, int nbest_size,
                      uint32_t shrink_at, std::vector<HostNBestPath> *out, HostNBestStats *stats) {
  out->clear();
  if (stats) *stats = HostNBestStats{};
  if (nb == 0) {  // {{{}, 0.0}} (:731-733)
    out->emplace_back();
    return;
  }
  const int N = NBestClamp(nbest_size);
  // SetSentence (:147-187)
  std::vector<uint32_t> cs;
  for (uint32_t q = 0; q < nb;) {
    cs.push_back(q);
    const uint32_t cl = OneCharLen(s[q]);
    q += std::min(cl, nb - q);
  }
  const uint32_t nc = static_cast<uint32_t>(cs.size());
  cs.push_back(nb);
  struct Node {
    float score, bt;
    int32_t id, prev, next;  // next: in its end list
    uint32_t pos, len;
  };
  std::vector<Node> nodes;
  std::vector<int32_t> end_head(nc + 1, -1), end_tail(nc + 1, -1), bfirst(nc + 1, 0), bcount(nc + 1, 0);
  auto add = [&](uint32_t p, uint32_t len, int32_t id, float sc) {
    const int32_t nd = static_cast<int32_t>(nodes.size());
    nodes.push_back(Node{sc, 0.f, id, -1, -1, p, len});
    const uint32_t e = p + len;
    if (end_tail[e] < 0) end_head[e] = nd;
    else nodes[end_tail[e]].next = nd;
    end_tail[e] = nd;
  };
  add(0, 0, -1, 0.f);  // BOS: node 0, ends at 0
  nodes.push_back(Node{0.f, 0.f, -1, -1, -1, nc, 0});  // EOS: node 1, begins at nc
  bfirst[nc] = 1;
  bcount[nc] = 1;
  // PopulateNodes (:535-604)
  for (uint32_t p = 0; p < nc; ++p) {
    bfirst[p] = static_cast<int32_t>(nodes.size());
    bool single = false;
    uint32_t base = t.p.root_base, cpos = p;
    for (uint32_t q = cs[p]; q < nb; ++q) {
      const uint32_t c = s[q];
      if (c == 0) break;
      const uint32_t node = base ^ c;
      if (node >= t.num_units) break;
      const uint32_t u = t.units[node];
      if ((u & 0xFFu) != c) break;
      base = u >> 9;
      if (u & 0x100u) {
        while (cs[cpos] < q + 1) ++cpos;
        const uint32_t length = cpos - p;
        const int32_t v = t.values[node];
        const int32_t kind = v >> kKindShift;
        if (kind == kKindUnused) continue;
        const int32_t id = v & kIdMask;
        const float sc = kind == kKindUserDefined
                             ? static_cast<float>(static_cast<double>(static_cast<float>(length) * t.p.max_score) + 1.0)
                             : t.scores[id];
        add(p, length, id, sc);
        if (length == 1) single = true;
      }
    }
    if (!single) add(p, 1, t.p.unk_id, t.p.unk_score);
    bcount[p] = static_cast<int32_t>(nodes.size()) - bfirst[p];
  }
  // Viterbi (:222-261): strict >, the first left node wins.
  for (uint32_t p = 0; p <= nc; ++p)
    for (int32_t k = 0; k < bcount[p]; ++k) {
      Node &r = nodes[bfirst[p] + k];
      int32_t best = -1;
      float best_score = 0.f;
      for (int32_t l = end_head[p]; l >= 0; l = nodes[l].next) {
        const float sc = nodes[l].bt + r.score;
        if (best < 0 || sc > best_score) {
          best = l;
          best_score = sc;
        }
      }
      r.prev = best;
      r.bt = best_score;
    }
  auto emit = [&](const std::vector<int32_t> &path) {  // node indices in sentence order
    out->emplace_back();
    HostNBestPath &r = out->back();
    float score = 0.f;
    for (int32_t nd : path) {
      score = score + nodes[nd].score;
      r.ids.push_back(nodes[nd].id);
      r.lens.push_back(cs[nodes[nd].pos + nodes[nd].len] - cs[nodes[nd].pos]);
    }
    r.score = score;
  };
  std::vector<int32_t> path;
  if (N == 1) {  // {Viterbi()} (:347-349)
    for (int32_t nd = nodes[1].prev; nd > 0; nd = nodes[nd].prev) path.push_back(nd);
    std::reverse(path.begin(), path.end());
    emit(path);
    return;
  }
  // A* from EOS (:398-475).
  struct Hyp {
    int32_t node, next;
    float gx;
  };
  std::vector<Hyp> hyps;
  std::vector<NBestKey> heap(1);
  uint32_t hs = 0;
  auto push = [&](NBestKey k) {
    if (heap.size() < hs + 1u) heap.resize(2 * heap.size());
    NBestPush(heap.data(), &hs, k);
  };
  hyps.push_back(Hyp{1, -1, nodes[1].score});
  push(NBestKey{nodes[1].score, 0});
  uint64_t max_agenda = 1, shrinks = 0;
  while (hs > 0) {
    const int32_t top = NBestPop(heap.data(), &hs).hyp;
    const int32_t tn = hyps[top].node;
    if (tn == 0) {  // BOS: a result
      path.clear();
      for (int32_t h = hyps[top].next; hyps[h].next != -1; h = hyps[h].next) path.push_back(hyps[h].node);
      emit(path);
      if (static_cast<int>(out->size()) == N) break;
      continue;
    }
    const float gx = hyps[top].gx;
    for (int32_t l = end_head[nodes[tn].pos]; l >= 0; l = nodes[l].next) {
      const int32_t h = static_cast<int32_t>(hyps.size());
      hyps.push_back(Hyp{l, top, nodes[l].score + gx});
      push(NBestKey{nodes[l].bt + gx, h});
    }
    max_agenda = std::max<uint64_t>(max_agenda, hs);
    if (hs >= shrink_at) {  // (:464-474)
      ++shrinks;
      const uint32_t keep = std::min<uint32_t>(kNBestMinAgenda, static_cast<uint32_t>(N) * 10u);
      std::vector<NBestKey> kept(std::max<uint32_t>(keep, 1));
      uint32_t ks = 0;
      for (uint32_t i = 0; i < keep && hs > 0; ++i) NBestPush(kept.data(), &ks, NBestPop(heap.data(), &hs));
      heap.swap(kept);
      hs = ks;
    }
  }
  if (stats) {
    stats->hyps = hyps.size();
    stats->max_agenda = max_agenda;
    stats->shrinks = shrinks;
  }
}

}  // namespace spm_amd
