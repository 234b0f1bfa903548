// Host side of the pruning step's NBest(2) (unigram_model_trainer.cc:348-371):
// the lattice the trainer re-runs for pieces whose A* search outgrew the
// device slab of spm_hip_prune_nbest, and that call's launch plan.  Host code
// only (csrc/trainer.cc, csrc/estep_kernels.hip's host half, csrc/
// prune_selftest.cc).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <queue>
#include <string>
#include <utility>
#include <vector>

#include "double_array.h"
#include "normalizer.h"

namespace spm_amd {

// Lattice (unigram_model.cc:147-261, NBest :339-477) + PopulateNodes
// (:535-604) with the TrainerModel quirks (unk_id 0, every piece NORMAL).
struct HostLattice {
  struct Node {
    int pos, length, id;
    float score, bt;
    int prev;
  };
  std::vector<Node> nodes;
  std::vector<std::vector<int>> begin_nodes, end_nodes;
  int len = 0;
  // Of the last NBest2(): hypotheses allocated (EOS included), agenda shrinks.
  uint64_t hyps = 0, shrinks = 0;

  void Build(const std::string &s, const DoubleArray &trie, const std::vector<float> &score,
             float min_score, std::vector<std::pair<int32_t, size_t>> *res) {
    std::vector<size_t> surface;
    for (size_t i = 0; i < s.size();) {
      surface.push_back(i);
      i += std::min<size_t>(OneCharLen(static_cast<uint8_t>(s[i])), s.size() - i);
    }
    surface.push_back(s.size());
    len = static_cast<int>(surface.size()) - 1;
    nodes.clear();
    begin_nodes.assign(len + 1, {});
    end_nodes.assign(len + 1, {});
    nodes.push_back({0, 0, -1, 0.f, 0.f, -1});    // BOS
    nodes.push_back({len, 0, -1, 0.f, 0.f, -1});  // EOS
    end_nodes[0].push_back(0);
    begin_nodes[len].push_back(1);
    const float unk_score = min_score - 10.0f;  // kUnkPenalty
    for (int b = 0; b < len; ++b) {
      trie.CommonPrefixSearch(s.data() + surface[b], s.size() - surface[b], res);
      bool has_single = false;
      for (auto &r : *res) {
        const size_t e = surface[b] + r.second;
        int c = b;
        while (surface[c] < e) ++c;
        const int length = c - b;
        Insert(b, length, r.first, score[r.first]);
        if (length == 1) has_single = true;
      }
      if (!has_single) Insert(b, 1, 0, unk_score);
    }
  }
  void Insert(int pos, int length, int id, float sc) {
    const int k = static_cast<int>(nodes.size());
    nodes.push_back({pos, length, id, sc, 0.f, -1});
    begin_nodes[pos].push_back(k);
    end_nodes[pos + length].push_back(k);
  }
  std::vector<int> Viterbi() {
    for (int pos = 0; pos <= len; ++pos)
      for (int r : begin_nodes[pos]) {
        int best = -1;
        float best_score = 0.f;
        for (int l : end_nodes[pos]) {
          const float sc = nodes[l].bt + nodes[r].score;
          if (best < 0 || sc > best_score) {
            best = l;
            best_score = sc;
          }
        }
        if (best < 0) return {};
        nodes[r].prev = best;
        nodes[r].bt = best_score;
      }
    std::vector<int> out;
    for (int k = nodes[begin_nodes[len][0]].prev; nodes[k].prev >= 0; k = nodes[k].prev)
      out.push_back(k);
    std::reverse(out.begin(), out.end());
    return out;
  }
  // A* n-best with the same std::priority_queue ordering as the reference.
  std::vector<std::vector<int>> NBest2() {
    struct Hyp {
      int node;
      Hyp *next;
      float fx, gx;
    };
    struct Cmp {
      bool operator()(Hyp *a, Hyp *b) const { return a->fx < b->fx; }
    };
    using Agenda = std::priority_queue<Hyp *, std::vector<Hyp *>, Cmp>;
    const size_t nbest_size = 2;
    std::deque<Hyp> pool;
    Agenda agenda;
    std::vector<std::vector<int>> results;
    const int eos = begin_nodes[len][0], bos = end_nodes[0][0];
    pool.push_back(Hyp{eos, nullptr, nodes[eos].score, nodes[eos].score});
    agenda.push(&pool.back());
    shrinks = 0;
    Viterbi();
    while (!agenda.empty()) {
      Hyp *top = agenda.top();
      agenda.pop();
      if (top->node == bos) {
        results.emplace_back();
        for (Hyp *h = top->next; h->next != nullptr; h = h->next) results.back().push_back(h->node);
        if (results.size() == nbest_size) break;
        continue;
      }
      for (int l : end_nodes[nodes[top->node].pos]) {
        pool.push_back(Hyp{l, top, nodes[l].bt + top->gx, nodes[l].score + top->gx});
        agenda.push(&pool.back());
      }
      if (agenda.size() >= 100000) {
        Agenda na;
        const int size = std::min<int>(512, static_cast<int>(nbest_size * 10));
        for (int i = 0; i < size; ++i) {
          na.push(agenda.top());
          agenda.pop();
        }
        agenda = std::move(na);
        ++shrinks;
      }
    }
    hyps = pool.size();
    return results;
  }
};

// Launch plan of spm_hip_prune_nbest: one lane per piece with a slab of its
// own, lanes striding over the pieces.  `lanes` lanes take pieces, each on
// slab `slab_bytes` wide; `reserve_bytes` is what the call reserves for them,
// and the grid's blocks of kPruneNBestBlock lanes cover them (a last block's
// lanes past `lanes` do nothing).
constexpr uint32_t kPruneNBestBlock = 64;
constexpr uint32_t kPruneNBestMaxHyps = 4096;
constexpr uint64_t kPruneNBestMaxLanes = 16384;
constexpr uint64_t kPruneNBestScratch = 1ull << 30;

inline uint64_t NBestSlab(uint32_t nb, int K, uint32_t max_hyps) {
  const uint64_t cap = static_cast<uint64_t>(nb) * K + 2;
  return ((static_cast<uint64_t>(nb) + 1) * 5 + cap * 7 + static_cast<uint64_t>(max_hyps) * 5) * 4 + 64;
}

struct PruneNBestPlan {
  uint64_t lanes, slab_bytes, reserve_bytes;
  uint32_t grid;
};

// V pieces of at most max_nb bytes, K = the trie's most prefix matches + 1.
// The scratch stays within kPruneNBestScratch unless one block's worth of
// slabs is already larger.
inline PruneNBestPlan PlanPruneNBest(uint64_t V, uint32_t max_nb, int K) {
  PruneNBestPlan p;
  p.slab_bytes = NBestSlab(max_nb, K, kPruneNBestMaxHyps);
  p.lanes = std::min<uint64_t>(std::max<uint64_t>(V, 1), kPruneNBestMaxLanes);
  while (p.lanes > kPruneNBestBlock && p.lanes * p.slab_bytes > kPruneNBestScratch) p.lanes /= 2;
  p.reserve_bytes = p.lanes * p.slab_bytes;
  p.grid = static_cast<uint32_t>((p.lanes + kPruneNBestBlock - 1) / kPruneNBestBlock);
  return p;
}

}  // namespace spm_amd
