// Self-test driver of the pruning step's host side (tests/
// test_prune_host_cpu.py).  CPU only: no device call.
//
//   prune_selftest prune LIST [INDEX...]
//     LIST holds one piece per line: the piece's bytes in hex, a space, its
//     float score's bits in hex.  Runs what the trainer runs for a piece the
//     device flags for the host (BuildDoubleArray over the list, HostLattice::
//     Build + NBest2 of the piece over its own string) on every piece, or on
//     the pieces INDEX..., and prints per piece
//       "<index> <keep> <hypotheses> <shrinks> <alternative ids...>"
//   prune_selftest plan V MAX_BYTES K [V MAX_BYTES K ...]
//     prints spm_hip_prune_nbest's launch plan for V pieces of at most
//     MAX_BYTES bytes with K nodes per position, one row per triple:
//       "<lanes> <slab bytes> <reserved bytes> <grid> <block>"
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "double_array.h"
#include "host_prune_nbest.h"

namespace {

int HexDigit(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

bool ReadList(const char *path, std::vector<std::string> *pieces, std::vector<float> *scores) {
  std::ifstream ifs(path);
  if (!ifs) return false;
  std::string line;
  while (std::getline(ifs, line)) {
    if (line.empty()) continue;
    const size_t sp = line.find(' ');
    if (sp == std::string::npos || sp % 2 != 0 || line.size() != sp + 9) return false;
    std::string piece;
    for (size_t q = 0; q < sp; q += 2) {
      const int hi = HexDigit(line[q]), lo = HexDigit(line[q + 1]);
      if (hi < 0 || lo < 0) return false;
      piece.push_back(static_cast<char>(hi << 4 | lo));
    }
    const uint32_t bits = static_cast<uint32_t>(std::strtoul(line.c_str() + sp + 1, nullptr, 16));
    float sc;
    std::memcpy(&sc, &bits, 4);
    pieces->push_back(piece);
    scores->push_back(sc);
  }
  return !pieces->empty();
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 3 && std::string(argv[1]) == "prune") {
    std::vector<std::string> pieces;
    std::vector<float> score;
    if (!ReadList(argv[2], &pieces, &score)) {
      std::fprintf(stderr, "%s: cannot read a piece list\n", argv[2]);
      return 1;
    }
    const size_t V = pieces.size();
    std::vector<std::pair<std::string, int32_t>> keys(V);
    float min_score = FLT_MAX;
    for (size_t i = 0; i < V; ++i) {
      keys[i] = {pieces[i], static_cast<int32_t>(i)};
      min_score = std::min(min_score, score[i]);
    }
    spm_amd::DoubleArray trie;
    std::string err;
    if (!spm_amd::BuildDoubleArray(keys, &trie, &err)) {
      std::fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
    std::vector<size_t> todo;
    for (int a = 3; a < argc; ++a) {
      const size_t i = static_cast<size_t>(std::strtoull(argv[a], nullptr, 10));
      if (i >= V) {
        std::fprintf(stderr, "index %s out of range\n", argv[a]);
        return 1;
      }
      todo.push_back(i);
    }
    if (todo.empty())
      for (size_t i = 0; i < V; ++i) todo.push_back(i);
    spm_amd::HostLattice L;
    std::vector<std::pair<int32_t, size_t>> res;
    for (size_t i : todo) {
      // PruneSentencePieces (unigram_model_trainer.cc:355-370), as the
      // trainer's host re-run decides it.
      L.Build(pieces[i], trie, score, min_score, &res);
      const auto nb = L.NBest2();
      int keep = 1;
      std::vector<int> alt;
      if (nb.size() == 1) {
        keep = 1;
      } else if (nb[0].size() >= 2) {
        keep = 0;
      } else if (nb[0].size() == 1) {
        keep = 1;
        for (int k : nb[1]) alt.push_back(L.nodes[k].id);
      }
      std::printf("%zu %d %llu %llu", i, keep, static_cast<unsigned long long>(L.hyps),
                  static_cast<unsigned long long>(L.shrinks));
      for (int id : alt) std::printf(" %d", id);
      std::printf("\n");
    }
    return 0;
  }
  if (argc >= 5 && (argc - 2) % 3 == 0 && std::string(argv[1]) == "plan") {
    for (int a = 2; a < argc; a += 3) {
      const uint64_t V = std::strtoull(argv[a], nullptr, 10);
      const uint32_t max_nb = static_cast<uint32_t>(std::strtoul(argv[a + 1], nullptr, 10));
      const int K = std::atoi(argv[a + 2]);
      const spm_amd::PruneNBestPlan p = spm_amd::PlanPruneNBest(V, std::max<uint32_t>(max_nb, 1), K);
      std::printf("%llu %llu %llu %u %u\n", static_cast<unsigned long long>(p.lanes),
                  static_cast<unsigned long long>(p.slab_bytes), static_cast<unsigned long long>(p.reserve_bytes),
                  p.grid, spm_amd::kPruneNBestBlock);
    }
    return 0;
  }
  std::fprintf(stderr, "usage: %s prune LIST [INDEX...] | plan V MAX_BYTES K [V MAX_BYTES K ...]\n", argv[0]);
  return 2;
}
