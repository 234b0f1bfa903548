// Self-test driver of the n-best search (tests/test_nbest_cpu.py, tests/
// test_gpu_nbest_cli.py).
//
//   nbest_selftest host MODEL N [SHRINK_AT] < normalized lines
//     CPU only: runs host_nbest.h (the batch call's third tier) on every line
//     over a host-only handle's tables and prints, per line,
//       "<paths> <hypotheses> <largest agenda> <shrinks>"
//     and then one row per path: the score's float bits in hex and the
//     path's id:byte-length tokens; on stderr, the time spent in the
//     search itself ("host_nbest: L lines in S s").
//   nbest_selftest proc MODEL N LINE
//     prints the status code of SentencePieceProcessor::NBestEncode.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "device_model.h"
#include "host_nbest.h"
#include "processor.h"

int main(int argc, char **argv) {
  if (argc >= 4 && std::string(argv[1]) == "host") {
    std::ifstream ifs(argv[2], std::ios::binary);
    if (!ifs) {
      std::fprintf(stderr, "%s: cannot open\n", argv[2]);
      return 1;
    }
    const std::string blob((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
    spm_hip_model *m = nullptr;
    if (spm_hip_model_load_host_only(blob.data(), blob.size(), &m) != SPM_OK) {
      std::fprintf(stderr, "%s\n", spm_hip_last_error());
      return 1;
    }
    if (m->model_type != spm_amd::kUnigram) {
      std::fprintf(stderr, "not a unigram model\n");
      return 1;
    }
    const int N = std::atoi(argv[3]);
    const uint32_t shrink_at = argc > 4 ? static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10))
                                        : spm_amd::kNBestMaxAgenda;
    const spm_amd::HostNBestTables t{m->trie.units.data(), static_cast<uint32_t>(m->trie.units.size()),
                                     m->trie.values.data(), m->host_scores.data(), m->up};
    std::vector<spm_amd::HostNBestPath> paths;
    spm_amd::HostNBestStats stats;
    std::string line;
    double seconds = 0.0;
    uint64_t lines = 0;
    while (std::getline(std::cin, line)) {
      const auto t0 = std::chrono::steady_clock::now();
      spm_amd::HostNBest(t, reinterpret_cast<const uint8_t *>(line.data()), static_cast<uint32_t>(line.size()), N,
                         shrink_at, &paths, &stats);
      seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      ++lines;
      std::printf("%zu %llu %llu %llu\n", paths.size(), static_cast<unsigned long long>(stats.hyps),
                  static_cast<unsigned long long>(stats.max_agenda), static_cast<unsigned long long>(stats.shrinks));
      for (const auto &p : paths) {
        uint32_t bits;
        std::memcpy(&bits, &p.score, 4);
        std::printf("%08x", bits);
        for (size_t k = 0; k < p.ids.size(); ++k) std::printf(" %d:%u", p.ids[k], p.lens[k]);
        std::printf("\n");
      }
    }
    std::fprintf(stderr, "host_nbest: %llu lines in %.6f s\n", static_cast<unsigned long long>(lines), seconds);
    spm_hip_model_free(m);
    return 0;
  }
  if (argc == 5 && std::string(argv[1]) == "proc") {
    spm_amd::SentencePieceProcessor sp;
    auto st = sp.Load(argv[2]);
    if (!st.ok()) {
      std::fprintf(stderr, "%s\n", st.message.c_str());
      return 1;
    }
    std::vector<std::vector<int>> ids;
    st = sp.NBestEncode(argv[4], std::atoi(argv[3]), &ids);
    std::printf("%d\n", st.code);
    return 0;
  }
  std::fprintf(stderr, "usage: %s host MODEL N [SHRINK_AT] < lines | proc MODEL N LINE\n", argv[0]);
  return 2;
}
