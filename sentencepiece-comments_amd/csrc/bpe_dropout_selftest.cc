// Self-test driver of SentencePieceProcessor::SampleEncode on a BPE model
// (tests/test_gpu_bpe_dropout_cli.py): bpe_dropout_selftest MODEL SEED LINE
// prints, one per output line, the ids of two successive SampleEncode(LINE,
// -1, 0.5) draws, the same two again after SetRandomSeed(SEED) is repeated,
// the pieces of a third replay's first draw, the ids of SampleEncode with
// nbest_size 5 after one more SetRandomSeed(SEED), the ids of SampleEncode
// with nbest_size 1 and of Encode, and the status code of nbest_size 513.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "processor.h"

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s MODEL SEED LINE\n", argv[0]);
    return 2;
  }
  spm_amd::SentencePieceProcessor sp;
  auto st = sp.Load(argv[1]);
  if (!st.ok()) {
    std::fprintf(stderr, "%s\n", st.message.c_str());
    return 1;
  }
  const uint64_t seed = std::strtoull(argv[2], nullptr, 10);
  const std::string line = argv[3];
  auto print_ids = [](const std::vector<int> &ids) {
    for (size_t k = 0; k < ids.size(); ++k) std::printf(k ? " %d" : "%d", ids[k]);
    std::printf("\n");
  };
  std::vector<int> ids;
  for (int round = 0; round < 2; ++round) {
    sp.SetRandomSeed(seed);
    for (int draw = 0; draw < 2; ++draw) {
      st = sp.SampleEncode(line, -1, 0.5f, &ids);
      if (!st.ok()) {
        std::fprintf(stderr, "%s\n", st.message.c_str());
        return 1;
      }
      print_ids(ids);
    }
  }
  sp.SetRandomSeed(seed);
  std::vector<std::string> pieces;
  st = sp.SampleEncode(line, -1, 0.5f, &pieces);
  if (!st.ok()) return 1;
  for (size_t k = 0; k < pieces.size(); ++k) std::printf(k ? " %s" : "%s", pieces[k].c_str());
  std::printf("\n");
  sp.SetRandomSeed(seed);
  if (!sp.SampleEncode(line, 5, 0.5f, &ids).ok()) return 1;
  print_ids(ids);
  if (!sp.SampleEncode(line, 1, 0.5f, &ids).ok()) return 1;
  print_ids(ids);
  if (!sp.Encode(line, &ids).ok()) return 1;
  print_ids(ids);
  std::printf("%d\n", sp.SampleEncode(line, 513, 0.5f, &ids).code);
  return 0;
}
