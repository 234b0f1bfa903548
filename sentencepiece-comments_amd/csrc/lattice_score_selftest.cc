// Self-test driver of SentencePieceProcessor::CalculateEntropy and
// SampleEncodeAndScore (tests/test_gpu_lattice_score.py):
//   lattice_score_selftest MODEL SEED ALPHA LINE...
// prints "entropy BITS" (the float's bits in hex) for every LINE from one
// batched call and again "entropy1 BITS" for the first LINE alone; then, for
// the first LINE, four blocks of three samples "ids BITS id id .." each:
// after SetRandomSeed(SEED), the next call, after SetRandomSeed(SEED) again
// (a replay of the first) and the pieces overload after a third reseed
// ("pieces BITS piece piece .."); last "wor CODE MESSAGE".  A call that fails
// prints "error NAME CODE MESSAGE" instead and ends the program with 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "processor.h"

namespace {
unsigned Bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s MODEL SEED ALPHA LINE...\n", argv[0]);
    return 2;
  }
  spm_amd::SentencePieceProcessor sp;
  auto st = sp.Load(argv[1]);
  if (!st.ok()) {
    std::fprintf(stderr, "%s\n", st.message.c_str());
    return 1;
  }
  const uint64_t seed = std::strtoull(argv[2], nullptr, 10);
  const float alpha = std::strtof(argv[3], nullptr);
  const std::vector<std::string> lines(argv + 4, argv + argc);
  std::vector<float> h;
  st = sp.CalculateEntropy(lines, alpha, &h);
  if (!st.ok()) {
    std::printf("error CalculateEntropy %d %s\n", st.code, st.message.c_str());
  } else {
    for (float x : h) std::printf("entropy %08x\n", Bits(x));
    float one = 0.f;
    if (!sp.CalculateEntropy(lines[0], alpha, &one).ok()) return 1;
    std::printf("entropy1 %08x\n", Bits(one));
  }
  std::vector<std::pair<std::vector<int>, float>> ids;
  for (int block = 0; block < 3; ++block) {
    if (block != 1) sp.SetRandomSeed(seed);
    st = sp.SampleEncodeAndScore(lines[0], 3, alpha, false, false, &ids);
    if (!st.ok()) {
      std::printf("error SampleEncodeAndScore %d %s\n", st.code, st.message.c_str());
      return 0;
    }
    for (const auto &row : ids) {
      std::printf("ids %08x", Bits(row.second));
      for (int id : row.first) std::printf(" %d", id);
      std::printf("\n");
    }
  }
  sp.SetRandomSeed(seed);
  std::vector<std::pair<std::vector<std::string>, float>> pieces;
  if (!sp.SampleEncodeAndScore(lines[0], 3, alpha, false, false, &pieces).ok()) return 1;
  for (const auto &row : pieces) {
    std::printf("pieces %08x", Bits(row.second));
    for (const auto &p : row.first) std::printf(" %s", p.c_str());
    std::printf("\n");
  }
  st = sp.SampleEncodeAndScore(lines[0], 3, alpha, true, false, &ids);
  std::printf("wor %d %s\n", st.code, st.message.c_str());
  return 0;
}
