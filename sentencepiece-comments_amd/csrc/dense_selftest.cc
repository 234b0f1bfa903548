// Self-test driver of SentencePieceProcessor::EncodeDense / SampleEncodeDense
// (tests/test_gpu_dense.py): dense_selftest MODEL OPTIONS ROW_LEN PAD_ID FLAGS
// MODE [LINE...], OPTIONS the encode extra options ("" for none), MODE one of
//   pad | pack : EncodeDense of the lines.  Prints "dense rows R row_len L
//                tokens T cut C dropped D", then per row "ids ...", and
//                "lengths ..." + per row "mask ..." (pad) or per row "seq ..."
//                and "pos ..." (pack), all read back from the device pointers
//                of the DenseBatch.
//   sample     : SetRandomSeed(12345), two SampleEncodeBatch(-1, 0.5) calls,
//                each printed as "batch" and per line "ids ..."; then
//                SetRandomSeed(12345) again and two SampleEncodeDense(-1, 0.5)
//                calls printed as under pad.
//   hostonly   : LoadHostOnly, then "code <EncodeDense status> <SampleEncodeDense status>".
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "processor.h"

namespace {

using spm_amd::SentencePieceProcessor;

template <typename T>
std::vector<T> Down(const T *d, uint64_t count) {
  std::vector<T> h(count);
  if (count && hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) {
    std::fprintf(stderr, "device read failed\n");
    std::exit(1);
  }
  return h;
}

template <typename T>
void PrintRows(const char *name, const std::vector<T> &v, uint64_t rows, uint64_t L) {
  for (uint64_t r = 0; r < rows; ++r) {
    std::printf("%s", name);
    for (uint64_t c = 0; c < L; ++c) std::printf(" %d", static_cast<int>(v[r * L + c]));
    std::printf("\n");
  }
}

void PrintDense(const SentencePieceProcessor::DenseBatch &b, const std::vector<int32_t> &ids, bool pack) {
  std::printf("dense rows %llu row_len %u tokens %llu cut %llu dropped %llu\n",
              static_cast<unsigned long long>(b.rows), b.row_len, static_cast<unsigned long long>(b.tokens),
              static_cast<unsigned long long>(b.cut), static_cast<unsigned long long>(b.dropped));
  const uint64_t L = b.row_len, slots = b.rows * L;
  PrintRows("ids", ids, b.rows, L);
  if (pack) {
    PrintRows("seq", Down(b.seq, slots), b.rows, L);
    PrintRows("pos", Down(b.pos, slots), b.rows, L);
  } else {
    PrintRows("lengths", Down(b.lengths, b.rows), 1, b.rows);
    PrintRows("mask", Down(b.mask, slots), b.rows, L);
  }
}

int Check(const spm_amd::Status &st) {
  if (st.ok()) return 0;
  std::fprintf(stderr, "%d %s\n", st.code, st.message.c_str());
  return 1;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: %s MODEL OPTIONS ROW_LEN PAD_ID FLAGS pad|pack|sample|hostonly [LINE...]\n", argv[0]);
    return 2;
  }
  SentencePieceProcessor::DenseOptions o;
  o.row_len = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
  o.pad_id = static_cast<int32_t>(std::strtol(argv[4], nullptr, 10));
  o.flags = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
  const std::string mode = argv[6];
  o.pack = mode == "pack";
  const std::vector<std::string> lines(argv + 7, argv + argc);
  SentencePieceProcessor sp;
  SentencePieceProcessor::DenseBatch b;
  std::vector<int32_t> ids;
  if (mode == "hostonly") {
    std::ifstream in(argv[1], std::ios::binary);
    const std::string proto((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (Check(sp.LoadHostOnly(proto))) return 1;
    std::printf("code %d %d\n", sp.EncodeDense(lines, o, &b, &ids).code,
                sp.SampleEncodeDense(lines, -1, 0.5f, o, &b, &ids).code);
    return 0;
  }
  if (Check(sp.Load(argv[1])) || Check(sp.SetEncodeExtraOptions(argv[2]))) return 1;
  if (mode == "pad" || mode == "pack") {
    if (Check(sp.EncodeDense(lines, o, &b, &ids))) return 1;
    PrintDense(b, ids, o.pack);
    return 0;
  }
  if (mode != "sample") return 2;
  sp.SetRandomSeed(12345);
  for (int call = 0; call < 2; ++call) {
    std::vector<std::vector<int>> rows;
    if (Check(sp.SampleEncodeBatch(lines, -1, 0.5f, &rows, nullptr))) return 1;
    std::printf("batch\n");
    for (const auto &row : rows) {
      std::printf("ids");
      for (int i : row) std::printf(" %d", i);
      std::printf("\n");
    }
  }
  sp.SetRandomSeed(12345);
  for (int call = 0; call < 2; ++call) {
    if (Check(sp.SampleEncodeDense(lines, -1, 0.5f, o, &b, &ids))) return 1;
    PrintDense(b, ids, false);
  }
  return 0;
}
