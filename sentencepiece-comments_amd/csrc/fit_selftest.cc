// Self-test driver of SentencePieceProcessor::EncodeDense with pack and whole
// (tests/test_gpu_fit.py): fit_selftest MODEL OPTIONS ROW_LEN PAD_ID FLAGS
// [LINE...].  Prints "fit rows R row_len L tokens T cut C dropped D", then per
// row "ids ...", "seq ...", "pos ...", then "row_lengths ..." and "place ...",
// all read back from the device pointers of the DenseBatch.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "processor.h"

namespace {

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
    for (uint64_t c = 0; c < L; ++c) std::printf(" %lld", static_cast<long long>(v[r * L + c]));
    std::printf("\n");
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s MODEL OPTIONS ROW_LEN PAD_ID FLAGS [LINE...]\n", argv[0]);
    return 2;
  }
  using spm_amd::SentencePieceProcessor;
  SentencePieceProcessor::DenseOptions o;
  o.row_len = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
  o.pad_id = static_cast<int32_t>(std::strtol(argv[4], nullptr, 10));
  o.flags = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
  o.pack = o.whole = true;
  const std::vector<std::string> lines(argv + 6, argv + argc);
  SentencePieceProcessor sp;
  SentencePieceProcessor::DenseBatch b;
  std::vector<int32_t> ids;
  spm_amd::Status st = sp.Load(argv[1]);
  if (st.ok()) st = sp.SetEncodeExtraOptions(argv[2]);
  if (st.ok()) st = sp.EncodeDense(lines, o, &b, &ids);
  if (!st.ok()) {
    std::fprintf(stderr, "%d %s\n", st.code, st.message.c_str());
    return 1;
  }
  std::printf("fit rows %llu row_len %u tokens %llu cut %llu dropped %llu\n",
              static_cast<unsigned long long>(b.rows), b.row_len, static_cast<unsigned long long>(b.tokens),
              static_cast<unsigned long long>(b.cut), static_cast<unsigned long long>(b.dropped));
  const uint64_t L = b.row_len, slots = b.rows * L;
  PrintRows("ids", ids, b.rows, L);
  PrintRows("seq", Down(b.seq, slots), b.rows, L);
  PrintRows("pos", Down(b.pos, slots), b.rows, L);
  PrintRows("row_lengths", Down(b.row_lengths, b.rows), 1, b.rows);
  // UINT64_MAX prints as -1.
  PrintRows("place", Down(b.place, lines.size()), 1, lines.size());
  return 0;
}
