// Self-test driver of SentencePieceProcessor::EncodeDense with window
// (tests/test_gpu_window.py): window_selftest MODEL OPTIONS ROW_LEN PAD_ID
// STRIDE KEEP_FIRST KEEP_LAST [LINE...].  Prints "window rows R row_len L
// tokens T multi M", then per row "ids ...", "pos ...", "fresh ...", then
// "lengths ...", "row_sentence ..." and "first_row ...", all read back from
// the device pointers of the DenseBatch.
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
  if (argc < 8) {
    std::fprintf(stderr, "usage: %s MODEL OPTIONS ROW_LEN PAD_ID STRIDE KEEP_FIRST KEEP_LAST [LINE...]\n", argv[0]);
    return 2;
  }
  using spm_amd::SentencePieceProcessor;
  SentencePieceProcessor::DenseOptions o;
  o.row_len = static_cast<uint32_t>(std::strtoul(argv[3], nullptr, 10));
  o.pad_id = static_cast<int32_t>(std::strtol(argv[4], nullptr, 10));
  o.window = true;
  o.stride = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
  o.keep_first = std::strtoul(argv[6], nullptr, 10) != 0;
  o.keep_last = std::strtoul(argv[7], nullptr, 10) != 0;
  const std::vector<std::string> lines(argv + 8, argv + argc);
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
  const std::vector<uint64_t> stats = Down(b.stats, 2);
  std::printf("window rows %llu row_len %u tokens %llu multi %llu\n", static_cast<unsigned long long>(b.rows),
              b.row_len, static_cast<unsigned long long>(b.tokens), static_cast<unsigned long long>(stats[1]));
  const uint64_t L = b.row_len, slots = b.rows * L;
  PrintRows("ids", ids, b.rows, L);
  PrintRows("pos", Down(b.pos, slots), b.rows, L);
  PrintRows("fresh", Down(b.fresh, slots), b.rows, L);
  PrintRows("lengths", Down(b.lengths, b.rows), 1, b.rows);
  PrintRows("row_sentence", Down(b.row_sentence, b.rows), 1, b.rows);
  PrintRows("first_row", Down(b.first_row, lines.size() + 1), 1, lines.size() + 1);
  return 0;
}
