// text_rows_selftest MODEL FORMAT(id|piece) EXTRA_OPTIONS FILE
// SentencePieceProcessor::EncodeTextRows over the whole file as one buffer;
// the rows go to stdout.  The same rows are built from EncodeBatch over the
// file's std::getline lines, and the exit status is 1 if the two differ.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "processor.h"

int main(int argc, char **argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s model id|piece extra_options file\n", argv[0]);
    return 2;
  }
  const bool want_ids = std::string(argv[2]) == "id";
  spm_amd::SentencePieceProcessor sp;
  auto st = sp.Load(argv[1]);
  if (st.ok()) st = sp.SetEncodeExtraOptions(argv[3]);
  if (!st.ok()) {
    std::fprintf(stderr, "%s\n", st.message.c_str());
    return 2;
  }
  std::ifstream in(argv[4], std::ios::binary);
  const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::string rows;
  st = sp.EncodeTextRows(text.data(), text.size(), want_ids ? sp.kTextRowsId : sp.kTextRowsPiece, &rows);
  if (!st.ok()) {
    std::fprintf(stderr, "EncodeTextRows: %d %s\n", st.code, st.message.c_str());
    return 2;
  }
  std::fwrite(rows.data(), 1, rows.size(), stdout);
  std::ifstream again(argv[4], std::ios::binary);
  std::vector<std::string> lines;
  for (std::string line; std::getline(again, line);) lines.push_back(line);
  std::vector<std::vector<int>> ids;
  std::vector<std::vector<std::string>> pieces;
  st = sp.EncodeBatch(lines, want_ids ? &ids : nullptr, want_ids ? nullptr : &pieces);
  if (!st.ok()) return 2;
  std::string host;
  for (size_t i = 0; i < lines.size(); ++i) {
    const size_t m = want_ids ? ids[i].size() : pieces[i].size();
    for (size_t k = 0; k < m; ++k) {
      if (k) host += ' ';
      host += want_ids ? std::to_string(ids[i][k]) : pieces[i][k];
    }
    host += '\n';
  }
  if (host != rows) {
    std::fprintf(stderr, "text rows differ from EncodeBatch\n");
    return 1;
  }
  return 0;
}
