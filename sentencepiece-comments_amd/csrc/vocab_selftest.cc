// Test driver of the processor's vocabulary calls (tests/test_vocab_cpu.py,
// tests/test_gpu_vocab.py): vocab_selftest MODEL [--host] reads one command
// per line from stdin, fields separated by tabs, and answers on stdout.
//   set P1 P2 ...            SetVocabulary            -> "ok" | "error CODE MESSAGE"
//   reset                    ResetVocabulary          -> same
//   load FILE THRESHOLD      LoadVocabulary           -> same
//   unused                   -> "unused" and IsUnused(id) of every id
//   encode LINE              Encode(LINE, &ids)       -> "ids ..."
//   pieces LINE              Encode(LINE, &pieces)    -> "pieces ..."
//   batch FILE START COUNT   EncodeBatch of the lines -> COUNT "ids ..." lines
//   single FILE START COUNT  Encode(line, &ids) of each line -> the same
//   nbest FILE START COUNT N NBestEncodeBatch         -> per line "paths K", then K "ids ..." lines
//   sample FILE START COUNT ALPHA  SampleEncodeBatch(nbest_size = -1), seed 7 -> COUNT "ids ..." lines
//   count FILE START COUNT   CountPieces (accumulating) -> "counts" and "ID:COUNT" of every non-zero id
// --host loads tables only (LoadHostOnly): set / reset / load / unused work.
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "processor.h"

namespace {

std::vector<std::string> Fields(const std::string &line) {
  std::vector<std::string> v;
  size_t at = 0;
  while (true) {
    const size_t e = line.find('\t', at);
    v.push_back(line.substr(at, e == std::string::npos ? std::string::npos : e - at));
    if (e == std::string::npos) break;
    at = e + 1;
  }
  return v;
}

std::vector<std::string> Lines(const std::string &file, size_t start, size_t count) {
  std::ifstream in(file, std::ios::binary);
  std::vector<std::string> out;
  std::string line;
  for (size_t i = 0; std::getline(in, line) && out.size() < count; ++i)
    if (i >= start) out.push_back(line);
  return out;
}

void PrintIds(const std::vector<int> &ids) {
  std::cout << "ids";
  for (int id : ids) std::cout << ' ' << id;
  std::cout << '\n';
}

bool Report(const spm_amd::Status &st) {
  if (st.ok()) return true;
  std::cout << "error " << st.code << ' ' << st.message << '\n';
  return false;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::cerr << "usage: vocab_selftest MODEL [--host] < commands\n";
    return 2;
  }
  const bool host = argc > 2 && std::string(argv[2]) == "--host";
  spm_amd::SentencePieceProcessor sp;
  spm_amd::Status st;
  if (host) {
    std::ifstream in(argv[1], std::ios::binary);
    const std::string proto((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    st = sp.LoadHostOnly(proto);
  } else {
    st = sp.Load(argv[1]);
  }
  if (!st.ok()) {
    std::cerr << st.message << '\n';
    return 1;
  }
  sp.SetRandomSeed(7);
  std::vector<uint64_t> counts;
  std::string cmd;
  while (std::getline(std::cin, cmd)) {
    const std::vector<std::string> f = Fields(cmd);
    const std::string &op = f[0];
    auto num = [&](size_t k) { return k < f.size() ? std::stoul(f[k]) : 0ul; };
    if (op == "set") {
      if (Report(sp.SetVocabulary(std::vector<std::string>(f.begin() + 1, f.end())))) std::cout << "ok\n";
    } else if (op == "reset") {
      if (Report(sp.ResetVocabulary())) std::cout << "ok\n";
    } else if (op == "load" && f.size() >= 3) {
      if (Report(sp.LoadVocabulary(f[1], std::stoi(f[2])))) std::cout << "ok\n";
    } else if (op == "unused") {
      std::cout << "unused";
      for (int id = 0; id < sp.GetPieceSize(); ++id) std::cout << ' ' << (sp.IsUnused(id) ? 1 : 0);
      std::cout << '\n';
    } else if (op == "encode" && f.size() >= 2) {
      std::vector<int> ids;
      if (Report(sp.Encode(f[1], &ids))) PrintIds(ids);
    } else if (op == "pieces" && f.size() >= 2) {
      std::vector<std::string> pieces;
      if (Report(sp.Encode(f[1], &pieces))) {
        std::cout << "pieces";
        for (const auto &p : pieces) std::cout << ' ' << p;
        std::cout << '\n';
      }
    } else if (op == "batch" && f.size() >= 4) {
      std::vector<std::vector<int>> ids;
      if (Report(sp.EncodeBatch(Lines(f[1], num(2), num(3)), &ids, nullptr)))
        for (const auto &row : ids) PrintIds(row);
    } else if (op == "single" && f.size() >= 4) {
      for (const auto &line : Lines(f[1], num(2), num(3))) {
        std::vector<int> ids;
        if (!Report(sp.Encode(line, &ids))) break;
        PrintIds(ids);
      }
    } else if (op == "nbest" && f.size() >= 5) {
      std::vector<std::vector<std::vector<int>>> ids;
      if (Report(sp.NBestEncodeBatch(Lines(f[1], num(2), num(3)), std::stoi(f[4]), &ids, nullptr, nullptr)))
        for (const auto &paths : ids) {
          std::cout << "paths " << paths.size() << '\n';
          for (const auto &row : paths) PrintIds(row);
        }
    } else if (op == "sample" && f.size() >= 5) {
      std::vector<std::vector<int>> ids;
      if (Report(sp.SampleEncodeBatch(Lines(f[1], num(2), num(3)), -1, std::stof(f[4]), &ids, nullptr)))
        for (const auto &row : ids) PrintIds(row);
    } else if (op == "count" && f.size() >= 4) {
      if (Report(sp.CountPieces(Lines(f[1], num(2), num(3)), &counts))) {
        std::cout << "counts";
        for (size_t id = 0; id < counts.size(); ++id)
          if (counts[id]) std::cout << ' ' << id << ':' << counts[id];
        std::cout << '\n';
      }
    } else {
      std::cout << "error 3 bad command\n";
    }
  }
  return 0;
}
