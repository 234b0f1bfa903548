// spm_decode — drop-in for the reference CLI (src/spm_decode_main.cc:25-150):
// --model, --output, --input_format=piece|id, --output_format=string|proto,
// --extra_options, input files as the remaining arguments (stdin when none).
//
// The reference decodes one line at a time.  Here lines are read in batches
// (--batch_lines) and decoded with SentencePieceProcessor::DecodeBatch, on the
// device for large batches; the output is byte-identical: one text line per
// input line, in input order.  A line is split on single spaces with empty
// fields dropped (string_util::Split, util.cc:32-49), ids are parsed with
// atoi, and --output_format=proto decodes and prints nothing, as the
// reference does (its WriteLine is commented out).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "processor.h"

namespace {

struct Flags {
  std::string model, input_format = "piece", output_format = "string", output, extra_options;
  long batch_lines = 1 << 20;
};

void Usage(const char *argv0) {
  std::cout << "Usage: " << argv0 << " [options] files\n\n"
            << "   --model (model file name)  type: string default: \n"
            << "   --output (output filename)  type: string default: \n"
            << "   --input_format (choose from piece or id)  type: string default: piece\n"
            << "   --output_format (choose from string or proto)  type: string default: string\n"
            << "   --extra_options (':' separated encoder extra options, e.g., "
               "\"reverse:bos:eos\")  type: string default: \n"
            << "   --batch_lines (lines per decode batch)  type: int64 default: 1048576\n";
}

[[noreturn]] void Die(const std::string &msg) {
  std::cerr << msg << std::endl;
  std::exit(1);
}

// CommandLineGetFlag semantics (flags.cc): --k=v, --k v, -k=v; bare --k is
// "true" for booleans.
bool GetFlag(int argc, char **argv, int *i, std::string *key, std::string *value) {
  std::string a = argv[*i];
  if (a.size() < 2 || a[0] != '-') return false;
  a = a.substr(a[1] == '-' ? 2 : 1);
  const size_t eq = a.find('=');
  if (eq != std::string::npos) {
    *key = a.substr(0, eq);
    *value = a.substr(eq + 1);
    return true;
  }
  *key = a;
  if (*i + 1 < argc && argv[*i + 1][0] != '-') {
    *value = argv[++*i];
  } else {
    *value = "true";
  }
  return true;
}

// string_util::Split(line, " "): fields between single spaces, empty ones dropped.
void SplitLine(const std::string &line, std::vector<std::string> *out) {
  out->clear();
  size_t pos = 0, found;
  while ((found = line.find(' ', pos)) != std::string::npos) {
    if (found > pos) out->push_back(line.substr(pos, found - pos));
    pos = found + 1;
  }
  if (line.size() > pos) out->push_back(line.substr(pos));
}

}  // namespace

int main(int argc, char **argv) {
  Flags f;
  std::vector<std::string> rest;
  for (int i = 1; i < argc; ++i) {
    std::string k, v;
    if (!GetFlag(argc, argv, &i, &k, &v)) {
      rest.push_back(argv[i]);
      continue;
    }
    if (k == "help") {
      Usage(argv[0]);
      return 0;
    } else if (k == "version") {
      std::cout << "sentencepiece-mi355x 0.1.82" << std::endl;
      return 0;
    } else if (k == "model") {
      f.model = v;
    } else if (k == "input_format") {
      f.input_format = v;
    } else if (k == "output_format") {
      f.output_format = v;
    } else if (k == "output") {
      f.output = v;
    } else if (k == "extra_options") {
      f.extra_options = v;
    } else if (k == "batch_lines") {
      f.batch_lines = std::max(1L, std::atol(v.c_str()));
    } else if (k == "minloglevel") {
    } else {
      Usage(argv[0]);
      Die("Unknown/Invalid flag " + k);
    }
  }
  if (f.model.empty()) {
    Usage(argv[0]);
    Die("--model is required.");
  }
  if (f.input_format != "piece" && f.input_format != "id") Die("Unknown input format: " + f.input_format);
  if (f.output_format != "string" && f.output_format != "proto") Die("Unknown output format: " + f.output_format);
  const bool from_ids = f.input_format == "id";
  const bool print = f.output_format == "string";

  spm_amd::SentencePieceProcessor sp;
  auto st = sp.Load(f.model);
  if (!st.ok()) Die(st.message);
  st = sp.SetDecodeExtraOptions(f.extra_options);
  if (!st.ok()) Die(st.message);

  std::ofstream ofs;
  std::ostream *out = &std::cout;
  if (!f.output.empty()) {
    ofs.open(f.output, std::ios::binary);
    if (!ofs) Die("\"" + f.output + "\": cannot open");
    out = &ofs;
  }
  if (rest.empty()) rest.push_back("");  // stdin

  std::vector<std::vector<std::string>> pieces;
  std::vector<std::vector<int>> ids;
  std::vector<std::string> texts, fields;
  std::vector<std::vector<spm_amd::SentencePieceProcessor::DecodedPiece>> spt;
  std::string buf;
  auto flush = [&]() {
    if (pieces.empty() && ids.empty()) return;
    auto s = from_ids ? sp.DecodeBatch(ids, &texts, print ? nullptr : &spt)
                      : sp.DecodeBatch(pieces, &texts, print ? nullptr : &spt);
    if (!s.ok()) Die(s.message);
    if (print) {
      buf.clear();
      for (const auto &t : texts) {
        buf += t;
        buf += '\n';
      }
      out->write(buf.data(), buf.size());
    }
    pieces.clear();
    ids.clear();
  };
  for (const auto &fn : rest) {
    std::ifstream ifs;
    std::istream *in = &std::cin;
    if (!fn.empty()) {
      ifs.open(fn, std::ios::binary);
      if (!ifs) Die("\"" + fn + "\": No such file or directory");
      in = &ifs;
    }
    std::string line;
    while (std::getline(*in, line)) {
      SplitLine(line, &fields);
      if (from_ids) {
        ids.emplace_back();
        for (const auto &s : fields) ids.back().push_back(std::atoi(s.c_str()));
      } else {
        pieces.push_back(fields);
      }
      if (static_cast<long>(from_ids ? ids.size() : pieces.size()) >= f.batch_lines) flush();
    }
  }
  flush();
  return 0;
}
