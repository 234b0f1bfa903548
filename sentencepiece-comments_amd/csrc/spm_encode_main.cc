// spm_encode — drop-in for the reference CLI (src/spm_encode_main.cc:52-223)
// for --output_format=id|piece|sample_id|sample_piece|nbest_id|nbest_piece,
// with batched device encoding.  sample_* is SampleEncode(line, --nbest_size,
// --alpha) (spm_encode_main.cc:133-144): --nbest_size=-1 samples from the
// whole lattice on the device, 0 or 1 is the plain encode; the reference's
// default of 10 (sampling among the n best) is not implemented and exits
// with a message.  With a BPE model sample_* is BPE-dropout with probability
// --alpha, whatever --nbest_size is (the package ignores it there).
// nbest_* is NBestEncode(line, --nbest_size)
// (spm_encode_main.cc:154-169): one output line per path of every input
// line, best first.  --random_seed (not in the reference) makes a run
// reproducible.
//
// --vocabulary / --vocabulary_threshold (spm_encode_main.cc:70-72) restrict
// the pieces the encoder emits (SentencePieceProcessor::LoadVocabulary), and
// --generate_vocabulary (:98-109, :196-201) writes "piece\tcount" lines
// instead of a segmentation: every emitted piece that is neither unknown nor
// control, by count descending, then piece ascending.  The pieces are counted
// on the device (SentencePieceProcessor::CountPieces).  Counts are 64-bit
// here: the reference's int would overflow on the corpora this engine is
// meant for; below 2^31 the output is byte-identical to the reference's.
//
// The reference encodes one line at a time (spm_encode_main.cc:189-191).
// Here lines are read in batches (--batch_lines), normalized and encoded on
// the device in one call per batch (SentencePieceProcessor::EncodeBatch;
// ids also get the device id epilogue); the output is byte-identical:
// one output line per input line, pieces / ids joined by " ".  Lines are
// read with std::getline semantics (a trailing '\r' is kept,
// filesystem.cc:42-44).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "processor.h"

namespace {

struct Flags {
  std::string model, output_format = "piece", output, extra_options, vocabulary;
  int vocabulary_threshold = 0;
  bool generate_vocabulary = false;
  long batch_lines = 1 << 20;
  int nbest_size = 10;
  float alpha = 0.5f;
  bool has_seed = false;
  unsigned long long random_seed = 0;
};

void Usage(const char *argv0) {
  std::cout << "Usage: " << argv0 << " [options] files\n\n"
            << "   --model (model file name)  type: string default: \n"
            << "   --output_format (choose from piece, id, sample_piece, sample_id, nbest_piece or nbest_id)  "
               "type: string default: piece\n"
            << "   --output (output filename)  type: string default: \n"
            << "   --extra_options (':' separated encoder extra options, e.g., "
               "\"reverse:bos:eos\")  type: string default: \n"
            << "   --nbest_size (nbest_*: number of segmentations per line; sample_*: -1 samples from the "
               "whole lattice, 0 or 1 is the best segmentation, larger values are not implemented; ignored with a "
               "BPE model, which samples by BPE-dropout)  "
               "type: int32 default: 10\n"
            << "   --alpha (smoothing parameter for sampling mode)  type: double default: 0.5\n"
            << "   --vocabulary (Restrict the vocabulary. The encoder only emits the tokens in \"vocabulary\" "
               "file)  type: string default: \n"
            << "   --vocabulary_threshold (Words with frequency < threshold will be treated as OOV)  "
               "type: int32 default: 0\n"
            << "   --generate_vocabulary (Generates vocabulary file instead of segmentation)  "
               "type: bool default: false\n"
            << "   --random_seed (seed of the sampler; unset: random)  type: uint64 default: \n"
            << "   --batch_lines (lines per device batch)  type: int64 default: 1048576\n";
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
    } else if (k == "output_format") {
      f.output_format = v;
    } else if (k == "output") {
      f.output = v;
    } else if (k == "extra_options") {
      f.extra_options = v;
    } else if (k == "batch_lines") {
      f.batch_lines = std::max(1L, std::atol(v.c_str()));
    } else if (k == "nbest_size") {
      f.nbest_size = std::atoi(v.c_str());
    } else if (k == "alpha") {
      f.alpha = static_cast<float>(std::atof(v.c_str()));
    } else if (k == "random_seed") {
      f.has_seed = true;
      f.random_seed = std::strtoull(v.c_str(), nullptr, 10);
    } else if (k == "vocabulary") {
      f.vocabulary = v;
    } else if (k == "vocabulary_threshold") {
      f.vocabulary_threshold = std::atoi(v.c_str());
    } else if (k == "generate_vocabulary") {
      // A boolean takes no separate value: a word after the bare flag that is
      // no boolean is an input file.
      const bool no = v == "false" || v == "0" || v == "f" || v == "no";
      f.generate_vocabulary = !no;
      if (!no && v != "true" && v != "1" && v != "t" && v != "yes") rest.push_back(v);
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
  const bool sample = f.output_format == "sample_id" || f.output_format == "sample_piece";
  const bool nbest = f.output_format == "nbest_id" || f.output_format == "nbest_piece";
  const bool want_ids = f.output_format == "id" || f.output_format == "sample_id" || f.output_format == "nbest_id";
  if (!f.generate_vocabulary && !sample && !nbest && f.output_format != "id" && f.output_format != "piece")
    Die("output_format \"" + f.output_format +
        "\": only piece, id, sample_piece, sample_id, nbest_piece and nbest_id are implemented by the device "
        "engine");

  spm_amd::SentencePieceProcessor sp;
  auto st = sp.Load(f.model);
  if (!st.ok()) Die(st.message);
  st = sp.SetEncodeExtraOptions(f.extra_options);
  if (!st.ok()) Die(st.message);
  if (f.has_seed) sp.SetRandomSeed(f.random_seed);
  if (!f.vocabulary.empty()) {
    st = sp.LoadVocabulary(f.vocabulary, f.vocabulary_threshold);
    if (!st.ok()) Die(st.message);
  }

  std::ofstream ofs;
  std::ostream *out = &std::cout;
  if (!f.output.empty()) {
    ofs.open(f.output, std::ios::binary);
    if (!ofs) Die("\"" + f.output + "\": cannot open");
    out = &ofs;
  }
  if (rest.empty()) rest.push_back("");  // stdin

  std::vector<std::string> batch;
  std::vector<std::vector<int>> ids;
  std::vector<std::vector<std::string>> pieces;
  std::vector<std::vector<std::vector<int>>> nbest_ids;
  std::vector<std::vector<std::vector<std::string>>> nbest_pieces;
  std::string buf;
  std::vector<uint64_t> counts;
  auto flush = [&]() {
    if (batch.empty()) return;
    if (f.generate_vocabulary) {
      auto s = sp.CountPieces(batch, &counts);
      if (!s.ok()) Die(s.message);
      batch.clear();
      return;
    }
    if (nbest) {
      auto s = sp.NBestEncodeBatch(batch, f.nbest_size, want_ids ? &nbest_ids : nullptr,
                                   want_ids ? nullptr : &nbest_pieces, nullptr);
      if (!s.ok()) Die(s.message);
      for (size_t i = 0; i < batch.size(); ++i) {
        const size_t paths = want_ids ? nbest_ids[i].size() : nbest_pieces[i].size();
        for (size_t p = 0; p < paths; ++p) {
          buf.clear();
          if (want_ids) {
            for (size_t k = 0; k < nbest_ids[i][p].size(); ++k) {
              if (k) buf += ' ';
              buf += std::to_string(nbest_ids[i][p][k]);
            }
          } else {
            for (size_t k = 0; k < nbest_pieces[i][p].size(); ++k) {
              if (k) buf += ' ';
              buf += nbest_pieces[i][p][k];
            }
          }
          buf += '\n';
          out->write(buf.data(), buf.size());
        }
      }
      batch.clear();
      return;
    }
    auto s = sample ? sp.SampleEncodeBatch(batch, sp.IsBpe() ? -1 : f.nbest_size, f.alpha, want_ids ? &ids : nullptr,
                                           want_ids ? nullptr : &pieces)
                    : sp.EncodeBatch(batch, want_ids ? &ids : nullptr, want_ids ? nullptr : &pieces);
    if (!s.ok()) Die(s.message);
    for (size_t i = 0; i < batch.size(); ++i) {
      buf.clear();
      if (want_ids) {
        for (size_t k = 0; k < ids[i].size(); ++k) {
          if (k) buf += ' ';
          buf += std::to_string(ids[i][k]);
        }
      } else {
        for (size_t k = 0; k < pieces[i].size(); ++k) {
          if (k) buf += ' ';
          buf += pieces[i][k];
        }
      }
      buf += '\n';
      out->write(buf.data(), buf.size());
    }
    batch.clear();
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
      batch.push_back(line);
      if (static_cast<long>(batch.size()) >= f.batch_lines) flush();
    }
  }
  flush();
  if (f.generate_vocabulary) {
    std::vector<std::pair<std::string, uint64_t>> vocab;
    for (size_t id = 0; id < counts.size(); ++id)
      if (counts[id] && !sp.IsUnknown(static_cast<int>(id)) && !sp.IsControl(static_cast<int>(id)))
        vocab.emplace_back(sp.IdToPiece(static_cast<int>(id)), counts[id]);
    std::sort(vocab.begin(), vocab.end(), [](const auto &a, const auto &b) {
      return a.second > b.second || (a.second == b.second && a.first < b.first);
    });
    for (const auto &it : vocab) {
      buf = it.first + "\t" + std::to_string(it.second) + "\n";
      out->write(buf.data(), buf.size());
    }
  }
  return 0;
}
