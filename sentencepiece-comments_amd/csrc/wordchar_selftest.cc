// Self-test driver of SentencePieceProcessor on WORD / CHAR models (tests/
// test_gpu_wordchar_cli.py): wordchar_selftest MODEL [PIECE-OR-LINE...] prints
//   "size N unk U bos B eos E pad P"
//   per id: "id <id> piece_to_id <PieceToId(IdToPiece(id))> unknown control unused <score bits>"
//   per argument: "arg piece_to_id <id>", "encode <code> <code>" (the status
//   of Encode to ids and to pieces), "ids ...", "pieces ..." (Encode of the
//   argument as a line, pieces separated by tabs) and "sample <code>
//   nbest <code>" (the status codes of SampleEncode(-1) and NBestEncode(2)).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "processor.h"

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s MODEL [PIECE-OR-LINE...]\n", argv[0]);
    return 2;
  }
  spm_amd::SentencePieceProcessor sp;
  const auto st = sp.Load(argv[1]);
  if (!st.ok()) {
    std::fprintf(stderr, "%s\n", st.message.c_str());
    return 1;
  }
  std::printf("size %d unk %d bos %d eos %d pad %d\n", sp.GetPieceSize(), sp.unk_id(), sp.bos_id(), sp.eos_id(),
              sp.pad_id());
  for (int id = 0; id < sp.GetPieceSize(); ++id) {
    const float score = sp.GetScore(id);
    uint32_t bits;
    std::memcpy(&bits, &score, 4);
    std::printf("id %d piece_to_id %d %d %d %d %08x\n", id, sp.PieceToId(sp.IdToPiece(id)), sp.IsUnknown(id) ? 1 : 0,
                sp.IsControl(id) ? 1 : 0, sp.IsUnused(id) ? 1 : 0, bits);
  }
  for (int a = 2; a < argc; ++a) {
    const std::string arg = argv[a];
    std::printf("arg piece_to_id %d\n", sp.PieceToId(arg));
    std::vector<int> ids;
    std::vector<std::string> pieces;
    // A token that is a CONTROL piece consumes no surface, so the reference's
    // PopulateSentencePieceText fails such a line (INTERNAL); the codes are
    // printed, and no ids or pieces then.
    const int code_ids = sp.Encode(arg, &ids).code, code_pieces = sp.Encode(arg, &pieces).code;
    std::printf("encode %d %d\n", code_ids, code_pieces);
    if (code_ids != SPM_OK) ids.clear();
    if (code_pieces != SPM_OK) pieces.clear();
    std::printf("ids");
    for (int i : ids) std::printf(" %d", i);
    std::printf("\npieces");
    for (const auto &p : pieces) std::printf("\t%s", p.c_str());
    std::vector<std::vector<int>> nbest;
    std::printf("\nsample %d nbest %d\n", sp.SampleEncode(arg, -1, 0.5f, &ids).code,
                sp.NBestEncode(arg, 2, &nbest).code);
  }
  return 0;
}
