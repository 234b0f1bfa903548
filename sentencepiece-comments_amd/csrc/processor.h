// C++ mirror of sentencepiece::SentencePieceProcessor's encode surface
// (reference src/sentencepiece_processor.h:176-470) on top of the C-ABI.
//
// Same names, argument meaning and error behaviour as the reference for the
// calls on the hot path: Load / LoadFromSerializedProto, SetEncodeExtraOptions,
// Encode(ids), Encode(pieces), PieceToId / IdToPiece / GetPieceSize /
// IsUnknown / IsControl / unk_id / bos_id / eos_id / pad_id, and for the way
// back: SetDecodeExtraOptions, Decode(ids), Decode(pieces) and their batched
// form DecodeBatch (spm_hip_decode_batch on the device).  Encode is
// batched: EncodeBatch runs the device normalizer and the device encode over
// the whole batch; Encode(ids) also runs the id epilogue of
// PopulateSentencePieceText (unk merge, control pieces) + ApplyExtraOptions
// on the device, Encode(pieces) applies it per line on the host.  Small
// Encode(ids) batches (one line included) go through the pure stream calls
// with one upload and one synchronization (EncodeIdsSmall).  Like the
// reference's processor, one instance is not for concurrent Encode calls.
#pragma once

#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/spm_hip.h"
#include "model_proto.h"

namespace spm_amd {

struct Status {
  int code = SPM_OK;  // util::error::Code
  std::string message;
  bool ok() const { return code == SPM_OK; }
  static Status Ok() { return Status(); }
};

class SentencePieceProcessor {
 public:
  SentencePieceProcessor() = default;
  ~SentencePieceProcessor();
  SentencePieceProcessor(const SentencePieceProcessor &) = delete;
  SentencePieceProcessor &operator=(const SentencePieceProcessor &) = delete;

  Status Load(const std::string &filename);
  Status LoadFromSerializedProto(const std::string &serialized);
  // Tables only, nothing on the device (spm_hip_model_load_host_only): the
  // piece queries and the three vocabulary calls work, every encode and decode
  // call is an error and the model's self-test samples are not run.  For tools
  // and tests on machines without a GPU.
  Status LoadHostOnly(const std::string &serialized);
  Status status() const;

  // "bos", "eos", "reverse" separated by ':' (sentencepiece_processor.cc:981-1010).
  Status SetEncodeExtraOptions(const std::string &extra_options);

  Status Encode(const std::string &input, std::vector<int> *ids) const;
  Status Encode(const std::string &input, std::vector<std::string> *pieces) const;
  // Batched encode: ids and/or pieces (either may be null).
  Status EncodeBatch(const std::vector<std::string> &inputs, std::vector<std::vector<int>> *ids,
                     std::vector<std::vector<std::string>> *pieces) const;

  // SampleEncode (sentencepiece_processor.cc:622-659), batched.  nbest_size
  // > 512 is an error; 0 or 1 is exactly Encode; < 0 draws one segmentation
  // per line from the unigram lattice on the device with inverse temperature
  // alpha (spm_hip_sample_encode_batch; a WORD or CHAR model gives
  // SPM_UNIMPLEMENTED); > 1 (sampling among the n best) is SPM_UNIMPLEMENTED:
  // use nbest_size = -1 (NBestEncode below returns the n best themselves).
  // A BPE model samples by BPE-dropout for every nbest_size but 0 and 1 (the
  // package ignores nbest_size there; 0 and 1 staying Encode is this
  // processor's contract): the merge loop of Encode with each candidate merge
  // skipped with probability alpha (spm_hip_bpe_dropout_encode_batch).
  // Unknown-run merge (or the byte-fallback expansion) and the
  // extra options apply as in Encode.  Line i of the k-th sampled call uses
  // the random stream of global index (lines sampled so far) + i under the
  // processor's seed, so repeated calls on one line give fresh draws and a
  // fixed seed replays the whole sequence.
  Status SampleEncode(const std::string &input, int nbest_size, float alpha, std::vector<int> *ids) const;
  Status SampleEncode(const std::string &input, int nbest_size, float alpha,
                      std::vector<std::string> *pieces) const;
  Status SampleEncodeBatch(const std::vector<std::string> &inputs, int nbest_size, float alpha,
                           std::vector<std::vector<int>> *ids,
                           std::vector<std::vector<std::string>> *pieces) const;
  // Seed of the sampler (default: from std::random_device); restarts the
  // sentence counter.
  void SetRandomSeed(uint64_t seed);

  // CalculateEntropy of the `sentencepiece` package: the entropy of a line's
  // segmentation distribution at inverse temperature alpha, from the device
  // (spm_hip_entropy_batch).  A model that is not unigram gives INTERNAL
  // "CalculateEntropy is not available for the current model.".
  Status CalculateEntropy(const std::string &input, float alpha, float *entropy) const;
  Status CalculateEntropy(const std::vector<std::string> &inputs, float alpha, std::vector<float> *entropy) const;

  // SampleEncodeAndScore of the package: num_samples segmentations of a line
  // drawn from the unigram lattice, each with its log-probability
  // (spm_hip_sample_encode_and_score_batch).  Unknown-run merge, extra
  // options and the byte epilogue apply as in SampleEncode, and the lines'
  // global indices advance as there, so a fixed seed replays.  wor or
  // include_best (sampling without replacement) gives SPM_UNIMPLEMENTED; a
  // model that is not unigram gives INTERNAL "SampleEncodeAndScore is not
  // available for the current model."; a line whose normalized text is empty
  // gives INTERNAL "SampleEncodeAndScore returns empty result.", as in the
  // package.
  Status SampleEncodeAndScore(const std::string &input, int num_samples, float alpha, bool wor, bool include_best,
                              std::vector<std::pair<std::vector<int>, float>> *ids) const;
  Status SampleEncodeAndScore(const std::string &input, int num_samples, float alpha, bool wor, bool include_best,
                              std::vector<std::pair<std::vector<std::string>, float>> *pieces) const;
  Status SampleEncodeAndScoreBatch(const std::vector<std::string> &inputs, int num_samples, float alpha, bool wor,
                                   bool include_best,
                                   std::vector<std::vector<std::pair<std::vector<int>, float>>> *ids,
                                   std::vector<std::vector<std::pair<std::vector<std::string>, float>>> *pieces) const;

  // NBestEncode (sentencepiece_processor.cc:588-609), batched: the nbest_size
  // (clamped to [1, 1024]) best segmentations of every line, best first, from
  // the device A* search (spm_hip_nbest_encode_batch); a line with fewer
  // paths returns fewer.  Unknown-run merge and the extra options apply to
  // every path.  scores: the paths' model scores.  Each output may be null.
  // A model that is not unigram gives INTERNAL "NBestEncode returns empty
  // result.", as the reference does.  Large batches run in chunks.
  Status NBestEncode(const std::string &input, int nbest_size, std::vector<std::vector<int>> *ids) const;
  Status NBestEncode(const std::string &input, int nbest_size, std::vector<std::vector<std::string>> *pieces) const;
  Status NBestEncodeBatch(const std::vector<std::string> &inputs, int nbest_size,
                          std::vector<std::vector<std::vector<int>>> *ids,
                          std::vector<std::vector<std::vector<std::string>>> *pieces,
                          std::vector<std::vector<float>> *scores) const;

  // Vocabulary restriction (sentencepiece_processor.cc:203-274), with the
  // reference's names, errors and results.  SetVocabulary (UNIGRAM and BPE
  // models only): CONTROL, UNKNOWN and USER_DEFINED pieces stay, any other
  // piece becomes NORMAL if it is in valid_vocab or one character long, else
  // UNUSED.  ResetVocabulary: every UNUSED piece becomes NORMAL, those UNUSED
  // in the model file included.  LoadVocabulary: "piece[\tfreq]" lines (freq
  // defaults to 1), pieces with freq >= threshold go to SetVocabulary.  As in
  // the reference only the types change: the scores the model took at Load
  // (the unknown score among them) stay, so a restricted processor is not the
  // processor of a model file whose types were edited.  proto_ and the device
  // model change together (spm_hip_model_set_piece_types), so every encode
  // call that follows sees the restriction.  Not for use concurrently with
  // any other call on the instance.
  Status SetVocabulary(const std::vector<std::string> &valid_vocab);
  Status ResetVocabulary();
  Status LoadVocabulary(const std::string &filename, int threshold);

  // Dense id batches: Encode (or SampleEncode) of every line, then the final
  // ids as one rectangular int32 tensor that stays on the device
  // (spm_hip_pad_ids / spm_hip_pack_ids), for a training or inference loop on
  // the same GPU.  pack = false: one line per row, padded with pad_id or cut
  // to row_len (flags: SPM_DENSE_PAD_LEFT, SPM_DENSE_TRUNCATE_LEFT,
  // SPM_DENSE_KEEP_END).  pack = true: the lines' ids run on as one stream of
  // row_len slots per row (flags must be 0).  The extra options are part of
  // the ids, so they apply before padding.
  struct DenseOptions {
    uint32_t row_len = 0;
    int32_t pad_id = 0;
    uint32_t flags = 0;
    bool pack = false;
  };
  // Device pointers, owned by the processor and valid until the next call on
  // the instance; the work that fills them is enqueued on the null stream.
  struct DenseBatch {
    const int32_t *ids = nullptr;      // [rows, row_len]
    const int32_t *lengths = nullptr;  // pad: [rows], tokens kept per row
    const uint8_t *mask = nullptr;     // pad: [rows, row_len], 1 on token slots
    const int32_t *seq = nullptr;      // pack: [rows, row_len], the slot's line, -1 on padding
    const int32_t *pos = nullptr;      // pack: [rows, row_len], the slot's position in its line
    const uint64_t *stats = nullptr;   // pad: {lines cut, tokens dropped}; pack: {rows, tokens}
    uint64_t rows = 0;                 // pad: the lines; pack: ceil(tokens / row_len)
    uint32_t row_len = 0;
    uint64_t tokens = 0;  // final ids of the batch before padding
    // Only with host_ids (the call then waits for the device): the stats of pad.
    uint64_t cut = 0, dropped = 0;
  };
  // Nothing but the id count comes back to the host unless host_ids is given
  // (then it receives the rows * row_len ids).  A WORD or CHAR model takes its
  // host id epilogue as in Encode; the ids go back up and through the same
  // kernel.  A host-only processor gives SPM_FAILED_PRECONDITION.
  Status EncodeDense(const std::vector<std::string> &inputs, const DenseOptions &options, DenseBatch *out,
                     std::vector<int32_t> *host_ids = nullptr) const;
  // SampleEncodeBatch in place of the encode: the same seed rules, the same
  // advance of the sentence counter and the same refusals for nbest_size.
  Status SampleEncodeDense(const std::vector<std::string> &inputs, int nbest_size, float alpha,
                           const DenseOptions &options, DenseBatch *out,
                           std::vector<int32_t> *host_ids = nullptr) const;

  // counts[id] += the occurrences of id in Encode(line, &ids) of every input
  // line (extra options applied; counts grows to GetPieceSize()).  Normalize,
  // encode, id epilogue and count run on the device (spm_hip_count_ids); only
  // the counters come back.  Accumulates over calls.
  Status CountPieces(const std::vector<std::string> &inputs, std::vector<uint64_t> *counts) const;

  // Decode (sentencepiece_processor.cc:341-370, :670-733).  One piece of
  // SentencePieceText: surface = text[begin, end).
  struct DecodedPiece {
    std::string piece;
    int id = 0;
    std::string surface;
    uint32_t begin = 0, end = 0;
  };
  // "bos", "eos", "reverse" separated by ':', applied to the piece list in
  // the order given (ParseExtraOptions :981-1023, ApplyExtraOptions :945-979).
  Status SetDecodeExtraOptions(const std::string &extra_options);
  Status Decode(const std::vector<int> &ids, std::string *detokenized) const;
  Status Decode(const std::vector<std::string> &pieces, std::string *detokenized) const;
  // Batched: texts[i] is the text of line i; spt (may be null) receives every
  // line's pieces in final order with their surfaces.  Batches of at least
  // kDecodeDeviceMinTokens tokens run on the device in one call
  // (spm_hip_decode_batch); smaller ones, and every line that holds a piece
  // outside the vocabulary (its own bytes are its surface), run the same
  // rules in a loop on the host.  Unlike the reference, which indexes the
  // piece table unchecked, an id outside [0, GetPieceSize()) is
  // SPM_OUT_OF_RANGE.
  Status DecodeBatch(const std::vector<std::vector<int>> &ids, std::vector<std::string> *texts,
                     std::vector<std::vector<DecodedPiece>> *spt = nullptr) const;
  Status DecodeBatch(const std::vector<std::vector<std::string>> &pieces, std::vector<std::string> *texts,
                     std::vector<std::vector<DecodedPiece>> *spt = nullptr) const;
  // Where DecodeBatch runs: kDecodeAuto picks by the batch's token count.
  // SPM_HIP_DECODE_PATH=host|device sets the initial value.
  enum DecodePath { kDecodeAuto = 0, kDecodeHost = 1, kDecodeDevice = 2 };
  void SetDecodePath(DecodePath path) { decode_path_ = path; }
  // Token count from which the device call (upload, decode, download) beats
  // the host loop.  Measured by tools/decode_bench.py on the c2 ids
  // (profiles/pr13_decode.txt): at 17493 tokens the host loop takes 0.135 ms
  // and the device call 0.157 ms, at 70100 tokens 0.672 ms against 0.199 ms;
  // the lines cross near 21 k tokens, and the next power of two is used.
  static constexpr uint64_t kDecodeDeviceMinTokens = 32768;

  // The model is a BPE model (its SampleEncode is BPE-dropout).
  bool IsBpe() const { return proto_.trainer_spec.model_type == kBpe; }
  int GetPieceSize() const;
  int PieceToId(const std::string &piece) const;
  const std::string &IdToPiece(int id) const;
  float GetScore(int id) const;
  bool IsUnknown(int id) const;
  bool IsControl(int id) const;
  // A BYTE piece ("<0x00>" ... "<0xFF>") of a model trained with
  // byte_fallback.  Under byte fallback Encode replaces every unknown token by
  // the BYTE pieces of its bytes instead of <unk>, and Decode turns runs of
  // BYTE pieces back into text (invalid UTF-8 gives U+FFFD per byte).
  bool IsByte(int id) const;
  bool IsUnused(int id) const;
  int unk_id() const;
  int bos_id() const;
  int eos_id() const;
  int pad_id() const;

 private:
  enum ExtraOption { REVERSE, BOS, EOS };
  spm_hip_model *model_ = nullptr;
  ModelProtoView proto_;
  std::unordered_map<std::string, int> pieces_, reserved_;
  int byte_ids_[256];  // byte fallback: byte -> id of its BYTE piece (-1 without)
  std::vector<ExtraOption> extra_;
  std::string extra_str_;  // the accepted option string, for the device epilogue
  std::vector<ExtraOption> decode_extra_;
  std::string decode_extra_str_;
  DecodePath decode_path_ = kDecodeAuto;
  Status ParseExtraOptions(const std::string &opts, std::vector<ExtraOption> *out) const;
  // One line's (piece, id) list -> options applied, text and pieces.
  void DecodeLineHost(std::vector<std::pair<std::string, int>> *row, std::string *text,
                      std::vector<DecodedPiece> *spt) const;
  // rows[i]: line i as (piece, id); oov[i]: it holds a piece outside the vocabulary.
  Status DecodeRows(std::vector<std::vector<std::pair<std::string, int>>> *rows, const std::vector<char> &oov,
                    std::vector<std::string> *texts, std::vector<std::vector<DecodedPiece>> *spt) const;
  Status status_{SPM_INTERNAL, "Model is not initialized."};
  // Sampler: the seed and the number of lines sampled so far (the next
  // call's index_base).
  mutable uint64_t sample_seed_ = 0, sample_count_ = 0;
  mutable bool sample_seeded_ = false;
  struct SampleSpec {
    float theta;
    uint64_t seed, index_base;
  };
  Status LoadImpl(const std::string &serialized, bool host_only);
  bool host_only_ = false;
  Status SyncTypes();  // the handle's piece types -> proto_
  // A batch on the device after normalize + encode (DeviceEncode), and its id
  // epilogue (DeviceFinalize); the buffers are dev_'s.
  struct DeviceBatch {
    uint8_t *d_norm = nullptr;
    uint64_t *d_norm_off = nullptr;
    int32_t *d_ids = nullptr;
    uint32_t *d_len = nullptr;
    uint64_t *d_tok = nullptr;
    uint64_t total = 0;  // normalized bytes
  };
  Status DeviceEncode(const std::vector<std::string> &inputs, const SampleSpec *sample, DeviceBatch *b) const;
  Status DeviceNormalize(const std::vector<std::string> &inputs, uint8_t **d_norm, uint64_t **d_norm_off,
                         uint64_t *total) const;
  Status DeviceFinalize(const DeviceBatch &b, uint64_t n, int32_t **d_out, uint64_t **d_out_off, uint64_t *fin) const;
  // EncodeDense / SampleEncodeDense.
  Status RunDense(const std::vector<std::string> &inputs, const SampleSpec *sample, const DenseOptions &options,
                  DenseBatch *out, std::vector<int32_t> *host_ids) const;
  // EncodeBatch; with `sample` the device sampler stands in for the encode.
  Status RunBatch(const std::vector<std::string> &inputs, std::vector<std::vector<int>> *ids,
                  std::vector<std::vector<std::string>> *pieces, const SampleSpec *sample) const;
  // PopulateSentencePieceText + ApplyExtraOptions over one path's tokens.
  Status PopulateText(const char *normalized, uint64_t nlen, const int32_t *tok_ids, const uint32_t *tok_len,
                      uint64_t count, std::vector<std::pair<std::string, int>> *out) const;
  // Grow-only device staging for EncodeBatch (raw lines → normalized → ids).
  struct Staging {
    void *ptr[15] = {};
    size_t cap[15] = {};
    void *Get(int k, size_t bytes);
    ~Staging();
  };
  mutable Staging dev_;
  // Small Encode(ids) batches (EncodeIdsSmall): a private stream and a
  // grow-only pinned host block.
  struct SmallPath {
    void *stream = nullptr;
    uint8_t *pin = nullptr;
    size_t pin_cap = 0;
    ~SmallPath();
  };
  mutable SmallPath small_;
  // true: *ids filled; false: take the general path (capacity guess exceeded).
  Status EncodeIdsSmall(const std::vector<std::string> &inputs, std::vector<std::vector<int>> *ids,
                        bool *done) const;
};

}  // namespace spm_amd
