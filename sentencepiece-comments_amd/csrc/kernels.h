// Kernel launch interfaces (internal; the public boundary is include/spm_hip.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.h"
#include "normalize_device.h"

namespace spm_amd {

// Words of the per-call status block (zeroed by the host at the start of
// every encode call, stream-ordered).
enum : int {
  kStFlagged = 0,   // sentences the fast kernel handed to the general kernel
  kStMaxNb = 1,     // longest flagged sentence (bytes)
  kStError = 2,     // bit 0: a flagged sentence outgrew the device general path
  kStTicket = 3,    // tile tickets of the fast kernel
  kStOverflow = 4,  // flagged sentences longer than the general kernel's lane slab
  kStScanTicket = 5,// tile tickets of the fix-up scan
  kStCoopRest = 6,  // flagged sentences the cooperative kernel handed to the general kernel
  kStCoopQueue = 7, // the cooperative list kernel's work queue (next list entry)
  kStCoopLong = 8,  // coop partition: long sentences (taken first)
  kStCoopShort = 9, // coop partition: the others
  kStWords = 16
};

// Token-offset entry of a flagged sentence (fast kernel output): bit 63 set,
// low bits the (exclusive) offset; the fix-up kernels strip it.
constexpr uint64_t kTokFlag = 1ull << 63;

// Unigram encode of one batch (unigram_encode.hip).  The fast kernel writes
// each tile's (256 sentences) tokens densely into slot[off[256 t] ..] with
// tile-local token offsets in tok_off and the tile's count in tile_count[t];
// LaunchTileCompact scans the counts and places every tile, so ids[] /
// piece_len[] / tok_off[] are then final for every sentence it handled.  A
// sentence it cannot handle exactly is appended to `flagged`, gets zero
// tokens and its tok_off[i + 1] entry carries kTokFlag; the general kernel
// and the fix-up kernels (all device-guarded by the flagged count, so they
// are no-ops in the common case) then splice its tokens in.
struct UnigramLaunch {
  const uint8_t *bytes;
  const uint64_t *off;
  uint64_t n;
  uint64_t capacity;         // caller's bound on off[n] (every scratch buffer is sized by it)
  const uint32_t *units;     // byte kernel: (0xFF-padded unit, node score) pairs
  const uint32_t *gen_units; // the plain double array (general kernel)
  const int32_t *values;
  const float *scores;
  uint32_t num_units;
  const uint32_t *piece_tab; // byte kernel: piece -> (id, score) table (piece_table.h; nullptr: trie re-walk)
  uint32_t piece_mask, piece_seed;  // the table's header words
  UnigramParams p;
  int32_t *ids;              // dense output (written by the fix-up / tile compaction)
  uint32_t *len;             // nullable
  uint64_t *tok_off;         // n + 1
  uint8_t *bp;               // back-pointer scratch: >= offsets[n] + 16 bytes
  uint32_t *flagged;         // n entries
  uint32_t *status;          // kStWords
  uint64_t *tile_count;      // FastTiles(n) tile token counts
  uint64_t corrupt_bp;       // debug: zero this sentence's EOS back-pointer (~0: off)
  const uint32_t *chain;     // caller's status word (nullable): skip everything if non-zero
  int32_t *slot_ids;         // tile-dense token slots (capacity entries)
  uint32_t *slot_len;        // nullable
  uint32_t *bpn;             // kWide: trie unit per byte position (capacity + 16 entries)
  // Single-tile host calls (EncodeHostSmall): the block first zeroes words
  // [0, stage_zero) of stage_dst (the status block) and copies words
  // [stage_zero, stage_words) of the call's input image (offsets, bytes)
  // from pinned host memory, and at its end publishes the status words to
  // host_pub[1..kStWords] and then pub_seq to host_pub[0].
  const uint32_t *stage_src;
  uint32_t *stage_dst;
  uint32_t stage_zero;
  uint32_t stage_words;
  uint32_t *host_pub;
  uint32_t pub_seq;
  // Wide / char kernels: sentences of >= coop_min_nb bytes (0: none) are
  // flagged without a walk, for the wave-cooperative kernel (coop_encode.hip).
  uint32_t coop_min_nb;
};

enum class UnigramKernel : int { kGeneralOnly = 0, kByte = 1, kChar = 2, kWide = 3 };

// The unigram trainer E-step's forward pass in the byte kernel (estep mode):
// per sentence Z (alpha of EOS), N (lattice nodes), ntok (Viterbi().size(),
// kNone when flagged to the general E-step kernel), alpha at every char start
// at A[offset], flagged list + fstatus[0] count / [1] max flagged bytes.
struct EStepForwardOut {
  float *A;
  float *Z;
  uint32_t *N;
  uint32_t *ntok;
  uint32_t *flagged;
  uint32_t *fstatus;
  // Tile-transposed alpha (null: A only).  Tile t = sentences [256t, 256t +
  // 256); the pass's lane l of tile t walks sentence 256t + lanemap[256t + l]
  // (its length sort) and writes alpha of byte position p < kATRows to
  // AT[(t * kATRows + p) * 256 + l], so a wave's 64 lanes store one 256-byte
  // run per position instead of 64 scattered dwords; positions >= kATRows go
  // to A.  colmap[i] = the lane of sentence i (the backward pass sets 0xFFFF
  // for a general-path sentence).  The backward pass reads AT with the same
  // lane assignment.
  float *AT = nullptr;
  uint8_t *lanemap = nullptr;
  uint16_t *colmap = nullptr;
};
constexpr uint32_t kATRows = 64;

inline uint64_t FastTiles(uint64_t n) { return (n + 255) / 256; }
hipError_t LaunchUnigramEStepForward(const UnigramLaunch &l, const EStepForwardOut &e, hipStream_t st);
}  // namespace spm_amd
struct spm_hip_model;
namespace spm_amd {
// spm_hip_api.cc: the E-step forward pass through a TrainerModel's byte
// kernel (ok: the model encodes with the byte kernel, W = 16).
bool EStepByteForwardOk(const spm_hip_model *m);
int EStepByteForward(spm_hip_model *m, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint64_t bytes_end,
                     uint8_t *bp, uint32_t *ctl, const EStepForwardOut &e, hipStream_t st);
constexpr uint64_t kScanTiles = 1024;  // look-back tiles of the fix-up scan

// The fast kernel for the model's kernel kind: kByte (ring W = 16, the c2
// kernel) or kChar (W = 16/32/64).
hipError_t LaunchUnigramFast(UnigramKernel kind, int ring_width, const UnigramLaunch &l, hipStream_t st);

// General kernel (the reference lattice literally) over a list of sentences:
// list == nullptr means all of them (count ignored, list_n used); otherwise
// *count entries of list.  Sentences longer than max_nb go to ovf_list /
// *ovf_count when ovf_list is set, else set bit 0 of *error and get 0 tokens.
// Tokens are written right-aligned in the sentence's own byte range of
// slot_ids / slot_len, counts to ntok[i].
struct GeneralLaunch {
  const uint32_t *list;
  const uint32_t *count;
  uint64_t list_n;
  uint8_t *scratch;
  uint64_t slab_bytes;
  uint32_t max_nb;
  uint32_t threads;
  uint32_t *ovf_list;
  uint32_t *ovf_count;
  uint32_t *error;
  int32_t *slot_ids;
  uint32_t *slot_len;
  uint32_t *ntok;
};
hipError_t LaunchUnigramGeneral(const UnigramLaunch &l, const GeneralLaunch &g, hipStream_t st);

// Unigram SampleEncode (unigram_sample.hip): one segmentation per sentence
// drawn from the lattice with theta-scaled scores (Lattice::Sample,
// unigram_model.cc:488-526); draw k of sentence i comes from the stream of
// sample_rng.h at global index index_base + i.  Both kernels write a
// sentence's tokens right-aligned in its own byte range of slot_ids /
// slot_len and the count to ntok[i] (the general kernel's contract);
// LaunchCompact then packs them.
//
// Fast tier: one sentence per lane over all n sentences.  A / M: alpha and
// the node-distance mask per byte position, capacity + n + 1 entries each
// (position q of sentence i at off[i] + i + q; the launcher zeroes M).  A
// sentence it cannot sample exactly is appended to `flagged`
// (status[kStFlagged] counts, status[kStMaxNb] = the longest) for the exact
// tier.  A batch beyond `capacity` sets bit 1 of status[kStError].
struct SampleFastArgs {
  const uint8_t *bytes;
  const uint64_t *off;
  uint64_t n;
  uint64_t capacity;
  const uint32_t *units;  // the plain double array
  const int32_t *values;
  const float *scores;
  uint32_t num_units;
  UnigramParams p;
  float theta;
  uint64_t seed;
  uint64_t index_base;
  float *A;
  uint64_t *M;
  int32_t *slot_ids;
  uint32_t *slot_len;     // nullable
  uint32_t *ntok;
  uint32_t *flagged;      // n entries
  uint32_t *status;       // kStWords
};
hipError_t LaunchUnigramSampleFast(const SampleFastArgs &a, hipStream_t st);

// Exact tier: the literal lattice over a list of sentences (list == nullptr:
// all list_n of them), slabs of UnigramGeneralSlabBytes as in GeneralLaunch;
// sentences longer than max_nb go to ovf_list when it is set, else set bit 0
// of *error.  A backward step that does not move left sets bit 2 of *error.
struct SampleExactArgs {
  const uint8_t *bytes;
  const uint64_t *off;
  const uint32_t *units;
  const int32_t *values;
  const float *scores;
  uint32_t num_units;
  UnigramParams p;
  float theta;
  uint64_t seed;
  uint64_t index_base;
  int32_t *slot_ids;
  uint32_t *slot_len;
  uint32_t *ntok;
  const uint32_t *list;
  const uint32_t *count;
  uint64_t list_n;
  uint8_t *scratch;
  uint64_t slab_bytes;
  uint32_t max_nb;
  uint32_t *ovf_list;
  uint32_t *ovf_count;
  uint32_t *error;
  uint32_t lanes;
};
hipError_t LaunchUnigramSampleExact(const SampleExactArgs &a, hipStream_t st);

// Unigram lattice scores (unigram_lattice_score.hip): the entropy of every
// sentence's segmentation distribution, and num_samples drawn segmentations
// per sentence with their log-probabilities, over the sampler's forward pass
// A[p].  Two tiers each, bit-identical, with the sampler's flag / overflow /
// error contract (SampleFastArgs, SampleExactArgs).
//
// Entropy, fast tier: A and H per byte position, capacity + n + 1 floats each
// (position q of sentence i at off[i] + i + q; the launcher fills A with the
// "no node yet" pattern and zeroes H).  entropy[i] = -H[len]; log_z[i] =
// A[len] when log_z is set.  A sentence with a trie leaf inside a UTF-8 char
// is flagged.
struct EntropyFastArgs {
  const uint8_t *bytes;
  const uint64_t *off;
  uint64_t n;
  uint64_t capacity;
  const uint32_t *units;  // the plain double array
  const int32_t *values;
  const float *scores;
  uint32_t num_units;
  UnigramParams p;
  float theta;
  float *A;
  float *H;
  float *entropy;         // n
  float *log_z;           // n, nullable
  uint32_t *flagged;      // n entries
  uint32_t *status;       // kStWords
};
hipError_t LaunchUnigramEntropyFast(const EntropyFastArgs &a, hipStream_t st);

struct EntropyExactArgs {
  const uint8_t *bytes;
  const uint64_t *off;
  const uint32_t *units;
  const int32_t *values;
  const float *scores;
  uint32_t num_units;
  UnigramParams p;
  float theta;
  float *entropy;
  float *log_z;           // nullable
  const uint32_t *list;
  const uint32_t *count;
  uint64_t list_n;
  uint8_t *scratch;
  uint64_t slab_bytes;
  uint32_t max_nb;
  uint32_t *ovf_list;
  uint32_t *ovf_count;
  uint32_t *error;
  uint32_t lanes;
};
hipError_t LaunchUnigramEntropyExact(const EntropyExactArgs &a, hipStream_t st);

// Sample and score: the sampler's arguments, num_samples walks per sentence.
// Row r = i * num_samples + j is sample j of sentence i: its tokens are
// right-aligned in entries [num_samples * off[i] + j * nb, .. + nb) of
// slot_ids / slot_len (nb = the sentence's bytes), its count in ntok[r] and
// its score in score[r].  X (fast tier): capacity + n + 1 words, the chosen
// node per begin position of the walk at hand.
struct ScoreFastArgs {
  SampleFastArgs s;
  uint32_t num_samples;
  uint64_t *X;
  float *score;
};
hipError_t LaunchUnigramScoreFast(const ScoreFastArgs &a, hipStream_t st);
struct ScoreExactArgs {
  SampleExactArgs s;
  uint32_t num_samples;
  float *score;
};
hipError_t LaunchUnigramScoreExact(const ScoreExactArgs &a, hipStream_t st);

// Rows of ntok (n * num_samples of them) scanned into tok_off (rows + 1), and
// the rows' tokens gathered from the slots into ids / piece_len (nullable).
hipError_t LaunchScoreScan(const uint32_t *ntok, uint64_t rows, uint64_t *tok_off, void *tmp, size_t *tmp_bytes,
                           hipStream_t st);
hipError_t LaunchScoreGather(const uint64_t *off, uint64_t n, uint32_t num_samples, const int32_t *slot_ids,
                             const uint32_t *slot_len, const uint64_t *tok_off, int32_t *ids, uint32_t *piece_len,
                             hipStream_t st);

// Unigram NBestEncode (unigram_nbest.hip): the n best segmentations of every
// sentence (Lattice::NBest, unigram_model.cc:339-478), one sentence per lane
// over a list (list == nullptr: all list_n sentences).  Per-lane slabs of
// UnigramNBestSlabBytes(max_nb, K, max_hyps).  A sentence longer than max_nb,
// or whose search needs more than max_hyps hypotheses or reaches the
// reference's agenda shrink, is appended to ovf_list and writes nothing.
// Every other sentence i writes npaths[i], the token count and score of its
// path k at [i * nbest + k], and its paths' tokens one after the other from
// staging entry stage[i], claimed from *stage_cursor; when the claim ends
// beyond stage_cap the tokens are not written (the cursor tells the host how
// much staging the call needs).
constexpr uint64_t kNBestHostStage = 1ull << 63;  // stage[i]: the block is in the host tier's staging
struct NBestLaunch {
  const uint8_t *bytes;
  const uint64_t *off;
  const uint32_t *units;  // the plain double array
  const int32_t *values;
  const float *scores;
  uint32_t num_units;
  UnigramParams p;
  int32_t nbest;          // clamped to [1, 1024]
  const uint32_t *list;
  const uint32_t *count;
  uint64_t list_n;
  uint8_t *scratch;
  uint64_t slab_bytes;
  uint32_t max_nb;
  uint32_t max_hyps;
  uint32_t lanes;
  uint32_t *ovf_list;     // n entries
  uint32_t *ovf_count;
  uint32_t *npaths;       // n
  uint64_t *stage;        // n
  uint32_t *path_ntok;    // n * nbest
  float *path_score;      // n * nbest
  int32_t *stage_ids;     // stage_cap
  uint32_t *stage_len;    // nullable
  uint64_t stage_cap;
  unsigned long long *stage_cursor;
};
uint64_t UnigramNBestSlabBytes(uint32_t max_nb, int trie_results_size, uint32_t max_hyps);
hipError_t LaunchUnigramNBest(const NBestLaunch &a, hipStream_t st);
// path_off[n + 1] = scan of npaths (tmp == nullptr: the scan's scratch size).
hipError_t LaunchNBestPathOffsets(const uint32_t *npaths, uint64_t n, uint64_t *path_off, void *tmp,
                                  size_t *tmp_bytes, hipStream_t st);
// ptok[total_paths] = the paths' token counts in output order and
// tok_off[total_paths + 1] their scan (tmp == nullptr: the scratch size).
hipError_t LaunchNBestTokOffsets(uint64_t n, uint32_t nbest, const uint32_t *npaths, const uint64_t *path_off,
                                 const uint32_t *path_ntok, uint64_t total_paths, uint32_t *ptok, uint64_t *tok_off,
                                 void *tmp, size_t *tmp_bytes, hipStream_t st);
// Every sentence's staged block (device staging, or the host tier's when
// stage[i] carries kNBestHostStage) to its place in ids / piece_len, and its
// paths' scores to scores.
struct NBestGather {
  uint64_t n;
  uint32_t nbest;
  const uint64_t *path_off;
  const uint64_t *tok_off;
  const uint64_t *stage;
  const float *path_score;
  const int32_t *stage_ids;
  const uint32_t *stage_len;
  const int32_t *host_ids;
  const uint32_t *host_len;
  int32_t *ids;
  uint32_t *piece_len;    // nullable
  float *scores;
};
hipError_t LaunchNBestGather(const NBestGather &g, hipStream_t st);

// Wave-cooperative encode (coop_encode.hip): one sentence per wavefront over a
// device list (or all list_n sentences when list is null).  Output contract of
// the general kernel: tokens right-aligned in slot_ids / slot_len of the
// sentence's byte range, ntok[i]; sentences it does not take are appended to
// rest / *rest_count.  Scratch rows by char ordinal (see slab_chars below):
// 16 + 32 bytes per char.
constexpr int kCoopSlots = 8;
struct CoopArgs {
  const uint8_t *bytes;
  const uint64_t *off;
  const uint32_t *uvs;     // (0xFF-padded unit, node score) pairs (NaN: no usable node)
  const int32_t *values;
  uint32_t num_units;
  UnigramParams p;
  const uint32_t *list;
  const uint32_t *count;
  uint64_t list_n;
  int32_t *slot_ids;
  uint32_t *slot_len;      // nullable
  uint32_t *ntok;
  uint32_t *rest;
  uint32_t *rest_count;
  // Scratch by CHAR START ordinal of the sentence: kCoopSlots chosen lnodes
  // (length | slot << 7 | chars << 10) and kCoopSlots trie nodes per char.
  // slab_chars = 0: the sentence's rows start at its byte offset b0 (a
  // sentence has at most nb chars: capacity = the call's bytes); otherwise
  // wave w (blockIdx * 4 + wave) owns rows [w * slab_chars, (w + 1) *
  // slab_chars) and a sentence of more chars goes to the general kernel.
  uint16_t *pv_scratch;    // 16-byte aligned
  uint32_t *nd_scratch;    // 16-byte aligned
  uint32_t max_len;        // longest node in bytes (pieces, and 4 for UNK); <= 56
  const uint32_t *chain;   // asynchronous chain status (nullable)
  uint64_t *prof;          // debug (SPM_HIP_COOP_PROF): 8 cycle / size counters, nullable
  uint64_t slab_chars;     // 0: rows at b0; else per-wave slabs of this many chars
  // List kernel work queue (nullable: static grid stride): waves take list
  // entries one at a time from *queue; with `part` the k-th entry is
  // part[k] for k < *part_long (the long sentences, first), else
  // part[part_n - 1 - (k - *part_long)].
  uint32_t *queue;
  const uint32_t *part;
  const uint32_t *part_long;
  uint64_t part_n;
};
// Sentences of at least this many bytes start first (the longest lines
// decide the list kernel's tail).
constexpr uint32_t kCoopLongNb = 2048;
hipError_t LaunchCoopPartition(const uint32_t *list, const uint32_t *count, const uint64_t *off, uint64_t n,
                               uint32_t *part, uint32_t *n_long, uint32_t *n_short, hipStream_t st);
// Per-wave slab of the list kernel (coop_list_kernel) and its grid cap (3
// blocks of 4 waves are resident per CU: more blocks only queue).
constexpr uint64_t kCoopSlabChars = 16384;
constexpr uint32_t kCoopMaxBlocks = 768;
hipError_t LaunchCoopEncode(const CoopArgs &a, uint32_t max_blocks, hipStream_t st);
inline uint32_t CoopBlocks(uint64_t n, uint32_t max_blocks = kCoopMaxBlocks) {
  const uint64_t b = (n + 3) / 4;
  return static_cast<uint32_t>(b < max_blocks ? b : max_blocks);
}

// One-block host call of <= kCoopSmallMax sentences (EncodeHostSmall): input
// image [offsets | bytes] staged from pinned host memory (CoopCall::
// stage_words words to stage_dst; a.off = the staged offsets, a.bytes = the
// image, the bytes at CoopCall::in_at), outputs (tok, ids, len) and the
// publication (host_pub[1] = 0 ok / 1 re-run on the lane kernels, then
// host_pub[0] = pub_seq) written into pinned host memory.
constexpr uint32_t kCoopSmallMax = 16;
struct CoopSmallArgs {
  CoopArgs a;
  const uint32_t *stage_src;
  uint32_t *stage_dst;
};
struct CoopCall;
hipError_t LaunchCoopSmall(const CoopSmallArgs &s, const CoopCall &c, hipStream_t st);
// Small raw-line calls (coop_encode.hip coop_raw_kernel): one block, n <=
// kCoopSmallMax raw lines; each wave normalizes a line (NormalizePrefix of
// 64 positions at a time, the state machine on one lane), encodes it with
// CoopEncodeSentence and merges its unknown runs; outputs and the completion
// word go to host memory.  The staged image is [raw offsets | raw bytes];
// line i's normalized bytes go to a.bytes + 4 raw_off[i] + 8 i (capacity
// 4 len + 8).
// (Per call, CoopCall: n, stage_words, in_at = the raw bytes' offset in the
// staged image, ids_cap, tok = out_off (host, n + 1), ids (host), host_pub.)
struct CoopRawArgs {
  CoopArgs a;
  NormTables t;
  const uint32_t *stage_src;
  uint32_t *stage_dst;
  const uint8_t *types;      // piece type bits (epilogue.h), num_types entries
  int32_t num_types;
};
hipError_t LaunchCoopRaw(const CoopRawArgs &s, const CoopCall &c, hipStream_t st);

// What varies between the one-block small calls (coop_small_kernel /
// coop_raw_kernel / the service kernel): sizes, the input's place in the
// staged image and the host-memory outputs.
struct CoopCall {
  uint32_t n;
  uint32_t stage_words;
  uint32_t pub_seq;
  uint32_t pad;
  uint64_t in_at;       // small: staged byte offset of the sentence bytes (b0 = in_at + off[i]); raw: of the raw bytes
  uint64_t ids_cap;     // raw: capacity of ids
  uint64_t *tok;        // small: token offsets; raw: out_off (n + 1)
  int32_t *ids;
  uint32_t *len;        // small: piece byte lengths (nullable)
  uint32_t *host_pub;   // [0] sequence, [1] 0 = done, 1 = not taken
};
// BPE small calls (bpe_line.hip): one block, n <= kCoopSmallMax lines, one
// wave per line, one launch per call.  bpe_small_kernel takes normalized
// sentences (the staged image [offsets | bytes], sentence i at bytes + in_at +
// off[i]) and writes tok, ids and len; bpe_raw_kernel takes raw lines (image
// [raw offsets | raw bytes], line i's normalized bytes at bytes + 4 raw_off[i]
// + 8 i as in CoopRawArgs), merges unknown runs and writes tok (out_off) and
// ids.  A wave's tokens wait in slot_ids / slot_len from the sentence's byte
// offset on.  A line of more than kBpeLineMaxBytes normalized bytes, a pushed
// UNUSED piece or (irregular models) a char outside the vocabulary publishes
// "not taken" (host_pub[1] = 1) and writes no output.
constexpr uint32_t kBpeLineMaxBytes = 1024;
struct BpeLineArgs {
  const uint32_t *units;       // the symbol trie
  const int32_t *values;       // leaf -> entry index
  const int32_t *entry_piece;
  const int32_t *entry_out;
  const int32_t *piece_out;
  const uint4 *pair_ent;       // (right id, left id, merged id | unused << 31, score rank)
  uint64_t pair_mask;
  uint32_t root_base;
  int32_t unk_id;
  int32_t irregular;
  const uint8_t *bytes;        // small: the staged image; raw: the normalized bytes (written)
  int32_t *slot_ids;
  uint32_t *slot_len;          // small only
  const uint32_t *stage_src;
  uint32_t *stage_dst;
};
struct BpeRawArgs {
  BpeLineArgs a;
  NormTables t;
  const uint8_t *types;        // piece type bits (epilogue.h), num_types entries
  int32_t num_types;
};
hipError_t LaunchBpeSmall(const BpeLineArgs &a, const CoopCall &c, hipStream_t st);
hipError_t LaunchBpeRaw(const BpeRawArgs &s, const CoopCall &c, hipStream_t st);

// BPE-dropout batch tier (bpe_dropout.hip): one normalized sentence per
// wavefront, BpeEncodeLineWave with each probed pair masked by the sentence's
// draw stream (sample_rng.h: key SampleKey(seed, index_base + i), draw number
// start << 32 | end of the pair's bytes, dropped when the draw's 53 bits are
// below `threshold` = ceil(alpha * 2^53)).  t: the model's tables with bytes =
// the batch, slot_ids / slot_len (nullable) the right-aligned slots; stage_*
// unused.  A sentence it does not take (over kBpeLineMaxBytes bytes, a pushed
// UNUSED piece, a char outside an irregular vocabulary) is flagged for the
// general kernel (ntok = ~0, `flagged`, status[kStFlagged / kStMaxNb]).
// rest / rest_count (nullable, zeroed count): with them the sentences of <=
// kBpeDropShortBytes bytes run first on slabs of that size (more waves per
// CU) and the longer ones from the `rest` list on full slabs.
constexpr uint32_t kBpeDropShortBytes = 128;
struct BpeDropoutLaunch {
  BpeLineArgs t;
  const uint64_t *off;
  uint64_t n;
  uint32_t *ntok;
  uint32_t *flagged;
  uint32_t *status;          // kStWords
  uint64_t capacity;         // caller's bound on off[n]
  const uint32_t *chain;     // asynchronous chain status (nullable)
  uint64_t threshold, seed, index_base;
  uint32_t *rest, *rest_count;
};
hipError_t LaunchBpeDropout(const BpeDropoutLaunch &d, hipStream_t st);

// Resident service kernel for small calls (coop_service_kernel): one block
// polls `box` in pinned coherent host memory; the host writes `call` and
// then `seq` = (sequence & 0x3FFFFFFF) | kind << 30 (kind 1 = normalized
// batch with `small`'s tables, 2 = raw lines with `raw`'s); the block serves
// it exactly as coop_small_kernel / coop_raw_kernel would and publishes the
// result the same way.  It exits when `stop` is set or after idle_ticks
// wall-clock ticks without a request (then alive = 0).
struct CoopServiceBox {
  uint32_t seq;
  uint32_t stop;
  uint32_t alive;  // device: 1 from start to exit
  uint32_t served;  // device: requests served by this launch
  CoopCall call;
  // device (diagnostics, SPM_HIP_SERVICE_PROF): wall-clock ticks summed over
  // the served requests: seq seen -> call copied, -> result published.
  uint64_t ticks_copy, ticks_busy;
};
struct CoopServiceArgs {
  CoopSmallArgs small;
  CoopRawArgs raw;
  CoopServiceBox *box;
  uint32_t last;        // the box's seq at launch (a different seq is a request)
  uint64_t idle_ticks;
};
hipError_t LaunchCoopService(const CoopServiceArgs &s, hipStream_t st);
uint64_t UnigramGeneralSlabBytes(uint32_t max_nb, int trie_results_size);

// Fix-up chain after the general kernel (all no-ops when status[kStFlagged]
// is 0): fast-path tokens move to their sentences' right-aligned slots, the
// counts are re-scanned into tok_off, and every sentence is compacted back
// into ids/len.  Writes the call's final status code to out_status (nullable).
struct FixupLaunch {
  const uint64_t *off;
  uint64_t n;
  int32_t *ids;
  uint32_t *len;
  uint64_t *tok_off;
  int32_t *slot_ids;
  uint32_t *slot_len;
  const uint32_t *ntok;      // general kernel counts (flagged sentences)
  uint32_t *cnt;             // n scratch
  uint32_t *status;
  uint64_t *scan_desc;       // kScanTiles, zeroed
  uint32_t *out_status;
};
hipError_t LaunchEncodeFixup(const FixupLaunch &f, hipStream_t st);

// status[0] = code unless it is already non-zero (first error wins), on st.
hipError_t LaunchStatusSetFirst(uint32_t *status, uint32_t code, hipStream_t st);

// After the fast kernel: tile t's tokens sit densely at slot[off[256 t]],
// tile_count[t] = their count, tok_off holds tile-local inclusive offsets.
// Scans the tile counts (tile_prefix: tiles + 1 entries) and moves every
// tile to its final place with coalesced copies, rebasing tok_off.
hipError_t LaunchTileCompact(const uint64_t *off, uint64_t n, const uint64_t *tile_count, uint64_t *tile_prefix,
                             const int32_t *slot_ids, const uint32_t *slot_len, int32_t *ids, uint32_t *len,
                             uint64_t *tok_off, void *scan_tmp, size_t *scan_tmp_bytes, const uint32_t *status,
                             hipStream_t st);

// Dense CSR output from right-aligned slots (general-only and BPE paths):
// tok_off = exclusive scan of ntok; sentence i's tokens come from
// slot[off[i+1] - ntok[i]].  Skipped when status[kStError] bit 1 (the batch
// exceeded the caller's capacity) is set.
hipError_t LaunchCompact(const uint64_t *off, uint64_t n, const uint32_t *ntok, const int32_t *slot_ids,
                         const uint32_t *slot_len, int32_t *ids, uint32_t *piece_len, uint64_t *tok_off,
                         void *scan_tmp, size_t *scan_tmp_bytes, const uint32_t *status, uint32_t *out_status,
                         hipStream_t st);

// WORD / CHAR encode (wordchar_kernels.hip).  Tokens are views into the
// input, so the kernels mark the bytes that start a token (mark: one byte per
// input byte, whole tiles of kWcTile), count the marks per tile, scan, and
// look every marked span up in the exact-match table (wordchar_table.h).
// LaunchWordCharTile marks by the tile tier's shortcut and appends the
// sentences where it differs from the reference's OneCharLen walk to
// `flagged` (status[kStFlagged] counts them, sflag: zeroed, one word per
// sentence); LaunchWordCharGeneral re-marks those (all = false) or every
// sentence (all = true, which also sets status[kStFlagged] = n) with the
// reference's sequential loop; LaunchWordCharOutput writes ids / len /
// tok_off and the call's status (RESOURCE_EXHAUSTED when off[n] > capacity).
constexpr uint32_t kWcTile = 2048;
inline uint64_t WordCharTiles(uint64_t capacity) { return capacity / kWcTile + 1; }
struct WordCharLaunch {
  const uint8_t *bytes;
  const uint64_t *off;
  uint64_t n;
  uint64_t capacity;         // caller's bound on off[n]
  uint64_t tiles;            // WordCharTiles(capacity)
  int32_t word;              // 1: WORD (SplitIntoWords), 0: CHAR (PrefixMatch)
  const uint32_t *tab;       // WordCharEntry[tab_mask + 1]
  uint32_t tab_mask;
  const uint8_t *keys;       // the entries' key bytes
  uint32_t max_piece_bytes;  // a longer token is unknown without a lookup
  int32_t unk_id;
  const uint32_t *ud_units;  // CHAR: user-defined symbol trie (nullable)
  uint32_t ud_num_units;
  uint8_t *mark;             // tiles * kWcTile bytes, 8-byte aligned
  uint32_t *sflag;           // n, zeroed
  uint32_t *flagged;         // n
  uint32_t *status;          // kStWords
  uint32_t *tile_count;      // tiles
  uint32_t *tile_first;      // tiles: first mark of the tile (kWcTile: none)
  uint64_t *tile_prefix;     // tiles + 1
  uint32_t *tile_sent;       // tiles: first sentence that starts in or after the tile
  uint64_t *tile_next;       // tiles: position of the first mark in a later tile (~0: none)
  int32_t *ids;
  uint32_t *len;             // nullable
  uint64_t *tok_off;         // n + 1
  const uint32_t *chain;     // caller's status word (nullable): idle if non-zero
  uint32_t *out_status;      // the same word, for the call's own status
};
hipError_t LaunchWordCharEmpty(uint64_t *tok_off, const uint32_t *chain, hipStream_t st);  // n == 0
hipError_t LaunchWordCharSentences(const WordCharLaunch &l, hipStream_t st);  // first: fills tile_sent
hipError_t LaunchWordCharTile(const WordCharLaunch &l, hipStream_t st);
hipError_t LaunchWordCharGeneral(const WordCharLaunch &l, bool all, hipStream_t st);
hipError_t LaunchWordCharOutput(const WordCharLaunch &l, hipStream_t st);

// Vocabulary restriction and piece counting (vocab_kernels.hip).  kind: one
// byte per piece id (0 other, kKindUserDefined, kKindUnused).
// Unigram: the kind bits of every leaf's value and, when uvs is not null, the
// usable-node score (the piece's score, NaN when UNUSED) of the (unit, score)
// table; USER_DEFINED leaves are left alone.
hipError_t LaunchVocabRetagUnigram(const uint32_t *units, int32_t *values, uint32_t *uvs, const float *scores,
                                   const uint8_t *kind, uint32_t num_units, uint32_t num_pieces, hipStream_t st);
// BPE: the unused bit of the merged piece in every pair entry (uint4 slots).
hipError_t LaunchVocabRetagBpe(void *pair_ent, uint64_t slots, const uint8_t *kind, uint32_t num_pieces,
                               hipStream_t st);
// counts[id] += occurrences of id in ids[0, n), n <= 2^31 (the LDS bins are
// 32 bits wide).  An id outside [0, num_pieces) is skipped and sets bit 0 of
// *status.  Vocabularies of up to kCountLdsMaxPieces pieces are binned in
// LDS per workgroup, kCountTile tokens per workgroup step.
constexpr uint32_t kCountLdsMaxPieces = 32768;
constexpr uint32_t kCountTile = 4096;
hipError_t LaunchVocabCount(const int32_t *ids, uint64_t n, uint64_t *counts, uint32_t num_pieces, uint32_t *status,
                            hipStream_t st);

}  // namespace spm_amd
