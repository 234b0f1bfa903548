/*
 * spm_hip.h — C-ABI of the MI355X-native SentencePiece encode / E-step engine.
 *
 * This is the drop-in boundary for the hot path of SentencePiece v0.1.82
 * (ycaptain/SentencePiece-comments).  Every entry point is plain C: pointers,
 * sizes and int status codes; no torch or C++ types.  Status codes are the
 * values of util::error::Code (reference src/sentencepiece_processor.h:101-119);
 * HIP failures map to SPM_INTERNAL.  No entry point aborts or throws.
 *
 * Reference interfaces replaced:
 *   spm_hip_model_load   ModelFactory::Create (src/model_factory.cc:26-47) +
 *                        unigram::Model::Model (src/unigram_model.cc:677-695) /
 *                        bpe::Model::Model (src/bpe_model.cc:26-31) +
 *                        ModelInterface::InitializePieces (src/model_interface.cc:101-144)
 *   spm_hip_encode_batch ModelInterface::Encode(normalized) (src/model_interface.h:117),
 *                        batched over sentences: unigram::Model::Encode
 *                        (src/unigram_model.cc:705-720) and bpe::Model::Encode
 *                        (src/bpe_model.cc:37-199)
 *   spm_hip_finalize_ids SentencePieceProcessor::PopulateSentencePieceText +
 *                        ApplyExtraOptions (src/sentencepiece_processor.cc:488-551,
 *                        :945-979), id part
 *   spm_hip_decode_batch SentencePieceProcessor::Decode(ids) (src/sentencepiece_processor.cc:
 *                        670-733) with the decode extra options (:945-979)
 *   spm_hip_estep        unigram::Trainer::RunEStep (src/unigram_model_trainer.cc:237-287)
 *   spm_hip_seed_mine    unigram::Trainer::MakeSeedSentencePieces
 *                        (src/unigram_model_trainer.cc:124-225) + esaxx
 *                        (third_party/esaxx/esa.hxx:37-122)
 */
#ifndef SPM_HIP_H_
#define SPM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this ABI (struct layouts and entry-point signatures).  Structs
 * such as spm_hip_model_info may change between versions; callers built
 * against another version must not use them (check spm_hip_abi_version()). */
#define SPM_HIP_ABI_VERSION 3
int spm_hip_abi_version(void);

/* util::error::Code (sentencepiece_processor.h:101-119). */
enum spm_status {
  SPM_OK = 0,
  SPM_CANCELLED = 1,
  SPM_UNKNOWN = 2,
  SPM_INVALID_ARGUMENT = 3,
  SPM_NOT_FOUND = 5,
  SPM_PERMISSION_DENIED = 7,
  SPM_RESOURCE_EXHAUSTED = 8,
  SPM_FAILED_PRECONDITION = 9,
  SPM_OUT_OF_RANGE = 11,
  SPM_UNIMPLEMENTED = 12,
  SPM_INTERNAL = 13
};

/* TrainerSpec::ModelType (sentencepiece_model.proto:29-34). */
enum spm_model_type { SPM_UNIGRAM = 1, SPM_BPE = 2, SPM_WORD = 3, SPM_CHAR = 4 };

typedef struct spm_hip_model spm_hip_model;

typedef struct spm_hip_model_info {
  int32_t model_type;       /* spm_model_type */
  int32_t piece_size;       /* ModelProto.pieces_size() */
  int32_t unk_id;           /* index of the UNKNOWN piece */
  int32_t max_piece_chars;  /* longest matchable piece, in UTF-8 chars
                               (WORD / CHAR: over every piece type) */
  int32_t trie_results_size;/* unigram: max prefix matches per position */
  int32_t trie_units;       /* device double-array size (units) */
  float min_score;          /* unigram: min over NORMAL scores */
  float max_score;          /* unigram: max(FLT_MIN, NORMAL scores) */
  int32_t ring_width;       /* unigram fast kernel ring W (16/32/64; > longest
                               piece in bytes), 0 = general kernel only */
  int32_t fast_variant;     /* unigram encode kernel: 1 byte-position kernel
                               (W = 16), 2 char-position kernel, 3 wide-char
                               kernel (ring of 16 chars), 0 general only.
                               BPE: the kernel first in line: 1 lane kernel
                               with rank ids, merged id = base - rank; 2 lane
                               kernel with rank ids, merged id from the rank
                               table; 3 lane kernel with 32-bit symbol words
                               (tied merge scores); 4 half kernel (>= 32768
                               pieces); 0 general kernel only (user-defined
                               symbols).  WORD / CHAR: 1 the tile tier runs
                               first (token starts marked per byte tile, the
                               general tier takes only flagged sentences), 0
                               every sentence goes to the general tier (a CHAR
                               model with USER_DEFINED pieces).  Also set on a
                               host-only handle. */
} spm_hip_model_info;

/* Counters of the last encode call (host-visible after it returns). */
typedef struct spm_hip_encode_stats {
  uint64_t sentences;
  uint64_t tokens;
  uint64_t general_path;    /* sentences re-run by the exact general kernel */
  float fast_kernel_ms;     /* HIP-event time of the fast kernel launch (0 if
                               timing is off, see spm_hip_model_set_timing) */
  float general_kernel_ms;  /* same for the general kernel */
  uint64_t coop_rest;       /* of general_path: sentences the wave-cooperative
                               kernel took first and handed on to the general
                               kernel (host batch calls) */
} spm_hip_encode_stats;

/* Parses a serialized ModelProto, validates it like InitializePieces and
 * uploads the device-resident tables (trie, scores, piece types) to the
 * current HIP device.  *out is NULL on failure. */
int spm_hip_model_load(const void *model_proto, size_t len, spm_hip_model **out);
/* Same parsing/validation and host tables, no device work (CPU-only use:
 * normalization, info).  Encode calls on such a handle return
 * SPM_FAILED_PRECONDITION. */
int spm_hip_model_load_host_only(const void *model_proto, size_t len, spm_hip_model **out);
void spm_hip_model_free(spm_hip_model *model);
/* Unigram model over a bare piece list with the trainer's TrainerModel
 * semantics (unigram_model_trainer.cc:97-119, unigram_model_trainer.h:39-89):
 * all pieces NORMAL, value = list index, unk_id 0, UNK score min - 10.  Used
 * by the pruning step's Viterbi (PruneSentencePieces :377-421) through
 * spm_hip_encode_batch.  HOST pointers. */
int spm_hip_model_from_pieces(const uint8_t *piece_bytes, const uint64_t *piece_offsets,
                              const float *scores, uint64_t num_pieces, spm_hip_model **out);
int spm_hip_model_get_info(const spm_hip_model *model, spm_hip_model_info *info);

/* Batched ModelInterface::Encode over normalized sentences, DEVICE pointers.
 *   d_norm_bytes   : concatenated normalized UTF-8 bytes (CSR values)
 *   d_offsets      : uint64[n+1] byte offsets of each sentence
 *   d_ids          : int32 output, capacity >= offsets[n] (one token per byte
 *                    is the upper bound)
 *   d_piece_len    : optional (may be NULL) uint32 byte length of each piece;
 *                    pieces are views into the input, in order
 *   d_tok_offsets  : uint64[n+1] output CSR offsets into d_ids
 *   stream         : hipStream_t (NULL = default stream)
 * BLOCKING: reads offsets[n], enqueues the work on `stream`, waits for it and
 * returns the status the reference's Encode would (util::Status).  Empty
 * sentences yield zero tokens (unigram_model.cc:706-708).  Pipelines use
 * spm_hip_encode_batch_async. */
int spm_hip_encode_batch(spm_hip_model *model, const uint8_t *d_norm_bytes,
                         const uint64_t *d_offsets, uint64_t n, int32_t *d_ids,
                         uint32_t *d_piece_len, uint64_t *d_tok_offsets, void *stream);

/* Same encode as a pure stream call: no host synchronization, all work
 * enqueued on `stream`.
 *   capacity : the caller's bound on offsets[n] (d_ids and d_piece_len hold
 *              at least that many entries); every scratch buffer is sized by
 *              it, so the offsets are never read back.
 *   d_status : DEVICE uint32 status word, zeroed by the caller before a chain
 *              of asynchronous calls.  Every kernel of these calls does
 *              nothing once it is non-zero, and the first failure stores its
 *              spm_status code (first error wins): RESOURCE_EXHAUSTED when
 *              offsets[n] > capacity, or when a sentence the fast kernel
 *              handed to the exact general kernel is longer than its device
 *              scratch (> 256 KiB; spm_hip_encode_batch handles those).
 * The return value reports argument and enqueue errors only.  Models whose
 * encode needs host-sized scratch (unigram pieces of >= 64 bytes, BPE with
 * user-defined symbols, force_general) fall back to the blocking path; WORD
 * and CHAR models never do (both of their tiers are pure stream calls). */
int spm_hip_encode_batch_async(spm_hip_model *model, const uint8_t *d_norm_bytes,
                               const uint64_t *d_offsets, uint64_t n, uint64_t capacity, int32_t *d_ids,
                               uint32_t *d_piece_len, uint64_t *d_tok_offsets, uint32_t *d_status,
                               void *stream);

/* Same contract with HOST buffers; stages through pooled device buffers and
 * returns after the results are copied back.  Small calls of a unigram model
 * (<= 16 sentences: one cooperative launch; <= 256: one tile of the fast
 * kernel) read the input from and write the results to pinned memory.  A BPE
 * model's calls of <= 16 sentences take one launch too (bpe_small_kernel, one
 * wave per sentence) when SPM_HIP_BPE_SMALL_HOST=1 is set: every sentence of
 * <= 1024 bytes is taken; a longer one, a merge that pushes an UNUSED piece
 * and, on a model some of whose pieces hold a char that is no piece itself, a
 * char outside the vocabulary hand the call to the staged path, whose stats
 * then carry coop_rest = n.  Models with USER_DEFINED pieces and
 * force_general never try it.  After 8 such calls in a row the launch is
 * skipped, and tried again on every 64th call. */
int spm_hip_encode_batch_host(spm_hip_model *model, const uint8_t *norm_bytes,
                              const uint64_t *offsets, uint64_t n, int32_t *ids,
                              uint32_t *piece_len, uint64_t *tok_offsets);

/* Batched SentencePieceProcessor::SampleEncode with nbest_size < 0
 * (sentencepiece_processor.cc:622-659): one segmentation per sentence drawn
 * from the unigram lattice (Lattice::Sample, unigram_model.cc:488-526) —
 * subword regularization.  Buffers, blocking behaviour and outputs follow the
 * contract of spm_hip_encode_batch.
 *
 * Lattice: that of Model::PopulateNodes (unigram_model.cc:535-604): positions
 * are chars as SetSentence cuts them, UNUSED pieces are skipped, a
 * USER_DEFINED piece scores length * max_score + 1, one UNK node of score
 * min_score - 10 stands where no one-char piece matched, the trie walk stops
 * at a NUL byte.
 *
 * Forward pass (all terms float): A[0] = 0 and, for each char position p,
 *   A[p] = LogSumExp over nodes (b, p), in ascending b, of
 *          fl(theta * score) + A[b],
 * the first term initialising A[p]; LogSumExp is the reference's
 * (unigram_model.cc:51-63: float storage, double exp / log, the 50 cutoff).
 * This is Lattice::Sample's alpha, which depends on a node's begin position
 * only.
 *
 * Backward pass, from e = len: the candidates are the nodes ending at e in
 * ascending begin order (end_nodes_ insertion order, the longest piece
 * first) with weights
 *   w_i = (float) exp((double) fl(fl(A[b_i] + fl(theta * s_i)) - A[e])),
 * S = w_0 + w_1 + .. summed in double in that order.  Draw u picks the first
 * i with u < (w_0 + .. + w_i) / S, else the last candidate
 * (std::discrete_distribution over probs).  The node becomes a token and
 * e = b_i, until e = 0.  Tokens come out in sentence order; an empty
 * sentence gives zero tokens.
 *
 * Random stream: stateless and counter based, so a result depends neither on
 * the batch shape nor on the kernel that ran the sentence.  On uint64,
 *   mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *           z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   sentence i of a call has global index g = index_base + i,
 *   key = mix(seed + 0x9E3779B97F4A7C15 * (g + 1)),
 *   draw k: u = (mix(key + 0x9E3779B97F4A7C15 * (k + 1)) >> 11) * 2^-53,
 * k = 0 at EOS, counting up along the backward walk; no draw is spent once
 * e = 0.  The reference seeds an mt19937 from random_device, which cannot be
 * reproduced; what is kept is the distribution and the arithmetic above.
 *
 * Status: theta not finite -> SPM_INVALID_ARGUMENT.  A model that is not
 * unigram -> SPM_UNIMPLEMENTED: the reference logs "Not implemented" and
 * returns an empty result (model_interface.h:137-141), which over a C
 * ABI would be indistinguishable from empty input.  A host-only handle ->
 * SPM_FAILED_PRECONDITION.  spm_hip_model_last_stats reports general_path =
 * the sentences the exact (literal lattice) kernel took: those the fast
 * kernel cannot sample exactly (a piece of more than 64 bytes on the walk, a
 * trie leaf inside a UTF-8 char, more than 16 nodes ending at one position),
 * or all of them under spm_hip_model_set_force_general; both kernels run the
 * same float operations in the same order and agree bit for bit. */
int spm_hip_sample_encode_batch(spm_hip_model *model, const uint8_t *d_norm_bytes,
                                const uint64_t *d_offsets, uint64_t n, float theta, uint64_t seed,
                                uint64_t index_base, int32_t *d_ids, uint32_t *d_piece_len,
                                uint64_t *d_tok_offsets, void *stream);
/* Same contract with HOST buffers (offsets start at 0). */
int spm_hip_sample_encode_batch_host(spm_hip_model *model, const uint8_t *norm_bytes,
                                     const uint64_t *offsets, uint64_t n, float theta, uint64_t seed,
                                     uint64_t index_base, int32_t *ids, uint32_t *piece_len,
                                     uint64_t *tok_offsets);
/* Host only: draw `draw` of the sentence with global index `index` under
 * `seed`, the stream above (*u in [0, 1), a multiple of 2^-53). */
int spm_hip_sample_uniform(uint64_t seed, uint64_t index, uint64_t draw, double *u);

/* BPE-dropout: batched SampleEncode of a BPE model, as bpe::Model::SampleEncode
 * of the `sentencepiece` package (0.2.x, bpe_model.cc) does it.  Arguments,
 * capacity, layout and d_piece_len are those of spm_hip_sample_encode_batch;
 * one draw per sentence.  (The vendored v0.1.82 reference has no BPE sampling.)
 *
 * The rule: the merge loop of Encode pops the agenda in order (score
 * descending, left index ascending), discards stale entries, and then drops
 * the popped pair for good with probability alpha, else merges it.  The
 * initial split, the user-defined freeze, rev_merge and the resegmentation of
 * UNUSED pieces are those of Encode.  alpha <= 0 never drops (the result is
 * Encode's), alpha >= 1 always drops (one token per initial symbol); values
 * outside [0, 1], the infinities included, clamp.
 *
 * Random stream: spm_hip_sample_encode_batch's, one decision per pair, named
 * by the pair's bytes.  With start = the offset of the left symbol's first
 * byte in the normalized sentence and end = the offset one past the right
 * symbol's last byte (symbols only grow, so no (start, end) is offered twice
 * in one sentence), sentence i of a call (g = index_base + i) drops the pair
 * when
 *   spm_hip_sample_uniform(seed, g, ((uint64_t) start << 32) | end, &u),
 *   u < (double) alpha,
 * which the kernels test as (mix(..) >> 11) < ceil((double) alpha * 2^53)
 * (spm_hip_bpe_dropout_threshold).  A result depends on (seed, g, sentence,
 * alpha) only: not on the batch, the kernel that ran the sentence or the
 * launch geometry.  The package draws from a process-wide mt19937; what is
 * kept is the distribution.
 *
 * Status: NaN alpha -> SPM_INVALID_ARGUMENT.  A model that is not BPE ->
 * SPM_UNIMPLEMENTED (unigram models sample with
 * spm_hip_sample_encode_batch, which in turn keeps answering
 * SPM_UNIMPLEMENTED for BPE models).  A host-only handle ->
 * SPM_FAILED_PRECONDITION.  n = 0 is fine.  spm_hip_model_last_stats reports
 * general_path = the sentences the literal kernel took: sentences of more
 * than 1024 bytes, those that probe an UNUSED piece or (models whose pieces
 * do not all split into pieces) hold a char outside the vocabulary, every
 * sentence of a model with USER_DEFINED pieces or under
 * spm_hip_model_set_force_general; both kernels give the same result. */
int spm_hip_bpe_dropout_encode_batch(spm_hip_model *model, const uint8_t *d_norm_bytes,
                                     const uint64_t *d_offsets, uint64_t n, float alpha, uint64_t seed,
                                     uint64_t index_base, int32_t *d_ids, uint32_t *d_piece_len,
                                     uint64_t *d_tok_offsets, void *stream);
/* Same contract with HOST buffers (offsets start at 0). */
int spm_hip_bpe_dropout_encode_batch_host(spm_hip_model *model, const uint8_t *norm_bytes,
                                          const uint64_t *offsets, uint64_t n, float alpha, uint64_t seed,
                                          uint64_t index_base, int32_t *ids, uint32_t *piece_len,
                                          uint64_t *tok_offsets);
/* Host only: the integer threshold of alpha, ceil((double) alpha * 2^53)
 * clamped to [0, 2^53].  NaN -> SPM_INVALID_ARGUMENT. */
int spm_hip_bpe_dropout_threshold(float alpha, uint64_t *threshold);

/* Batched SentencePieceProcessor::CalculateEntropy of the `sentencepiece`
 * package (0.2.x): the entropy of every sentence's segmentation distribution
 * at inverse temperature theta, DEVICE pointers, unigram models.
 *
 * Lattice and forward pass A[p]: those of spm_hip_sample_encode_batch above.
 * One float H[p] per char position: H[0] = 0 and, over the nodes (b, p) in
 * ascending b (end_nodes_ order), with s the node's score,
 *   lp   = fl(fl(fl(theta * s) + A[b]) - A[p])
 *   H[p] = fl(H[p] + fl((float) exp((double) lp) * fl(H[b] + lp))).
 * d_entropy[i] = -H[len]; d_log_z[i] (nullable) = A[len], the log partition
 * at theta.  An empty sentence gives -0.0f and log partition 0.  The package
 * takes exp in float; on the package's own fixtures the two agree in all bits
 * on more than 99 % of the lines and within a few units in the last place
 * on the rest.
 *
 * BLOCKING.  Status: theta not finite -> SPM_INVALID_ARGUMENT; a model that
 * is not unigram -> SPM_UNIMPLEMENTED; a host-only handle ->
 * SPM_FAILED_PRECONDITION.  spm_hip_model_last_stats reports general_path =
 * the sentences the exact (literal lattice) kernel took: those with a trie
 * leaf inside a UTF-8 char, or all of them under
 * spm_hip_model_set_force_general.  Both kernels run the same float
 * operations in the same order and agree bit for bit. */
int spm_hip_entropy_batch(spm_hip_model *model, const uint8_t *d_norm_bytes, const uint64_t *d_offsets,
                          uint64_t n, float theta, float *d_entropy, float *d_log_z, void *stream);
/* Same contract with HOST buffers (offsets start at 0). */
int spm_hip_entropy_batch_host(spm_hip_model *model, const uint8_t *norm_bytes, const uint64_t *offsets,
                               uint64_t n, float theta, float *entropy, float *log_z);

/* Batched SampleEncodeAndScore of the package, sampling with replacement
 * (wor = false, include_best = false): num_samples segmentations per sentence
 * drawn as spm_hip_sample_encode_batch draws one, each with its
 * log-probability.  The forward pass runs once per sentence, the backward
 * walk num_samples times.
 *
 * Rows: row i * num_samples + j is sample j of sentence i.
 *   d_tok_offsets : uint64[n * num_samples + 1], row r owns tokens
 *                   [tok_offsets[r], tok_offsets[r + 1])
 *   d_ids / d_piece_len (nullable) : token_capacity entries
 *   d_scores      : float[n * num_samples]
 * token_capacity = num_samples * offsets[n] always suffices.  When the rows
 * hold more tokens than token_capacity the call returns
 * SPM_RESOURCE_EXHAUSTED with d_tok_offsets and d_scores written (so
 * tok_offsets[n * num_samples] is the need) and d_ids / d_piece_len untouched.
 *
 * Score of a row, all float: T = 0, T = fl(T + fl(theta * s)) over the row's
 * nodes from the first to the last, score = fl(T - A[len]).  A row of an
 * empty sentence has no tokens and score 0.
 *
 * Random stream: sample j of the sentence with global index g = index_base +
 * i depends on (seed, g, j) alone.  With mix and the constants of
 * spm_hip_sample_encode_batch,
 *   seed_0 = seed,  seed_j = mix(seed + 0xD1B54A32D192ED03 * j) for j > 0,
 *   key = mix(seed_j + 0x9E3779B97F4A7C15 * (g + 1)),
 * and the draws of the walk follow from the key as above.  So sample 0 is
 * exactly spm_hip_sample_encode_batch's result for (seed, index_base), and
 * sample j is its result for (seed_j, index_base); spm_hip_sample_seed gives
 * seed_j to the host, and spm_hip_sample_uniform(seed_j, g, k, &u) the draws.
 *
 * BLOCKING.  Status: theta not finite or num_samples == 0 ->
 * SPM_INVALID_ARGUMENT; n * num_samples >= 2^31 - 1 -> SPM_OUT_OF_RANGE; a
 * model that is not unigram -> SPM_UNIMPLEMENTED; a host-only handle ->
 * SPM_FAILED_PRECONDITION.  Tiers and spm_hip_model_last_stats as for
 * spm_hip_sample_encode_batch. */
int spm_hip_sample_encode_and_score_batch(spm_hip_model *model, const uint8_t *d_norm_bytes,
                                          const uint64_t *d_offsets, uint64_t n, uint32_t num_samples,
                                          float theta, uint64_t seed, uint64_t index_base, int32_t *d_ids,
                                          uint64_t token_capacity, uint32_t *d_piece_len,
                                          uint64_t *d_tok_offsets, float *d_scores, void *stream);
/* Same contract with HOST buffers (offsets start at 0). */
int spm_hip_sample_encode_and_score_batch_host(spm_hip_model *model, const uint8_t *norm_bytes,
                                               const uint64_t *offsets, uint64_t n, uint32_t num_samples,
                                               float theta, uint64_t seed, uint64_t index_base, int32_t *ids,
                                               uint64_t token_capacity, uint32_t *piece_len,
                                               uint64_t *tok_offsets, float *scores);
/* Host only: seed_j of the stream above. */
int spm_hip_sample_seed(uint64_t seed, uint64_t sample, uint64_t *seed_out);

/* Batched unigram::Model::NBestEncode (unigram_model.cc:729-753 over
 * Lattice::NBest :339-478): the nbest_size best segmentations of every
 * sentence, DEVICE pointers.  Output is model level, like
 * spm_hip_encode_batch: one UNK token per unknown char, no merge.
 *
 * Lattice: that of Model::PopulateNodes, as spelled out above for the
 * sampler.  nbest_size is clamped to [1, 1024] (<= 0 counts as 1).
 *
 * N = 1: the Viterbi path, exactly what spm_hip_encode_batch returns.
 * N >= 2: Viterbi first gives every node its backtrace_score (strict >, the
 * first left node wins).  A* then runs from EOS over hypotheses (node, next,
 * fx, gx), all float: a popped hypothesis pushes one child per node l ending
 * at its node's position, in end_nodes_ insertion order, with
 *   gx = fl(score[l] + gx_top),  fx = fl(backtrace_score[l] + gx_top).
 * The agenda is a binary heap ordered by fx < and moved as libstdc++'s
 * push_heap / pop_heap move a std::priority_queue, which decides the order of
 * equal-fx hypotheses.  A popped BOS hypothesis is a result; the search ends
 * at N results or with an empty agenda, so a lattice with fewer paths returns
 * fewer.  When the agenda holds >= 100000 entries its top min(512, 10 N) are
 * popped in order into a new agenda and the rest dropped.  A path's score is
 * the float sum of its node scores in sentence order starting from 0.0f (it
 * is not fx).  An empty sentence yields one path with no tokens and score 0.
 *
 * Output, a two-level CSR in sentence order (it depends neither on the batch
 * shape nor on the tier that ran a sentence):
 *   d_path_offsets : uint64[n + 1], sentence i owns paths
 *                    [path_offsets[i], path_offsets[i + 1]), best first
 *   d_tok_offsets  : uint64[path_capacity + 1], path p owns tokens
 *                    [tok_offsets[p], tok_offsets[p + 1])
 *   d_ids / d_piece_len (nullable) : token_capacity entries
 *   d_scores       : float[path_capacity]
 *   total_paths / total_tokens : HOST outputs (nullable)
 * path_capacity = n * clamp(N) and token_capacity = clamp(N) * offsets[n]
 * always suffice (at most N paths per sentence, at most one token per byte
 * per path).  When a total exceeds its capacity the call returns
 * SPM_RESOURCE_EXHAUSTED with both totals set and writes none of the five
 * output arrays; a second call with the totals as capacities succeeds.
 *
 * Tiers: a first kernel launch gives every lane an arena of 40 N + 4 L + 64
 * hypotheses (L = the longest sentence, at most 256 bytes); sentences that
 * are longer or outgrow it run again with the same pool split among fewer
 * lanes (16 times the arena); what still does not fit, and every search whose
 * agenda reaches the 100000-entry shrink, is done on the host by the same
 * search over the model's host tables.  All three agree bit for bit.  The
 * host tier runs on one thread and moves each of its sentences separately: it
 * is meant for the few that land there.
 *
 * Memory, kept by the stream's workspace until the model is freed or
 * spm_hip_model_release_stream: search scratch up to 4 GiB, 8 n N bytes of
 * per-path counts and scores, and token staging of N * offsets[n] entries
 * (a third of that, then the exact need, beyond 32 M entries).
 *
 * BLOCKING, like spm_hip_encode_batch.  Status: a model that is not unigram
 * -> SPM_UNIMPLEMENTED (the reference's model returns an empty result there,
 * which the processor turns into INTERNAL; over a C ABI an empty result would
 * be indistinguishable from empty input).  A host-only handle ->
 * SPM_FAILED_PRECONDITION.  spm_hip_model_last_stats reports the call's
 * sentences and tokens, general_path = sentences (every one runs the literal
 * lattice) and, with timing on, general_kernel_ms = the two search launches. */
int spm_hip_nbest_encode_batch(spm_hip_model *model, const uint8_t *d_norm_bytes,
                               const uint64_t *d_offsets, uint64_t n, int32_t nbest_size,
                               int32_t *d_ids, uint32_t *d_piece_len, uint64_t token_capacity,
                               uint64_t *d_tok_offsets, float *d_scores, uint64_t path_capacity,
                               uint64_t *d_path_offsets, uint64_t *total_paths,
                               uint64_t *total_tokens, void *stream);
/* Same contract with HOST buffers (offsets start at 0). */
int spm_hip_nbest_encode_batch_host(spm_hip_model *model, const uint8_t *norm_bytes,
                                    const uint64_t *offsets, uint64_t n, int32_t nbest_size,
                                    int32_t *ids, uint32_t *piece_len, uint64_t token_capacity,
                                    uint64_t *tok_offsets, float *scores, uint64_t path_capacity,
                                    uint64_t *path_offsets, uint64_t *total_paths,
                                    uint64_t *total_tokens);
/* Testing knob: hypothesis arenas of the first and the second device tier
 * (0 = automatic, the sizes above). */
int spm_hip_model_set_nbest_max_hyps(spm_hip_model *model, uint32_t first, uint32_t second);
/* Of the last n-best call on the handle: sentences the second device tier
 * ran, and sentences the host ran. */
int spm_hip_nbest_last_stats(const spm_hip_model *model, uint64_t *second_pass, uint64_t *host_path);

/* Normalizer::Normalize (normalizer.cc:88-211) on host threads, batched:
 * raw CSR lines in, normalized CSR out.  out capacity: 3*in_off[n] + 3*n
 * bytes.  norm_to_orig is not produced.  num_threads <= 0 → hardware
 * concurrency. */
int spm_hip_normalize_batch(const spm_hip_model *model, const uint8_t *in, const uint64_t *in_off,
                            uint64_t n, uint8_t *out, uint64_t *out_off, int num_threads);

/* Normalizer::Normalize (normalizer.cc:88-211, NormalizePrefix :231-300 over
 * the model's precompiled charsmap and user-defined PrefixMatcher) on the
 * device, batched.  DEVICE pointers: raw CSR in (d_in, d_in_off[n+1]),
 * normalized CSR out (d_out, d_out_off[n+1]).  *total receives the normalized
 * byte count; if it exceeds out_capacity nothing is written and the call
 * returns SPM_RESOURCE_EXHAUSTED (allocate *total bytes and call again).
 * norm_to_orig is not produced.  One small read-back (the total). */
int spm_hip_normalize_batch_device(spm_hip_model *model, const uint8_t *d_in,
                                   const uint64_t *d_in_off, uint64_t n, uint8_t *d_out,
                                   uint64_t out_capacity, uint64_t *d_out_off, uint64_t *total,
                                   void *stream);

/* Pure stream version (no host synchronization): the normalized size is not
 * returned; if it exceeds out_capacity (3 * in_off[n] + 3 * n always
 * suffices) nothing is written and *d_status := SPM_RESOURCE_EXHAUSTED (see
 * spm_hip_encode_batch_async for the status-word contract).
 * d_norm_to_orig may be NULL (layout as in the _align variant below). */
int spm_hip_normalize_batch_device_async(spm_hip_model *model, const uint8_t *d_in,
                                         const uint64_t *d_in_off, uint64_t n, uint8_t *d_out,
                                         uint64_t out_capacity, uint64_t *d_out_off,
                                         uint32_t *d_norm_to_orig, uint32_t *d_status, void *stream);

/* Same, also producing norm_to_orig (Normalizer::Normalize's third output,
 * normalizer.cc:88-211): d_norm_to_orig receives, for sentence i, d_out_off
 * [i+1] - d_out_off[i] + 1 uint32 entries at d_norm_to_orig[d_out_off[i] + i]
 * (capacity out_capacity + n): the byte offset in the raw line of the
 * NormalizePrefix chunk each normalized byte came from, then the final
 * `consumed`.  Where the reference returns an empty vector (empty or
 * all-whitespace input) the single entry is the consumed byte count. */
int spm_hip_normalize_batch_device_align(spm_hip_model *model, const uint8_t *d_in,
                                         const uint64_t *d_in_off, uint64_t n, uint8_t *d_out,
                                         uint64_t out_capacity, uint64_t *d_out_off,
                                         uint32_t *d_norm_to_orig, uint64_t *total, void *stream);

/* One SentencePieceText::SentencePiece (sentencepiece.proto) as offsets:
 * piece = normalized[norm_begin, norm_end) of its sentence (empty for the
 * bos/eos pieces of the extra options: piece = IdToPiece(id)), surface =
 * raw line[begin, end). */
typedef struct spm_hip_piece {
  int32_t id;
  uint32_t begin, end;          /* byte offsets into the raw line */
  uint32_t norm_begin, norm_end;/* byte offsets into the normalized line */
} spm_hip_piece;

/* SentencePieceProcessor::Encode(input, SentencePieceText*) on the device
 * (sentencepiece_processor.cc:553-575): Normalize with norm_to_orig, model
 * Encode, PopulateSentencePieceText (:488-551: UNKNOWN runs merged, begin/end
 * through norm_to_orig) and ApplyExtraOptions (:945-979).  DEVICE pointers:
 * raw CSR in; normalized CSR out (capacity norm_capacity bytes, offsets
 * d_norm_off[n+1]); d_norm_to_orig (norm_capacity + n entries, layout as
 * above); pieces CSR out (capacity piece_capacity; d_piece_off[n+1]).
 * *total_norm / *total_pieces receive the sizes; if one exceeds its
 * capacity nothing further is written and SPM_RESOURCE_EXHAUSTED is
 * returned (norm_capacity + n * (bos/eos options) pieces always suffice). */
int spm_hip_encode_spt(spm_hip_model *model, const char *extra_options, const uint8_t *d_raw,
                       const uint64_t *d_raw_off, uint64_t n, uint8_t *d_norm, uint64_t norm_capacity,
                       uint64_t *d_norm_off, uint32_t *d_norm_to_orig, spm_hip_piece *d_pieces,
                       uint64_t piece_capacity, uint64_t *d_piece_off, uint64_t *total_norm,
                       uint64_t *total_pieces, void *stream);

/* Id epilogue of SentencePieceProcessor::Encode(ids) on the device:
 * PopulateSentencePieceText (sentencepiece_processor.cc:488-551 — runs of
 * UNKNOWN pieces merge into one id, :525-529) + ApplyExtraOptions (:945-979)
 * with the option string of SetEncodeExtraOptions ("bos:eos:reverse", parsed
 * as ParseExtraOptions :981-1010; NULL or "" = none).  DEVICE pointers:
 * d_ids / d_tok_offsets[n+1] as produced by spm_hip_encode_batch; output
 * d_out_ids (capacity out_capacity ids; tok_offsets[n] + n * (number of bos
 * and eos options) always suffices) and d_out_offsets[n+1].  *total (may be
 * NULL) receives the output id count; if it exceeds out_capacity nothing is
 * written and SPM_RESOURCE_EXHAUSTED is returned.  One small read-back. */
int spm_hip_finalize_ids(spm_hip_model *model, const char *extra_options, const int32_t *d_ids,
                         const uint64_t *d_tok_offsets, uint64_t n, int32_t *d_out_ids,
                         uint64_t out_capacity, uint64_t *d_out_offsets, uint64_t *total,
                         void *stream);

/* Pure stream version of spm_hip_finalize_ids (status-word contract of
 * spm_hip_encode_batch_async; the output count is in d_out_offsets[n]). */
int spm_hip_finalize_ids_async(spm_hip_model *model, const char *extra_options, const int32_t *d_ids,
                               const uint64_t *d_tok_offsets, uint64_t n, int32_t *d_out_ids,
                               uint64_t out_capacity, uint64_t *d_out_offsets, uint32_t *d_status,
                               void *stream);

/* Byte fallback (TrainerSpec.byte_fallback, field 35: the model carries 256
 * pieces "<0x00>" ... "<0xFF>" of type BYTE = 6).  BYTE pieces are reserved
 * like CONTROL pieces: never matched against text, outside the trie, the BPE
 * pair tables and min_score / max_score.  A BYTE piece in a model without the
 * flag, a BYTE piece whose name is no "<0xXX>", and a model with the flag but
 * without all 256 bytes are load errors, with the sentencepiece package's
 * messages.  *enabled: the flag.  byte_ids (may be NULL): the id of every
 * byte's piece, taken from the pieces' names; -1 without byte fallback.
 * Works on a host-only handle.
 *
 * spm_hip_model_set_piece_types, _set_vocabulary and _reset_vocabulary leave
 * BYTE pieces as they are (get_piece_types reports 6; exchanging BYTE with any
 * other type is SPM_INVALID_ARGUMENT).  This is this engine's rule. */
int spm_hip_model_byte_fallback(const spm_hip_model *model, int *enabled, int32_t byte_ids[256]);

/* spm_hip_finalize_ids for a byte-fallback model.  There PopulateSentencePiece
 * Text does not merge UNKNOWN runs: every UNKNOWN token is replaced by one
 * BYTE id per byte of its normalized text (consecutive unknown chars expand
 * separately), and the extra options apply afterwards ("reverse" reverses the
 * byte ids too).  That needs each token's bytes, so the call takes, besides
 * the arguments of spm_hip_finalize_ids, the normalized text the tokens came
 * from (d_norm_bytes, d_norm_offsets[n+1]: the input of spm_hip_encode_batch)
 * and d_piece_len (the piece lengths spm_hip_encode_batch writes; the tokens
 * of a sentence cover exactly its bytes).  Capacity: normalized bytes + n *
 * (number of bos and eos options) ids always suffice.  On a model without
 * byte fallback the result is that of spm_hip_finalize_ids and the text is
 * not read; on a byte-fallback model spm_hip_finalize_ids[_async] returns
 * SPM_INVALID_ARGUMENT and names this call.  spm_hip_encode_spt needs no
 * sibling: on a byte-fallback model it writes the byte pieces with norm_begin
 * == norm_end (piece = IdToPiece(id)); all byte pieces of a token but the
 * last have begin == end == the token's begin, the last one carries the
 * token's whole surface.  spm_hip_encode_raw_small_host returns
 * SPM_UNIMPLEMENTED for a byte-fallback model. */
int spm_hip_finalize_ids_bytes(spm_hip_model *model, const char *extra_options, const int32_t *d_ids,
                               const uint32_t *d_piece_len, const uint64_t *d_tok_offsets, uint64_t n,
                               const uint8_t *d_norm_bytes, const uint64_t *d_norm_offsets,
                               int32_t *d_out_ids, uint64_t out_capacity, uint64_t *d_out_offsets,
                               uint64_t *total, void *stream);

/* Pure stream version (status-word contract of spm_hip_encode_batch_async; the
 * output count is in d_out_offsets[n]; ids that do not fit: nothing is written
 * and *d_status := SPM_RESOURCE_EXHAUSTED). */
int spm_hip_finalize_ids_bytes_async(spm_hip_model *model, const char *extra_options, const int32_t *d_ids,
                                     const uint32_t *d_piece_len, const uint64_t *d_tok_offsets, uint64_t n,
                                     const uint8_t *d_norm_bytes, const uint64_t *d_norm_offsets,
                                     int32_t *d_out_ids, uint64_t out_capacity, uint64_t *d_out_offsets,
                                     uint32_t *d_status, void *stream);

/* Batched SentencePieceProcessor::Decode(ids) on the device
 * (sentencepiece_processor.cc:670-733): ids -> text.  DEVICE pointers:
 * d_ids / d_tok_offsets[n+1] as produced by spm_hip_encode_batch or
 * spm_hip_finalize_ids (the offsets index d_ids and need not start at 0).
 *
 * Per sentence: the id list, then the option string of
 * SetDecodeExtraOptions ("bos:eos:reverse" applied in the order given,
 * ApplyExtraOptions :945-979, parsed as ParseExtraOptions :981-1023 with its
 * messages; NULL or "" = none), then the surfaces left to right: a CONTROL
 * id gives "", the UNKNOWN id gives TrainerSpec.unk_surface (" \xE2\x81\x87 "
 * unless the model sets it), any other id gives its piece with every U+2581
 * replaced by one space, after one leading U+2581 is dropped if the text built
 * so far is empty (so [<s>, U+2581, U+2581, U+2581 ABC] decodes to "ABC").
 * BYTE ids (byte fallback): a maximal run of consecutive BYTE ids of one
 * sentence, in final order, is decoded greedily as UTF-8 - a valid sequence
 * of k bytes (trail bytes 0x80..0xBF, no overlong form, no surrogate, at most
 * U+10FFFF) gives k - 1 empty surfaces and the char on its last id, a byte
 * that starts no valid sequence inside the run gives U+FFFD.  Byte surfaces
 * are never space-converted or stripped, and a non-empty one makes the text
 * non-empty.  spm_hip_model_decode_bound counts 4 bytes for a BYTE id.
 *
 * Output: d_out_bytes (capacity out_capacity bytes; tokens *
 * spm_hip_model_decode_bound always suffices, tokens counting the bos/eos
 * pieces) and d_out_offsets[n+1], sentence i = bytes [offsets[i],
 * offsets[i+1]).  d_piece_begin (may be NULL): one uint32 per output token in
 * final order (tok_offsets[n] - tok_offsets[0] + n * (number of bos and eos
 * options) entries), the sentence-relative byte offset where the token's
 * surface begins (SentencePieceText begin; end = the next token's begin, or
 * the sentence's length).  *total (may be NULL) receives the byte count.
 * d_out_bytes == NULL counts only: the offsets and *total, nothing else.
 * If the text exceeds out_capacity, the offsets and *total are produced, no
 * text byte and no begin is written and SPM_RESOURCE_EXHAUSTED is returned.
 *
 * The reference indexes pieces(id) unchecked; here an id outside [0,
 * piece_size) gives SPM_OUT_OF_RANGE (the message names the first such
 * sentence and id) and no output is written at all.  One small read-back. */
int spm_hip_decode_batch(spm_hip_model *model, const char *extra_options, const int32_t *d_ids,
                         const uint64_t *d_tok_offsets, uint64_t n, uint8_t *d_out_bytes,
                         uint64_t out_capacity, uint64_t *d_out_offsets, uint32_t *d_piece_begin,
                         uint64_t *total, void *stream);

/* Pure stream version of spm_hip_decode_batch (status-word contract of
 * spm_hip_encode_batch_async: nothing is read or written once *d_status is
 * non-zero; OUT_OF_RANGE or RESOURCE_EXHAUSTED land there, first error wins;
 * the byte count is in d_out_offsets[n]). */
int spm_hip_decode_batch_async(spm_hip_model *model, const char *extra_options, const int32_t *d_ids,
                               const uint64_t *d_tok_offsets, uint64_t n, uint8_t *d_out_bytes,
                               uint64_t out_capacity, uint64_t *d_out_offsets, uint32_t *d_piece_begin,
                               uint32_t *d_status, void *stream);

/* Same contract with HOST buffers (offsets start at 0): uploads, decodes on
 * the device and downloads.  On a host-only handle the same result comes from
 * a plain loop on the calling thread, no GPU needed. */
int spm_hip_decode_batch_host(spm_hip_model *model, const char *extra_options, const int32_t *ids,
                              const uint64_t *tok_offsets, uint64_t n, uint8_t *out_bytes,
                              uint64_t out_capacity, uint64_t *out_offsets, uint32_t *piece_begin,
                              uint64_t *total);

/* The longest surface of any id, in bytes: tokens * bound sizes a decode
 * output without the count call.  Works on host-only handles. */
int spm_hip_model_decode_bound(const spm_hip_model *model, uint32_t *max_surface_bytes);

/* Debug/testing knob: 1 = route every sentence through the exact general
 * kernel (reference-structured lattice), 0 = fast path with automatic
 * fallback (default). */
int spm_hip_model_set_force_general(spm_hip_model *model, int force);
/* 1 = record HIP events around each kernel launch (on the caller's stream)
 * and report their durations in spm_hip_encode_stats. */
int spm_hip_model_set_timing(spm_hip_model *model, int enable);
int spm_hip_model_last_stats(const spm_hip_model *model, spm_hip_encode_stats *stats);
/* Timing enabled: waits for `stream`, then returns the fast-kernel durations
 * (ms, HIP events on `stream`) of the encode calls made on it since the last
 * drain — at most the last 64 — oldest first, and resets the record. */
int spm_hip_model_drain_kernel_times(spm_hip_model *model, void *stream, float *ms, uint32_t capacity,
                                     uint32_t *count);
/* Debug/testing knob: the unigram fast kernel zeroes the EOS back-pointer of
 * sentence `sentence` (batch index; < 0 = off) after its forward pass, as a
 * corrupted scratch byte would.  The backtrace's bound check must turn that
 * into a general-kernel re-run of the sentence (exact output). */
int spm_hip_model_set_debug_corrupt_bp(spm_hip_model *model, int64_t sentence);
/* Tuning/testing knob: unigram models on the wide-char or char fast kernel
 * hand every sentence of at least `min_nb` normalized bytes to the
 * wave-cooperative kernel (one sentence per wavefront, coop_encode.hip);
 * 0 = never.  Default 128 (SPM_HIP_COOP_MIN_NB / SPM_HIP_COOP=0 at load).
 * Byte-kernel models ignore it. */
int spm_hip_model_set_coop_min_nb(spm_hip_model *model, uint32_t min_nb);
/* Tuning/testing knob: where the cooperative kernel's per-char scratch rows
 * live in a batch call.  mode 0 = automatic (rows by byte offset when the
 * call is smaller than the per-wave slabs, else one slab per wave), 1 =
 * always per-wave slabs, 2 = always by byte offset.  slab_chars = chars per
 * wave slab (0: the default 16384); a sentence of more chars goes to the
 * general kernel. */
int spm_hip_model_set_coop_slab(spm_hip_model *model, int mode, uint32_t slab_chars);
/* Releases the encode workspace (device scratch) kept for `stream` after
 * waiting for it.  A handle keeps at most 16 per-stream workspaces and
 * releases the least recently used idle one beyond that; each holds about
 * 13 bytes per normalized input byte of the largest batch seen on its
 * stream plus a 50 MB general-path pool. */
int spm_hip_model_release_stream(spm_hip_model *model, void *stream);

/* ---------------------------------------------------------------------------
 * Unigram trainer E-step (RunEStep, unigram_model_trainer.cc:237-287).
 * pieces: CSR of the TrainerModel piece list (value = list index), scores[V].
 * TrainerModel quirks reproduced: unk_id 0, max_score 0, all pieces NORMAL
 * (unigram_model_trainer.h:39-89).
 * mode: SPM_ESTEP_FAST  — per-sentence fp64 contributions reduced in fp64,
 *                         rounded to float once (not bit-equal to any thread
 *                         count of the reference; tolerance-checked);
 *       SPM_ESTEP_PARITY— emulates num_threads = T ordered float buckets, bit
 *                         exact against the reference at that T.
 * All pointers are DEVICE pointers; expected[V] float, obj float[1], ntok
 * int64[1] are written on `stream`.
 * ------------------------------------------------------------------------ */
enum spm_estep_mode { SPM_ESTEP_FAST = 0, SPM_ESTEP_PARITY = 1 };

typedef struct spm_hip_pieces spm_hip_pieces;

/* Builds the device trie for a piece list (host pointers). */
int spm_hip_pieces_create(const uint8_t *piece_bytes, const uint64_t *piece_offsets,
                          const float *scores, uint64_t num_pieces, spm_hip_pieces **out);
void spm_hip_pieces_free(spm_hip_pieces *pieces);
/* New scores for the same piece list (the next E-step when the M-step only
 * changed scores), keeping the trie and the work buffers.  No call on
 * `pieces` may be in flight on any stream.  num_pieces must equal the
 * create call's (else SPM_OUT_OF_RANGE).  Replaces rebuilding the
 * TrainerModel after each M-step (unigram_model_trainer.cc:97 SetSentencePieces,
 * called at :574) when the M-step kept every piece. */
int spm_hip_pieces_set_scores(spm_hip_pieces *pieces, const float *scores, uint64_t num_pieces);

int spm_hip_estep(spm_hip_pieces *pieces, const uint8_t *d_sent_bytes,
                  const uint64_t *d_sent_offsets, const int64_t *d_freq, uint64_t n,
                  int64_t all_sentence_freq, int mode, int num_threads,
                  float *d_expected, float *d_obj, int64_t *d_ntok, void *stream);

/* Split form for sharded (multi-GPU) E-steps.  The caller owns and zeroes the
 * accumulators and may all-reduce (sum) them across ranks between the two
 * calls (RCCL over xGMI):
 *   FAST  : acc = double[V], acc_obj = double[1], ntok_acc = int64[1]
 *   PARITY: acc = float[T*V] (bucket-major), acc_obj = float[T], ntok_acc = int64[T]
 * Sentence k of this call has global index index_base + k*index_stride; in
 * PARITY mode it belongs to bucket (global index mod T), and every sentence of
 * a bucket must be accumulated on one device, in ascending global order
 * (e.g. rank r of W with T == W passes the sentences r, r+W, ... with
 * index_base = r, index_stride = W).  Zero rows of other ranks' buckets make
 * a SUM all-reduce exact. */
int spm_hip_estep_accumulate(spm_hip_pieces *pieces, const uint8_t *d_sent_bytes,
                             const uint64_t *d_sent_offsets, const int64_t *d_freq, uint64_t n,
                             int64_t all_sentence_freq, int mode, int num_threads,
                             uint64_t index_base, uint64_t index_stride, void *d_acc,
                             void *d_acc_obj, int64_t *d_ntok_acc, void *stream);
int spm_hip_estep_finalize(spm_hip_pieces *pieces, int mode, int num_threads, const void *d_acc,
                           const void *d_acc_obj, const int64_t *d_ntok_acc, float *d_expected,
                           float *d_obj, int64_t *d_ntok, void *stream);
/* PARITY accumulation folds run on a library stream beside `stream`, and an
 * accumulate call normally makes `stream` wait for them before it returns.
 * With SPM_ESTEP_DEFER_FOLD or-ed into `mode`, the call returns without that
 * wait, so a caller feeding many calls (e.g. a corpus larger than its device
 * buffer) keeps the last fold of one call overlapped with the next call's
 * walks.  The accumulators are then complete on `stream` only after
 * spm_hip_estep_sync(pieces, stream) or spm_hip_estep_finalize (which syncs
 * first); read, reduce or free them only after one of the two. */
#define SPM_ESTEP_DEFER_FOLD 0x100
int spm_hip_estep_sync(spm_hip_pieces *pieces, void *stream);
const char *spm_hip_pieces_last_error(const spm_hip_pieces *pieces);
/* The E-step forward pass: 0 (default) the encode byte kernel's E-step mode
 * for accumulate calls of >= 2^20 sentences when the TrainerModel's pieces
 * are whole chars of < 16 bytes (else estep_forward_kernel); 1 that mode for
 * every call it applies to; 2 always estep_forward_kernel.  Results are
 * identical; this selects speed (and lets tests cover both passes). */
int spm_hip_pieces_set_forward(spm_hip_pieces *pieces, int mode);
/* PARITY record counts since the piece set was created: lattice-node records
 * written and records kept after the drop of provable no-ops (a record below
 * a quarter ulp of a lower bound of its float accumulator cannot change it;
 * estep_kernels.hip estep_threshold_kernel).  Diagnostics for the bench. */
int spm_hip_estep_record_stats(spm_hip_pieces *pieces, uint64_t *written, uint64_t *kept);
/* 1 = record HIP events around every accumulate chunk's forward pass and
 * backward pass on the caller's stream (bench roofline). */
int spm_hip_pieces_set_timing(spm_hip_pieces *pieces, int enable);
/* Timing enabled: waits for the recorded events and returns the summed
 * forward / backward pass durations (ms) and the chunk count since the last
 * call, releasing the events. */
int spm_hip_estep_kernel_times(spm_hip_pieces *pieces, double *forward_ms, double *backward_ms, uint64_t *chunks);

/* NBest(2) of PruneSentencePieces (unigram_model_trainer.cc:348-371, over
 * Lattice::NBest unigram_model.cc:339-477) for every piece of the list, on
 * the device, one piece per lane: the lattice of the piece's own string under
 * the TrainerModel, Viterbi, and the A* agenda with std::priority_queue's
 * exact heap order.  DEVICE pointers: the piece CSR (the list `pieces` was
 * created from, longest piece <= max_piece_bytes); d_keep[V]: 1 = always
 * keep, 0 = not, 2 = the search outgrew the device slab (caller re-runs that
 * piece on the host); d_alt at d_alt_off[i] (capacity: the piece's char
 * count) receives d_alt_n[i] ids of the second-best path when d_keep[i] == 1
 * (the reference's `alternatives`).  The slab holds 4096 hypotheses per
 * piece; the environment variable SPM_HIP_PRUNE_MAX_HYPS (tests; clamped to
 * [2, 4096]) lowers the count at which a piece is flagged 2. */
int spm_hip_prune_nbest(spm_hip_pieces *pieces, const uint8_t *d_piece_bytes,
                        const uint64_t *d_piece_off, uint8_t *d_keep, int32_t *d_alt,
                        const uint64_t *d_alt_off, uint32_t *d_alt_n, uint32_t max_piece_bytes,
                        void *stream);

/* Shard plan of a W-rank E-step (spm_train --num_gpus; csrc/shard_plan.h):
 * rank `rank`'s segments as (index_base, index_stride, count) triples, the
 * arguments it passes to spm_hip_estep_accumulate.  Replaces the reference's
 * thread fan-out (unigram_model_trainer.cc:237-287, sentence i -> thread
 * i mod T) with bucket ownership per rank.  Writes at most `capacity`
 * triples into segs (3 * capacity uint64), the full count into *num_segments.
 * Host only (no device calls). */
int spm_hip_estep_shard_plan(uint64_t n, int mode, int num_threads, int world, int rank,
                             uint64_t *segs, uint64_t capacity, uint64_t *num_segments);

/* The rank that accumulates PARITY bucket `bucket` (0 <= bucket < num_threads)
 * under spm_hip_estep_shard_plan with `world` ranks — the rank spm_train's
 * cross-rank reduction gathers that float row from (RCCL send/recv or host
 * copy).  -1 on invalid arguments.  Host only. */
int spm_hip_estep_bucket_owner(int bucket, int num_threads, int world);

/* ---------------------------------------------------------------------------
 * Seed sentencepieces of the unigram trainer: MakeSeedSentencePieces
 * (unigram_model_trainer.cc:124-225, suffix array + internal nodes by esaxx,
 * esa.hxx:37-122), on the current HIP device.  HOST pointers in, results in
 * a host-side handle.
 *   sentences : CSR of the trainer's sentences after LoadSentences (normalized,
 *               rare chars replaced by U+2585), before the whitespace split
 *   chars / char_freq : the required chars with their freq-weighted counts
 *               (LoadSentences' chars_count restricted to required_chars_ —
 *               equal to the all_chars map of :131-139); every char of the
 *               sentences must be listed or be U+2585
 * Result (in seed order, ToLogProb applied): num_chars single chars sorted by
 * (count desc, UTF-8 asc), then substrings sorted by ((R-L)*D desc, suffix-
 * tree node index asc), up to seed_sentencepiece_size entries in total.
 * Limits: total chars + sentences < 2^32, sentences < 65535 chars,
 * max_sentencepiece_length <= 254.
 * ------------------------------------------------------------------------ */
typedef struct spm_hip_seed_options {
  int32_t max_sentencepiece_length;  /* TrainerSpec default 16 */
  int32_t split_by_unicode_script;   /* default 1 */
  int32_t split_by_number;           /* default 1 */
  int32_t split_by_whitespace;       /* default 1 */
  int32_t treat_whitespace_as_suffix;/* default 0 */
  int64_t seed_sentencepiece_size;   /* default 1000000 */
} spm_hip_seed_options;

typedef struct spm_hip_seeds spm_hip_seeds;

int spm_hip_seed_mine(const uint8_t *sent_bytes, const uint64_t *sent_offsets, uint64_t n,
                      const uint32_t *chars, const int64_t *char_freq, uint64_t num_chars,
                      const spm_hip_seed_options *opt, spm_hip_seeds **out);
/* Same with the sentences already in HBM (DEVICE pointers; chars/char_freq/
 * opt stay host pointers). */
int spm_hip_seed_mine_device(const uint8_t *d_sent_bytes, const uint64_t *d_sent_offsets, uint64_t n,
                             const uint32_t *chars, const int64_t *char_freq, uint64_t num_chars,
                             const spm_hip_seed_options *opt, spm_hip_seeds **out);
uint64_t spm_hip_seeds_size(const spm_hip_seeds *seeds);
const uint8_t *spm_hip_seeds_bytes(const spm_hip_seeds *seeds);     /* CSR values */
const uint64_t *spm_hip_seeds_offsets(const spm_hip_seeds *seeds);  /* size + 1 */
const float *spm_hip_seeds_scores(const spm_hip_seeds *seeds);      /* log-probs */
int spm_hip_seeds_stats(const spm_hip_seeds *seeds, uint64_t *num_chars, uint64_t *candidates,
                        float *device_ms);
/* Stage times of the substring pipeline (diagnostics): [0] upload + UTF-8
 * decode, [1] first radix sort (corpora split into parts: the split), [2]
 * the other sort passes (all rounds / parts), [3] capped
 * LCP + min pyramid + candidate nodes, [4] node sorts + gather + download
 * (device ms between stream events, host allocation gaps included), [5]
 * host wall ms inside hipMalloc, [6] prefix-doubling rounds. */
int spm_hip_seeds_stage_times(const spm_hip_seeds *seeds, float *ms, uint32_t capacity, uint32_t *count);
void spm_hip_seeds_free(spm_hip_seeds *seeds);
const char *spm_hip_seed_last_error(void);

/* ---------------------------------------------------------------------------
 * BPE trainer pair census (bpe::Trainer::Train, bpe_model_trainer.cc:200-230,
 * with the first UpdateActiveSymbols' ComputeFreq :87-113): the sentences
 * (DEVICE CSR + freq) decoded to code points, the unique chars and the unique
 * adjacent pairs in first-occurrence order (the reference's symbol creation
 * order), each pair's positions (EncodePos = sid << 32 | l << 16 | r, the
 * ones ComputeFreq keeps) and freq (sum of sentence freq over them).
 * Results live in a host-side handle.  Sentences of more than 65536 chars
 * return SPM_OUT_OF_RANGE (the reference CHECK-fails in EncodePos).
 * ------------------------------------------------------------------------ */
typedef struct spm_hip_bpe_census spm_hip_bpe_census;
int spm_hip_bpe_pair_census(const uint8_t *d_sent_bytes, const uint64_t *d_sent_offsets,
                            const int64_t *d_freq, uint64_t n, spm_hip_bpe_census **out,
                            void *stream);
void spm_hip_bpe_census_free(spm_hip_bpe_census *census);
const char *spm_hip_bpe_census_last_error(void);
/* Accessors (sizes via the *_size outputs). */
int spm_hip_bpe_census_view(const spm_hip_bpe_census *census, const uint32_t **char_codes,
                            const uint64_t **char_offsets, const uint32_t **unique_chars,
                            uint64_t *num_unique_chars, const uint64_t **pair_keys,
                            const uint64_t **pair_freq, const uint64_t **pair_pos_offsets,
                            const uint64_t **pair_positions, uint64_t *num_pairs, float *device_ms);

/* ---------------------------------------------------------------------------
 * BPE merge loop: the pair-frequency refresh of UpdateActiveSymbols
 * (bpe_model_trainer.cc:153-183 -> ComputeFreq :87-113, every bigram whose
 * freq was reset) on device-resident state.  create() uploads the sentences'
 * symbol ids (flat; sentence i = [sent_offsets[i], sent_offsets[i + 1]); -1 =
 * a char merged into its left neighbour), the sentence freqs and every
 * bigram's position set as (symbol id, EncodePos) entries sorted by (symbol,
 * position).  Each run() first applies the merge loop's changes since the
 * previous run -- symbol writes (flat index << 32 | uint32 value), positions
 * the host erased, positions inserted (sorted by (symbol, position); only
 * those still in the set) -- then recomputes the freq of every `todo`
 * symbol (triples: symbol id, left symbol id, right symbol id) exactly as
 * ComputeFreq does, erasing the positions it erases.  freq_out[k] is the
 * k-th todo symbol's freq; the erased positions come back as (symbol,
 * position) views valid until the next call; the caller removes them from its
 * own sets.  Host pointers throughout; one call = one upload, one
 * synchronization.
 *
 * The order within a run() is writes, erases, inserts, todo.  So a position
 * in both the erase and the insert list ends in the set, an erase of a
 * position that is not in the set does nothing, and a position erased earlier
 * (by the caller or by a refresh) may be inserted again: it is then in the set
 * once.  Left to the caller: at most one write per flat index (they are
 * scattered in parallel); the insert list sorted and free of duplicates, and
 * no insert of a position that is in the device's set already (it would be
 * held, and counted, twice); each symbol at most once in `todo`; every
 * position inside its sentence.  A symbol without entries has freq 0.  With
 * num_todo == 0 the changes are applied and *num_erased is 0.  Erased entries
 * keep their slot, so num_entries of stats() only grows.
 * ------------------------------------------------------------------------ */
typedef struct spm_hip_bpe_refresh spm_hip_bpe_refresh;
int spm_hip_bpe_refresh_create(const int32_t *syms, const uint64_t *sent_offsets, const int64_t *sent_freq,
                               uint64_t num_sentences, const uint32_t *pos_sym, const uint64_t *pos_key,
                               uint64_t num_positions, void *stream, spm_hip_bpe_refresh **out);
int spm_hip_bpe_refresh_run(spm_hip_bpe_refresh *refresh, const uint64_t *sym_writes, uint64_t num_writes,
                            const uint32_t *ins_sym, const uint64_t *ins_key, uint64_t num_inserts,
                            const uint32_t *del_sym, const uint64_t *del_key, uint64_t num_erases,
                            const uint32_t *todo, uint64_t num_todo, uint64_t *freq_out,
                            const uint32_t **erased_sym, const uint64_t **erased_key, uint64_t *num_erased);
/* Entries held (alive or erased) and the device time of all runs so far. */
int spm_hip_bpe_refresh_stats(const spm_hip_bpe_refresh *refresh, uint64_t *num_entries, float *device_ms);
void spm_hip_bpe_refresh_free(spm_hip_bpe_refresh *refresh);

/* ---------------------------------------------------------------------------
 * Diagnostics (measurement only; not part of the reference surface).
 * Trie work of unigram Encode over a batch of normalized sentences (HOST
 * pointers), counted on host threads the way the reference's PopulateNodes
 * walks darts (unigram_model.cc:535-604, darts.h:469-512): one walk per char
 * start; every byte step is one dependent unit load (the mismatching probe
 * included), every matched leaf one value/score load.  units_below[k] counts
 * the unit loads that hit a unit index < (512 << k): how much of the walk an
 * LDS-resident top of the array of that size would serve.
 * ------------------------------------------------------------------------ */
typedef struct spm_hip_trie_stats {
  uint64_t char_starts;
  uint64_t unit_loads;
  uint64_t leaf_loads;
  uint64_t max_depth;
  uint64_t units_below[8];
  /* Wave-schedule model of the fast kernel (256-sentence blocks sorted by
   * length, 64-lane waves, byte positions walked in lockstep pairs): sum over
   * waves of the dependent load rounds, and the same if every lane walked its
   * own positions back to back (two chains per lane). */
  uint64_t lockstep_rounds;
  uint64_t decoupled_rounds;
  uint64_t waves;
} spm_hip_trie_stats;
int spm_hip_model_trie_stats(const spm_hip_model *model, const uint8_t *norm_bytes,
                             const uint64_t *offsets, uint64_t n, int num_threads,
                             spm_hip_trie_stats *out);

/* Diagnostic (works on host-only handles): looks bytes[0:len) up in the
 * piece -> (id, node score) table the byte kernel's backtrace reads, on the
 * host copy and with the kernel's hash and probe sequence.  SPM_OK: found,
 * *id and *score (nullable) are the usable trie node's id and score (a
 * USER_DEFINED piece: chars * max_score + 1).  SPM_NOT_FOUND: no usable
 * node has these bytes (UNUSED pieces, inner nodes, an embedded NUL, the
 * empty key, more than 15 bytes).  SPM_FAILED_PRECONDITION: the model has no
 * such table (not a byte-kernel model). */
int spm_hip_model_piece_lookup(const spm_hip_model *model, const uint8_t *bytes, uint64_t len, int32_t *id,
                               float *score);

/* Raw lines -> the final ids of SentencePieceProcessor::Encode(line, &ids)
 * (sentencepiece_processor.cc:319-330: Normalizer::Normalize, normalizer.cc:
 * 88-211; ModelInterface::Encode, unigram_model.cc:705-720 / bpe_model.cc:
 * 37-199; the unknown-run merge of PopulateSentencePieceText, :488-551) with
 * no extra options, for 1..16 lines of a unigram or BPE model in ONE device
 * launch: raw image up and ids down through pinned host memory, one
 * completion word polled (the per-line path of spm_encode_main.cc:189-191).
 * ids_cap entries in ids, n + 1 offsets in out_off.  SPM_UNIMPLEMENTED: the
 * fused path does not take this call, nothing was written: run
 * spm_hip_normalize_batch_device + spm_hip_encode_batch + spm_hip_finalize_ids
 * instead.  Never taken: more lines, a line of > 1024 bytes, a WORD or CHAR
 * model, a byte-fallback model, force_general, a unigram model without a fast
 * kernel, a BPE model with USER_DEFINED pieces.  Unigram: not taken when a
 * sentence's lattice needs the general kernel.  BPE (bpe_raw_kernel, one wave
 * per line): not taken when a line's normalized form has > 1024 bytes, when a
 * merge pushes an UNUSED piece (a restricted vocabulary: it needs the general
 * kernel's resegmentation) and, on a model some of whose pieces hold a char
 * that is no piece itself, on a char outside the vocabulary; after 8 such
 * calls in a row the launch is skipped (SPM_UNIMPLEMENTED at once), every
 * 64th call tries again, a taken call and spm_hip_model_set_piece_types start
 * the count over.  A BPE call's stats: sentences = n; tokens when taken;
 * coop_rest = n when the kernel ran and handed the call back.
 * SPM_RESOURCE_EXHAUSTED: more ids than ids_cap (4 * raw bytes + 8 * n + 64
 * always suffices). */
int spm_hip_encode_raw_small_host(spm_hip_model *model, const uint8_t *raw, const uint64_t *raw_off,
                                  uint64_t n, int32_t *ids, uint64_t ids_cap, uint64_t *out_off);

/* Vocabulary restriction (SentencePieceProcessor::SetVocabulary /
 * ResetVocabulary, sentencepiece_processor.cc:203-245): piece types change
 * on the loaded model, in place.  As in the reference, only the types
 * change: the model built at load stays, so min_score / max_score and with
 * them the unknown score (min_score - 10) and the USER_DEFINED node scores,
 * the trie and the BPE pair and rank tables keep their load-time contents.
 * A restricted handle is therefore NOT the handle of a model file whose types
 * were edited.  Everything this engine derives from the types is brought up
 * to date: max_piece_chars, the unigram kernel tier and ring width (get_info
 * reports them), the near-tie bound, the cooperative kernel's switch (reset
 * to its default rule), the kind bits and usable-node scores of the per-unit
 * tables and the unused bit of the BPE pair entries (re-tagged on the device
 * from one uploaded byte per piece), the byte kernel's piece table and the
 * BPE per-piece kinds (rebuilt on the host).  The call waits for all work of
 * this handle's streams, ends its resident small-call servers (the next small
 * call restarts them) and returns when the tables are in place; it must not
 * overlap any other call on the handle.  Works on host-only handles (info,
 * piece_lookup and the host n-best tier follow).
 *
 * types: ModelProto::SentencePiece::Type per piece id (1 NORMAL, 2 UNKNOWN,
 * 3 CONTROL, 4 USER_DEFINED, 5 UNUSED), n = piece_size.  Only NORMAL <->
 * UNUSED changes are accepted: SPM_INVALID_ARGUMENT for any other change or a
 * wrong n, and nothing is changed then. */
int spm_hip_model_set_piece_types(spm_hip_model *model, const uint8_t *types, uint64_t n);
int spm_hip_model_get_piece_types(const spm_hip_model *model, uint8_t *types, uint64_t n);
/* SetVocabulary's rule over the model's own pieces: CONTROL, UNKNOWN and
 * USER_DEFINED pieces stay; any other piece becomes NORMAL if it is one of
 * the num_pieces given (CSR: piece_bytes, piece_offsets[num_pieces + 1]) or
 * is one character long (OneCharLen(piece) == piece.size()), else UNUSED.
 * UNIGRAM and BPE models only: otherwise SPM_INTERNAL "Vocabulary constraint
 * is only enabled in subword units."  ResetVocabulary: every UNUSED piece
 * becomes NORMAL, on any model type. */
int spm_hip_model_set_vocabulary(spm_hip_model *model, const uint8_t *piece_bytes, const uint64_t *piece_offsets,
                                 uint64_t num_pieces);
int spm_hip_model_reset_vocabulary(spm_hip_model *model);

/* Piece counting (spm_encode --generate_vocabulary, spm_encode_main.cc:
 * 98-109): d_counts[id] += the occurrences of id in d_ids[0, num_tokens),
 * d_counts = uint64[piece_size], accumulated over calls (zero it first).  An
 * id outside [0, piece_size) is skipped, never used as an index, and sets bit
 * 0 of *d_status (nullable).  Enqueued on `stream`, no host synchronization.
 * Equal ids are summed on chip before global memory is touched: in
 * per-workgroup LDS bins for up to 32768 pieces, else by a wave-level
 * combine.  The _host form takes host pointers (counts is read, added to
 * and written back; *status nullable) and blocks. */
int spm_hip_count_ids(spm_hip_model *model, const int32_t *d_ids, uint64_t num_tokens, uint64_t *d_counts,
                      uint32_t *d_status, void *stream);
int spm_hip_count_ids_host(spm_hip_model *model, const int32_t *ids, uint64_t num_tokens, uint64_t *counts,
                           uint32_t *status);

/* Dense id batches: a final id CSR on the device as the rectangular int32
 * tensor a training or inference loop on the same GPU takes, without a trip
 * to the host.  No reference counterpart (the reference returns one
 * std::vector<int> per sentence).  DEVICE pointers: d_ids / d_offsets[n+1] as
 * produced by spm_hip_encode_batch or spm_hip_finalize_ids; the offsets index
 * d_ids and need not start at 0.  row_len = L.  Any int32 is a legal pad_id
 * (the model's own pad id is -1 unless trained otherwise; -100 is a common
 * label filler).
 *
 * Pad: one sentence per row.  len = offsets[i+1] - offsets[i], k = min(len, L).
 * Tokens [0, k) go to columns [0, k) and pad_id to [k, L).  Flags:
 *   SPM_DENSE_PAD_LEFT       the tokens go to columns [L-k, L), the pads in front
 *   SPM_DENSE_TRUNCATE_LEFT  tokens [len-k, len) are kept
 *   SPM_DENSE_KEEP_END       a sentence that is cut keeps its outermost token on
 *                            the cut side: cut on the right, the last kept slot
 *                            holds token len-1; cut on the left, the first kept
 *                            slot holds token 0.  A bos / eos of the extra
 *                            options survives; L = 1 is legal and gives that token
 * Outputs: d_out[n*L]; nullable d_lengths[n] (int32, = k), d_mask[n*L] (uint8,
 * 1 on token slots) and d_stats[2] (uint64: sentences cut, tokens dropped).  An
 * empty sentence gives a row of pads with length 0.
 *
 * Pack: the LM-pretraining layout.  The sentences' ids run on, in order, as
 * one stream of T = offsets[n] - offsets[0] slots; slot t stands in row t / L,
 * column t % L, and the rest of the last row holds pad_id.  Empty sentences
 * contribute nothing.  Outputs: d_out[rows_capacity*L]; nullable d_seq (int32
 * per slot: the index i of the slot's sentence, -1 on padding), d_pos (int32
 * per slot: t - (offsets[i] - offsets[0]), which keeps counting where a
 * sentence crosses a row edge; 0 on padding) and d_stats[2] (uint64: rows
 * needed = ceil(T / L), T).  Rows beyond rows_capacity are not written and
 * rows between ceil(T / L) and rows_capacity are not touched, so a caller who
 * sized by d_stats[0], or by the total spm_hip_finalize_ids returns, gets
 * exactly its rows.  Packing whole sentences into rows without splitting them
 * (bin packing) is out of scope.
 *
 * The device calls are pure stream calls in the sense of the _async entries:
 * they allocate nothing, do not synchronize and read nothing back, and every
 * failure is an argument check on the host before anything is enqueued.  They
 * take no model handle (they need no workspace), so any stream will do.
 * SPM_INVALID_ARGUMENT: row_len == 0 or > INT32_MAX, a null d_out or
 * d_offsets, an unknown flag bit.  SPM_OUT_OF_RANGE: pack with n > INT32_MAX
 * (seq is int32); pad with n * row_len past 64 bits.  n == 0 is fine: no
 * output slot is written and d_stats = {0, 0}.  The _host forms take host
 * pointers, run the same per-slot rule in a plain loop on the calling thread
 * and never touch the GPU. */
#define SPM_DENSE_PAD_LEFT 0x1u
#define SPM_DENSE_TRUNCATE_LEFT 0x2u
#define SPM_DENSE_KEEP_END 0x4u
int spm_hip_pad_ids(const int32_t *d_ids, const uint64_t *d_offsets, uint64_t n, uint32_t row_len,
                    int32_t pad_id, uint32_t flags, int32_t *d_out, int32_t *d_lengths, uint8_t *d_mask,
                    uint64_t *d_stats, void *stream);
int spm_hip_pack_ids(const int32_t *d_ids, const uint64_t *d_offsets, uint64_t n, uint32_t row_len,
                     int32_t pad_id, uint64_t rows_capacity, int32_t *d_out, int32_t *d_seq, int32_t *d_pos,
                     uint64_t *d_stats, void *stream);
int spm_hip_pad_ids_host(const int32_t *ids, const uint64_t *offsets, uint64_t n, uint32_t row_len,
                         int32_t pad_id, uint32_t flags, int32_t *out, int32_t *lengths, uint8_t *mask,
                         uint64_t *stats);
int spm_hip_pack_ids_host(const int32_t *ids, const uint64_t *offsets, uint64_t n, uint32_t row_len,
                          int32_t pad_id, uint64_t rows_capacity, int32_t *out, int32_t *seq, int32_t *pos,
                          uint64_t *stats);

/* Device memory this library holds in the calling process (every block it
 * allocates: models' workspaces, E-step piece sets, trainer corpus and
 * scratch): live bytes now and the high-water mark since the last reset.
 * No reference counterpart (the reference holds no device memory); bench.py
 * reports the peak per rank. */
int spm_hip_device_bytes(uint64_t *live, uint64_t *peak);
void spm_hip_device_peak_reset(void);

/* Human-readable message of the last error on this thread. */
const char *spm_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SPM_HIP_H_ */
