// Device id epilogue (PopulateSentencePieceText unk merge + ApplyExtraOptions),
// see epilogue_kernels.hip.  Internal; the public entry is spm_hip_finalize_ids.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/spm_hip.h"

namespace spm_amd {

// Per-piece type bits (ModelProto::SentencePiece::Type, sentencepiece_model.proto).
constexpr uint8_t kPieceUnknown = 1;
constexpr uint8_t kPieceControl = 2;
constexpr uint8_t kPieceByte = 4;

constexpr int kMaxExtras = 32;

// Extra options folded on the host: out = pre · mid (reversed?) · post.
struct EpilogueExtras {
  int32_t ids[2 * kMaxExtras];  // [0, num_pre): pre; [kMaxExtras, kMaxExtras + num_post): post
  uint32_t num_pre;
  uint32_t num_post;
  uint32_t reversed;
};

// chain (nullable): an asynchronous call's status word; the kernels do
// nothing once it is non-zero, and an output larger than cap_limit is not
// written (chain := RESOURCE_EXHAUSTED).
hipError_t LaunchEpilogueCount(const int32_t *ids, const uint64_t *tok_off, uint64_t n, const uint8_t *types,
                               int32_t num_types, uint32_t extras, uint64_t *count, hipStream_t st,
                               const uint32_t *chain = nullptr);
hipError_t LaunchEpilogueWrite(const int32_t *ids, const uint64_t *tok_off, uint64_t n, const uint8_t *types,
                               int32_t num_types, const EpilogueExtras &x, const uint64_t *out_off,
                               int32_t *out, hipStream_t st, uint64_t cap_limit = ~0ull,
                               uint32_t *chain = nullptr);

// SentencePieceText epilogue: the merged pieces with begin/end through
// norm_to_orig (layout of spm_hip_normalize_batch_device_align).
hipError_t LaunchSptWrite(const int32_t *ids, const uint32_t *lens, const uint64_t *tok_off, uint64_t n,
                          const uint8_t *types, int32_t num_types, const EpilogueExtras &x,
                          const uint32_t *n2o, const uint64_t *norm_off, const uint64_t *out_off,
                          spm_hip_piece *out, hipStream_t st);

// The epilogue of a byte-fallback model (byte_epilogue_kernels.hip): an
// UNKNOWN token becomes one BYTE id per byte of its normalized text.
struct ByteEpilogueLaunch {
  const int32_t *ids;       // model-level tokens of the batch
  const uint32_t *len;      // their byte lengths
  const uint64_t *tok_off;  // n + 1
  uint64_t n;
  const uint8_t *norm;       // normalized bytes
  const uint64_t *norm_off;  // n + 1
  const uint8_t *types;
  int32_t num_types;
  const int32_t *byte_ids;  // 256: byte -> id of its BYTE piece
  EpilogueExtras x;
  uint64_t *block_sum;  // 2 * kDecodeBlocks words
  uint64_t *ctl;        // [0]: the output count (written by the count launch)
  uint32_t *chain;      // status word, never null: nothing runs once it is non-zero
  bool check_capacity;  // the count launch sets RESOURCE_EXHAUSTED when the count exceeds capacity
  uint64_t capacity;
  uint64_t *out_off;       // n + 1
  int32_t *out;            // ids, or
  spm_hip_piece *out_spt;  // pieces (non-null selects them), with
  const uint32_t *n2o;     // norm_to_orig (layout of spm_hip_normalize_batch_device_align)
};
// Count, offset and fill passes: out_off[n + 1], ctl[0].
hipError_t LaunchByteEpilogueCount(const ByteEpilogueLaunch &a, hipStream_t st);
// Write and extras passes; needs the offsets of the count launch.
hipError_t LaunchByteEpilogueWrite(const ByteEpilogueLaunch &a, hipStream_t st);

}  // namespace spm_amd
