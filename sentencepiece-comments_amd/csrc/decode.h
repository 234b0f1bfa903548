// Decode (ids -> text): the per-id surface table, the host loop and the
// device launches of decode_kernels.hip.  Internal; the public entries are
// spm_hip_decode_batch and its siblings.
//
// Reference: SentencePieceProcessor::Decode (sentencepiece_processor.cc:670-733)
// after ApplyExtraOptions (:945-979).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "epilogue.h"

namespace spm_amd {

// Tokens per sub-tile (one per thread of a block) and per tile: a block scans
// and copies kDecodeSubTile tokens at a time, and block ranges are multiples
// of kDecodeTile tokens.
constexpr uint32_t kDecodeSubTile = 256;
constexpr uint32_t kDecodeTile = 1024;
// Blocks of every token pass; block b owns one contiguous token range.
constexpr uint32_t kDecodeBlocks = 1024;
// Longest surface the table accepts (a sub-tile's byte count stays in 32 bits).
constexpr uint32_t kDecodeMaxSurface = 1u << 22;

// Per-id decoded surface: `meta[id]` = (byte length << 1) | strip, `off[id]`
// its start in `bytes`.  The surface has every U+2581 replaced by a space; a
// CONTROL id has length 0, the UNKNOWN id holds unk_surface.  strip = 1: the
// piece starts with U+2581 and loses its first byte while the text is empty.
struct DecodeTable {
  std::vector<uint32_t> meta, off;
  std::vector<uint8_t> bytes;
  uint32_t max_surface = 0;
};

// Control words of one call (device, uint64 each).
enum DecodeCtl : int { kDcTotal = 0, kDcBadKey = 1, kDcBadSentence = 2, kDcBadId = 3, kDcStatus = 4, kDcWords = 5 };

struct DecodeLaunch {
  const int32_t *ids;
  const uint64_t *tok_off;
  uint64_t n;
  const uint32_t *meta, *off;
  const uint8_t *bytes;
  int32_t num_pieces;
  EpilogueExtras x;
  uint32_t *first;      // n words: first position whose stripped surface is non-empty
  uint64_t *block_sum;  // kDecodeBlocks words
  uint64_t *ctl;        // kDcWords words; kDcBadKey preset to ~0, the rest 0
  uint32_t *chain;      // status word: nothing runs once it is non-zero
  uint8_t *out;         // nullable: count only
  uint64_t capacity;
  uint64_t *out_off;
  uint32_t *piece_begin;  // nullable
};
// Enqueues the whole call (first-position pass, count pass, write pass, offset
// fill) on st.  resolve_bad: also resolve the first out-of-range id into
// ctl[kDcBadSentence], ctl[kDcBadId].
hipError_t LaunchDecode(const DecodeLaunch &a, bool resolve_bad, hipStream_t st);

// The same computation as a plain loop over host buffers.  Returns 0, or
// SPM_OUT_OF_RANGE with *bad_sentence / *bad_id set and nothing written.
// out == nullptr counts only; out_off[n + 1] is always written on success, the
// text and piece_begin only if the total fits `capacity`.
inline int DecodeHostLoop(const DecodeTable &t, const EpilogueExtras &x, const int32_t *ids,
                          const uint64_t *tok_off, uint64_t n, uint8_t *out, uint64_t capacity,
                          uint64_t *out_off, uint32_t *piece_begin, uint64_t *bad_sentence, int32_t *bad_id) {
  const int32_t v = static_cast<int32_t>(t.meta.size());
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t k = tok_off[i]; k < tok_off[i + 1]; ++k)
      if (ids[k] < 0 || ids[k] >= v) {
        *bad_sentence = i;
        *bad_id = ids[k];
        return SPM_OUT_OF_RANGE;
      }
  const uint32_t extras = x.num_pre + x.num_post;
  for (int pass = 0; pass < 2; ++pass) {
    const bool write = pass == 1;
    if (write && (!out || out_off[n] > capacity)) break;
    uint64_t pos = 0, g = 0;
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t b = tok_off[i], m = tok_off[i + 1] - b, count = m + extras;
      const uint64_t begin = pos;
      bool empty = true;  // the text of this sentence is still empty
      for (uint64_t p = 0; p < count; ++p, ++g) {
        int32_t id;
        if (p < x.num_pre) id = x.ids[p];
        else if (p < x.num_pre + m) id = ids[b + (x.reversed ? m - 1 - (p - x.num_pre) : p - x.num_pre)];
        else id = x.ids[kMaxExtras + (p - x.num_pre - m)];
        const uint32_t strip = empty ? (t.meta[id] & 1u) : 0u;
        const uint32_t len = (t.meta[id] >> 1) - strip;
        if (write) {
          if (len) std::memcpy(out + pos, t.bytes.data() + t.off[id] + strip, len);
          if (piece_begin) piece_begin[g] = static_cast<uint32_t>(pos - begin);
        }
        pos += len;
        if (len) empty = false;
      }
      if (!write) out_off[i] = begin;
    }
    if (!write) out_off[n] = pos;
  }
  return SPM_OK;
}

}  // namespace spm_amd
