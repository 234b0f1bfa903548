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

// meta[id] of a BYTE piece (byte fallback): the flag and the piece's byte in
// the low 8 bits.  A table surface is at most kDecodeMaxSurface bytes, so the
// flag bit is free, and a model without BYTE pieces never sets it.
constexpr uint32_t kDecodeByteFlag = 0x80000000u;

// Bytes of the valid UTF-8 sequence that starts at b[0] when `avail` bytes are
// left in the run, 0 when there is none: trail bytes 0x80..0xBF, no overlong
// form, no surrogate, at most U+10FFFF.
__host__ __device__ inline uint32_t Utf8ValidLen(const uint8_t *b, uint32_t avail) {
  const uint32_t b0 = b[0];
  if (b0 < 0x80) return 1;
  if (avail >= 2 && (b0 & 0xE0) == 0xC0) {
    const uint32_t cp = ((b0 & 0x1Fu) << 6) | (b[1] & 0x3Fu);
    return (b[1] & 0xC0) == 0x80 && cp >= 0x80 ? 2 : 0;
  }
  if (avail >= 3 && (b0 & 0xF0) == 0xE0) {
    const uint32_t cp = ((b0 & 0x0Fu) << 12) | ((b[1] & 0x3Fu) << 6) | (b[2] & 0x3Fu);
    return (b[1] & 0xC0) == 0x80 && (b[2] & 0xC0) == 0x80 && cp >= 0x800 && !(cp >= 0xD800 && cp < 0xE000) ? 3 : 0;
  }
  if (avail >= 4 && (b0 & 0xF8) == 0xF0) {
    const uint32_t cp = ((b0 & 0x07u) << 18) | ((b[1] & 0x3Fu) << 12) | ((b[2] & 0x3Fu) << 6) | (b[3] & 0x3Fu);
    return (b[1] & 0xC0) == 0x80 && (b[2] & 0xC0) == 0x80 && (b[3] & 0xC0) == 0x80 && cp >= 0x10000 && cp <= 0x10FFFF
               ? 4
               : 0;
  }
  return 0;
}

// Surface of one BYTE token inside its run (a maximal sequence of consecutive
// BYTE tokens of one sentence, final order), decoded greedily as UTF-8: a
// valid sequence of k bytes gives k - 1 empty surfaces and the char on its
// last token, a byte that starts no valid sequence gives U+FFFD.  A trail
// byte never starts a sequence and a sequence holds only trail bytes after
// its lead, so every lead byte of the run is reached by the greedy walk, and
// a trail byte is inside a sequence exactly when one of the 3 bytes before it
// starts a valid sequence that reaches it.  Hence the surface follows from
// the token's byte and 3 neighbours on each side: w[k] is the byte at distance
// k - 3, lo / hi (0..3) count the neighbours before / after that belong to the
// run.  Returns the surface's length (0..4) and its bytes in out.
__host__ __device__ inline uint32_t ByteRunSurface(const uint8_t w[7], uint32_t lo, uint32_t hi, uint8_t out[4]) {
  const uint8_t c = w[3];
  if ((c & 0xC0) == 0x80) {
    for (uint32_t d = 1; d <= lo; ++d) {
      const uint32_t avail = d + 1 + hi < 4 ? d + 1 + hi : 4;
      const uint32_t v = Utf8ValidLen(w + 3 - d, avail);
      if (v <= d) continue;
      if (v != d + 1) return 0;  // inside the sequence, not its last byte
      for (uint32_t k = 0; k < v; ++k) out[k] = w[3 - d + k];
      return v;
    }
  } else {
    const uint32_t v = Utf8ValidLen(w + 3, 1 + hi);
    if (v == 1) {
      out[0] = c;
      return 1;
    }
    if (v > 1) return 0;
  }
  out[0] = 0xEF;  // U+FFFD
  out[1] = 0xBF;
  out[2] = 0xBD;
  return 3;
}

// Per-id decoded surface: `meta[id]` = (byte length << 1) | strip, `off[id]`
// its start in `bytes`.  The surface has every U+2581 replaced by a space; a
// CONTROL id has length 0, the UNKNOWN id holds unk_surface.  strip = 1: the
// piece starts with U+2581 and loses its first byte while the text is empty.
struct DecodeTable {
  std::vector<uint32_t> meta, off;
  std::vector<uint8_t> bytes;
  uint32_t max_surface = 0;
  bool has_bytes = false;  // some id is a BYTE piece (meta = kDecodeByteFlag | byte)
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
  bool has_bytes;  // DecodeTable::has_bytes: the kernels with the byte-run rule
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
      auto id_at = [&](uint64_t q) -> int32_t {  // the id at position q of the sentence, final order
        if (q < x.num_pre) return x.ids[q];
        if (q < x.num_pre + m) return ids[b + (x.reversed ? m - 1 - (q - x.num_pre) : q - x.num_pre)];
        return x.ids[kMaxExtras + (q - x.num_pre - m)];
      };
      for (uint64_t p = 0; p < count; ++p, ++g) {
        const int32_t id = id_at(p);
        uint32_t strip = 0, len;
        uint8_t lit[4];
        const uint8_t *src;
        if (t.meta[id] & kDecodeByteFlag) {
          // The byte run around p, at most 3 tokens each way.
          uint8_t w[7] = {};
          w[3] = static_cast<uint8_t>(t.meta[id]);
          uint32_t lo = 0, hi = 0;
          while (lo < 3 && p > lo && (t.meta[id_at(p - lo - 1)] & kDecodeByteFlag)) {
            ++lo;
            w[3 - lo] = static_cast<uint8_t>(t.meta[id_at(p - lo)]);
          }
          while (hi < 3 && p + hi + 1 < count && (t.meta[id_at(p + hi + 1)] & kDecodeByteFlag)) {
            ++hi;
            w[3 + hi] = static_cast<uint8_t>(t.meta[id_at(p + hi)]);
          }
          len = ByteRunSurface(w, lo, hi, lit);
          src = lit;
        } else {
          strip = empty ? (t.meta[id] & 1u) : 0u;
          len = (t.meta[id] >> 1) - strip;
          src = t.bytes.data() + t.off[id] + strip;
        }
        if (write) {
          if (len) std::memcpy(out + pos, src, len);
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
