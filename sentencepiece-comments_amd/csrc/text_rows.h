// Text rows: the text around the encode kernels.  A byte buffer of lines as
// the sentence CSR every batch entry takes (split), and a final id CSR or the
// piece records of spm_hip_encode_spt as the text spm_encode prints (id rows,
// piece rows).  Internal; the public entries are spm_hip_split_lines,
// spm_hip_format_id_rows, spm_hip_format_piece_rows and their _host siblings.
// The per-row rules are stated once here, as the host loops; the kernels of
// text_rows.hip compute the same bytes.
//
//   split     : std::getline.  A line ends at '\n' (a '\r' before it is kept),
//               a final fragment without '\n' is a line, a buffer that ends in
//               '\n' gives no extra line, every other byte passes through.
//   id rows   : the ids of a row in decimal joined by ' ', then '\n'.
//   piece rows: the pieces of a row joined by ' ', then '\n'.  The piece of a
//               record is normalized[norm_begin, norm_end) of its sentence, or
//               IdToPiece(id) where that span is empty (SentencePieceProcessor::
//               Encode(input, &pieces), sentencepiece_processor.cc).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/spm_hip.h"

namespace spm_amd {

// Blocks of every pass; block b owns one contiguous range of the input, a
// multiple of the pass's tile, and the blocks' output bases come from a
// decoupled look-back over kTextBlocks descriptors.
// (spm_amd.py mirrors the four constants for the tests' tile edges: TEXT_BLOCKS ...)
constexpr uint32_t kTextBlocks = 1024;
constexpr uint32_t kSplitTile = 4096;  // bytes: 256 threads x one 16-byte load
constexpr uint32_t kIdTile = 1024;     // items: 256 threads x 4 consecutive items
constexpr uint32_t kIdMaxWidth = 11;   // 10 digits and the separator
constexpr uint32_t kPieceTile = 256;   // items: one per thread
// The forms that run unless a measurement knob says otherwise (text_rows.hip);
// chosen by profiles/pr39_text_rows.txt: the LDS image beats direct stores in
// the split (0.114 / 0.136 ms) and ties them in id rows; piece rows is flat
// for a bound of 16 to 128 bytes and slower below (and in the layout over
// output bytes, 0).
constexpr bool kTextDirectDefault = false;
constexpr uint32_t kPieceWaveOverDefault = 32;
// Scratch words (uint64): the control words, then the descriptors.
enum TextCtl : int { kTcTicket = 0, kTcError = 1, kTcWords = 8 };
static_assert((kTcWords + kTextBlocks) * 8 <= SPM_HIP_TEXT_ROWS_SCRATCH_BYTES, "scratch");

// Decimal digits of a non-negative id: compares, no division.
__host__ __device__ inline uint32_t DecimalDigits(uint32_t v) {
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
         (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}

// The device piece-string table: piece i = bytes[off[i], off[i + 1]).
struct PieceStrings {
  const uint32_t *off;
  const uint8_t *bytes;
  int32_t num_pieces;
};

// Enqueue on st.  scratch: SPM_HIP_TEXT_ROWS_SCRATCH_BYTES, 8-byte aligned.
// counts: 2 words (see spm_hip.h); status: the call's status word.
hipError_t LaunchSplitLines(const uint8_t *in, uint64_t nbytes, uint8_t *out, uint64_t *off, uint64_t line_cap,
                            uint64_t *counts, uint32_t *status, void *scratch, hipStream_t st);
hipError_t LaunchIdRows(const int32_t *ids, const uint64_t *off, uint64_t n, uint8_t *out, uint64_t cap,
                        uint64_t *row_off, uint32_t *status, void *scratch, hipStream_t st);
hipError_t LaunchPieceRows(const spm_hip_piece *pieces, const uint64_t *piece_off, uint64_t n, const uint8_t *norm,
                           const uint64_t *norm_off, PieceStrings tab, uint8_t *out, uint64_t cap,
                           uint64_t *row_off, uint32_t *status, void *scratch, hipStream_t st);

// ---- the same results as plain loops over host buffers ----

// counts[0] = lines, counts[1] = bytes of the lines.  off[k] is written for
// k <= line_cap only; out holds nbytes.  Returns 0 or SPM_RESOURCE_EXHAUSTED.
inline int SplitLinesHostLoop(const uint8_t *in, uint64_t nbytes, uint8_t *out, uint64_t *off, uint64_t line_cap,
                              uint64_t *counts) {
  uint64_t lines = 0, w = 0;
  off[0] = 0;
  for (uint64_t p = 0; p < nbytes; ++p) {
    if (in[p] != '\n') {
      out[w++] = in[p];
      continue;
    }
    if (++lines <= line_cap) off[lines] = w;
  }
  if (nbytes && in[nbytes - 1] != '\n' && ++lines <= line_cap) off[lines] = w;
  if (counts) {
    counts[0] = lines;
    counts[1] = w;
  }
  return lines > line_cap ? SPM_RESOURCE_EXHAUSTED : SPM_OK;
}

// row_off[n + 1] is always written; text bytes only below cap.  Returns 0,
// SPM_OUT_OF_RANGE (a negative id; nothing is written) or
// SPM_RESOURCE_EXHAUSTED.
inline int IdRowsHostLoop(const int32_t *ids, const uint64_t *off, uint64_t n, uint8_t *out, uint64_t cap,
                          uint64_t *row_off) {
  for (uint64_t k = off[0]; k < off[n]; ++k)
    if (ids[k] < 0) return SPM_OUT_OF_RANGE;
  uint64_t w = 0;
  auto put = [&](uint8_t c) {
    if (w < cap) out[w] = c;
    ++w;
  };
  for (uint64_t i = 0; i < n; ++i) {
    row_off[i] = w;
    for (uint64_t k = off[i]; k < off[i + 1]; ++k) {
      if (k != off[i]) put(' ');
      uint32_t v = static_cast<uint32_t>(ids[k]);
      uint8_t d[10];
      const uint32_t nd = DecimalDigits(v);
      for (uint32_t j = nd; j-- > 0; v /= 10) d[j] = static_cast<uint8_t>('0' + v % 10);
      for (uint32_t j = 0; j < nd; ++j) put(d[j]);
    }
    put('\n');
  }
  row_off[n] = w;
  return w > cap ? SPM_RESOURCE_EXHAUSTED : SPM_OK;
}

// tab_off / tab_bytes: the piece strings on the host.  Returns 0,
// SPM_OUT_OF_RANGE (an empty span whose id is outside the table, or a span
// outside its sentence; nothing is written) or SPM_RESOURCE_EXHAUSTED.
inline int PieceRowsHostLoop(const spm_hip_piece *pieces, const uint64_t *piece_off, uint64_t n, const uint8_t *norm,
                             const uint64_t *norm_off, const uint32_t *tab_off, const uint8_t *tab_bytes,
                             int32_t num_pieces, uint8_t *out, uint64_t cap, uint64_t *row_off) {
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t k = piece_off[i]; k < piece_off[i + 1]; ++k) {
      const spm_hip_piece &p = pieces[k];
      if (p.norm_end > p.norm_begin ? p.norm_end > norm_off[i + 1] - norm_off[i] : (p.id < 0 || p.id >= num_pieces))
        return SPM_OUT_OF_RANGE;
    }
  uint64_t w = 0;
  auto put = [&](const uint8_t *src, uint64_t len) {
    if (w < cap) std::memcpy(out + w, src, static_cast<size_t>(len < cap - w ? len : cap - w));
    w += len;
  };
  const uint8_t sp = ' ', nl = '\n';
  for (uint64_t i = 0; i < n; ++i) {
    row_off[i] = w;
    for (uint64_t k = piece_off[i]; k < piece_off[i + 1]; ++k) {
      const spm_hip_piece &p = pieces[k];
      if (k != piece_off[i]) put(&sp, 1);
      if (p.norm_end > p.norm_begin) put(norm + norm_off[i] + p.norm_begin, p.norm_end - p.norm_begin);
      else put(tab_bytes + tab_off[p.id], tab_off[p.id + 1] - tab_off[p.id]);
    }
    put(&nl, 1);
  }
  row_off[n] = w;
  return w > cap ? SPM_RESOURCE_EXHAUSTED : SPM_OK;
}

}  // namespace spm_amd
