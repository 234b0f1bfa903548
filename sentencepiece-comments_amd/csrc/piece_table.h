// Piece -> (id, node score) table of the byte kernel's writing backtrace:
// the key layout and the hash, shared by the host builder (spm_hip_api.cc)
// and the kernel (unigram_encode.hip) so the two cannot disagree.
//
// A key is 16 bytes: the piece bytes zero-padded to 15 plus the length in the
// last byte (an input NUL therefore never aliases padding).  An entry is 32
// bytes (key, id, score, pad), so a probe is a 16-byte and an 8-byte load
// inside one cache line.  Every stored key sits at one of its two hashed
// positions (two-choice / cuckoo placement, one entry per position): a lookup
// is at most kPieceProbes entry loads, which the builder proves for every key.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SPM_PT_HD __host__ __device__
#else
#define SPM_PT_HD
#endif

namespace spm_amd {

constexpr int kPieceProbes = 2;           // entry loads per lookup, at most
constexpr uint32_t kPieceKeyBytes = 15;   // longest key (the byte kernel's pieces are < 16 bytes)
constexpr uint32_t kPieceEmpty = ~0u;     // k[3] of an empty entry: length byte 255, no key has it

struct PieceEntry {
  uint32_t k[4];
  int32_t id;
  float score;
  uint32_t pad[2];
};
static_assert(sizeof(PieceEntry) == 32, "two entries per 64-byte line");

// The table image (host copy and device buffer alike): this header in the
// first 32 bytes, then mask + 1 entries (a power of two).
struct PieceTableHeader {
  uint32_t mask;  // capacity - 1
  uint32_t seed;
  uint32_t pad[6];
};
static_assert(sizeof(PieceTableHeader) == sizeof(PieceEntry), "entries stay 32-byte aligned");

// The two positions of a key.
SPM_PT_HD inline void PieceHash(uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3, uint32_t seed, uint32_t mask,
                                uint32_t *p0, uint32_t *p1) {
  uint32_t h = (k0 ^ seed) * 0x9E3779B1u;
  h = (h ^ (h >> 15) ^ k1) * 0x85EBCA77u;
  h = (h ^ (h >> 13) ^ k2) * 0xC2B2AE3Du;
  h = (h ^ (h >> 16) ^ k3) * 0x27D4EB2Fu;
  h ^= h >> 15;
  *p0 = h & mask;
  *p1 = ((h * 0x165667B1u) >> 14) & mask;  // capacity <= 2^18
}

// Key words of bytes[0:len), 1 <= len <= kPieceKeyBytes (host side; the
// kernel masks its 16 loaded bytes to the same words).
inline void PieceKey(const uint8_t *bytes, uint32_t len, uint32_t k[4]) {
  uint8_t b[16] = {};
  for (uint32_t i = 0; i < len; ++i) b[i] = bytes[i];
  b[15] = static_cast<uint8_t>(len);
  for (int w = 0; w < 4; ++w)
    k[w] = static_cast<uint32_t>(b[4 * w]) | static_cast<uint32_t>(b[4 * w + 1]) << 8 |
           static_cast<uint32_t>(b[4 * w + 2]) << 16 | static_cast<uint32_t>(b[4 * w + 3]) << 24;
}

// Host lookup of key words k in a table image (header + entries): the same
// kPieceProbes positions the kernel loads.
inline bool PieceTableFind(const uint32_t *img, const uint32_t k[4], int32_t *id, float *score) {
  uint32_t p[kPieceProbes];
  PieceHash(k[0], k[1], k[2], k[3], img[1], img[0], &p[0], &p[1]);
  for (int t = 0; t < kPieceProbes; ++t) {
    const uint32_t *e = img + 8 * (static_cast<uint64_t>(p[t]) + 1);
    if (e[0] == k[0] && e[1] == k[1] && e[2] == k[2] && e[3] == k[3]) {
      *id = static_cast<int32_t>(e[4]);
      __builtin_memcpy(score, &e[5], 4);
      return true;
    }
  }
  return false;
}

}  // namespace spm_amd
