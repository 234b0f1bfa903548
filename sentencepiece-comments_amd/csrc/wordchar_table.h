// Exact-match table of the WORD / CHAR models: piece bytes -> PieceToId
// (model_interface.cc:87-97).  Shared by the host builder (spm_hip_api.cc)
// and the kernels (wordchar_kernels.hip) so the two cannot disagree.
//
// Open addressing with linear probing over a power-of-two number of 16-byte
// entries {hash, id, key offset, key length}; the key bytes of every entry
// sit in one blob and a hit is verified byte by byte, so keys of any length
// (and with any byte, NUL included) are exact.  A key of at most 4 bytes (every
// char) is kept in the key offset field itself, so its lookup is one entry
// load and no blob access.  An entry of length 0 is empty
// (pieces are never empty).  The builder keeps the load at or below 1/2, so a
// probe sequence always ends at an empty entry.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spm_amd {

struct WordCharEntry {
  uint32_t hash, id, key_off, key_len;
};

// FNV-1a over the key bytes.
__host__ __device__ inline uint32_t WordCharHash(const uint8_t *s, uint32_t len) {
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < len; ++i) h = (h ^ s[i]) * 16777619u;
  return h;
}

// A key of <= 4 bytes as the entry's key_off word (little-endian, zero padded).
__host__ __device__ inline uint32_t WordCharPack(const uint8_t *s, uint32_t len) {
  uint32_t v = 0;
  for (uint32_t i = 0; i < len; ++i) v |= static_cast<uint32_t>(s[i]) << (8 * i);
  return v;
}

// id of s[0:len), or `miss`.  mask = entries - 1.
__host__ __device__ inline int32_t WordCharFind(const WordCharEntry *tab, uint32_t mask, const uint8_t *keys,
                                                const uint8_t *s, uint32_t len, int32_t miss) {
  const uint32_t h = WordCharHash(s, len);
  uint32_t slot = h & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
    const WordCharEntry e = tab[slot];
    if (e.key_len == 0) return miss;
    if (e.hash != h || e.key_len != len) continue;
    if (len <= 4) {
      if (e.key_off == WordCharPack(s, len)) return static_cast<int32_t>(e.id);
      continue;
    }
    const uint8_t *k = keys + e.key_off;
    uint32_t i = 0;
    while (i < len && k[i] == s[i]) ++i;
    if (i == len) return static_cast<int32_t>(e.id);
  }
  return miss;
}

}  // namespace spm_amd
