// BPE encode of one normalized sentence by one wavefront (gfx950): what the
// small host calls (bpe_line.hip) and the BPE-dropout batch kernel
// (bpe_dropout.hip) share.  Device only; every definition is local to the
// including file.
//
// BpeEncodeLineWave — one wave, one normalized sentence of up to kMaxBytes
//   bytes.  A symbol is named by the byte position it starts at, so the
//   initial split (OneCharLen steps clamped to the sentence) needs no
//   compaction and a token's byte length is the distance to the next live
//   symbol.  Lane l owns the positions [l * per, (l + 1) * per), per =
//   ceil(nb / 64) (1 or 2 on a line of prose, 16 at 1024 bytes): ownership is
//   blocked, so the lowest lane that holds the wave's maximal key also holds
//   the lowest position with it.  Symbol state sits in the wave's LDS slab,
//   16 bytes per position: the pair key (the merged piece's score rank, as in
//   bpe_fast_kernel; 0: no pair), the symbol, the pair's merged piece, and
//   the links to the next and the previous live symbol.  Each lane keeps the
//   maximal key of its own positions, and the lowest position that has it, in
//   registers.  Per merge: one DPP wave maximum, a ballot for the lowest lane,
//   a readlane for its position L; L's neighbours come from LDS (the same
//   address in every lane: a broadcast); lane 0 relinks; lanes 0 and 1 probe
//   the two new pairs in one divergent call of PairLookupFused; the (at most
//   three) lanes that own L, its dead right neighbour and its left neighbour
//   scan their positions' keys again.  At most (symbols - 1) merges.
//   Not taken (kNone), by bpe_fast_kernel's rules: a pushed pair whose merged
//   piece is UNUSED (it needs the general kernel's resegmentation) and, on an
//   irregular model, a char outside the vocabulary; and a sentence longer
//   than the bound.
//   kDrop (BPE-dropout): a probed pair that BpeDropped names gets key 0, so
//   the arg-max runs over the live adjacent pairs that have not been dropped.
//   The pair (left, right) is named by the left symbol's first byte and the
//   byte one past the right symbol's last: symbols only grow, so no name
//   comes twice in a sentence and the mask is a pure function of it.
#pragma once

#include <hip/hip_runtime.h>

#include "bpe_device.h"
#include "coop_wave.h"

namespace spm_amd {
namespace {

constexpr uint32_t kNoSym = 0xFFFFu;  // next: no live symbol starts here; prev: the first symbol

// One wave's symbol state, by byte position.
template <uint32_t kMaxBytes>
struct BpeLineSymsT {
  uint32_t key[kMaxBytes];   // score rank of the pair (this, next live symbol); 0: no pair
  int32_t sym[kMaxBytes];    // pieces_ id; a char outside pieces_: -1 - PieceToId
  int32_t pres[kMaxBytes];   // the pair's merged piece
  uint16_t next[kMaxBytes];  // start of the next live symbol (nb: the last one), or kNoSym
  uint16_t prev[kMaxBytes];  // start of the previous live symbol, or kNoSym
};
using BpeLineSyms = BpeLineSymsT<kBpeLineMaxBytes>;
static_assert(sizeof(BpeLineSyms) == 16 * kBpeLineMaxBytes, "16 bytes of state per position");
static_assert(kBpeLineMaxBytes < kNoSym && kBpeLineMaxBytes % 64 == 0, "16-bit links; 64 lanes share the positions");

__device__ __forceinline__ uint32_t Uniform(uint32_t v) {
  return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

// Encodes the normalized sentence s[0, nb) with one wave: its tokens' ids to
// out_ids[0, ntok) (and their byte lengths to out_len, nullable), in order
// (kRightAlign: to [nb - ntok, nb), the batch tiers' slot layout); returns
// ntok, or kNone when the sentence is not taken.  Wave-uniform result; all 64
// lanes call it together.
template <uint32_t kMaxBytes, bool kDrop, bool kRightAlign>
__device__ uint32_t BpeEncodeLineWave(const BpeArgs &a, BpeLineSymsT<kMaxBytes> &S, const uint8_t *__restrict__ s,
                                      uint32_t nb, int32_t *__restrict__ out_ids, uint32_t *__restrict__ out_len,
                                      const BpeDropKey &drop) {
  static_assert(kMaxBytes < kNoSym && kMaxBytes % 64 == 0, "16-bit links; 64 lanes share the positions");
  const uint32_t lane = threadIdx.x & 63;
  nb = Uniform(nb);
  if (nb == 0) return 0;
  if (nb > kMaxBytes) return kNone;
  const uint32_t per = (nb + 63) >> 6;
  const uint32_t p0 = min(lane * per, nb), p1 = min(p0 + per, nb);
  auto cont = [](uint32_t c) { return (c & 0xC0u) == 0x80u; };
  // ---- 1. the initial split (bpe_model.cc:121-131): OneCharLen steps from 0,
  // clamped to the sentence.  On structurally valid UTF-8 the chain is the
  // non-continuation bytes, which every position checks for itself; anything
  // else walks the chain on one lane.
  bool odd = false;
  for (uint32_t p = p0; p < p1; ++p) {
    const uint32_t c = s[p];
    uint32_t cl = OneCharLenB(c);
    if (cl > nb - p) cl = nb - p;
    const bool start = !cont(c);
    if (p == 0 && !start) odd = true;
    if (start) {
      for (uint32_t j = 1; j < cl; ++j)
        if (!cont(s[p + j])) odd = true;
      if (p + cl < nb && cont(s[p + cl])) odd = true;
    }
    S.key[p] = cl;
    S.next[p] = static_cast<uint16_t>(start ? p + cl : kNoSym);
    S.prev[p] = static_cast<uint16_t>(kNoSym);
  }
  if (__builtin_amdgcn_ballot_w64(odd) != 0) {
    for (uint32_t p = p0; p < p1; ++p) S.next[p] = static_cast<uint16_t>(kNoSym);
    WaveSync();
    if (lane == 0)
      for (uint32_t p = 0; p < nb;) {  // (every step is >= 1 byte)
        const uint32_t cl = S.key[p];
        S.next[p] = static_cast<uint16_t>(p + cl);
        p += cl;
      }
  }
  WaveSync();
  // ---- 2. the chars' symbols and the links back.
  bool bad = false;
  for (uint32_t p = p0; p < p1; ++p) {
    const uint32_t q = S.next[p];
    if (q != kNoSym) {
      if (q < nb) S.prev[q] = static_cast<uint16_t>(p);
      // Symbol id (pieces_ id) and PieceToId of a single char.
      int32_t sym = -1, out = a.unk_id;
      const int32_t e = ExactEntry(a, s + p, q - p);
      if (e >= 0) {
        sym = a.entry_piece[e];
        out = a.entry_out[e];
      }
      if (a.irregular && sym < 0) bad = true;
      S.sym[p] = sym >= 0 ? sym : -1 - out;
    }
    S.key[p] = 0;
    S.pres[p] = -1;
  }
  WaveSync();
  // ---- 3. the initial pairs; each lane's best key and the lowest position
  // that has it.
  uint32_t bkey = 0, bpos = p0;
  auto rescan = [&]() {
    bkey = 0;
    bpos = p0;
    for (uint32_t p = p0; p < p1; ++p) {
      const uint32_t k = S.key[p];
      if (k > bkey) {
        bkey = k;
        bpos = p;
      }
    }
  };
  for (uint32_t p = p0; p < p1; ++p) {
    const uint32_t q = S.next[p];
    if (q == kNoSym || q >= nb) continue;
    uint32_t rank = 0;
    bool unused = false;
    const int32_t r = PairLookupFused(a, S.sym[p], S.sym[q], &rank, &unused);
    if (r < 0) continue;
    if (unused) bad = true;
    if constexpr (kDrop) {  // (q starts a symbol: next[q] is its end)
      if (BpeDropped(drop, p, S.next[q])) continue;
    }
    S.pres[p] = r;
    S.key[p] = rank;
  }
  if (__builtin_amdgcn_ballot_w64(bad) != 0) return kNone;
  rescan();
  WaveSync();
  // ---- 4. merges until no adjacent pair is in the vocabulary.  A pushed
  // UNUSED piece only marks the sentence (checked once after the loop, as in
  // bpe_fast_kernel); `bad` is per lane in here and does not steer the loop,
  // which stays convergent for the DPP maximum.
  for (uint32_t it = 1; it < nb; ++it) {
    const uint32_t m = WaveMaxU(bkey);
    if (m == 0) break;
    const uint64_t cand = __builtin_amdgcn_ballot_w64(bkey == m);
    const int owner = __ffsll(static_cast<long long>(cand)) - 1;
    const uint32_t L = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(bpos), owner));
    // L, its neighbours and their symbols: the same LDS address in every lane.
    const uint32_t R = Uniform(S.next[L]), P = Uniform(S.prev[L]);
    const int32_t merged = static_cast<int32_t>(Uniform(static_cast<uint32_t>(S.pres[L])));
    if (R >= nb) {  // (a pair always has a live right symbol)
      bad = true;
      break;
    }
    const uint32_t RR = Uniform(S.next[R]);
    const int32_t psym = P != kNoSym ? static_cast<int32_t>(Uniform(static_cast<uint32_t>(S.sym[P]))) : -1;
    const int32_t rrsym = RR < nb ? static_cast<int32_t>(Uniform(static_cast<uint32_t>(S.sym[RR]))) : -1;
    uint32_t rr_end = 0;  // kDrop: the end of RR's symbol
    if constexpr (kDrop) rr_end = RR < nb ? Uniform(S.next[RR]) : 0u;
    WaveSync();
    if (lane == 0) {
      S.sym[L] = merged;
      S.next[L] = static_cast<uint16_t>(RR);
      S.next[R] = static_cast<uint16_t>(kNoSym);
      S.key[R] = 0;
      if (RR < nb) S.prev[RR] = static_cast<uint16_t>(L);
    }
    // New pairs: (P, L) then (L, RR) — the reference's push order.  Both
    // probes run in one divergent call (lanes 0 and 1).
    const bool probe_p = lane == 0 && P != kNoSym, probe_l = lane == 1 && RR < nb;
    int32_t q = -1;
    uint32_t qs = 0u;
    bool qu = false;
    if (probe_p || probe_l) q = PairLookupFused(a, probe_p ? psym : merged, probe_p ? merged : rrsym, &qs, &qu);
    if (q >= 0 && qu) bad = true;  // (before the mask: rev_merge records dropped pairs too)
    if constexpr (kDrop) {
      // (P, L) spans [P, RR) — RR is nb at the sentence's end —, (L, RR) spans [L, rr_end).
      if (q >= 0 && BpeDropped(drop, probe_p ? P : L, probe_p ? RR : rr_end)) q = -1;
    }
    if (probe_p) {
      S.pres[P] = q;
      S.key[P] = q >= 0 ? qs : 0u;
    }
    if (lane == 1) {
      S.pres[L] = q;
      S.key[L] = q >= 0 ? qs : 0u;
    }
    WaveSync();
    // (P == kNoSym lies in no lane's range.)
    if ((L >= p0 && L < p1) || (R >= p0 && R < p1) || (P >= p0 && P < p1)) rescan();
  }
  if (__builtin_amdgcn_ballot_w64(bad) != 0) return kNone;
  // ---- 5. the live symbols in order: PieceToId of the final symbol (=
  // entry_out of an unmerged char outside pieces_).
  uint32_t cnt = 0;
  for (uint32_t p = p0; p < p1; ++p) cnt += S.next[p] != kNoSym ? 1u : 0u;
  uint32_t incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(incl, o);
    if (lane >= static_cast<uint32_t>(o)) incl += y;
  }
  const uint32_t nt = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
  uint32_t j = incl - cnt + (kRightAlign ? nb - nt : 0u);
  for (uint32_t p = p0; p < p1; ++p) {
    const uint32_t q = S.next[p];
    if (q == kNoSym) continue;
    const int32_t sym = S.sym[p];
    out_ids[j] = sym >= 0 ? a.piece_out[sym] : -1 - sym;
    if (out_len) out_len[j] = q - p;
    ++j;
  }
  WaveSync();  // the slab is the next line's
  return nt;
}

}  // namespace
}  // namespace spm_amd
