// BPE encode of models with user-defined symbols for gfx950 (MI355X): the
// frozen-symbol tier, ahead of the literal bpe_general_kernel.
//
// The reference's split (bpe_model.cc:121-131) walks the sentence from byte 0;
// at each symbol start the longest USER_DEFINED piece that prefixes the rest
// becomes one frozen symbol, otherwise the step is OneCharLen.
// MaybeAddNewSymbolPair returns at once for a frozen neighbour, so no merge
// ever crosses a frozen symbol: merges on its two sides never meet, the agenda
// order (score, then left index) restricted to one gap between frozen symbols
// is the same relative order, and the sentence's tokens are its gaps' tokens
// with the frozen ids between them (the argument bpe_words.hip makes for word
// cuts).  BpeEncodeLineWave<.., kFrozen = true> takes the frozen symbols as
// single symbols that never pair: one call per sentence, the gaps merge in
// the routine's one arg-max loop.
//
// bpe_frozen_kernel — one sentence per wavefront, <= kBpeLineMaxBytes bytes,
//   four waves per block, in bpe_dropout_kernel's two launches: sentences of
//   <= kBpeDropShortBytes bytes on 2 KiB of line-wave state, the others from a
//   device-side list on the full 16 KiB.
//   1. Match, 64 bytes per step, one byte per lane.  A lane whose byte is no
//      continuation byte and passes the 256-bit filter of the bytes a
//      user-defined piece starts with walks the trie of the user-defined
//      pieces from there and keeps the longest match (the walk ends at a NUL
//      byte, as the literal kernel's does).  A step without such a byte costs
//      one ballot.  The same pass checks that the OneCharLen walk is the
//      non-continuation bytes (the half kernel's and the word tier's check).
//   2. Resolve.  On a regular walk the reference reaches position q iff q is a
//      non-continuation byte at or past the end of the last accepted match.
//      A wave-uniform loop over the ballot's set bits accepts the candidates
//      in order and carries the cover end from step to step (a match may run
//      across steps); every lane learns whether its byte starts a frozen
//      symbol (its length), lies inside one, or neither, and leaves that in
//      the line-wave state's key column.
//   3. Encode: BpeEncodeLineWave, ids and piece lengths to the sentence's
//      right-aligned slots, which bpe_compact_kernel reads.
//   Handed on to the literal kernel (d.literal, status[kStBpeLiteral]): a
//   sentence of more than kBpeLineMaxBytes bytes, a walk-irregular one, a
//   pushed UNUSED piece, a char outside an irregular vocabulary.
//   The model qualifies (BpeDevice::frozen_ok) when every user-defined piece
//   is whole chars without a NUL byte: a match then ends where a char ends.
//   LDS: the trie sits in LDS when it has <= kFrozenLdsUnits units (8 KiB;
//   the double array grows in blocks of 256 units) and is read from global
//   memory otherwise.  Short launch: 4 x 2 KiB + 8 KiB = 16 KiB per
//   block, so the CU's wave limit binds, not its 160 KiB; full launch: 4 x
//   16 KiB + 8 KiB = 72 KiB, two blocks = 8 waves per CU, as bpe_wave_kernel.
#include <hip/hip_runtime.h>

#include "bpe_device.h"
#include "bpe_line_wave.h"
#include "kernels.h"

namespace spm_amd {
namespace {

constexpr int kFrozenWaves = 4;
constexpr uint32_t kFrozenLdsUnits = 2048;

__device__ __forceinline__ BpeArgs FrozenArgs(const BpeFrozenLaunch &d) {
  BpeArgs a = BpeArgsOf(d.t);
  a.off = d.off;
  a.n = d.n;
  a.ntok = d.ntok;
  a.status = d.status;
  a.capacity = d.capacity;
  a.chain = d.chain;
  return a;
}

// kShort: every sentence of the batch, the ones over kMaxBytes bytes to
// d.rest; else the sentences of d.rest.
template <uint32_t kMaxBytes, bool kShort, bool kTrieLds>
__global__ __launch_bounds__(64 * kFrozenWaves) void bpe_frozen_kernel(BpeFrozenLaunch d) {
  __shared__ BpeLineSymsT<kMaxBytes> slab[kFrozenWaves];
  __shared__ uint32_t lds_filter[8];
  __shared__ uint32_t lds_units[kTrieLds ? kFrozenLdsUnits : 1];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const BpeArgs a = FrozenArgs(d);
  if (BpeSkip(a)) return;
  // Every sentence counts as flagged (stats.general_path), as in the text tiers.
  if (kShort && blockIdx.x == 0 && threadIdx.x == 0) d.status[kStFlagged] = static_cast<uint32_t>(d.n);
  const uint64_t count = kShort ? d.n : d.status[kStBpeFrozenRest];
  if (count == 0) return;
  const uint32_t *__restrict__ gunits = d.ud + 8;
  if (threadIdx.x < 8) lds_filter[threadIdx.x] = d.ud[threadIdx.x];
  if constexpr (kTrieLds)
    for (uint32_t u = threadIdx.x; u < d.ud_units; u += 64 * kFrozenWaves) lds_units[u] = gunits[u];
  __syncthreads();
  auto unit = [&](uint32_t node) -> uint32_t {
    if constexpr (kTrieLds) return lds_units[node];
    else return gunits[node];
  };
  BpeLineSymsT<kMaxBytes> &S = slab[wv];
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * kFrozenWaves + wv;
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kFrozenWaves;
  uint32_t done = 0, longest = 0;
  for (uint64_t jl = wave; jl < count; jl += nwaves) {
    const uint32_t i = kShort ? static_cast<uint32_t>(jl) : d.rest[jl];
    const uint64_t b0 = d.off[i];
    const uint64_t nb64 = d.off[i + 1] - b0;
    if (kShort) longest = max(longest, nb64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(nb64));
    auto hand_on = [&]() {
      if (lane == 0) {
        a.ntok[i] = 0xFFFFFFFFu;
        d.literal[atomicAdd(&d.status[kStBpeLiteral], 1u)] = i;
      }
    };
    if (nb64 > kBpeLineMaxBytes) {
      hand_on();
      continue;
    }
    if (nb64 > kMaxBytes) {  // (kShort only: the full state holds kBpeLineMaxBytes)
      if (lane == 0) d.rest[atomicAdd(&d.status[kStBpeFrozenRest], 1u)] = i;
      continue;
    }
    const uint32_t nb = static_cast<uint32_t>(nb64);
    const uint8_t *__restrict__ s = a.bytes + b0;
    WaveSync();  // the slab was the last sentence's
    // ---- 1 + 2. match and resolve, 64 bytes per step.
    bool odd = false;
    uint32_t cover = 0;  // wave-uniform: end of the last accepted match
    for (uint32_t st = 0; st < nb; st += 64) {
      const uint32_t p = st + lane;
      const bool in = p < nb;
      const uint32_t c = in ? s[p] : 0x80u;
      uint32_t len = 0;
      if ((c & 0xC0u) == 0x80u) {
        if (p == 0) odd = true;
      } else {
        uint32_t cl = OneCharLenB(c);
        if (cl > nb - p) cl = nb - p;
        for (uint32_t j = 1; j < cl; ++j)
          if ((s[p + j] & 0xC0u) != 0x80u) odd = true;
        if (p + cl < nb && (s[p + cl] & 0xC0u) == 0x80u) odd = true;
        if ((lds_filter[c >> 5] >> (c & 31u)) & 1u) {
          // PrefixMatcher::PrefixMatch: the longest user-defined piece from p.
          uint32_t base = d.ud_root;
          for (uint32_t t = p; t < nb; ++t) {
            const uint32_t ch = s[t];
            if (ch == 0) break;
            const uint32_t node = base ^ ch;
            if (node >= d.ud_units) break;
            const uint32_t u = unit(node);
            if ((u & 0xFFu) != ch) break;
            base = u >> 9;
            if (u & 0x100u) len = t + 1 - p;
          }
        }
      }
      uint32_t mark = p < cover ? kFrozenInside : 0u;
      for (uint64_t cm = __builtin_amdgcn_ballot_w64(len != 0); cm != 0; cm &= cm - 1) {
        const int b = __ffsll(static_cast<long long>(cm)) - 1;
        const uint32_t q = st + static_cast<uint32_t>(b);
        if (q < cover) continue;  // inside an accepted match: the walk never stops here
        cover = q + static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(len), b));
        if (p == q) mark = cover - q;
        else if (p > q && p < cover) mark = kFrozenInside;
      }
      if (in) S.key[p] = mark;
    }
    if (__builtin_amdgcn_ballot_w64(odd) != 0) {
      hand_on();
      continue;
    }
    WaveSync();
    // ---- 3. encode, the frozen symbols as single symbols that never pair.
    const uint32_t nt = BpeEncodeLineWave<kMaxBytes, false, true, true>(
        a, S, s, nb, a.slot_ids + b0, a.slot_len ? a.slot_len + b0 : nullptr, BpeDropKey{});
    if (nt == kNone) {
      hand_on();
      continue;
    }
    if (lane == 0) a.ntok[i] = nt;
    ++done;
  }
  if (lane == 0 && done) atomicAdd(&d.status[kStBpeFrozenDone], done);
  if (kShort && lane == 0 && longest) atomicMax(&d.status[kStMaxNb], longest);
}

template <bool kTrieLds>
hipError_t LaunchFrozen(const BpeFrozenLaunch &d, hipStream_t st) {
  // Grid-stride: the first launch over the batch, the second over a
  // device-side list of up to n sentences (it reads a zero count and returns
  // when every sentence is short).
  const uint64_t b64 = (d.n + kFrozenWaves - 1) / kFrozenWaves;
  const dim3 grid(static_cast<unsigned>(b64 < 4096 ? b64 : 4096)), block(64 * kFrozenWaves);
  hipLaunchKernelGGL((bpe_frozen_kernel<kBpeDropShortBytes, true, kTrieLds>), grid, block, 0, st, d);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((bpe_frozen_kernel<kBpeLineMaxBytes, false, kTrieLds>), grid, block, 0, st, d);
  return hipGetLastError();
}

}  // namespace

hipError_t LaunchBpeFrozen(const BpeFrozenLaunch &d, hipStream_t st) {
  if (d.n == 0) return hipSuccess;
  return d.ud_units <= kFrozenLdsUnits ? LaunchFrozen<true>(d, st) : LaunchFrozen<false>(d, st);
}

}  // namespace spm_amd
