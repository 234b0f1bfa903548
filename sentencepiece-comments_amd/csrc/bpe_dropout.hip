// BPE-dropout encode for gfx950 (MI355X): SampleEncode of a BPE model, the
// batch tier.
//
// Reference: bpe::Model::SampleEncode of the sentencepiece package
// (bpe_model.cc): the greedy merge loop of Encode, where each pair popped
// from the agenda (after the stale check) is dropped for good with
// probability alpha.  Restated as in bpe_kernels.hip: repeatedly merge the
// arg-max over the live adjacent pairs that have not been dropped, the
// smallest left index on ties.  The decision is a pure function of the pair's
// name (first byte of the left symbol, byte past the right symbol) in the
// sentence's counter-based stream (sample_rng.h), so it may be taken when
// the pair is probed: a draw depends on (seed, global sentence index, pair
// name) only, never on the batch, the tier or the launch geometry.
//
// bpe_dropout_kernel<kMaxBytes> — one sentence per wavefront, kDropWaves
//   waves per block, BpeEncodeLineWave<kMaxBytes, true, true> on the wave's
//   LDS slab (16 bytes per byte position), tokens to the sentence's
//   right-aligned slots.  The full bound (kBpeLineMaxBytes) costs 16 KiB per
//   wave, 64 KiB per block: two blocks per CU.  The short instantiation
//   (kBpeDropShortBytes: 2 KiB per wave) takes the sentences up to its bound
//   and lists the others in `rest` for the full one.  Sentences the wave does
//   not take are flagged for bpe_general_kernel<true>.
#include <hip/hip_runtime.h>

#include "bpe_device.h"
#include "bpe_line_wave.h"
#include "kernels.h"

namespace spm_amd {
namespace {

constexpr int kDropWaves = 4;

// kShort: every sentence of the batch, the longer ones to `rest`; else the
// sentences of `rest` (every sentence when rest == nullptr).
template <uint32_t kMaxBytes, bool kShort>
__global__ __launch_bounds__(64 * kDropWaves) void bpe_dropout_kernel(BpeDropoutLaunch d) {
  __shared__ BpeLineSymsT<kMaxBytes> slab[kDropWaves];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if ((d.chain && *d.chain) || d.off[d.n] > d.capacity) {  // (BpeSkip of bpe_kernels.hip)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&d.status[kStError], 2u);
    return;
  }
  BpeArgs a{};
  a.bytes = d.t.bytes;
  a.off = d.off;
  a.n = d.n;
  a.units = d.t.units;
  a.values = d.t.values;
  a.entry_piece = d.t.entry_piece;
  a.entry_out = d.t.entry_out;
  a.piece_out = d.t.piece_out;
  a.pair_ent = d.t.pair_ent;
  a.pair_mask = d.t.pair_mask;
  a.root_base = d.t.root_base;
  a.unk_id = d.t.unk_id;
  a.irregular = d.t.irregular;
  a.slot_ids = d.t.slot_ids;
  a.slot_len = d.t.slot_len;
  a.ntok = d.ntok;
  a.flagged = d.flagged;
  a.status = d.status;
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * kDropWaves + wv;
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kDropWaves;
  const bool listed = !kShort && d.rest != nullptr;
  const uint64_t count = listed ? *d.rest_count : d.n;
  for (uint64_t jl = wave; jl < count; jl += nwaves) {
    const uint64_t i = listed ? d.rest[jl] : jl;
    const uint64_t b0 = d.off[i];
    const uint64_t nb64 = d.off[i + 1] - b0;
    if (nb64 > kMaxBytes) {
      if (lane == 0) {
        if (kShort) d.rest[atomicAdd(d.rest_count, 1u)] = static_cast<uint32_t>(i);
        else FlagSentence(a, i, static_cast<uint32_t>(nb64 < 0xFFFFFFFFull ? nb64 : 0xFFFFFFFFull));
      }
      continue;
    }
    const uint32_t nb = static_cast<uint32_t>(nb64);
    const BpeDropKey key{SampleKey(d.seed, d.index_base + i), d.threshold};
    const uint32_t nt = BpeEncodeLineWave<kMaxBytes, true, true>(
        a, slab[wv], a.bytes + b0, nb, a.slot_ids + b0, a.slot_len ? a.slot_len + b0 : nullptr, key);
    if (lane == 0) {
      if (nt == kNone) FlagSentence(a, i, nb);
      else a.ntok[i] = nt;
    }
  }
}

}  // namespace

hipError_t LaunchBpeDropout(const BpeDropoutLaunch &d, hipStream_t st) {
  if (d.n == 0) return hipSuccess;
  // Grid-stride over the sentences: enough blocks to fill the device at
  // either slab size.
  const uint64_t blocks64 = (d.n + kDropWaves - 1) / kDropWaves;
  const unsigned blocks = static_cast<unsigned>(blocks64 < 8192 ? blocks64 : 8192);
  if (d.rest) {
    hipLaunchKernelGGL((bpe_dropout_kernel<kBpeDropShortBytes, true>), dim3(blocks), dim3(64 * kDropWaves), 0, st, d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((bpe_dropout_kernel<kBpeLineMaxBytes, false>), dim3(blocks), dim3(64 * kDropWaves), 0, st, d);
  return hipGetLastError();
}

}  // namespace spm_amd
