// BPE encode of one line per wavefront for gfx950 (MI355X): the small host
// calls of a BPE model in ONE launch (SentencePieceProcessor::Encode(line,
// &ids), called once per line by spm_encode; spm_hip_encode_batch_host of a
// few normalized sentences), the BPE siblings of coop_raw_kernel and
// coop_small_kernel.
//
// Reference: bpe::Model::Encode (bpe_model.cc:37-199), restated as in
// bpe_kernels.hip: repeatedly merge the live adjacent pair with the highest
// score, the smallest left index on ties; the new pairs are (prev, merged),
// then (merged, next-next); the end is when no live adjacent pair is a piece.
//
// BpeEncodeLineWave (bpe_line_wave.h) — one wave, one normalized sentence of
//   up to kBpeLineMaxBytes bytes; shared with the BPE-dropout batch kernel
//   (bpe_dropout.hip).
// bpe_raw_kernel / bpe_small_kernel — one block of kCWaves waves, n <=
//   kCoopSmallMax lines, wave w takes lines w, w + kCWaves, ...: the staged
//   image from pinned host memory; per wave the raw-line normalizer
//   (NormalizeLineWave, raw only), the encode, and the unknown-run merge of
//   PopulateSentencePieceText (raw only); then the block's token offsets, the
//   ids (and piece lengths) into the pinned image, and the publication word.
//   Every loop is bounded; nothing polls.
#include <hip/hip_runtime.h>

#include "bpe_device.h"
#include "bpe_line_wave.h"
#include "coop_wave.h"

namespace spm_amd {
namespace {

// The normalizer's tables and the symbol state are live one after the other.
union BpeLineWave {
  CoopWave norm;
  BpeLineSyms s;
};

struct BpeLineShared {
  BpeLineWave w[kCWaves];
  uint32_t ntok[kCoopSmallMax + 1];
  uint32_t failed;
};
static_assert(sizeof(BpeLineShared) <= 80 * 1024, "two blocks per CU's 160 KiB of LDS");

// One block, c.n <= kCoopSmallMax lines of one host call.  kRaw: raw lines in,
// final ids of Encode(line, &ids) out; else normalized sentences in, ids,
// piece lengths (c.len) and token offsets out.
template <bool kRaw>
__device__ void BpeLineBody(const BpeLineArgs &l, const NormTables *t, const uint8_t *types, int32_t num_types,
                            const CoopCall &c, BpeLineShared &sh) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // The image comes from host memory the host rewrites between calls:
  // system-scope loads (no cache may hold it), as CoopStageAndRoot does.
  for (uint32_t k = static_cast<uint32_t>(tid); k < c.stage_words; k += 64 * kCWaves)
    l.stage_dst[k] = __hip_atomic_load(const_cast<uint32_t *>(l.stage_src) + k, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
  if (tid == 0) sh.failed = 0;
  __threadfence_block();
  __syncthreads();
  BpeArgs a{};
  a.units = l.units;
  a.values = l.values;
  a.entry_piece = l.entry_piece;
  a.entry_out = l.entry_out;
  a.piece_out = l.piece_out;
  a.pair_ent = l.pair_ent;
  a.pair_mask = l.pair_mask;
  a.root_base = l.root_base;
  a.unk_id = l.unk_id;
  a.irregular = l.irregular;
  const uint64_t *off = reinterpret_cast<const uint64_t *>(l.stage_dst);
  // Line i's bytes, and its tokens while they wait for the block's offsets,
  // sit at row(i) of bytes / slot_ids / slot_len.
  auto row = [&](uint32_t i) -> uint64_t { return kRaw ? 4 * off[i] + 8ull * i : c.in_at + off[i]; };
  for (uint32_t i = static_cast<uint32_t>(wave); i < c.n; i += kCWaves) {
    const uint64_t b0 = row(i);
    uint32_t nb = static_cast<uint32_t>(off[i + 1] - off[i]);
    if (kRaw) {
      const uint8_t *raw = reinterpret_cast<const uint8_t *>(l.stage_dst) + c.in_at + off[i];
      nb = NormalizeLineWave(*t, sh.w[wave].norm, raw, nb, const_cast<uint8_t *>(l.bytes) + b0, 4 * nb + 8);
    }
    int32_t *tok = l.slot_ids + b0;
    uint32_t nt = nb == kNone ? kNone
                              : BpeEncodeLineWave<kBpeLineMaxBytes, false, false>(
                                    a, sh.w[wave].s, l.bytes + b0, nb, tok,
                                    kRaw || !c.len ? nullptr : l.slot_len + b0, BpeDropKey{});
    if (kRaw && nt != kNone) {
      __threadfence_block();
      WaveSync();
      nt = MergeUnknownRunsWave(tok, tok, nt, types, num_types);
    }
    if (lane == 0) {
      if (nt == kNone) sh.failed = 1;
      sh.ntok[i] = nt;
    }
  }
  __threadfence_block();
  __syncthreads();
  if (sh.failed == 0 && tid == 0) {  // token offsets (n <= kCoopSmallMax: one thread)
    uint64_t tot = 0;
    c.tok[0] = 0;
    for (uint32_t i = 0; i < c.n; ++i) {
      const uint32_t nt = sh.ntok[i];
      sh.ntok[i] = static_cast<uint32_t>(tot);
      tot += nt;
      c.tok[i + 1] = tot;
    }
    sh.ntok[c.n] = static_cast<uint32_t>(tot);
    if (tot > c.ids_cap) sh.failed = 1;
  }
  __syncthreads();
  const bool ok = sh.failed == 0;
  if (ok) {
    for (uint32_t i = static_cast<uint32_t>(wave); i < c.n; i += kCWaves) {
      const uint32_t t0 = sh.ntok[i], nt = sh.ntok[i + 1] - t0;
      const uint64_t b0 = row(i);
      for (uint32_t j = static_cast<uint32_t>(lane); j < nt; j += 64) {
        c.ids[t0 + j] = l.slot_ids[b0 + j];
        if (!kRaw && c.len) c.len[t0 + j] = l.slot_len[b0 + j];
      }
    }
  }
  CoopPublish(c, ok);
}

__global__ __launch_bounds__(64 * kCWaves) void bpe_raw_kernel(BpeRawArgs s, CoopCall c) {
  __shared__ BpeLineShared sh;
  BpeLineBody<true>(s.a, &s.t, s.types, s.num_types, c, sh);
}

__global__ __launch_bounds__(64 * kCWaves) void bpe_small_kernel(BpeLineArgs a, CoopCall c) {
  __shared__ BpeLineShared sh;
  BpeLineBody<false>(a, nullptr, nullptr, 0, c, sh);
}

}  // namespace

hipError_t LaunchBpeRaw(const BpeRawArgs &s, const CoopCall &c, hipStream_t st) {
  if (c.n == 0 || c.n > kCoopSmallMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bpe_raw_kernel, dim3(1), dim3(64 * kCWaves), 0, st, s, c);
  return hipGetLastError();
}

hipError_t LaunchBpeSmall(const BpeLineArgs &a, const CoopCall &c, hipStream_t st) {
  if (c.n == 0 || c.n > kCoopSmallMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bpe_small_kernel, dim3(1), dim3(64 * kCWaves), 0, st, a, c);
  return hipGetLastError();
}

}  // namespace spm_amd
