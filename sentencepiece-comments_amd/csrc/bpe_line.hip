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
// BpeEncodeLineWave — one wave, one normalized sentence of up to
//   kBpeLineMaxBytes bytes.  A symbol is named by the byte position it starts
//   at, so the initial split (OneCharLen steps clamped to the sentence) needs
//   no compaction and a token's byte length is the distance to the next live
//   symbol.  Lane l owns the positions [l * per, (l + 1) * per), per =
//   ceil(nb / 64) (1 or 2 on a line of prose, 16 at the bound): ownership is
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
// bpe_raw_kernel / bpe_small_kernel — one block of kCWaves waves, n <=
//   kCoopSmallMax lines, wave w takes lines w, w + kCWaves, ...: the staged
//   image from pinned host memory; per wave the raw-line normalizer
//   (NormalizeLineWave, raw only), the encode, and the unknown-run merge of
//   PopulateSentencePieceText (raw only); then the block's token offsets, the
//   ids (and piece lengths) into the pinned image, and the publication word.
//   Every loop is bounded; nothing polls.
#include <hip/hip_runtime.h>

#include "bpe_device.h"
#include "coop_wave.h"

namespace spm_amd {
namespace {

constexpr uint32_t kNoSym = 0xFFFFu;  // next: no live symbol starts here; prev: the first symbol

// One wave's symbol state, by byte position.
struct BpeLineSyms {
  uint32_t key[kBpeLineMaxBytes];   // score rank of the pair (this, next live symbol); 0: no pair
  int32_t sym[kBpeLineMaxBytes];    // pieces_ id; a char outside pieces_: -1 - PieceToId
  int32_t pres[kBpeLineMaxBytes];   // the pair's merged piece
  uint16_t next[kBpeLineMaxBytes];  // start of the next live symbol (nb: the last one), or kNoSym
  uint16_t prev[kBpeLineMaxBytes];  // start of the previous live symbol, or kNoSym
};
static_assert(sizeof(BpeLineSyms) == 16 * kBpeLineMaxBytes, "16 bytes of state per position");
static_assert(kBpeLineMaxBytes < kNoSym && kBpeLineMaxBytes % 64 == 0, "16-bit links; 64 lanes share the positions");

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

__device__ __forceinline__ uint32_t Uniform(uint32_t v) {
  return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

// Encodes the normalized sentence s[0, nb) with one wave: its tokens' ids to
// out_ids[0, ntok) (and their byte lengths to out_len, nullable), in order;
// returns ntok, or kNone when the sentence is not taken.  Wave-uniform result;
// all 64 lanes call it together.
__device__ uint32_t BpeEncodeLineWave(const BpeArgs &a, BpeLineSyms &S, const uint8_t *__restrict__ s, uint32_t nb,
                                      int32_t *__restrict__ out_ids, uint32_t *__restrict__ out_len) {
  const uint32_t lane = threadIdx.x & 63;
  nb = Uniform(nb);
  if (nb == 0) return 0;
  if (nb > kBpeLineMaxBytes) return kNone;
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
    if (q >= 0 && qu) bad = true;
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
  uint32_t j = incl - cnt;
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
                              : BpeEncodeLineWave(a, sh.w[wave].s, l.bytes + b0, nb, tok,
                                                  kRaw || !c.len ? nullptr : l.slot_len + b0);
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
