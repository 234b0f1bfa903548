// BPE encode of real text for gfx950 (MI355X): the two tiers between the
// first kernels (bpe_kernels.hip: lane / half, then fast) and the literal
// bpe_general_kernel.  Both consume the sentences the first kernels flagged.
// bpe_split_kernel, ahead of bpe_fast_kernel, does that flagging for the
// sentences over 64 bytes.
//
// bpe_words_kernel — the word tier, for word-closed models: every piece is
//   "▁"* followed by chars other than "▁".  The reference (bpe_model.cc:37-199)
//   only merges adjacent symbols whose concatenation is a piece, so no merge
//   spans a cut, a "▁" that follows another char; merges on the two sides of
//   a cut never meet, the agenda order (score, then left index) restricted to
//   one word is the same relative order, and the sentence's tokens are its
//   words' tokens in order.
//   One flagged sentence of > 64 bytes per wavefront.  The wave first checks
//   that the sentence's OneCharLen walk is its non-continuation bytes (the
//   half kernel's check; otherwise a lead byte may swallow a "▁", and the
//   sentence goes unsplit to the wave tier).  It then scans the sentence 64
//   bytes per step from its last step to its first, finds the cuts by ballot
//   and queues the word starts in LDS; whenever 64 words wait (and at the
//   sentence's start) it encodes them one per LANE: symbol state in LDS
//   columns [char][lane] (pair key = the merged piece's score rank, symbol,
//   the pair's merged piece: 16 bits each), the live chars as a bit mask, per
//   merge the arg-max over the lane's keys (smallest left index on ties) and
//   the two new neighbour pairs probed in pair_ent together — the lane
//   kernel's rule and refusals.  The groups run from the sentence's last
//   words to its first, so a wave prefix sum over the lanes' token counts
//   places ids and piece lengths straight into the sentence's right-aligned
//   slots [off[i+1] - k, off[i+1]), which bpe_compact_kernel reads.
//   A word of more than kBpeWordChars chars (kernels.h: the lane bound; a
//   URL, a CJK line) is encoded by the whole wave with BpeEncodeLineWave if
//   it has <= kBpeLineMaxBytes bytes: its tokens wait in the slots of the
//   word's own bytes and move up once the group's counts are known.  A longer
//   word, a pushed UNUSED piece or a char outside an irregular vocabulary
//   hands the whole sentence to the literal kernel.
//   LDS per wave: 3 x 2 x 64 x kBpeWordChars = 6 KiB of columns, 512 B of
//   queue, and the line-wave state.  Two launches, as in bpe_dropout_kernel:
//   the first carries a state of kBpeDropShortBytes bytes (2 KiB; four waves
//   and 1 KiB of char entries per block: 35 KiB, four blocks = 16 waves in a
//   CU's 160 KiB) and lists a sentence with a longer word over the lane bound
//   in word_rest; the second takes that list with the full 16 KiB state (two
//   waves per block: 46 KiB, three blocks).  Prose stays in the first.
// bpe_wave_kernel — the wave tier: the flagged sentences of <= 1024 bytes the
//   word tier does not take (models that are not word-closed, walk-irregular
//   sentences), one per wavefront with BpeEncodeLineWave, in bpe_dropout_kernel's
//   layout: sentences of <= kBpeDropShortBytes bytes on 2 KiB slabs first, the
//   others from a list on 16 KiB slabs.  A flagged sentence of <= 64 bytes was
//   refused by bpe_fast_kernel for a reason this routine refuses too: straight
//   to the literal kernel, as is every refusal.
#include <hip/hip_runtime.h>

#include "bpe_device.h"
#include "bpe_line_wave.h"
#include "kernels.h"

namespace spm_amd {
namespace {

constexpr int kWordWavesShort = 4, kWordWavesFull = 2;
constexpr int kTextWaves = 4;
constexpr int kWC = kBpeWordChars;
static_assert(kWC <= 16, "16-bit live masks, 2 bits of char length per char in 32");

// One wave's lane columns [char][lane] and its queue of word starts.
struct WordCols {
  uint16_t key[kWC * 64];   // score rank of the pair (char, next live char); 0: no pair
  uint16_t sym[kWC * 64];   // pieces_ id; a char outside pieces_: ~PieceToId
  uint16_t pres[kWC * 64];  // the pair's merged piece
  uint32_t wq[128];         // starts of the words not yet encoded, descending
};

__device__ __forceinline__ int32_t Sym16(uint16_t v) { return static_cast<int16_t>(v); }

__device__ __forceinline__ BpeArgs TextArgs(const BpeTextLaunch &d) {
  BpeArgs a = BpeArgsOf(d.t);
  a.off = d.off;
  a.n = d.n;
  a.ntok = d.ntok;
  a.status = d.status;
  a.capacity = d.capacity;
  a.chain = d.chain;
  return a;
}

__device__ __forceinline__ void HandOn(uint32_t *list, uint32_t *count, uint32_t i) {
  list[atomicAdd(count, 1u)] = i;
}

__device__ __forceinline__ bool IsWs(const uint8_t *__restrict__ s, uint32_t p) {
  return s[p] == 0xE2u && s[p + 1] == 0x96u && s[p + 2] == 0x81u;
}

// Stores of some lanes to the slots are read by other lanes of the wave.
__device__ __forceinline__ void SlotSync() {
  __threadfence_block();
  WaveSync();
}

// The rest list of the lane / half kernel, split ahead of bpe_fast_kernel: a
// sentence of > 64 bytes is flagged here exactly as that kernel would flag it
// (ntok = ~0, an entry of `flagged`, kStFlagged, kStMaxNb), the others go on
// to it in fast_list.  One list entry per thread; a block takes its places in
// both lists with one atomicAdd each (bpe_fast_kernel pays an atomicAdd and an
// atomicMax on one cache line per flagged sentence, one sentence per wave:
// 20 ms for the 877 359 long lines of 1 M lines of prose).
constexpr int kSplitThreads = 256;
__global__ __launch_bounds__(kSplitThreads) void bpe_split_kernel(BpeTextLaunch d) {
  __shared__ uint32_t wcnt[2][kSplitThreads / 64], base[2];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const BpeArgs a = TextArgs(d);
  if (BpeSkip(a)) return;
  const uint64_t count = d.status[kStBpeRest];
  uint32_t longest = 0;
  for (uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * kSplitThreads; j0 < count;
       j0 += static_cast<uint64_t>(gridDim.x) * kSplitThreads) {
    const uint64_t j = j0 + threadIdx.x;
    const bool in = j < count;
    uint32_t i = 0;
    uint64_t nb = 0;
    if (in) {
      i = d.rest[j];
      nb = d.off[i + 1] - d.off[i];
    }
    const bool far = in && nb > 64;
    const uint64_t fm = __builtin_amdgcn_ballot_w64(far), nm = __builtin_amdgcn_ballot_w64(in && !far);
    if (lane == 0) {
      wcnt[0][wv] = static_cast<uint32_t>(__popcll(fm));
      wcnt[1][wv] = static_cast<uint32_t>(__popcll(nm));
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      uint32_t t = 0;
      for (int w = 0; w < kSplitThreads / 64; ++w) t += wcnt[threadIdx.x][w];
      base[threadIdx.x] = t ? atomicAdd(&d.status[threadIdx.x ? kStBpeFast : kStFlagged], t) : 0u;
    }
    __syncthreads();
    if (in) {
      const int which = far ? 0 : 1;
      uint32_t k = base[which] + static_cast<uint32_t>(__popcll((far ? fm : nm) & ((1ull << lane) - 1)));
      for (uint32_t w = 0; w < wv; ++w) k += wcnt[which][w];
      if (far) {
        d.ntok[i] = 0xFFFFFFFFu;
        d.flagged[k] = i;
        longest = max(longest, nb > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(nb));
      } else {
        d.fast_list[k] = i;
      }
    }
    __syncthreads();  // the next step rewrites the counts
  }
  longest = WaveMaxU(longest);
  if (lane == 0 && longest) atomicMax(&d.status[kStMaxNb], longest);
}

// kShort: the flagged sentences, with a line-wave state of kBpeDropShortBytes
// bytes; a sentence with a longer word over the lane bound waits in word_rest
// for the second launch, whose waves carry the full state.
template <uint32_t kSlabBytes, int kWordWaves, bool kShort>
__global__ __launch_bounds__(64 * kWordWaves) void bpe_words_kernel(BpeTextLaunch d) {
  __shared__ BpeLineSymsT<kSlabBytes> slab[kWordWaves];
  __shared__ WordCols cols[kWordWaves];
  __shared__ uint32_t lds_c1[256];  // CharEntryPacked of the one-byte chars
  __shared__ uint32_t lds_ws;       // and of U+2581
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const BpeArgs a = TextArgs(d);
  if (BpeSkip(a)) return;
  const uint32_t *__restrict__ list = kShort ? d.flagged : d.word_rest;
  const uint64_t count = d.status[kShort ? kStFlagged : kStBpeWordRest];
  if (count == 0) return;
  for (uint32_t c = threadIdx.x; c < 256; c += 64 * kWordWaves) lds_c1[c] = CharEntryPacked(a, c, 1);
  if (threadIdx.x == 0) lds_ws = CharEntryPacked(a, 0x8196E2u, 3);
  __syncthreads();
  WordCols &W = cols[wv];
  const uint32_t mask = static_cast<uint32_t>(a.pair_mask);
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * kWordWaves + wv;
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kWordWaves;
  uint32_t done = 0;
  for (uint64_t jl = wave; jl < count; jl += nwaves) {
    const uint32_t i = list[jl];
    const uint64_t b0 = d.off[i];
    const uint64_t nb64 = d.off[i + 1] - b0;
    // (<= 64 bytes: refused by the fast kernel; byte positions are 32-bit.)
    if (nb64 <= 64 || nb64 > 0x7FFFFFFFull) {
      if (lane == 0) HandOn(d.literal, d.status + kStBpeLiteral, i);
      continue;
    }
    const uint32_t nb = static_cast<uint32_t>(nb64);
    const uint8_t *__restrict__ s = a.bytes + b0;
    int32_t *const sid = a.slot_ids + b0;
    uint32_t *const sln = a.slot_len ? a.slot_len + b0 : nullptr;
    // ---- 1. the OneCharLen walk against the non-continuation bytes.
    bool odd = false;
    for (uint32_t p = lane; p < nb; p += 64) {
      const uint32_t c = s[p];
      if ((c & 0xC0u) == 0x80u) {
        if (p == 0) odd = true;
        continue;
      }
      uint32_t cl = OneCharLenB(c);
      if (cl > nb - p) cl = nb - p;
      for (uint32_t j = 1; j < cl; ++j)
        if ((s[p + j] & 0xC0u) != 0x80u) odd = true;
      if (p + cl < nb && (s[p + cl] & 0xC0u) == 0x80u) odd = true;
    }
    if (__builtin_amdgcn_ballot_w64(odd) != 0) {
      if (lane == 0) HandOn(d.wave_list, d.status + kStBpeWaveList, i);
      continue;
    }
    // ---- 2. the scan, last step first; groups of 64 words as they fill.
    uint32_t qn = 0;      // queued word starts
    uint32_t qend = nb;   // end of the first queued word
    uint32_t tail = 0;    // tokens placed, from the sentence's end
    bool refuse = false;  // wave-uniform: the sentence leaves this launch (to the literal kernel,
    bool defer = false;   // or, defer, to the launch with the full line-wave state)
    for (uint32_t ch = (nb + 63) >> 6; ch-- > 0 && !refuse;) {
      const uint32_t p = ch * 64 + lane;
      bool cut = p == 0;  // the first word starts the sentence
      if (p > 0 && p + 2 < nb) cut = IsWs(s, p) && !(p >= 3 && IsWs(s, p - 3));
      const uint64_t cm = __builtin_amdgcn_ballot_w64(cut);
      if (cut) W.wq[qn + __popcll((cm >> lane) >> 1)] = p;
      qn += __popcll(cm);
      WaveSync();
      while (!refuse && (qn >= 64 || (ch == 0 && qn > 0))) {
        const uint32_t g = qn < 64 ? qn : 64u;
        const bool has = lane < g;
        const uint32_t ws = has ? W.wq[lane] : 0u;
        const uint32_t we = has ? (lane ? W.wq[lane - 1] : qend) : 0u;
        const uint32_t next_qend = W.wq[g - 1];
        // -- the lane's word: chars, symbols, initial pairs.
        uint32_t nch = 0, clen = 0;  // clen: char k's byte length - 1 in bits 2k, 2k + 1
        bool big = has && we - ws > 4u * kWC, bad = false;
        if (has && !big) {
          for (uint32_t q = ws; q < we;) {
            if (nch == kWC) {
              big = true;
              break;
            }
            const uint32_t c0 = s[q];
            uint32_t L = OneCharLenB(c0);
            if (L > we - q) L = we - q;  // (a regular walk never crosses a cut)
            int32_t sym, out;
            if (L == 1 || (L == 3 && IsWs(s, q))) {
              const uint32_t so = L == 1 ? lds_c1[c0] : lds_ws;
              sym = static_cast<int16_t>(so & 0xFFFFu);
              out = static_cast<int32_t>(so >> 16);
            } else {
              const int32_t e = ExactEntry(a, s + q, L);
              sym = e >= 0 ? a.entry_piece[e] : -1;
              out = e >= 0 ? a.entry_out[e] : a.unk_id;
            }
            if (a.irregular && sym < 0) bad = true;
            W.sym[nch * 64 + lane] = static_cast<uint16_t>((sym >= 0 ? sym : ~out) & 0xFFFF);
            W.key[nch * 64 + lane] = 0;
            W.pres[nch * 64 + lane] = 0;
            clen |= (L - 1) << (2 * nch);
            ++nch;
            q += L;
          }
        }
        if (big) nch = 0;
        // Pairs (k, k + 1) of in-vocabulary symbols, four probes issued
        // together; a probe that meets another key walks on alone.
        for (uint32_t k0 = 0; k0 + 1 < nch; k0 += 4) {
          int32_t l[4], r[4];
          uint32_t h[4];
          uint4 e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t k = k0 + j;
            const bool en = k + 1 < nch;
            l[j] = en ? Sym16(W.sym[k * 64 + lane]) : -1;
            r[j] = en ? Sym16(W.sym[(k + 1) * 64 + lane]) : -1;
            const bool need = l[j] >= 0 && r[j] >= 0;
            h[j] = need ? PairHash((static_cast<uint64_t>(static_cast<uint32_t>(l[j])) << 32) |
                                   static_cast<uint32_t>(r[j])) & mask
                        : 0u;
            e[j] = need ? a.pair_ent[h[j]] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (l[j] < 0 || r[j] < 0) continue;
            uint4 x = e[j];
            uint32_t hh = h[j];
            while (!(x.x == static_cast<uint32_t>(r[j]) && x.y == static_cast<uint32_t>(l[j])) &&
                   !(x.x == 0xFFFFFFFFu && x.y == 0xFFFFFFFFu)) {
              hh = (hh + 1) & mask;
              x = a.pair_ent[hh];
            }
            if (x.x == 0xFFFFFFFFu && x.y == 0xFFFFFFFFu) continue;
            W.key[(k0 + j) * 64 + lane] = static_cast<uint16_t>(x.w);
            W.pres[(k0 + j) * 64 + lane] = static_cast<uint16_t>(x.z & 0x7FFFu);
            if ((x.z >> 31) != 0) bad = true;
          }
        }
        // The scan below reads the columns up to the group's longest word.
        uint32_t maxn = nch;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) maxn = max(maxn, static_cast<uint32_t>(__shfl_xor(static_cast<int>(maxn), o)));
        for (uint32_t k = nch; k < maxn; ++k) W.key[k * 64 + lane] = 0;
        // -- merges: the arg-max pair, smallest left index on ties.
        uint32_t live = (1u << nch) - 1u;
        bool act = !bad && nch > 1;
        while (__builtin_amdgcn_ballot_w64(act) != 0) {
          uint32_t bm = 0u;
          if (act)
            for (uint32_t q = 0; q < maxn; ++q)
              bm = max(bm, (static_cast<uint32_t>(W.key[q * 64 + lane]) << 4) | (15u - q));
          if ((bm >> 4) == 0u) act = false;
          if (!act) continue;
          const int Lk = 15 - static_cast<int>(bm & 15u);
          const uint32_t above = live & ~((2u << Lk) - 1u);
          if (above == 0u) {  // (a pair always has a live right char)
            bad = true;
            act = false;
            continue;
          }
          const int Rk = __builtin_ctz(above);
          const uint32_t above_r = live & ~((2u << Rk) - 1u);
          const int RRk = above_r ? __builtin_ctz(above_r) : -1;
          const uint32_t below = live & ((1u << Lk) - 1u);
          const int Pk = below ? 31 - __builtin_clz(below) : -1;
          const int32_t merged = W.pres[Lk * 64 + lane];
          live &= ~(1u << Rk);
          W.key[Rk * 64 + lane] = 0;
          // New pairs (P, L) and (L, RR) — the reference's push order.
          const int32_t symP = Pk >= 0 ? Sym16(W.sym[Pk * 64 + lane]) : -1;
          const int32_t symRR = RRk >= 0 ? Sym16(W.sym[RRk * 64 + lane]) : -1;
          int32_t mP, mL;
          uint32_t kP, kL;
          bool uP, uL;
          PairLookupFused2(a, symP, merged, Pk >= 0, merged, symRR, RRk >= 0, &mP, &kP, &uP, &mL, &kL, &uL);
          if (Pk >= 0) {
            W.key[Pk * 64 + lane] = static_cast<uint16_t>(mP >= 0 ? kP : 0u);
            W.pres[Pk * 64 + lane] = static_cast<uint16_t>(mP & 0x7FFF);
          }
          W.key[Lk * 64 + lane] = static_cast<uint16_t>(mL >= 0 ? kL : 0u);
          W.pres[Lk * 64 + lane] = static_cast<uint16_t>(mL & 0x7FFF);
          W.sym[Lk * 64 + lane] = static_cast<uint16_t>(merged);
          if ((mP >= 0 && uP) || (mL >= 0 && uL)) {
            bad = true;
            act = false;
          }
        }
        if (__builtin_amdgcn_ballot_w64(bad) != 0) {
          refuse = true;
          break;
        }
        // -- words over the lane bound, by the whole wave; their tokens wait
        // from the word's first slot on.
        uint32_t cnt = static_cast<uint32_t>(__popc(live));
        const uint64_t bigm = __builtin_amdgcn_ballot_w64(big);
        for (uint64_t bm = bigm; bm != 0 && !refuse; bm &= bm - 1) {
          const int b = __ffsll(static_cast<long long>(bm)) - 1;
          const uint32_t bs = static_cast<uint32_t>(__shfl(static_cast<int>(ws), b));
          const uint32_t be = static_cast<uint32_t>(__shfl(static_cast<int>(we), b));
          if (kShort && be - bs > kSlabBytes && be - bs <= kBpeLineMaxBytes) {
            refuse = defer = true;
            break;
          }
          const uint32_t nt = BpeEncodeLineWave<kSlabBytes, false, false>(
              a, slab[wv], s + bs, be - bs, sid + bs, sln ? sln + bs : nullptr, BpeDropKey{});
          if (nt == kNone) refuse = true;
          else if (lane == static_cast<uint32_t>(b)) cnt = nt;
        }
        if (refuse) break;
        // -- placement: lane 0 holds the group's last word.
        uint32_t incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t y = __shfl_up(incl, o);
          if (lane >= static_cast<uint32_t>(o)) incl += y;
        }
        const uint32_t total = static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63));
        const uint32_t dst = nb - tail - incl;  // the lane's first slot
        if (bigm != 0) {
          // The waiting tokens move up (never down), the last word's first:
          // a word's place may cover the waiting place of a later word, and
          // an earlier word's place this word's.
          SlotSync();
          for (uint64_t bm = bigm; bm != 0; bm &= bm - 1) {
            const int b = __ffsll(static_cast<long long>(bm)) - 1;
            const uint32_t src = static_cast<uint32_t>(__shfl(static_cast<int>(ws), b));
            const uint32_t to = static_cast<uint32_t>(__shfl(static_cast<int>(dst), b));
            const uint32_t nt = static_cast<uint32_t>(__shfl(static_cast<int>(cnt), b));
            if (to == src) continue;
            for (uint32_t c64 = (nt + 63) >> 6; c64-- > 0;) {
              const uint32_t t = c64 * 64 + lane;
              int32_t vid = 0;
              uint32_t vln = 0;
              if (t < nt) {
                vid = sid[src + t];
                if (sln) vln = sln[src + t];
              }
              SlotSync();
              if (t < nt) {
                sid[to + t] = vid;
                if (sln) sln[to + t] = vln;
              }
              SlotSync();
            }
          }
        }
        if (has && !big) {
          uint32_t j = dst, beg = 0, q = ws;
          int pk = -1;
          auto emit = [&](int k, uint32_t b, uint32_t e) {
            const int32_t symx = Sym16(W.sym[k * 64 + lane]);
            sid[j] = symx >= 0 ? a.piece_out[symx] : ~symx;
            if (sln) sln[j] = e - b;
            ++j;
          };
          for (uint32_t k = 0; k < nch; ++k) {
            if ((live >> k) & 1u) {
              if (pk >= 0) emit(pk, beg, q);
              pk = static_cast<int>(k);
              beg = q;
            }
            q += ((clen >> (2 * k)) & 3u) + 1u;
          }
          if (pk >= 0) emit(pk, beg, we);
        }
        tail += total;
        // The words left in the queue move to its front.
        const uint32_t rem = qn - g;
        const uint32_t keep = lane < rem ? W.wq[g + lane] : 0u;
        WaveSync();
        if (lane < rem) W.wq[lane] = keep;
        WaveSync();
        qend = next_qend;
        qn = rem;
      }
    }
    if (lane == 0) {
      if (defer) HandOn(d.word_rest, d.status + kStBpeWordRest, i);
      else if (refuse) HandOn(d.literal, d.status + kStBpeLiteral, i);
      else a.ntok[i] = tail;
    }
    if (!refuse) ++done;
    SlotSync();  // the next sentence reuses the queue and the slab
  }
  if (lane == 0 && done) atomicAdd(&d.status[kStBpeWordDone], done);
}

// kShort: the listed sentences on short slabs, the longer ones to wave_rest;
// else the sentences of wave_rest on full slabs.
template <uint32_t kMaxBytes, bool kShort>
__global__ __launch_bounds__(64 * kTextWaves) void bpe_wave_kernel(BpeTextLaunch d) {
  __shared__ BpeLineSymsT<kMaxBytes> slab[kTextWaves];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const BpeArgs a = TextArgs(d);
  if (BpeSkip(a)) return;
  const uint32_t *__restrict__ list = !kShort ? d.wave_rest : d.word_closed ? d.wave_list : d.flagged;
  const uint64_t count = d.status[!kShort ? kStBpeWaveRest : d.word_closed ? kStBpeWaveList : kStFlagged];
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * kTextWaves + wv;
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kTextWaves;
  uint32_t done = 0;
  for (uint64_t jl = wave; jl < count; jl += nwaves) {
    const uint32_t i = list[jl];
    const uint64_t b0 = d.off[i];
    const uint64_t nb64 = d.off[i + 1] - b0;
    if ((kShort && nb64 <= 64) || nb64 > kBpeLineMaxBytes) {
      if (lane == 0) HandOn(d.literal, d.status + kStBpeLiteral, i);
      continue;
    }
    if (nb64 > kMaxBytes) {
      if (lane == 0) HandOn(d.wave_rest, d.status + kStBpeWaveRest, i);
      continue;
    }
    const uint32_t nb = static_cast<uint32_t>(nb64);
    const uint32_t nt = BpeEncodeLineWave<kMaxBytes, false, true>(a, slab[wv], a.bytes + b0, nb, a.slot_ids + b0,
                                                                  a.slot_len ? a.slot_len + b0 : nullptr, BpeDropKey{});
    if (nt != kNone) ++done;
    if (lane == 0) {
      if (nt == kNone) HandOn(d.literal, d.status + kStBpeLiteral, i);
      else a.ntok[i] = nt;
    }
  }
  if (lane == 0 && done) atomicAdd(&d.status[kStBpeWaveDone], done);
}

}  // namespace

hipError_t LaunchBpeSplit(const BpeTextLaunch &d, hipStream_t st) {
  if (d.n == 0) return hipSuccess;
  const uint64_t b = (d.n + kSplitThreads - 1) / kSplitThreads;
  hipLaunchKernelGGL(bpe_split_kernel, dim3(static_cast<unsigned>(b < 1024 ? b : 1024)), dim3(kSplitThreads), 0, st, d);
  return hipGetLastError();
}

hipError_t LaunchBpeText(const BpeTextLaunch &d, hipStream_t st) {
  if (d.n == 0) return hipSuccess;
  // Grid-stride over device-side lists of up to n sentences.  The grids are
  // sized from n, not from the lists' counts (which only the device knows):
  // on a batch that flags nothing, each launch is full-width, reserves its
  // LDS and reads a zero count.  Measured on 10 M c3 sentences: inside the
  // run-to-run spread of the call.
  auto blocks = [&](int waves) {
    const uint64_t b = (d.n + waves - 1) / waves;
    return dim3(static_cast<unsigned>(b < 4096 ? b : 4096));
  };
  if (d.word_closed) {
    hipLaunchKernelGGL((bpe_words_kernel<kBpeDropShortBytes, kWordWavesShort, true>), blocks(kWordWavesShort),
                       dim3(64 * kWordWavesShort), 0, st, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((bpe_words_kernel<kBpeLineMaxBytes, kWordWavesFull, false>), blocks(kWordWavesFull),
                       dim3(64 * kWordWavesFull), 0, st, d);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((bpe_wave_kernel<kBpeDropShortBytes, true>), blocks(kTextWaves), dim3(64 * kTextWaves), 0, st, d);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((bpe_wave_kernel<kBpeLineMaxBytes, false>), blocks(kTextWaves), dim3(64 * kTextWaves), 0, st, d);
  return hipGetLastError();
}

}  // namespace spm_amd
