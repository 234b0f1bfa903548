// What the one-wave-per-line small-call kernels share (coop_encode.hip: unigram,
// bpe_line.hip: BPE): the wave's LDS slab, the wave-parallel raw-line
// normalizer, the unknown-run merge of the id epilogue and the publication of
// a call's completion to the host.  Device only; every definition is local to
// the including file.
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.h"
#include "epilogue.h"
#include "kernels.h"
#include "normalize_prefix.h"

namespace spm_amd {
namespace {

constexpr int kCK = kCoopSlots;  // node slots per char start
constexpr int kCPos = 256;       // LDS ring of byte positions
constexpr int kCWaves = 4;       // waves (independent sentences) per block

struct CoopWave {
  // Per byte position (ring): bit L-1 = a node of L bytes begins here
  // (0: no char start), and the nodes' Viterbi backtrace scores by slot.
  uint64_t lmask[kCPos];
  union {
    float bt[kCPos][kCK];
    struct {                      // backtrace: a 64-char block of
      uint32_t pv[64][kCK];       //   (chosen lnode (length | slot << 7 | chars << 10) | node index
                                  //   - the block's first << 16) by (char, slot), and
      uint16_t dpv[64 * kCK];     //   the dense window of chosen lnodes the rows come from
    } b;
  } u;
  uint8_t ordlo[kCPos];         // per byte position (ring): low 8 bits of its char ordinal
  uint32_t bytes[kCPos / 4];    // sentence bytes [w, w + 256) of the current window
  uint32_t start[64];           // the window's char starts
  float score[64][kCK];         // node scores of the window's k-th char start, by slot
};


// LDS written by some lanes is read by others of the same wave: keep the
// compiler's order (the wave issues LDS operations in order).
__device__ __forceinline__ void WaveSync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Publishes a small call's completion: host_pub[1] (0 done / 1 not taken),
// then the sequence word, after a system-scope fence over the outputs.
__device__ void CoopPublish(const CoopCall &c, bool ok) {
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    c.host_pub[1] = ok ? 0u : 1u;
    __threadfence_system();
    __hip_atomic_store(&c.host_pub[0], c.pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// NormalizePrefix (normalizer.cc:231-300) as (rlen | consumed << 16, source):
// source 0 = the input at p, 1 << 30 | off = the charsmap pool at off,
// 2 << 30 = U+FFFD.
__device__ uint2 NormalizePrefixPacked(const NormTables &t, const uint8_t *in, uint64_t n) {
  if (t.ud_units) {
    const uint32_t m = TrieLongest(t.ud_units, t.ud_num_units, in, n);
    if (m) return make_uint2(m | m << 16, 0u);
  }
  uint32_t value = 0;
  const uint32_t longest = CharsmapLongest(t, in, n, &value);
  if (longest == 0) {
    const uint32_t len = DValidCharLen(in, n);
    if (len == 0) return make_uint2(3u | 1u << 16, 2u << 30);
    return make_uint2(len | len << 16, 0u);
  }
  const uint8_t *r = t.pool + value;
  uint32_t l = 0;
  while (r[l]) ++l;
  return make_uint2(l | longest << 16, 1u << 30 | value);
}

// Raw bytes one call takes per line: the prefix table lives in W.u.bt.
constexpr uint32_t kRawMaxBytes = sizeof(float) * kCPos * kCK / sizeof(uint2);

// Normalizes in[0, n) into out (capacity cap); returns the length, or kNone
// when the line is longer than kRawMaxBytes or its output exceeds cap.
__device__ uint32_t NormalizeLineWave(const NormTables &t, CoopWave &W, const uint8_t *in_g, uint32_t n, uint8_t *out,
                                      uint32_t cap) {
  const int lane = threadIdx.x & 63;
  if (n > kRawMaxBytes) return kNone;
  uint2 *pref = reinterpret_cast<uint2 *>(&W.u.bt[0][0]);
  // The line's bytes in LDS (W.lmask, free until the encode): the state
  // machine's byte reads are on its serial chain.
  static_assert(sizeof(W.lmask) >= kRawMaxBytes, "raw line staging");
  uint8_t *lin = reinterpret_cast<uint8_t *>(W.lmask);
  for (uint32_t q = static_cast<uint32_t>(lane); q < n; q += 64) lin[q] = in_g[q];
  WaveSync();
  const uint8_t *in = lin;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t p = base + static_cast<uint32_t>(lane);
    if (p < n) pref[p] = NormalizePrefixPacked(t, in + p, n - p);
  }
  WaveSync();
  // The state machine, 64 chain positions at a time.  Serially it walks the
  // chain p -> p + consumed(p), skips leading single-space pieces, emits the
  // dummy prefix, drops a piece's leading spaces after a space, escapes
  // spaces, and finally drops the trailing whitespace units.  Here the chain
  // is walked with scalar readlanes over the lanes' consumed lengths; each
  // visited lane then knows its piece's prev_space (ballots: the last
  // earlier non-empty piece ends in a space), counts its output bytes and
  // whitespace units, takes its offset from one wave scan and writes its
  // bytes; the trailing whitespace run is carried from block to block.
  const bool rew = t.remove_extra_whitespaces, esc = t.escape_whitespaces;
  const uint32_t wsl = esc ? 3u : 1u;
  const bool prefix_ws = !t.suffix && t.add_dummy_prefix;
  uint32_t p = 0, olen = 0, run = 0;
  bool started = false, carry_ps = rew;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t q = base + static_cast<uint32_t>(lane);
    const uint2 x = q < n ? pref[q] : make_uint2(1u << 16, 0u);
    const uint32_t rlen = x.x & 0xFFFFu, src = x.y;
    auto rbyte = [&](uint32_t k) -> uint32_t {
      const uint32_t kind = src >> 30;
      if (kind == 0) return in[q + k];
      if (kind == 1) return t.pool[(src & 0x3FFFFFFFu) + k];
      return (0xBDBFEFu >> (8 * k)) & 0xFFu;  // U+FFFD
    };
    // Chain positions in this block (wave-uniform walk over the lanes'
    // consumed lengths; every consumed length is >= 1).
    const uint32_t lim = n < base + 64 ? n : base + 64;
    const uint32_t cons = x.x >> 16;
    uint64_t vis = 0;
    if (__builtin_amdgcn_ballot_w64(q < n && cons != 1u) == 0) {
      // Every position of the block consumes one byte (ASCII text without
      // charsmap rewrites): the chain is every position from p on.
      const uint64_t upto = lim - base == 64 ? ~0ull : (1ull << (lim - base)) - 1ull;
      if (p < lim) vis = upto & ~((1ull << (p - base)) - 1ull);
      p = p < lim ? lim : p;
    } else {
      while (p < lim) {
        vis |= 1ull << (p - base);
        p += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cons), static_cast<int>(p - base)));
      }
    }
    const bool mine = (vis >> lane) & 1;
    // Leading whitespace (remove_extra_whitespaces): visited single-space
    // pieces before the first other one emit nothing; the dummy prefix goes
    // in front of that first emitting piece.
    int first = -1;
    uint64_t emitm = vis;
    if (!started && vis) {
      uint64_t cand = vis;
      if (rew) {
        const uint64_t sp = __builtin_amdgcn_ballot_w64(mine && rlen == 1 && rbyte(0) == ' ');
        cand = vis & ~sp;
      }
      if (cand) {
        first = __builtin_ctzll(cand);
        emitm = vis & ~((1ull << first) - 1);
        started = true;
      } else {
        emitm = 0;
      }
    }
    const bool emit = (emitm >> lane) & 1;
    // prev_space of this lane's piece (rew only): does the last earlier
    // non-empty emitting piece end in a space?
    const uint64_t ne = __builtin_amdgcn_ballot_w64(emit && rlen > 0);
    const uint64_t ls = __builtin_amdgcn_ballot_w64(emit && rlen > 0 && rbyte(rlen - 1) == ' ');
    bool ps = false;
    if (rew) {
      const uint64_t below = ne & ((1ull << lane) - 1);
      ps = below ? ((ls >> (63 - __builtin_clzll(below))) & 1) != 0 : carry_ps;
    }
    // Output bytes and whitespace units of this lane's piece (count pass,
    // then the same loop writes).
    const bool dummy = prefix_ws && lane == first;
    uint32_t ob = 0, wsu = 0, wtail = 0;
    bool nonws = false;
    uint32_t k0 = 0;
    if (emit) {
      if (dummy) {
        ob = wsl;
        wsu = wtail = 1;
      }
      if (ps)
        while (k0 < rlen && rbyte(k0) == ' ') ++k0;
      for (uint32_t k = k0; k < rlen;) {
        const uint32_t b0 = rbyte(k);
        if (b0 == ' ') {
          ob += wsl;
          ++wsu;
          ++wtail;
          ++k;
          continue;
        }
        const uint32_t cl = min(OneCharLenDev(b0), rlen - k);
        const bool is_ws = esc && cl == 3 && b0 == 0xE2 && rbyte(k + 1) == 0x96 && rbyte(k + 2) == 0x81;
        ob += cl;
        if (is_ws) {
          ++wsu;
          ++wtail;
        } else {
          nonws = true;
          wtail = 0;
        }
        k += cl;
      }
    }
    // Offsets: one inclusive scan of (bytes | ws units << 16).
    const uint32_t packed = ob | wsu << 16;
    uint32_t incl = packed;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o);
      if (lane >= o) incl += y;
    }
    const uint32_t tot = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
    if (emit) {
      uint32_t o = olen + ((incl - packed) & 0xFFFFu);
      auto put = [&](uint32_t v) {
        if (o < cap) out[o] = static_cast<uint8_t>(v);
        ++o;
      };
      auto put_ws = [&]() {
        if (esc) {
          put(0xE2);
          put(0x96);
          put(0x81);
        } else {
          put(' ');
        }
      };
      if (dummy) put_ws();
      for (uint32_t k = k0; k < rlen;) {
        const uint32_t b0 = rbyte(k);
        if (b0 == ' ') {
          put_ws();
          ++k;
          continue;
        }
        const uint32_t cl = min(OneCharLenDev(b0), rlen - k);
        for (uint32_t j = 0; j < cl; ++j) put(rbyte(k + j));
        k += cl;
      }
    }
    olen += tot & 0xFFFFu;
    // The trailing whitespace run: from the last lane with a non-whitespace
    // char, or carried on through a block without one.
    const uint64_t nw = __builtin_amdgcn_ballot_w64(emit && nonws);
    const uint32_t tot_ws = tot >> 16;
    if (nw) {
      const int J = 63 - __builtin_clzll(nw);
      run = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(wtail), J)) + tot_ws -
            (static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), J)) >> 16);
    } else {
      run += tot_ws;
    }
    if (ne) carry_ps = ((ls >> (63 - __builtin_clzll(ne))) & 1) != 0;
  }
  uint32_t len = 0;
  if (started) {
    len = olen;
    if (rew && run > 0) len -= run * wsl;  // trailing whitespace (normalizer.cc:191-202)
    if (t.suffix && t.add_dummy_prefix) {
      const uint32_t o = len + static_cast<uint32_t>(lane);
      if (static_cast<uint32_t>(lane) < wsl && o < cap)
        out[o] = static_cast<uint8_t>(esc ? (0x8196E2u >> (8 * lane)) & 0xFFu : ' ');
      len += wsl;
    }
  }
  const bool ok = len <= cap;
  __threadfence_block();
  WaveSync();
  return ok ? len : kNone;
}
// Unknown runs merge (epilogue.h Emits) of one wave's nt tokens at src,
// compacted in order to tok[0, m) (tok <= src: the same buffer); 64 at a
// time, the previous token's unknown bit from the ballot (the chunk's first:
// carried).  Returns m.
__device__ uint32_t MergeUnknownRunsWave(int32_t *tok, const int32_t *src, uint32_t nt, const uint8_t *types,
                                         int32_t num_types) {
  const int lane = threadIdx.x & 63;
  uint32_t m = 0;
  bool prev_unk = false;
  for (uint32_t c0 = 0; c0 < nt; c0 += 64) {
    const uint32_t t = c0 + static_cast<uint32_t>(lane);
    const int32_t id = t < nt ? src[t] : 0;
    const uint8_t ty = (t < nt && id >= 0 && id < num_types) ? types[id] : 0;
    const bool unk = (ty & kPieceUnknown) != 0;
    const uint64_t um = __builtin_amdgcn_ballot_w64(unk && t < nt);
    const bool pu = lane == 0 ? prev_unk : ((um >> (lane - 1)) & 1) != 0;
    const bool emit = t < nt && ((ty & kPieceControl) != 0 || !(pu && unk));
    const uint64_t em = __builtin_amdgcn_ballot_w64(emit);
    WaveSync();  // every lane's load of this chunk before any store
    if (emit) tok[m + __popcll(em & ((1ull << lane) - 1))] = id;
    m += static_cast<uint32_t>(__popcll(em));
    const uint32_t last = (nt - c0 < 64 ? nt - c0 : 64) - 1;
    prev_unk = ((um >> last) & 1) != 0;
  }
  return m;
}

}  // namespace
}  // namespace spm_amd
