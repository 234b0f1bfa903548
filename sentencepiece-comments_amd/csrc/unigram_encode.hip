// Unigram Viterbi encode kernels for gfx950 (MI355X).
//
// Reference path: unigram::Model::Encode (unigram_model.cc:705-720) =
//   Lattice::SetSentence (:147-187) + Model::PopulateNodes (:535-604, a darts
//   commonPrefixSearch per char position) + Lattice::Viterbi (:222-261).
//
// unigram_fast_kernel — one sentence per lane, the lattice never materialised:
//   Viterbi's backtrace score of a node (b,e) with score s is
//     max_l fl(bt_l + s) over lnodes ending at b  ==  fl(T_b + s),
//   T_b = max bt of the nodes ending at b, because float rounding is monotone.
//   So the forward pass keeps only T per pending end position, in a register
//   ring indexed by the (static, unrolled) distance of the trie walk.  The
//   argmax *identity* (the back-pointer) is what float ties can change: the
//   reference takes the FIRST lnode in end_nodes order (= ascending begin)
//   with the maximal fl(bt_l + s).  Only the successive running-max setters of
//   an end position can win; a setter more than a few ulps below the final
//   max never ties.  So per end position the kernel keeps B (first setter of
//   T) and, when the previous setter is within the near-tie bound, an
//   "ambiguity" entry (T, T2, B2); the backtrace resolves
//   winner = (fl(T2+s) == fl(T+s)) ? B2 : B exactly.  A sentence whose ties
//   chain deeper, overflows the entry list, meets a trie leaf inside a UTF-8
//   char, holds a 0xFF byte (byte kernel) or has an inconsistent back-pointer
//   chain is flagged and re-run by unigram_general_kernel, a literal
//   restatement of the reference lattice.
//
// Two forward passes:
//   kByte (W = 16, models whose pieces are whole chars of < 16 bytes): every
//     byte position is visited, char starts found by the lead-byte chain;
//     positions walked in pairs (two independent trie-load chains per lane
//     up to depth 5, one chain per lane past it, a second pass for the lanes
//     with two deep chains),
//     inserts lagged one walk step behind their score loads (software
//     pipeline), back-pointers packed as 8-bit distances, 2 near-tie entries,
//     7 waves/SIMD.  (Round-2 A/B of the alternatives — LDS trie top, jump
//     table, lane-decoupled walk, 4-6 waves — is in DESIGN.md §4.)
//   kChar (W = 16/32/64): one char position at a time, full back-pointers,
//     4 near-tie entries, values + scores tables.
//
// Output: lanes count their tokens with a first backtrace, the block scans
// the counts in sentence order and the second backtrace writes ids / piece
// lengths densely into the tile's slot range (at the tile's first input
// byte); tile_compact_kernel then places every tile (compact.hip).  The byte
// encode kernel has no second backtrace: the count leaves the final chain in
// the back-pointer bytes, the lanes list their tokens as (offset, length)
// descriptors in LDS and the block looks them up one token per thread.
//
// Back-pointers: one byte per char position (end - winner begin), in LDS for
// byte positions < kLdsBpPos, beyond that in a global scratch array indexed
// like the input bytes (position nb — EOS — included).  The backtrace checks
// every step (begin < end) and flags the sentence otherwise, so a bad
// back-pointer can never spin a wave.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "device_common.h"
#include "kernels.h"
#include "lookback.h"  // status words
#include "piece_table.h"

namespace spm_amd {
namespace {

struct FastArgs {
  const uint8_t *__restrict__ bytes;
  const uint64_t *__restrict__ off;
  uint64_t n;
  uint64_t capacity;
  const uint32_t *__restrict__ units;
  const int32_t *__restrict__ values;
  const float *__restrict__ scores;
  uint32_t num_units;
  UnigramParams p;
  int32_t *__restrict__ ids;
  uint32_t *__restrict__ len;
  uint64_t *__restrict__ tok_off;
  uint8_t *__restrict__ bp;
  uint32_t *__restrict__ flagged;
  uint32_t *__restrict__ status;
  uint64_t *__restrict__ tile_count;
  uint64_t corrupt_bp;
  const uint32_t *__restrict__ chain;
  int32_t *__restrict__ slot_ids;  // tile-dense token slots (capacity entries)
  uint32_t *__restrict__ slot_len;
  EStepForwardOut e;               // E-step forward pass (kE instantiation only)
  uint32_t *__restrict__ bpn;      // kWide: trie unit of the best node ending at each byte position
  const uint32_t *stage_src;       // single-tile host call: input image in pinned host memory
  uint32_t *stage_dst;
  uint32_t stage_zero;             // leading words zeroed instead of copied (the status block)
  uint32_t stage_words;
  uint32_t *host_pub;              // single-tile host call: status words + sequence to host memory
  uint32_t pub_seq;
  uint32_t coop_min_nb;            // wide / char kernels: longer sentences go to the cooperative kernel
  const uint32_t *__restrict__ piece_tab;  // byte kernel: piece -> (id, score) table (piece_table.h), nullable
  uint32_t piece_mask, piece_seed;         // its header words
};

// Byte kB of w = kV (an inline constant, 0..64) in the lanes of wave mask m:
// one sub-dword select.  (Written as and / or / select the compiler spends
// two literal operations and a select on every byte but the lowest.)  The
// s_nop keeps the next instruction, which the compiler's hazard check cannot
// see into an asm for, one wait state from the sub-dword write (gfx940+: a
// vector instruction must not read such a result in the very next issue).
template <int kB, int kV>
__device__ __forceinline__ void SetByteIf(uint32_t &w, uint64_t m) {
  static_assert(kB >= 0 && kB < 4 && kV >= 0 && kV <= 64, "a byte of a dword, an inline constant");
  if constexpr (kB == 0)
    __asm__("s_mov_b64 vcc, %1\n\tv_cndmask_b32_sdwa %0, %0, %2, vcc dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE "
            "src0_sel:BYTE_0 src1_sel:DWORD\n\ts_nop 0" : "+v"(w) : "s"(m), "n"(kV) : "vcc");
  else if constexpr (kB == 1)
    __asm__("s_mov_b64 vcc, %1\n\tv_cndmask_b32_sdwa %0, %0, %2, vcc dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE "
            "src0_sel:BYTE_1 src1_sel:DWORD\n\ts_nop 0" : "+v"(w) : "s"(m), "n"(kV) : "vcc");
  else if constexpr (kB == 2)
    __asm__("s_mov_b64 vcc, %1\n\tv_cndmask_b32_sdwa %0, %0, %2, vcc dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE "
            "src0_sel:BYTE_2 src1_sel:DWORD\n\ts_nop 0" : "+v"(w) : "s"(m), "n"(kV) : "vcc");
  else
    __asm__("s_mov_b64 vcc, %1\n\tv_cndmask_b32_sdwa %0, %0, %2, vcc dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE "
            "src0_sel:BYTE_3 src1_sel:DWORD\n\ts_nop 0" : "+v"(w) : "s"(m), "n"(kV) : "vcc");
}

constexpr int kBlock = 256;
constexpr int kLdsBpPos = 64;  // back-pointer bytes kept in LDS per lane
constexpr int kEStepWaves = 4;  // E-step forward mode (alpha ring + fp64 LogSumExp)

// kE (byte kernel only): the unigram trainer E-step's forward pass on the same
// walk — besides the Viterbi ring it keeps the alpha ring of PopulateMarginal
// (unigram_model.cc:272-300: alpha of the nodes ending at each byte slot,
// LogSumExp over end_nodes in ascending begin order, which is the order the
// lagged inserts reach a slot), writes alpha at every char start, Z = alpha
// of EOS, the node count and Viterbi().size(), and skips the id output.
template <int W, bool kByte, int kWaves = kByte ? 7 : (W == 16 ? 4 : 1), bool kE = false, bool kWide = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves)))
void unigram_fast_kernel(FastArgs a) {
  static_assert(!kByte || W == 16, "the byte kernel's ring and window are sized for W = 16");
  static_assert(!kE || kByte, "the E-step forward pass is a byte-kernel mode");
  static_assert(!kWide || (!kByte && W == 16), "the wide-char pass rings 16 chars");
  // Back-pointer bytes of byte positions [0, kLdsBpPos) of each lane's
  // sentence: word (pos/4)*kBlock + tid, byte pos%4.
  __shared__ uint32_t lds_bp[(kLdsBpPos / 4) * kBlock];
  __shared__ uint32_t lds_scan[kBlock];
  __shared__ uint32_t lds_wave[kBlock / 64];
  __shared__ uint32_t lds_tile;
  // Byte kernel: (unit, score) of the root's 256 children, the first step of
  // every walk (32 % of the trie gathers), served by LDS instead of the
  // vector-memory address path the walk is bound by: 4.17 -> 4.08 ms per
  // 10 M c2 sentences (profiles/r03k_root_lds_ab.txt).
  constexpr bool kRootLds = kByte || kWide;
  // Byte encode kernel: the length sort's table, the root table and (once
  // both are dead) the output stage's token descriptors share one LDS buffer.
  // The tile's tokens are staged there, a window of kStageIds at a time, and
  // looked up and written out one per thread, as coalesced runs: written
  // straight from the backtrace (4 bytes per lane per step, scattered over
  // the tile's range) the ids were 640 of the kernel's 750 MB of HBM writes
  // and cost 420 MB of reads per 10 M sentences (profiles/r04u_pmc_c2_*.json).
  // The buffer fills what the 7-block occupancy leaves of the CU's LDS
  // (22.5 KB per block after allocation granularity; at 1472 ids the block
  // rounded past it, 6 blocks fit and the kernel ran 7 % slower).
  constexpr bool kStage = kByte && !kE;
  constexpr uint32_t kStageIds = kStage ? 1264u : 2u;
  __shared__ uint2 lds_union[kStageIds / 2];
  __shared__ uint32_t lds_sort_own[kStage ? 1 : 2 * kBlock];
  __shared__ uint2 lds_root_own[(kRootLds && !kStage) ? kBlock + (kE ? 1 : 0) : 1];  // kE: + the byte pass's entry 256
  uint32_t *const lds_stage = reinterpret_cast<uint32_t *>(lds_union);
  uint32_t *const lds_sort = kStage ? lds_stage : lds_sort_own;
  uint2 *const lds_root = kStage ? lds_union + kBlock : lds_root_own;
  uint8_t *lbp = reinterpret_cast<uint8_t *>(lds_bp);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  if constexpr (!kE) {
    // Single-tile host call: the status block is zeroed here and the rest of
    // the input image (offsets, bytes) comes from pinned host memory in one
    // coalesced pass
    // (no separate copy command on the per-call path).  The fences order
    // these stores before every later read of the same memory.
    if (a.stage_src) {
      for (uint32_t k = static_cast<uint32_t>(tid); k < a.stage_zero; k += kBlock) a.stage_dst[k] = 0u;
      for (uint32_t k = a.stage_zero + static_cast<uint32_t>(tid); k < a.stage_words; k += kBlock)
        a.stage_dst[k] = a.stage_src[k];
      __threadfence_block();
      __syncthreads();
    }
  }
  // An earlier step of an asynchronous chain failed: nothing to do.
  if (a.chain && *a.chain) return;
  const uint64_t total_bytes = a.off[a.n];
  // A batch larger than the caller's capacity (the scratch is sized by it):
  // every tile leaves before touching anything, the error is reported.
  if (total_bytes > a.capacity) {
    if (blockIdx.x == 0 && tid == 0) atomicOr(&a.status[kStError], 2u);
    return;
  }
  // Tiles in launch order (the look-back's progress guarantee).
  if (tid == 0) lds_tile = atomicAdd(&a.status[kStTicket], 1u);
  if constexpr (kRootLds) {
    const uint32_t nd = a.p.root_base ^ static_cast<uint32_t>(tid);
    uint2 r = nd < a.num_units ? reinterpret_cast<const uint2 *>(a.units)[nd] : make_uint2(0u, 0u);
    if constexpr (kByte) {
      // The byte pass takes a position's depth-1 node score from this table
      // as it stands: NaN unless byte `tid` has a root child, and for a
      // one-byte char (NUL included) the UNK node's score when it has no
      // usable single-char node (unigram_model.cc:597-601), so the forward
      // pass needs no UNK select for ASCII.  Only the score changes: the
      // backtrace looks the token up by its bytes, misses and emits unk_id.
      float sc = (r.x & 0xFFu) == static_cast<uint32_t>(tid) ? __uint_as_float(r.y) : __builtin_nanf("");
      if (tid < 0x80 && __builtin_isnan(sc)) sc = a.p.unk_score;
      r.y = __float_as_uint(sc);
      // Entry 256: what a position that is no char start reads (label 0xFF
      // matches no byte of an unflagged sentence, no node).
      if (tid == 0) lds_root[kBlock] = make_uint2(0xFFu, __float_as_uint(__builtin_nanf("")));
    }
    lds_root[tid] = r;
  }
  __syncthreads();
  const uint64_t tile = lds_tile;
  const uint64_t base = tile * kBlock;

  // Counting sort of the tile's sentences by length (0..255): each wave's 64
  // lanes then run similar trip counts.
  uint32_t sid;
  {
    uint32_t *hist = lds_sort, *perm = lds_sort + kBlock;
    const uint64_t ii = base + tid;
    const uint32_t len = ii < a.n ? static_cast<uint32_t>(a.off[ii + 1] - a.off[ii]) : 0u;
    // Exact up to 191 bytes, then 32-byte bins up to 2207 (paragraph-length
    // lines of real text would otherwise share one bin and a wave would run
    // as long as its longest line).
    const uint32_t bucket = len < 192 ? len : len < 2208 ? 192 + (len - 192) / 32 : kBlock - 1;
    hist[tid] = 0;
    __syncthreads();
    const uint32_t r = atomicAdd(&hist[bucket], 1u);
    __syncthreads();
    if (wave == 0) {  // exclusive scan of 256 bins, 4 per lane
      uint32_t v[4], tot = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = hist[lane * 4 + q];
        tot += v[q];
      }
      uint32_t x = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
      }
      uint32_t run = x - tot;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t c = v[q];
        hist[lane * 4 + q] = run;
        run += c;
      }
    }
    __syncthreads();
    perm[hist[bucket] + r] = static_cast<uint32_t>(tid);
    __syncthreads();
    sid = perm[tid];
  }
  const uint64_t i = base + sid;
  const bool valid = i < a.n;
  if constexpr (kE) {
    if (a.e.AT) {
      a.e.lanemap[base + tid] = static_cast<uint8_t>(sid);
      if (valid) a.e.colmap[i] = static_cast<uint16_t>(tid);
    }
  }
  const uint64_t b0 = valid ? a.off[i] : 0;
  const uint32_t nb = valid ? static_cast<uint32_t>(a.off[i + 1] - b0) : 0;

  // Byte kernel: the tile's bytes from its first aligned byte as a buffer
  // resource, lanes address them by a 32-bit offset (no per-lane 64-bit
  // pointers live in the walk).  The back-pointer scratch beyond the LDS
  // window is a second resource over the same offsets (bp + blk_al + lrel +
  // pos == bp + b0 + pos).  Its range is the scratch's own size, capacity +
  // 16 bytes, so it covers position nb of the batch's last sentence, one past
  // the last input byte (the round-2 hang: a back-pointer resource whose
  // num_records ended at the last input byte dropped exactly that store).
  // Buffer accesses also keep the compiler from merging the LDS and global
  // branches of bp_store / bp_load into flat accesses.
  const uint64_t blk_al = a.off[base] & ~3ull;
  const uint64_t blk_rem = total_bytes - blk_al;
  const int blk_nrec = static_cast<int>(blk_rem < 0x7FFFFFF0ull ? blk_rem : 0x7FFFFFF0ull);
  const auto bytes_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.bytes + blk_al), 0, blk_nrec, 0x00020000);
  const uint64_t bp_rem = a.capacity + 16 - blk_al;
  const auto bp_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      a.bp + blk_al, 0, static_cast<int>(bp_rem < 0x7FFFFFFFull ? bp_rem : 0x7FFFFFFFull), 0x00020000);
  const uint32_t lrel = static_cast<uint32_t>(b0 - blk_al);
  const uint8_t *__restrict__ s = a.bytes + b0;

  auto byte_at = [&](uint32_t q) -> uint32_t {
    if constexpr (kByte) return __builtin_amdgcn_raw_buffer_load_b8(bytes_rsrc, lrel + q, 0, 0);
    else return s[q];
  };
  auto bp_store = [&](uint32_t pos, uint32_t v) {
    if (pos < kLdsBpPos) lbp[((pos >> 2) * kBlock + tid) * 4 + (pos & 3)] = static_cast<uint8_t>(v);
    else __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(v), bp_rsrc, lrel + pos, 0, 0);
  };
  auto bp_load = [&](uint32_t pos) -> uint32_t {
    if (pos < kLdsBpPos) return lbp[((pos >> 2) * kBlock + tid) * 4 + (pos & 3)];
    return __builtin_amdgcn_raw_buffer_load_b8(bp_rsrc, lrel + pos, 0, 0);
  };

  // Near-tie entries (shared by both passes and the backtrace).
  constexpr int kAmb = kByte ? 2 : kAmbEntries;
  uint32_t ae[kAmb], aB2[kAmb];
  uint32_t aN2[kWide ? kAmb : 1];  // kWide: the second setter's trie unit
  float aT[kAmb], aT2[kAmb];
#pragma unroll
  for (int k = 0; k < kAmb; ++k) {
    ae[k] = kNone;
    aB2[k] = 0;
    aT[k] = 0.f;
    aT2[k] = 0.f;
    if constexpr (kWide) aN2[k] = kNone;
  }
  std::conditional_t<kByte, uint32_t, uint64_t> ambm = 0;  // bit d: ring slot d has an entry
  bool bad = false, any_amb = false;
  uint32_t e_nodes = 0;  // kE: lattice nodes (trie + UNK)
  float e_z = 0.f;       // kE: alpha of EOS
  const float tie_mag = a.p.tie_mag;
  // Maintain the near-tie entry of end position `end` (ring slot d) when a
  // setter replaces (t_old, b_old) by bt (nr: the two are near).
  auto amb_update = [&](auto dc, float bt, bool nr, uint32_t end, float t_old, uint32_t b_old,
                        uint32_t n_old = kNone) {
    constexpr int d = decltype(dc)::value;
    int slot = -1, free_slot = -1;
#pragma unroll
    for (int k = 0; k < kAmb; ++k) {
      if (ae[k] == end) slot = k;
      if (ae[k] == kNone && free_slot < 0) free_slot = k;
    }
    if (slot >= 0) {
#pragma unroll
      for (int k = 0; k < kAmb; ++k)
        if (k == slot) {
          if (NearTie(aT2[k], bt, tie_mag)) bad = true;  // 3-deep tie chain
          if (nr) {
            aT2[k] = t_old;
            aB2[k] = b_old;
            if constexpr (kWide) aN2[k] = n_old;
            aT[k] = bt;
          } else {
            ae[k] = kNone;
            ambm &= ~(static_cast<decltype(ambm)>(1) << d);
          }
        }
    } else if (nr) {
      if (free_slot < 0) bad = true;
      any_amb = true;
      ambm |= static_cast<decltype(ambm)>(1) << d;
#pragma unroll
      for (int k = 0; k < kAmb; ++k)
        if (k == free_slot) {
          ae[k] = end;
          aT2[k] = t_old;
          aB2[k] = b_old;
          if constexpr (kWide) aN2[k] = n_old;
          aT[k] = bt;
        }
    }
  };

  if constexpr (kByte) {
    // ---- Byte-position pass (units = (unit, score) pairs: the 0xFF-padded
    // image and the usable-node score or NaN per unit).  p is a char start iff the
    // lead-byte chain from 0 reaches it (OneCharLen clamped to the sentence,
    // unigram_model.cc:155-160 / util.h:389), so malformed UTF-8 needs no
    // special case.  Pieces split exactly into chars (checked at load), hence
    // a leaf reached from a char start ends at a char start.  Positions are
    // processed kU at a time against a ring T[k] = best score ending at
    // p0 + k (k < kR), shifted by kU per group.
    constexpr int kU = 4;
    constexpr int kR = W + kU - 1;      // 19 ring slots
    constexpr int kWin = (kR + 3) / 4;  // 5 window words (bytes p0 .. p0 + 19)
    constexpr int kBw = (W + 6) / 4;    // packed back-pointer words (4 slots each)
    constexpr int kNI = 2;              // positions walked together
    // (unit, node score) pairs: a.units is the interleaved table here.
    const auto uvs_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(a.units), 0,
                                                            static_cast<int>(a.num_units * 8u), 0x00020000);
    using UvT = decltype(__builtin_amdgcn_raw_buffer_load_b64(uvs_rsrc, 0u, 0, 0));
    float T[kR];
#pragma unroll
    for (int d = 0; d < kR; ++d) T[d] = d == 0 ? 0.f : -__builtin_inff();  // slot 0: BOS
    // kE: alpha ring.  A slot starts at -inf, so its first LogSumExp returns
    // the node's value exactly as the reference's init_mode does.
    float Ar[kE ? kR : 1];
#pragma unroll
    for (int d = 0; d < (kE ? kR : 1); ++d) Ar[d] = d == 0 ? 0.f : -__builtin_inff();
    // Slot k's back-pointer: distance end - begin (<= W - 1, invariant under
    // the ring shift) as a byte, four slots per register.
    uint32_t Bw[kBw];
#pragma unroll
    for (int m = 0; m < kBw; ++m) Bw[m] = 0;
    auto b_dist = [&](auto kc) -> uint32_t {
      constexpr int k = decltype(kc)::value;
      return (Bw[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    };
    // Offsets past the tile's buffer range (a > 2 GB tile) would read 0:
    // such a sentence takes the general kernel.
    // The output stage's token descriptors hold a tile-relative offset of 28
    // bits (kStage): a tile that spans more goes the same way.
    bad = valid && (b0 - blk_al) + nb >
                       (kStage && blk_nrec > 0x0FFFFFFF ? 0x0FFFFFFFull : static_cast<uint64_t>(blk_nrec));
    // Window: aligned dwords of the lane's bytes, spliced by alignbyte.
    const uint32_t sh = lrel & 3u;
    const uint32_t lane_al = lrel & ~3u;
    auto word_at = [&](uint32_t m) -> uint32_t {
      const uint32_t o = lane_al + 4u * m;
      if (o + 4 <= blk_rem) return __builtin_amdgcn_raw_buffer_load_b32(bytes_rsrc, o, 0, 0);
      // The batch's last, partial dword: byte loads (a dword load that
      // straddles num_records would read as 0).
      uint32_t x = 0;
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t)
        if (o + t < blk_rem) x |= static_cast<uint32_t>(a.bytes[blk_al + o + t]) << (8 * t);
      return x;
    };
    // Bytes q .. q+3 with zeros beyond nb; a 0xFF byte (the padded trie image
    // matches 0xFF on empty units) flags the sentence.
    auto finish = [&](uint32_t x, uint32_t q) -> uint32_t {
      if (q + 4 > nb) x &= q >= nb ? 0u : (1u << (8 * (nb - q))) - 1u;
      const uint32_t y = ~x;
      if (((y - 0x01010101u) & ~y & 0x80808080u) != 0) bad = true;
      return x;
    };
    uint32_t wprev = nb > 0 ? word_at(0) : 0u;
    uint32_t rw[kWin];
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const uint32_t q = 4 * k;
      const uint32_t wn = q < nb ? word_at(k + 1) : 0u;
      rw[k] = q < nb ? finish(__builtin_amdgcn_alignbyte(wn, wprev, sh), q) : 0u;
      wprev = wn;
    }
    auto byte_of = [&](auto tc) -> uint32_t {
      constexpr int t = decltype(tc)::value;
      return (rw[t >> 2] >> (8 * (t & 3))) & 0xFFu;
    };
    // The hot path keeps its per-lane predicates as wave masks in scalar
    // registers: a ballot of a compare is the compare itself, masks combine
    // on the scalar unit, and a select takes the mask as it is.  (A ballot of
    // a bool built from two conditions costs a 0/1 select and a second
    // compare on the vector unit, the bound of this kernel.)
    using Mask = uint64_t;
    auto lanes_of = [](Mask m) -> bool { return __builtin_amdgcn_inverse_ballot_w64(m); };
    bool amb_wave = false;  // wave-uniform: some lane has an open near-tie entry (ambm != 0)
    // Node [p, p + d) of position j with score sc (NaN: no usable node) into
    // slot j + d.  Nodes reach a slot in ascending begin order.  sc is NaN at
    // a position that is no char start, and holds a one-byte char's UNK node
    // already (the root table); ucl = the char's length where it has two or
    // more bytes (or is a stray tail byte), 0 elsewhere, unk_any = some lane
    // of the wave has ucl != 0.
    auto insert_one = [&](auto jc, auto dc, uint32_t p, float T0, float tie_bound, float A0, uint32_t ucl,
                          bool unk_any, float sc, int dmax) {
      constexpr int j = decltype(jc)::value;
      constexpr int d = decltype(dc)::value;
      if (d > 1 && d > dmax && !(d <= 4 && unk_any)) return;
      float s_node = sc;
      // UNK node (unigram_model.cc:597-601): no usable single-char node.
      if constexpr (d <= 4) {
        if (unk_any) s_node = (d == static_cast<int>(ucl) && __builtin_isnan(s_node)) ? a.p.unk_score : s_node;
      }
      const float bt = __fadd_rn(T0, s_node);
      constexpr int k = j + d;
      if constexpr (kE) {
        if (!__builtin_isnan(s_node)) {
          Ar[k] = LogSumExpDev(Ar[k], __fadd_rn(s_node, A0), false);
          ++e_nodes;
        }
      }
      // A slot's first setter of depth W - 1 finds the -inf the ring shift
      // put there, a constant to the compiler, which folds bt > -inf to an
      // ordered "!=" and then selects the UNORDERED compare for its ballot
      // (v_cmp_neq: true for a NaN bt, which then stays in the slot for good).
      // The slot's value is made opaque there, so the compare stays ">".
      float tk = T[k];
      if constexpr (d == W - 1) __asm__ volatile("" : "+v"(tk));
      const Mask gtm = __builtin_amdgcn_ballot_w64(bt > tk);  // false for NaN
      const Mask nearm = gtm & __builtin_amdgcn_ballot_w64(NearTieAt(tk, bt, tie_bound));
      if (nearm != 0 || amb_wave) {
        const bool nr = lanes_of(nearm);
        if (nr || (lanes_of(gtm) && ((ambm >> k) & 1)))
          amb_update(std::integral_constant<int, k>{}, bt, nr, p + d, T[k],
                     p + d - b_dist(std::integral_constant<int, k>{}));
        amb_wave = __builtin_amdgcn_ballot_w64(ambm != 0) != 0;
      }
      T[k] = lanes_of(gtm) ? bt : T[k];
      SetByteIf<k & 3, d>(Bw[k >> 2], gtm);
    };
    // The merged deep phase's insert at walk step e of the pair at jb = k + 1
    // - e (slot k, end position `end`): a lane carries one chain there, chain
    // 1 (begin jb + 1, node length e - 2) in the lanes of sm and chain 0
    // (begin jb, length e - 1) in the others; sc is the lane's own node score
    // and T0 / tie_bound its own position's.  No UNK select: e - 2 > 4.
    auto insert_m = [&](auto kc, auto ec, uint32_t end, Mask sm, float T0, float tie_bound, float sc) {
      constexpr int k = decltype(kc)::value;
      constexpr int e = decltype(ec)::value;
      static_assert(e - 2 > 4 && e - 2 < W && k < kR, "a deep node of the pair");
      const float bt = __fadd_rn(T0, sc);
      float tk = T[k];
      if constexpr (e >= W) __asm__ volatile("" : "+v"(tk));  // as insert_one's depth W - 1
      const Mask gtm = __builtin_amdgcn_ballot_w64(bt > tk);  // false for NaN
      const Mask nearm = gtm & __builtin_amdgcn_ballot_w64(NearTieAt(tk, bt, tie_bound));
      if (nearm != 0 || amb_wave) {
        const bool nr = lanes_of(nearm);
        if (nr || (lanes_of(gtm) && ((ambm >> k) & 1)))
          amb_update(std::integral_constant<int, k>{}, bt, nr, end, T[k], end - b_dist(std::integral_constant<int, k>{}));
        amb_wave = __builtin_amdgcn_ballot_w64(ambm != 0) != 0;
      }
      T[k] = lanes_of(gtm) ? bt : T[k];
      if constexpr (e - 1 < W) SetByteIf<k & 3, e - 1>(Bw[k >> 2], gtm & ~sm);
      SetByteIf<k & 3, e - 2>(Bw[k >> 2], gtm & sm);
    };
    // Walk steps 1 .. kMergeDepth test and gather both chains of a pair; past
    // them a lane carries one chain (see the merged deep phase below).  Chain
    // 1's node of length 4, the last with an UNK select, is inserted in every
    // lane at step 6, so the merged inserts start at step 7 at the earliest.
    // (Depth 4 with step 6 kept two-chain measured the same as 5, depth 6
    // 1.4 % slower: profiles/pr12_c2_merged_walk_ab.txt.)
    constexpr int kMergeDepth = 5;
    constexpr bool kMerge = !kE;  // the E-step mode keeps its two-chain deep steps
    static_assert(kMergeDepth >= 5 && kMergeDepth + 2 < W, "merged inserts hold no node of length <= 4");
    uint32_t next_start = 0;
    for (uint32_t p0 = 0; p0 <= nb; p0 += kU) {
      StaticFor<0, kU / kNI>([&](auto pc) {
        constexpr int jb = kNI * decltype(pc)::value;
        uint32_t pp[kNI], cl[kNI];
        uint32_t ucl = 0;  // byte q: position q's char length where its UNK node is not in the root table
        bool at[kNI], st[kNI], any[kNI], unk_any[kNI];
        // Char starts in order (next_start chains through the group).
        StaticFor<0, kNI>([&](auto qc) {
          constexpr int q = decltype(qc)::value, j = jb + q;
          pp[q] = p0 + j;
          at[q] = pp[q] <= nb && pp[q] == next_start;
          if (q == 0 && at[q] && pp[q] > 0) bp_store(pp[q], b_dist(std::integral_constant<int, j>{}));
          st[q] = at[q] && pp[q] < nb;
          any[q] = (__builtin_amdgcn_ballot_w64(pp[q] == next_start) & __builtin_amdgcn_ballot_w64(pp[q] < nb)) != 0;
          cl[q] = OneCharLenDev(byte_of(std::integral_constant<int, j>{}));
          if (cl[q] > nb - pp[q]) cl[q] = nb - pp[q];
          if constexpr (kE) {
            // The backward pass finds char starts as non-continuation bytes:
            // a char start must not be one, its tail bytes must all be.
            if (st[q]) {
              const uint32_t lead = byte_of(std::integral_constant<int, j>{});
              bool ok = (lead & 0xC0u) != 0x80u;
              StaticFor<1, 4>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                if (static_cast<uint32_t>(t) < cl[q] && (byte_of(std::integral_constant<int, j + t>{}) & 0xC0u) != 0x80u)
                  ok = false;
              });
              if (!ok) bad = true;
            }
          }
          if (st[q]) next_start = pp[q] + cl[q];
          // The UNK node of a one-byte char is in the root table; the others
          // (a multi-byte char, a stray tail byte) keep their select in the
          // inserts of depth <= 4, skipped when no lane of the wave has one.
          const uint32_t uq = st[q] && byte_of(std::integral_constant<int, j>{}) >= 0x80u ? cl[q] : 0u;
          ucl |= uq << (8 * q);
          unk_any[q] = __builtin_amdgcn_ballot_w64(uq != 0) != 0;
        });
        // Lagged inserts: position q's node of length dd is inserted at walk
        // step d = dd + 1 + q, right after the loads of step d are issued.
        // Its score load (issued at step dd) has landed by then, so each
        // score register lives about one step.  Every insert into slot
        // jb + d - 1 happens at step d in ascending q = ascending begin, as
        // end_nodes_ order requires; position q's own T0 and back-pointer
        // (slot jb + q, final after step q + 1) are read at step q + 2,
        // before its first insert.
        float sok[kNI][W];  // node score of depth d (NaN: no usable node)
        float T0q[kNI], Tbq[kNI];  // the position's own best score and its near-tie bound
        float A0q[kNI];
        int dm[kNI];
        uint32_t off[kNI], c[kNI];  // off: byte offset of the walk's next (unit, score) pair
        UvT uv[kNI];
        StaticFor<0, kNI>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          dm[q] = 0;
          T0q[q] = 0.f;
          Tbq[q] = 0.f;
        });
        bool go = any[0] || any[1];
        if (go) {
          StaticFor<0, kNI>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            c[q] = byte_of(std::integral_constant<int, jb + q>{});
            // The root's child from LDS; entry 256 where no char starts.
            const uint2 r = lds_root[st[q] ? c[q] : static_cast<uint32_t>(kBlock)];
            uv[q][0] = r.x;
            uv[q][1] = r.y;
          });
        }
        // Software pipeline: step d waits for the (unit, score) loads of
        // depth d, issues those of depth d + 1, and only then runs the lagged
        // inserts, so their VALU work overlaps the loads in flight.  One
        // 8-byte gather per walk step and lane carries both the unit and its
        // node score: the walk is bound by the vector-memory address path
        // (TA busy 84 % of the kernel with separate unit and score gathers,
        // profiles/r03g_ta_unigram_fast.txt), so a step costs one gather.
        // A lane whose walk has ended gathers pair 0, the root's own unit:
        // its label is 0xFF (as every empty unit's), which no byte of an
        // unflagged sentence matches, so the lane stays out without a flag
        // of its own, and "alive" is one compare per step.
        // Merged deep phase state (kMerge): the lanes that carry chain 1, the
        // lanes whose two chains are both alive at kMergeDepth (chain 1 of
        // those runs in a second pass, from its saved unit and score), the
        // lane's own T0 / tie bound, its byte selector (v_perm: byte t of the
        // window for chain 0, t + 1 for chain 1), the pending gather and the
        // label it will be tested against.
        Mask selm = 0, bothm = 0;
        bool mgo = false;
        uint32_t uB = 0, psel = 0, cm = 0;
        float sB = 0.f, sD = 0.f, T0m = 0.f, Tbm = 0.f;
        UvT muv;
        auto mbyte = [&](auto tc) -> uint32_t {
          constexpr int t = decltype(tc)::value;
          uint32_t hi = 0u;
          if constexpr ((t >> 2) + 1 < kWin) hi = rw[(t >> 2) + 1];
          return __builtin_amdgcn_perm(hi, rw[t >> 2], psel + static_cast<uint32_t>(t & 3));
        };
        // Enters a pass of the merged phase: lanes of `sm` carry chain 1, the
        // others chain 0; `alive` lanes continue from `unit` (alive at depth
        // kMergeDepth), the others gather pair 0 from here on.
        auto merged_enter = [&](Mask sm, Mask alive, uint32_t unit, float s_d) {
          selm = sm;
          const bool sl = lanes_of(sm);
          T0m = sl ? T0q[1] : T0q[0];
          Tbm = sl ? Tbq[1] : Tbq[0];
          psel = sl ? 0x0C0C0C01u : 0x0C0C0C00u;
          sD = s_d;
          cm = mbyte(std::integral_constant<int, jb + kMergeDepth>{});
          uint32_t o = lanes_of(alive) ? ((unit >> 9) ^ cm) << 3 : 0u;
          __asm__ volatile("" : "+v"(o));
          muv = __builtin_amdgcn_raw_buffer_load_b64(uvs_rsrc, o, 0, 0);
        };
        StaticFor<1, kMerge ? kMergeDepth + 2 : W + kNI>([&](auto dc) {
          constexpr int d = decltype(dc)::value;
          if constexpr (d < W && (!kMerge || d <= kMergeDepth)) {
            StaticFor<0, kNI>([&](auto qc) { sok[decltype(qc)::value][d] = __builtin_nanf(""); });
            if (go) {
              Mask alm[kNI];
              StaticFor<0, kNI>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                alm[q] = __builtin_amdgcn_ballot_w64((uv[q][0] & 0xFFu) == c[q]);
                // (Depth 1: the root table's score is masked already.)
                sok[q][d] = (d == 1 || lanes_of(alm[q])) ? __uint_as_float(uv[q][1]) : __builtin_nanf("");
                if (alm[q] != 0) dm[q] = d;
              });
              go = (alm[0] | alm[1]) != 0;
              if constexpr (kMerge && d == kMergeDepth) {
                // One gather per lane from here on: chain 1 where it alone
                // is alive, else chain 0.
                if (go) {
                  mgo = true;
                  bothm = alm[0] & alm[1];
                  uB = uv[1][0];
                  sB = sok[1][d];
                  const Mask sm = alm[1] & ~alm[0];
                  merged_enter(sm, alm[0] | alm[1], lanes_of(sm) ? uv[1][0] : uv[0][0], sok[1][d]);
                }
              } else if constexpr (d + 1 < W) {
                if (go) {
                  StaticFor<0, kNI>([&](auto qc) {
                    constexpr int q = decltype(qc)::value;
                    constexpr int t = jb + q + d;
                    c[q] = byte_of(std::integral_constant<int, t>{});
                    // 8 * (base ^ byte): byte t of the window at bits 3..10
                    // (what lies below is masked off with the unit's flags).
                    uint32_t c8;
                    if constexpr ((t & 3) != 0) c8 = (rw[t >> 2] >> (8 * (t & 3) - 3)) & 0x7FFu;
                    else c8 = (rw[t >> 2] & 0xFFu) << 3;
                    off[q] = lanes_of(alm[q]) ? ((uv[q][0] >> 6) ^ c8) & ~7u : 0u;
                    // The score is taken before the pair's registers are
                    // loaded again (left to itself the compiler takes it
                    // after, loads into a second register pair, and copies
                    // that one back behind a wait ahead of the inserts).
                    __asm__ volatile("" : "+v"(sok[q][d]), "+v"(off[q]));
                    uv[q] = __builtin_amdgcn_raw_buffer_load_b64(uvs_rsrc, off[q], 0, 0);
                  });
                }
              }
            }
          }
          StaticFor<0, kNI>([&](auto qc) {
            constexpr int q = decltype(qc)::value, j = jb + q, dd = d - 1 - q;
            if constexpr (dd == 1) {
              if (q > 0 && at[q] && pp[q] > 0) bp_store(pp[q], b_dist(std::integral_constant<int, j>{}));
              T0q[q] = T[j];
              Tbq[q] = TieBound(T0q[q], tie_mag);
              if constexpr (kE) {
                // Slot j is final here: alpha of this char start (or Z at EOS).
                A0q[q] = Ar[j];
                if (st[q]) {
                  if (a.e.AT && pp[q] < kATRows)
                    a.e.AT[(tile * kATRows + pp[q]) * kBlock + tid] = Ar[j];
                  else
                    a.e.A[b0 + pp[q]] = Ar[j];
                }
                if (at[q] && pp[q] == nb) e_z = Ar[j];
              }
            }
            if constexpr (dd >= 1 && dd < W) {
              if (any[q])
                insert_one(std::integral_constant<int, j>{}, std::integral_constant<int, dd>{}, pp[q], T0q[q],
                           Tbq[q], kE ? A0q[q] : 0.f, (ucl >> (8 * q)) & 0xFFu, unk_any[q], sok[q][dd], dm[q]);
            }
          });
        });
        // ---- Merged deep phase.  Past depth kMergeDepth a lane rarely has
        // both chains of its pair alive (a deep walk starts at a "▁"), so
        // step e > kMergeDepth tests one label, issues one gather and runs
        // one insert into slot jb + e - 1: chain 0's node of length e - 1 or
        // chain 1's of length e - 2, whichever chain the lane carries.  The
        // lanes with two deep chains carry chain 0 in pass A and chain 1 in
        // pass B, the same unrolled body run once more.  Ring slots are only
        // written here (a position's own slot is read at step q + 2), and a
        // slot still gets one lane's chain 0 node before its chain 1 node:
        // with one deep chain the other insert was a NaN no-op, with two,
        // pass A is complete before pass B starts.  Every slot sees the same
        // setters in the same order as in the two-chain walk.  (The two
        // near-tie entries are shared by all slots: a lane with two deep
        // chains whose entries fill up in pass A before a pass-B setter would
        // have freed one is flagged where the two-chain order was not, and
        // the general kernel then emits the same tokens.)
        if constexpr (kMerge) {
          if (mgo) {
#pragma clang loop unroll(disable)
            for (int pass = 0;; ++pass) {
              float S[W];  // the carried chain's node score of depth e (NaN: no usable node)
              S[kMergeDepth] = sD;
              int mdm = kMergeDepth;
              bool g = true;
              StaticFor<kMergeDepth + 1, W + kNI>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                if constexpr (e < W) {
                  S[e] = __builtin_nanf("");
                  if (g) {
                    const Mask al = __builtin_amdgcn_ballot_w64((muv[0] & 0xFFu) == cm);
                    S[e] = lanes_of(al) ? __uint_as_float(muv[1]) : __builtin_nanf("");
                    if (al != 0) mdm = e;
                    g = al != 0;
                    if constexpr (e + 1 < W) {
                      if (g) {
                        cm = mbyte(std::integral_constant<int, jb + e>{});
                        uint32_t o = lanes_of(al) ? ((muv[0] >> 9) ^ cm) << 3 : 0u;
                        __asm__ volatile("" : "+v"(S[e]), "+v"(o));
                        muv = __builtin_amdgcn_raw_buffer_load_b64(uvs_rsrc, o, 0, 0);
                      }
                    }
                  }
                }
                if constexpr (e >= kMergeDepth + 2) {
                  if (e - 2 <= mdm) {
                    float sc;
                    if constexpr (e - 1 < W) sc = lanes_of(selm) ? S[e - 2] : S[e - 1];
                    else sc = lanes_of(selm) ? S[e - 2] : __builtin_nanf("");
                    // No lane has a usable node here (three merged inserts in ten on c2): one compare.
                    if (__builtin_amdgcn_ballot_w64(sc == sc) != 0)
                      insert_m(std::integral_constant<int, jb + e - 1>{}, ec, pp[0] + static_cast<uint32_t>(e - 1), selm,
                               T0m, Tbm, sc);
                  }
                }
              });
              if (pass != 0 || bothm == 0) break;
              // Pass B: chain 1 of the lanes with two deep chains, every
              // other lane dead from the start.
              merged_enter(~static_cast<Mask>(0), bothm, uB, lanes_of(bothm) ? sB : __builtin_nanf(""));
            }
          }
        }
      });
      // Next group: shift the ring and the byte window by kU.
#pragma unroll
      for (int k = 0; k < kR; ++k) T[k] = k + kU < kR ? T[k + kU] : -__builtin_inff();
      if constexpr (kE) {
#pragma unroll
        for (int k = 0; k < kR; ++k) Ar[k] = k + kU < kR ? Ar[k + kU] : -__builtin_inff();
      }
#pragma unroll
      for (int m = 0; m < kBw; ++m) Bw[m] = m + 1 < kBw ? Bw[m + 1] : 0u;
      ambm >>= kU;
      if (amb_wave) amb_wave = __builtin_amdgcn_ballot_w64(ambm != 0) != 0;
#pragma unroll
      for (int k = 0; k + 1 < kWin; ++k) rw[k] = rw[k + 1];
      const uint32_t qn = p0 + kU + 4 * (kWin - 1);
      const uint32_t wn = qn < nb ? word_at(qn / 4 + 1) : 0u;
      rw[kWin - 1] = qn < nb ? finish(__builtin_amdgcn_alignbyte(wn, wprev, sh), qn) : 0u;
      wprev = wn;
    }
  } else if constexpr (kWide) {
    // ---- Wide-char pass (models whose pieces are whole chars, < 16 chars,
    // < 64 bytes, some >= 16 bytes: CJK vocabularies).  Ring slot c = the
    // position c CHARS ahead (a 3-byte char costs one slot, not three), so
    // the ring shifts by one slot per char; the walk consumes the sentence
    // from a 32-byte register window (three buffer loads per char position
    // instead of a byte gather per window byte), reads (unit, node score)
    // pairs (the byte kernel's table: one 8-byte gather per trie edge brings
    // the leaf's score), takes the root's children from LDS, inserts each
    // node as soon as its char boundary is reached (ascending length, then
    // UNK: begin_nodes_ order), and each slot keeps the trie unit of its best
    // node, so the backtrace reads the token's id instead of re-walking it.
    constexpr int Wc = W;
    const auto uvs_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(a.units), 0,
                                                            static_cast<int>(a.num_units * 8u), 0x00020000);
    float T[Wc];
    uint32_t B[Wc], Nd[Wc];  // best node's begin byte / trie unit (kNone: UNK) per slot
#pragma unroll
    for (int d = 0; d < Wc; ++d) {
      T[d] = 0.f;
      B[d] = 0;
      Nd[d] = kNone;
    }
    uint32_t has = 1;  // bit c: slot c holds a node
    auto insert = [&](auto dc, float bt, uint32_t begin, uint32_t end, uint32_t node) {
      constexpr int d = decltype(dc)::value;
      if (!((has >> d) & 1)) {
        has |= (1u << d);
        T[d] = bt;
        B[d] = begin;
        Nd[d] = node;
      } else if (bt > T[d]) {
        const bool nr = NearTie(T[d], bt, tie_mag);
        if (nr || ((ambm >> d) & 1)) amb_update(dc, bt, nr, end, T[d], B[d], Nd[d]);
        T[d] = bt;
        B[d] = begin;
        Nd[d] = node;
      }
    };
    // Window: the 32 bytes from byte q of the sentence, zero past its end.
    uint32_t r[8];
    auto load_window = [&](uint32_t q) {
      const uint32_t o = (lrel + q) & ~3u, sh = (lrel + q) & 3u;
      uint32_t w[9];
      if (static_cast<uint64_t>(o) + 36 <= static_cast<uint64_t>(blk_rem)) {
        const auto x0 = __builtin_amdgcn_raw_buffer_load_b128(bytes_rsrc, o, 0, 0);
        const auto x1 = __builtin_amdgcn_raw_buffer_load_b128(bytes_rsrc, o + 16, 0, 0);
        w[0] = x0[0];
        w[1] = x0[1];
        w[2] = x0[2];
        w[3] = x0[3];
        w[4] = x1[0];
        w[5] = x1[1];
        w[6] = x1[2];
        w[7] = x1[3];
        w[8] = __builtin_amdgcn_raw_buffer_load_b32(bytes_rsrc, o + 32, 0, 0);
      } else {  // the batch's last bytes: byte loads (a straddling dword reads 0)
#pragma unroll
        for (uint32_t k = 0; k < 9; ++k) {
          uint32_t x = 0;
#pragma unroll
          for (uint32_t t = 0; t < 4; ++t)
            if (o + 4 * k + t < blk_rem) x |= static_cast<uint32_t>(a.bytes[blk_al + o + 4 * k + t]) << (8 * t);
          w[k] = x;
        }
      }
      const uint32_t left = nb > q ? nb - q : 0u;  // sentence bytes in the window
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        uint32_t x = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
        const uint32_t b = 4u * k;
        if (b + 4 > left) x &= b >= left ? 0u : (1u << (8 * (left - b))) - 1u;
        r[k] = x;
      }
    };
    auto next_byte = [&]() -> uint32_t {  // consume the window's first byte
      const uint32_t c = r[0] & 0xFFu;
#pragma unroll
      for (int k = 0; k < 7; ++k) r[k] = __builtin_amdgcn_alignbyte(r[k + 1], r[k], 1);
      r[7] >>= 8;
      return c;
    };
    // Offsets past the tile's buffer range (a > 2 GB tile) would read 0:
    // such a sentence takes the general kernel.
    bad = valid && (b0 - blk_al) + nb > static_cast<uint64_t>(blk_nrec);
    // Long sentences: the wave-cooperative kernel (flagged without a walk).
    const bool coop = a.coop_min_nb && nb >= a.coop_min_nb;
    if (coop) bad = true;
    uint32_t pos = 0;  // byte offset of the current char position
    while (nb > 0 && !coop) {
      if (pos > 0) {
        bp_store(pos, pos - B[0]);
        a.bpn[b0 + pos] = Nd[0];
      }
      if (pos >= nb) break;
      const float T0 = T[0];
      load_window(pos);
      uint32_t base_u = a.p.root_base;
      uint32_t consumed = 0, woff = 0;  // bytes walked from pos; the window starts at pos + woff
      uint32_t clen0 = 1;
      bool alive = true, single = false;
      // The walk, one char (1-4 trie edges) per step c; a usable leaf at the
      // char boundary is inserted into slot c right away.
      StaticFor<1, Wc>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        if (alive && pos + consumed >= nb) alive = false;
        // Refill the window when the next char may not be in it (walks past
        // 28 bytes: pieces of 10+ CJK chars).
        const bool refill = alive && consumed - woff + 4 > 32;
        if (__builtin_amdgcn_ballot_w64(refill) != 0) {
          if (refill) {
            load_window(pos + consumed);
            woff = consumed;
          }
        }
        if (alive) {
          uint32_t L = OneCharLenDev(r[0] & 0xFFu);
          if (L > nb - pos - consumed) L = nb - pos - consumed;
          if (c == 1) clen0 = L;
          uint32_t u = 0, scb = 0, node = 0;
          for (uint32_t t = 0; t < L; ++t) {
            const uint32_t byte = next_byte();
            // 0xFF matches the padded image's empty units: general path.
            if (byte == 0xFFu) bad = true;
            node = base_u ^ byte;
            if (c == 1 && t == 0) {
              const uint2 x = lds_root[byte];
              u = x.x;
              scb = x.y;
            } else {
              const auto x = __builtin_amdgcn_raw_buffer_load_b64(uvs_rsrc, node * 8u, 0, 0);
              u = x[0];
              scb = x[1];
            }
            if ((u & 0xFFu) != byte) {
              alive = false;
              break;
            }
            base_u = u >> 9;
            if ((u & 0x100u) && t + 1 < L) bad = true;  // a leaf inside a UTF-8 char: general path
          }
          if (alive) {
            consumed += L;
            // A usable node (leaf, not UNUSED) is one with a non-NaN score.
            const float s_node = __uint_as_float(scb);
            if ((u & 0x100u) && !__builtin_isnan(s_node)) {
              insert(cc, __fadd_rn(T0, s_node), pos, pos + consumed, node);
              if (c == 1) single = true;
            }
          }
        }
        // UNK node (unigram_model.cc:597-601) after this position's trie nodes.
        if constexpr (c == Wc - 1) {
          if (!single) insert(std::integral_constant<int, 1>{}, __fadd_rn(T0, a.p.unk_score), pos, pos + clen0, kNone);
        }
      });
      // Advance one char: shift the ring by one slot.
#pragma unroll
      for (int d = 0; d + 1 < Wc; ++d) {
        T[d] = T[d + 1];
        B[d] = B[d + 1];
        Nd[d] = Nd[d + 1];
      }
      T[Wc - 1] = 0.f;
      B[Wc - 1] = 0;
      Nd[Wc - 1] = kNone;
      has >>= 1;
      ambm >>= 1;
      pos += clen0;
    }
  } else {
    // ---- Char-position pass: ring slot d = end position (current byte + d);
    // slot 0 of the first position is BOS (score 0, backtrace 0: FreeList
    // zero-fill, freelist.h:79).
    float T[W];
    uint32_t B[W];
#pragma unroll
    for (int d = 0; d < W; ++d) {
      T[d] = 0.f;
      B[d] = 0;
    }
    uint64_t has = 1;  // bit d: slot d holds a node
    // Long sentences: the wave-cooperative kernel (flagged without a walk).
    const bool coop = a.coop_min_nb && nb >= a.coop_min_nb;
    if (coop) bad = true;
    auto insert = [&](auto dc, float bt, uint32_t begin, uint32_t end) {
      constexpr int d = decltype(dc)::value;
      if (!((has >> d) & 1)) {
        has |= (1ull << d);
        T[d] = bt;
        B[d] = begin;
      } else if (bt > T[d]) {
        const bool nr = NearTie(T[d], bt, tie_mag);
        if (nr || ((ambm >> d) & 1)) amb_update(dc, bt, nr, end, T[d], B[d]);
        T[d] = bt;
        B[d] = begin;
      }
    };
    uint32_t pos = 0;  // byte offset of the current char position
    while (nb > 0 && !coop) {
      if (pos > 0) bp_store(pos, pos - B[0]);
      if (pos >= nb) break;
      const float T0 = T[0];
      // Bytes pos .. pos+W-1 (packed, little endian), zero past the batch.
      uint32_t win[W / 4];
#pragma unroll
      for (int k = 0; k < W / 4; ++k) {
        uint32_t x = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const uint64_t g = b0 + pos + 4 * k + t;
          x |= (g < total_bytes ? static_cast<uint32_t>(a.bytes[g]) : 0u) << (8 * t);
        }
        win[k] = x;
      }
      uint32_t base_u = a.p.root_base;
      uint32_t rem = 0;        // bytes left in the current char (0: next byte starts one)
      uint32_t clen0 = 1;      // byte length of the first char
      uint64_t cbmask = 0;     // bit d: a char ends after byte d
      uint64_t leafmask = 0;   // bit d: a piece ends at a char boundary after byte d
      uint32_t lnode[W];
      bool alive = true, single = false;
      // Phase 1: the walk, one trie edge (one byte) per step; d = byte distance.
      StaticFor<1, W>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        const uint32_t c = (win[(d - 1) >> 2] >> (8 * ((d - 1) & 3))) & 0xFFu;
        if (alive) {
          const uint32_t q = pos + d - 1;
          if (q >= nb) {
            alive = false;
          } else {
            if (rem == 0) {
              rem = OneCharLenDev(c);
              if (rem > nb - q) rem = nb - q;
              if (d == 1) clen0 = rem;
            }
            const uint32_t node = base_u ^ c;
            const uint32_t u = c ? a.units[node] : 0u;
            if ((u & 0xFFu) != c || c == 0) {
              alive = false;
            } else {
              base_u = u >> 9;
              --rem;
              if (rem == 0) cbmask |= 1ull << d;
              if (u & 0x100u) {
                if (rem != 0) {
                  bad = true;  // leaf inside a UTF-8 char: general path
                } else {
                  leafmask |= 1ull << d;
                  lnode[d] = node;
                }
              }
            }
          }
        }
      });
      // Phase 2: all leaf scores (independent loads), written over lnode[]:
      // a score, or a NaN tag 0x7FC00000|kind for USER_DEFINED / UNUSED.
      StaticFor<1, W>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        if ((leafmask >> d) & 1) {
          const int32_t v = a.values[lnode[d]];
          const int32_t k = v >> kKindShift;
          lnode[d] = k == 0 ? __float_as_uint(a.scores[v & kIdMask]) : (0x7FC00000u | k);
        }
      });
      // Phase 3: nodes in ascending length, then UNK (begin_nodes_ order).
      StaticFor<1, W>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        if ((leafmask >> d) & 1) {
          const uint32_t sb = lnode[d];
          const int32_t kind = (sb & 0x7FFFFFFFu) > 0x7F800000u ? static_cast<int32_t>(sb & 3u) : 0;
          if (kind != kKindUnused) {
            const float s_node = kind == kKindUserDefined
                                     ? UserDefinedScore(__popcll(cbmask & ((2ull << d) - 1)), a.p.max_score)
                                     : __uint_as_float(sb);
            insert(dc, __fadd_rn(T0, s_node), pos, pos + d);
            if (d == static_cast<int>(clen0)) single = true;
          }
        }
        // UNK node (unigram_model.cc:597-601) at the end of the first char.
        if constexpr (d <= 4) {
          if (d == static_cast<int>(clen0) && !single) insert(dc, __fadd_rn(T0, a.p.unk_score), pos, pos + clen0);
        }
      });
      // Advance one char (clen0 bytes): shift the ring.
      for (uint32_t t = 0; t < clen0; ++t) {
#pragma unroll
        for (int d = 0; d + 1 < W; ++d) {
          T[d] = T[d + 1];
          B[d] = B[d + 1];
        }
        T[W - 1] = 0.f;
        B[W - 1] = 0;
        has >>= 1;
        ambm >>= 1;
      }
      pos += clen0;
    }
  }

  // The lane's sentence index again, re-read from the permutation in LDS:
  // keeping the 64-bit index live across the walk cost a scratch spill.
  // (So would the slot's LDS address: it is formed again from a thread index
  // the compiler cannot match with the first one.)
  __asm__ volatile("" ::: "memory");
  int tid_e = tid;
  if constexpr (kByte) __asm__ volatile("" : "+v"(tid_e));
  const uint32_t sid_e = lds_sort[kBlock + tid_e];
  const uint64_t ie = base + sid_e;
  const bool valid_e = ie < a.n;
  // Debug knob (spm_hip_model_set_debug_corrupt_bp): zero one sentence's EOS
  // back-pointer after the forward pass, as a corrupted scratch byte would.
  if (a.corrupt_bp != ~0ull && valid_e && ie == a.corrupt_bp && nb > 0) bp_store(nb, 0);

  // Byte kernel: the token of `len` bytes at tile-relative offset `ro` (from
  // blk_al), by its bytes alone: the near-tie resolution of the counting
  // backtrace and the tile-balanced lookup of the output stage share it.
  auto token_of = [&](uint32_t ro, uint32_t len, int32_t *id_out, float *sc_out) {
    if constexpr (kByte) {
      // The token's bytes (< 16) from one aligned 16-byte load + one dword
      // instead of a byte gather per byte, walked through (unit, score) pairs:
      // the node score comes with the last unit, so only the id is one more
      // gather (the kernel is bound by its gathers' address work).
      const uint32_t o = ro & ~3u, sh = ro & 3u;
      uint32_t w[5];
      if (static_cast<uint64_t>(o) + 20 <= blk_rem) {
        const auto x = __builtin_amdgcn_raw_buffer_load_b128(bytes_rsrc, o, 0, 0);
        w[0] = x[0];
        w[1] = x[1];
        w[2] = x[2];
        w[3] = x[3];
        w[4] = __builtin_amdgcn_raw_buffer_load_b32(bytes_rsrc, o + 16, 0, 0);
      } else {  // the batch's last bytes: byte loads (a straddling dword reads 0)
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) {
          uint32_t x = 0;
#pragma unroll
          for (uint32_t t = 0; t < 4; ++t)
            if (o + 4 * k + t < blk_rem) x |= static_cast<uint32_t>(a.bytes[blk_al + o + 4 * k + t]) << (8 * t);
          w[k] = x;
        }
      }
      uint32_t r0 = __builtin_amdgcn_alignbyte(w[1], w[0], sh), r1 = __builtin_amdgcn_alignbyte(w[2], w[1], sh);
      uint32_t r2 = __builtin_amdgcn_alignbyte(w[3], w[2], sh), r3 = __builtin_amdgcn_alignbyte(w[4], w[3], sh);
      if constexpr (!kE) {
        if (a.piece_tab) {
          // The forward pass already stood on this token's node: instead of
          // walking its bytes from the root again (one dependent gather per
          // byte, in wave lockstep the longest token of 64 lanes), look the
          // bytes up in the piece table.  The key is the token's bytes
          // zero-padded, the length in the last byte; the table holds exactly
          // the usable trie nodes, so a miss is what the walk calls UNK (an
          // inner or UNUSED node, no node, a NUL inside the token).
          const int n = static_cast<int>(len);
          auto keep = [](uint32_t r, int nb) { return nb >= 4 ? r : nb <= 0 ? 0u : r & ~(~0u << (8 * nb)); };
          const uint32_t k0 = keep(r0, n), k1 = keep(r1, n - 4), k2 = keep(r2, n - 8);
          const uint32_t k3 = (keep(r3, n - 12) & 0x00FFFFFFu) | (len << 24);
          // (mask and seed come as kernel arguments: read from the table's
          // header they are vector loads behind the kernel's stores, and the
          // resource built from them is no longer wave-uniform.)
          const uint32_t tmask = a.piece_mask, tseed = a.piece_seed;
          const auto tab_rsrc = __builtin_amdgcn_make_buffer_rsrc(
              const_cast<uint32_t *>(a.piece_tab), 0, static_cast<int>((tmask + 2u) * 32u), 0x00020000);
          uint32_t p0, p1;
          PieceHash(k0, k1, k2, k3, tseed, tmask, &p0, &p1);
          const uint32_t o0 = (p0 + 1u) * 32u, o1 = (p1 + 1u) * 32u;
          const auto ka = __builtin_amdgcn_raw_buffer_load_b128(tab_rsrc, o0, 0, 0);
          const auto va = __builtin_amdgcn_raw_buffer_load_b64(tab_rsrc, o0 + 16u, 0, 0);
          bool hit = ka[0] == k0 && ka[1] == k1 && ka[2] == k2 && ka[3] == k3;
          uint32_t idv = va[0], scv = va[1];
          // The second position only for the lanes that missed the first (the
          // builder puts the frequent pieces first): loaded for every lane it
          // pulled a cold, mostly empty line per token through the L2
          // (TCC_MISS 9.2e6 -> 1.67e7 per launch).
          if (!hit) {
            const auto kb = __builtin_amdgcn_raw_buffer_load_b128(tab_rsrc, o1, 0, 0);
            const auto vb = __builtin_amdgcn_raw_buffer_load_b64(tab_rsrc, o1 + 16u, 0, 0);
            hit = kb[0] == k0 && kb[1] == k1 && kb[2] == k2 && kb[3] == k3;
            idv = vb[0];
            scv = vb[1];
          }
          hit = hit && len - 1u < kPieceKeyBytes;
          *id_out = hit ? static_cast<int32_t>(idv) : a.p.unk_id;
          *sc_out = hit ? __uint_as_float(scv) : a.p.unk_score;
          return;
        }
      }
      const auto uvs_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(a.units), 0,
                                                              static_cast<int>(a.num_units * 8u), 0x00020000);
      uint32_t nbase = a.p.root_base, node = 0, u = 0, scb = 0;
      bool found = true;
      for (uint32_t j = 0; j < len; ++j) {
        const uint32_t c = r0 & 0xFFu;
        r0 = __builtin_amdgcn_alignbyte(r1, r0, 1);
        r1 = __builtin_amdgcn_alignbyte(r2, r1, 1);
        r2 = __builtin_amdgcn_alignbyte(r3, r2, 1);
        r3 >>= 8;
        node = nbase ^ c;
        if (c == 0) {
          found = false;
          break;
        }
        const auto uv = __builtin_amdgcn_raw_buffer_load_b64(uvs_rsrc, node * 8u, 0, 0);
        u = uv[0];
        scb = uv[1];
        if ((u & 0xFFu) != c) {
          found = false;
          break;
        }
        nbase = u >> 9;
      }
      // A usable node (leaf, not UNUSED) is exactly one with a non-NaN score
      // in the pair table (the byte kernel's models have no NaN score).
      const float s_node = __uint_as_float(scb);
      if (found && len > 0 && !__builtin_isnan(s_node)) {
        *id_out = a.values[node] & kIdMask;
        *sc_out = s_node;
      } else {
        *id_out = a.p.unk_id;
        *sc_out = a.p.unk_score;
      }
    }
  };
  // Node (b, e) on the best path: exact-match walk, else UNK.
  uint32_t wide_node = kNone;  // kWide: the trie unit of the token the backtrace is at
  auto node_of = [&](uint32_t b, uint32_t e, int32_t *id_out, float *sc_out) {
    if constexpr (kWide) {
      // The forward pass kept the winner's unit (kNone: the UNK node).
      int32_t id = a.p.unk_id;
      float sc = a.p.unk_score;
      if (wide_node != kNone) {
        const int32_t v = a.values[wide_node];
        const int32_t kind = v >> kKindShift;
        id = v & kIdMask;
        if (kind == kKindUserDefined) {
          int chars = 0;
          for (uint32_t j = b; j < e; j += OneCharLenDev(byte_at(j))) ++chars;
          sc = UserDefinedScore(chars, a.p.max_score);
        } else {
          sc = a.scores[id];
        }
      }
      *id_out = id;
      *sc_out = sc;
      return;
    }
    if constexpr (kByte) {
      token_of(lrel + b, e - b, id_out, sc_out);
      return;
    }
    uint32_t nbase = a.p.root_base, node = 0, u = 0;
    bool found = true;
    for (uint32_t j = b; j < e; ++j) {
      const uint32_t c = byte_at(j);
      node = nbase ^ c;
      u = c ? a.units[node] : 0u;
      if ((u & 0xFFu) != c || c == 0) {
        found = false;
        break;
      }
      nbase = u >> 9;
    }
    int32_t id = a.p.unk_id;
    float sc = a.p.unk_score;
    if (found && (u & 0x100u)) {
      const int32_t v = a.values[node];
      const int32_t kind = v >> kKindShift;
      if (kind != kKindUnused) {
        id = v & kIdMask;
        if (kind == kKindUserDefined) {
          int chars = 0;
          for (uint32_t j = b; j < e; j += OneCharLenDev(byte_at(j))) ++chars;
          sc = UserDefinedScore(chars, a.p.max_score);
        } else {
          sc = a.scores[id];
        }
      }
    }
    *id_out = id;
    *sc_out = sc;
  };
  // Backtrace from EOS (score 0).  write=false only counts tokens (node
  // scores are needed only to resolve recorded near-ties).  Every step must
  // move left (begin < end): a zero or out-of-range back-pointer flags the
  // sentence instead of looping.  (kStage runs only the counting form.)
  auto backtrace = [&](bool write, int32_t *out_id, uint32_t *out_len, uint32_t kt) -> uint32_t {
    uint32_t e = nb, k = 0;
    float rs = 0.f;
    while (e > 0) {
      uint32_t b = e - bp_load(e);
      if constexpr (kWide) wide_node = (write || any_amb) ? a.bpn[b0 + e] : kNone;
      bool second = false;
#pragma unroll
      for (int t = 0; t < kAmb; ++t)
        if (ae[t] == e && __fadd_rn(aT2[t], rs) == __fadd_rn(aT[t], rs)) {
          b = aB2[t];
          second = true;
          if constexpr (kWide) wide_node = aN2[t];
        }
      // kStage: a token is also at most 15 bytes (its length is a descriptor's
      // 4 bits); b >= e wraps e - b - 1 past that.
      if ((kStage ? e - b - 1u >= 15u : b >= e) || k >= nb) {
        bad = true;
        return 0;
      }
      // kStage: the second setter won.  Its distance replaces the first
      // setter's in the back-pointer byte, so the chain this (counting) pass
      // leaves there is the final path and the describe pass follows it blind.
      if constexpr (kStage)
        if (second) bp_store(e, e - b);
      if (write || any_amb) {
        int32_t id;
        float sc;
        node_of(b, e, &id, &sc);
        if (write) {
          out_id[kt - 1 - k] = id;
          if (out_len) out_len[kt - 1 - k] = e - b;
        }
        rs = sc;
      }
      ++k;
      e = b;
    }
    return k;
  };
  uint32_t k = 0;
  if (valid_e && nb > 0 && !bad) k = backtrace(false, nullptr, nullptr, 0);
  if (bad) k = 0;
  if constexpr (kE) {
    // E-step outputs (estep_kernels.hip EArgs: Zlat, N, ntok; a flagged
    // sentence runs estep_general_kernel, which redoes all of it).
    if (valid_e) {
      a.e.Z[ie] = e_z;
      a.e.N[ie] = e_nodes;
      if (bad) {
        a.e.ntok[ie] = kNone;
        const uint32_t fk = atomicAdd(&a.e.fstatus[0], 1u);
        a.e.flagged[fk] = static_cast<uint32_t>(ie);
        atomicMax(&a.e.fstatus[1], nb);
      } else {
        a.e.ntok[ie] = k;
      }
    }
    return;
  }

  // Tile-exclusive scan of the token counts in SENTENCE order (lanes hold
  // the tile's sentences permuted by length), then the tile's global offset.
  lds_scan[sid_e] = k;
  __syncthreads();
  const uint32_t kk = lds_scan[tid];
  uint32_t x = kk;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) lds_wave[wave] = x;
  __syncthreads();
  uint32_t ex = x - kk;
  for (int w = 0; w < wave; ++w) ex += lds_wave[w];
  lds_scan[tid] = ex;
  // Tile-dense slots at the tile's first input byte (a tile has at most as
  // many tokens as bytes); tile_compact_kernel moves every tile to its final
  // offset once all tile counts are known, so no tile ever waits for
  // another (a decoupled look-back here measured 5.41 vs 4.63 ms per 10 M
  // sentences: finished tiles held their CU slots waiting for slower
  // predecessors, profiles/r03d_c2_output_ab.txt).
  if (tid == 0) a.tile_count[tile] = static_cast<uint64_t>(lds_wave[0]) + lds_wave[1] + lds_wave[2] + lds_wave[3];
  __syncthreads();                       // lds_scan[] complete
  const uint64_t rec = lds_scan[sid_e];  // tile-local exclusive offset
  const uint64_t dst = a.off[base] + rec;
  int32_t *__restrict__ out_ids = a.slot_ids;
  uint32_t *__restrict__ out_len = a.slot_len;
  if (valid_e) {
    if (bad) {
      const uint32_t fk = atomicAdd(&a.status[kStFlagged], 1u);
      a.flagged[fk] = static_cast<uint32_t>(ie);
      atomicMax(&a.status[kStMaxNb], nb);
      a.tok_off[ie + 1] = rec | kTokFlag;
    } else {
      if constexpr (!kStage)
        if (k) backtrace(true, out_ids + dst, out_len ? out_len + dst : nullptr, k);
      a.tok_off[ie + 1] = rec + k;
    }
  }
  if (tile == 0 && tid == 0) a.tok_off[0] = 0;
  if constexpr (kStage) {
    // The tile's tokens in windows of kStageIds tile-local indices, the last
    // window first (lanes walk their chain from the end).  Per window the
    // lanes describe their tokens in it — (tile-relative byte offset) << 4 |
    // length, following the back-pointer bytes and nothing else: the counting
    // pass validated the chain and resolved its near ties — and then the
    // block looks the window's tokens up one per thread, all lanes busy and
    // consecutive lanes storing consecutive words.  (Looked up in the lane's
    // own backtrace a token cost its ~120 vector instructions once per
    // lockstep round, the wave's longest lane many rounds: 11.2 rounds for
    // 4.3 tokens per lane on the c2 corpus, tools/backtrace_model.py.)
    // Every thread runs every window and both of its barriers; a flagged,
    // invalid or empty lane holds no tokens (k == 0).
    const uint32_t tot =
        __builtin_amdgcn_readfirstlane(lds_wave[0] + lds_wave[1] + lds_wave[2] + lds_wave[3]);  // block-uniform
    const uint32_t rec32 = static_cast<uint32_t>(rec);
    int32_t *__restrict__ dst_ids = out_ids + a.off[base];
    uint32_t *__restrict__ dst_len = out_len ? out_len + a.off[base] : nullptr;
    uint32_t e = nb, j = k;  // the lane's tokens [rec32, rec32 + j) are yet to be described, ending at byte e
    for (uint32_t w = (tot + kStageIds - 1u) / kStageIds; w-- > 0;) {
      const uint32_t lo = w * kStageIds;
      while (j > 0 && rec32 + j > lo) {
        const uint32_t d = bp_load(e);
        e -= d;
        --j;
        lds_stage[rec32 + j - lo] = ((lrel + e) << 4) | d;
      }
      __syncthreads();
      const uint32_t m = tot - lo < kStageIds ? tot - lo : kStageIds;
      for (uint32_t t = static_cast<uint32_t>(tid); t < m; t += kBlock) {
        const uint32_t desc = lds_stage[t];
        int32_t id;
        float sc;
        token_of(desc >> 4, desc & 15u, &id, &sc);
        dst_ids[lo + t] = id;
        if (dst_len) dst_len[lo + t] = desc & 15u;
      }
      if (w) __syncthreads();  // the next window overwrites the stage (w is block-uniform)
    }
  }
  if (a.host_pub) {
    // Single-tile host call: every wave's output stores (pinned host memory)
    // complete, then the status words and the sequence number the host
    // polls for (EncodeHostSmall) — instead of copy commands and a stream
    // synchronization.
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
      for (int k = 0; k < kStWords; ++k)
        a.host_pub[1 + k] = __hip_atomic_load(&a.status[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      __hip_atomic_store(&a.host_pub[0], a.pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---------------------------------------------------------------------------
// General kernel: the reference Lattice, literally (node lists, Viterbi over
// every (rnode, lnode) pair in end_nodes_ insertion order, strict '>').
// One listed sentence per lane, scratch slab per lane.
// ---------------------------------------------------------------------------
struct GeneralArgs {
  const uint8_t *__restrict__ bytes;
  const uint64_t *__restrict__ off;
  const uint32_t *__restrict__ units;
  const int32_t *__restrict__ values;
  const float *__restrict__ scores;
  UnigramParams p;
  int32_t *__restrict__ slot_ids;
  uint32_t *__restrict__ slot_len;
  uint32_t *__restrict__ ntok;
  const uint32_t *__restrict__ list;  // sentence indices (nullptr: identity)
  const uint32_t *__restrict__ count; // device count of `list`
  uint64_t list_n;                    // used when list == nullptr
  uint8_t *__restrict__ scratch;
  uint64_t slab_bytes;
  uint32_t max_nb;                    // slab sized for sentences <= max_nb bytes
  uint32_t *__restrict__ ovf_list;    // longer sentences go here (nullptr: error)
  uint32_t *__restrict__ ovf_count;
  uint32_t *__restrict__ error;
  uint32_t lanes;                     // slabs in scratch (lanes beyond stay idle)
};

__global__ __launch_bounds__(64) void unigram_general_kernel(GeneralArgs a) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= a.lanes) return;
  const uint64_t nthreads = a.lanes;
  const uint64_t total = a.list ? *a.count : a.list_n;
  const int K = a.p.trie_results_size + 1;
  for (uint64_t j = tid; j < total; j += nthreads) {
    const uint32_t i = a.list ? a.list[j] : static_cast<uint32_t>(j);
    const uint64_t b0 = a.off[i];
    const uint32_t nb = static_cast<uint32_t>(a.off[i + 1] - b0);
    if (nb == 0) {
      a.ntok[i] = 0;
      continue;
    }
    if (nb > a.max_nb) {
      if (a.ovf_list) {
        a.ovf_list[atomicAdd(a.ovf_count, 1u)] = i;
      } else {
        atomicOr(a.error, 1u);
        a.ntok[i] = 0;
      }
      continue;
    }
    const uint8_t *__restrict__ s = a.bytes + b0;
    uint8_t *slab = a.scratch + tid * a.slab_bytes;
    const uint32_t cap_nodes = nb * K + 2;
    // Slab carve (all 4-byte arrays).
    uint32_t *cs = reinterpret_cast<uint32_t *>(slab);        // nb + 1
    int32_t *end_head = reinterpret_cast<int32_t *>(cs + nb + 1);
    int32_t *end_tail = end_head + nb + 1;
    int32_t *bfirst = end_tail + nb + 1;
    int32_t *bcount = bfirst + nb + 1;
    float *nscore = reinterpret_cast<float *>(bcount + nb + 1);
    float *nbt = nscore + cap_nodes;
    int32_t *nid = reinterpret_cast<int32_t *>(nbt + cap_nodes);
    int32_t *nprev = nid + cap_nodes;
    int32_t *nnext = nprev + cap_nodes;  // next in end list
    uint32_t *npos = reinterpret_cast<uint32_t *>(nnext + cap_nodes);
    uint32_t *nlen = npos + cap_nodes;

    // SetSentence (:147-187)
    uint32_t nc = 0;
    for (uint32_t q = 0; q < nb;) {
      cs[nc++] = q;
      uint32_t cl = OneCharLenDev(s[q]);
      q += cl < nb - q ? cl : nb - q;
    }
    cs[nc] = nb;
    for (uint32_t p = 0; p <= nc; ++p) {
      end_head[p] = -1;
      end_tail[p] = -1;
      bfirst[p] = 0;
      bcount[p] = 0;
    }
    auto push_end = [&](uint32_t q, int32_t nd) {
      nnext[nd] = -1;
      if (end_tail[q] < 0) end_head[q] = nd;
      else nnext[end_tail[q]] = nd;
      end_tail[q] = nd;
    };
    int32_t nn = 0;
    // BOS
    nscore[0] = 0.f; nbt[0] = 0.f; nid[0] = -1; nprev[0] = -1; npos[0] = 0; nlen[0] = 0;
    push_end(0, 0);
    nn = 1;
    // EOS
    nscore[1] = 0.f; nbt[1] = 0.f; nid[1] = -1; nprev[1] = -1; npos[1] = nc; nlen[1] = 0;
    nn = 2;
    bfirst[nc] = 1;
    bcount[nc] = 1;
    // PopulateNodes (:535-604)
    for (uint32_t p = 0; p < nc; ++p) {
      bfirst[p] = nn;
      bool single = false;
      uint32_t base = a.p.root_base;
      uint32_t cpos = p;  // char index reached by the walk
      for (uint32_t q = cs[p]; q < nb; ++q) {
        const uint32_t c = s[q];
        if (c == 0) break;
        const uint32_t node = base ^ c;
        const uint32_t u = a.units[node];
        if ((u & 0xFFu) != c) break;
        base = u >> 9;
        if (u & 0x100u) {
          const uint32_t e = q + 1;
          while (cs[cpos] < e) ++cpos;  // get_chars_length
          const uint32_t length = cpos - p;
          const int32_t v = a.values[node];
          const int32_t kind = v >> kKindShift;
          if (kind == kKindUnused) continue;
          const int32_t nd = nn++;
          nid[nd] = v & kIdMask;
          nscore[nd] = kind == kKindUserDefined ? UserDefinedScore(length, a.p.max_score)
                                                : a.scores[v & kIdMask];
          npos[nd] = p;
          nlen[nd] = length;
          push_end(p + length, nd);
          if (length == 1) single = true;
        }
      }
      if (!single) {
        const int32_t nd = nn++;
        nid[nd] = a.p.unk_id;
        nscore[nd] = a.p.unk_score;
        npos[nd] = p;
        nlen[nd] = 1;
        push_end(p + 1, nd);
      }
      bcount[p] = nn - bfirst[p];
    }
    // Viterbi (:222-261)
    bool fail = false;
    for (uint32_t p = 0; p <= nc && !fail; ++p) {
      for (int32_t r = bfirst[p]; r < bfirst[p] + bcount[p]; ++r) {
        nprev[r] = -1;
        float best_score = 0.f;
        int32_t best = -1;
        for (int32_t l = end_head[p]; l >= 0; l = nnext[l]) {
          const float sc = __fadd_rn(nbt[l], nscore[r]);
          if (best < 0 || sc > best_score) {
            best = l;
            best_score = sc;
          }
        }
        if (best < 0) {
          fail = true;
          break;
        }
        nprev[r] = best;
        nbt[r] = best_score;
      }
    }
    int32_t *__restrict__ out_id = a.slot_ids + b0 + nb;
    uint32_t *__restrict__ out_len = a.slot_len ? a.slot_len + b0 + nb : nullptr;
    uint32_t k = 0;
    if (!fail) {
      for (int32_t nd = nprev[1]; nd >= 0 && nprev[nd] >= 0; nd = nprev[nd]) {
        ++k;
        out_id[-static_cast<int64_t>(k)] = nid[nd];
        if (out_len) out_len[-static_cast<int64_t>(k)] = cs[npos[nd] + nlen[nd]] - cs[npos[nd]];
      }
    }
    a.ntok[i] = k;
  }
}

}  // namespace

uint64_t UnigramGeneralSlabBytes(uint32_t max_nb, int trie_results_size) {
  const uint64_t nb = max_nb;
  const uint64_t cap_nodes = nb * (trie_results_size + 1) + 2;
  return ((nb + 1) * 5 + cap_nodes * 7) * 4 + 64;
}

hipError_t LaunchUnigramFast(UnigramKernel kind, int W, const UnigramLaunch &l, hipStream_t st) {
  FastArgs a{l.bytes, l.off, l.n, l.capacity, l.units, l.values, l.scores, l.num_units, l.p, l.ids, l.len,
             l.tok_off, l.bp, l.flagged, l.status, l.tile_count, l.corrupt_bp, l.chain, l.slot_ids, l.slot_len,
             EStepForwardOut{}, l.bpn, l.stage_src, l.stage_dst, l.stage_zero, l.stage_words, l.host_pub, l.pub_seq,
             l.coop_min_nb, l.piece_tab, l.piece_mask, l.piece_seed};
  const uint64_t blocks64 = FastTiles(l.n);
  if (blocks64 == 0) return hipSuccess;
  if (blocks64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
  // The staged image and the publication are one block's work.
  if ((l.stage_src || l.host_pub) && blocks64 != 1) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks64));
  // 7 waves/SIMD: 72 VGPRs, no spill.  8 waves (64 VGPRs, 14 spilled)
  // measured 6.78 vs 5.41 ms per 10 M sentences (profiles/r03c_c2_waves_ab.txt).
  if (kind == UnigramKernel::kByte && W == 16) {
    hipLaunchKernelGGL((unigram_fast_kernel<16, true>), grid, dim3(kBlock), 0, st, a);
  } else if (kind == UnigramKernel::kWide && W == 16) {
    hipLaunchKernelGGL((unigram_fast_kernel<16, false, 3, false, true>), grid, dim3(kBlock), 0, st, a);
  } else if (kind == UnigramKernel::kChar && W == 16) {
    hipLaunchKernelGGL((unigram_fast_kernel<16, false>), grid, dim3(kBlock), 0, st, a);
  } else if (kind == UnigramKernel::kChar && W == 32) {
    hipLaunchKernelGGL((unigram_fast_kernel<32, false>), grid, dim3(kBlock), 0, st, a);
  } else if (kind == UnigramKernel::kChar && W == 64) {
    hipLaunchKernelGGL((unigram_fast_kernel<64, false>), grid, dim3(kBlock), 0, st, a);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t LaunchUnigramEStepForward(const UnigramLaunch &l, const EStepForwardOut &e, hipStream_t st) {
  FastArgs a{l.bytes, l.off, l.n, l.capacity, l.units, l.values, l.scores, l.num_units, l.p, l.ids, l.len,
             l.tok_off, l.bp, l.flagged, l.status, l.tile_count, ~0ull, nullptr, nullptr, nullptr, e};
  const uint64_t blocks64 = FastTiles(l.n);
  if (blocks64 == 0) return hipSuccess;
  if (blocks64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
  // 4 waves/SIMD (128 VGPRs, 14 spilled): c4 FAST 0.272 vs 0.281 s/epoch at
  // 3 waves, PARITY 0.415 vs 0.410 (profiles/r03y_estep_byte_forward_ab.txt).
  hipLaunchKernelGGL((unigram_fast_kernel<16, true, kEStepWaves, true>), dim3(static_cast<unsigned>(blocks64)),
                     dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t LaunchUnigramGeneral(const UnigramLaunch &l, const GeneralLaunch &g, hipStream_t st) {
  GeneralArgs a{l.bytes, l.off, l.gen_units, l.values, l.scores, l.p, g.slot_ids, g.slot_len, g.ntok, g.list,
                g.count, g.list_n, g.scratch, g.slab_bytes, g.max_nb, g.ovf_list, g.ovf_count, g.error,
                g.threads};
  const unsigned blocks = (g.threads + 63) / 64;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(unigram_general_kernel, dim3(blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace spm_amd
