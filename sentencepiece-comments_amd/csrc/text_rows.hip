// Text rows on the device (text_rows.h): line split, id rows, piece rows.
//
// All three are a stream compaction or expansion whose output position depends
// on everything before it, and all three have one shape.  kTextBlocks blocks
// take a ticket; block t owns the t-th contiguous range of the input (a
// multiple of the pass's tile, computed on the device, so no size is needed on
// the host) and walks it twice:
//
//   count : the range's output size (newlines; text bytes).
//   base  : decoupled look-back over the kTextBlocks descriptors (lookback.h):
//           one value per block, the output before it.  For the split that
//           value is the lines before; the bytes before are the position
//           minus it.
//   write : one tile at a time.  A block scan of the tile places every lane's
//           output.
//
// How the bytes leave:
//   split, id rows : a lane owns 16 input bytes / 4 consecutive items and puts
//           its output bytes into an LDS image of the tile's output span, laid
//           out with the span's own phase inside a 16-byte granule.  The block
//           then stores the image with one 16-byte store per lane (byte stores
//           on the two ragged edges), so a wave's stores are one contiguous
//           1 KiB whatever the line or id lengths are.
//   piece rows : a piece runs from 1 byte to a whole unknown run.  A lane
//           copies its own piece of up to kPieceWaveOverDefault (32) bytes; a
//           longer one is copied by its wave, 64 consecutive bytes a step (a
//           ballot names the lanes with such a piece, shuffles hand out its
//           source, place and length).  No LDS, no barrier in the write.  The
//           bound is measured: flat from 16 to 128 bytes on real text, slower
//           at 4 and 8.  The other form that was built and measured, 13 %
//           slower, stays behind SPM_HIP_TEXT_ROWS_PIECE_WAVE=0: the tile's
//           starts in LDS and the write laid out over the output bytes, lane
//           o finding the item of byte o by binary search.
//   The split and id rows also run with every lane storing its own bytes
//   (SPM_HIP_TEXT_ROWS_FORM=direct): 19 % slower in the split, within 5 %
//   either way in id rows, so the image stays.
//
// An item of the two row passes is a token, or the terminator every row has
// after its tokens: item g belongs to row i with S(i) <= g < S(i+1), S(i) =
// off[i] - off[0] + i (token_tiles.h with one extra per row).  A token's bytes
// are its text and one separator (' ', or '\n' on the row's last token); the
// terminator of a row without tokens is the row's '\n', any other is empty.
//
// No atomics on the data path: the ticket, the look-back descriptors and the
// error word are all.  Errors found by a block go to the error word; the
// status word is read on entry and written only by the finish kernel, so every
// block of a pass sees the same value and the look-back chain is never cut.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "lookback.h"
#include "text_rows.h"
#include "token_tiles.h"

namespace spm_amd {
namespace {

__global__ __launch_bounds__(256) void text_init_kernel(uint64_t *__restrict__ scratch) {
  for (uint32_t i = threadIdx.x; i < kTcWords + kTextBlocks; i += 256) scratch[i] = 0;
}

// The t-th of kTextBlocks contiguous ranges of [0, total), a multiple of tile.
__device__ __forceinline__ Range TextRange(uint64_t total, uint32_t tile, uint64_t t) {
  uint64_t chunk = (total + kTextBlocks - 1) / kTextBlocks;
  chunk = (chunk + tile - 1) / tile * tile;
  Range r;
  r.begin = t * chunk;
  r.end = r.begin + chunk;
  if (r.begin > total) r.begin = total;
  if (r.end > total) r.end = total;
  return r;
}

__device__ __forceinline__ uint64_t TakeTicket(uint64_t *ctl, uint32_t *s_tile) {
  if (threadIdx.x == 0) *s_tile = atomicAdd(reinterpret_cast<uint32_t *>(ctl + kTcTicket), 1u);
  __syncthreads();
  return *s_tile;
}

// Output before block `tile`, given its own sum (every thread gets it).
__device__ __forceinline__ uint64_t BlockBase(uint64_t *desc, uint64_t tile, uint64_t sum, uint64_t *s_carry) {
  if (threadIdx.x < 64) {
    const uint64_t pre = LookbackExclusive(desc, tile, sum, threadIdx.x);
    if (threadIdx.x == 0) *s_carry = pre;
  }
  __syncthreads();
  return *s_carry;
}

// Stores the LDS image of the output span [obase, obase + cnt): byte k of the
// span stands at s[ph + k], ph = the span's phase in a 16-byte granule of out.
// Nothing at or past cap is written.
__device__ __forceinline__ void FlushImage(uint8_t *__restrict__ out, uint64_t obase, uint32_t cnt, uint64_t cap,
                                           const uint8_t *s, uint32_t ph) {
  const uint32_t end = ph + cnt;
  for (uint32_t lo = threadIdx.x * 16u; lo < end; lo += 256u * 16u) {
    const uint64_t at = obase + lo;  // index of s[lo] in out, plus ph
    if (lo >= ph && lo + 16 <= end && at - ph + 16 <= cap) {
      *reinterpret_cast<uint4 *>(out + (at - ph)) = *reinterpret_cast<const uint4 *>(s + lo);
    } else {
      for (uint32_t b = lo < ph ? ph : lo; b < lo + 16 && b < end; ++b)
        if (obase + b - ph < cap) out[obase + b - ph] = s[b];
    }
  }
}

// ---------------------------------------------------------------- split ----

// 16 bytes of the input in aligned coordinates: q = position + mis, mis = the
// base's offset in its 16-byte granule, so a whole granule is one aligned
// load.  A granule that straddles either end of the buffer is read byte by
// byte, its bytes outside the buffer are 0 and not valid.
struct Granule {
  uint32_t w[4];
  uint32_t valid, nl;  // 16-bit masks
};

__device__ __forceinline__ uint32_t NewlineBits(uint32_t x) {  // 0x80 in every byte that is '\n', exact
  x ^= 0x0A0A0A0Au;
  const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  return ~(t | x | 0x7F7F7F7Fu);
}

__device__ __forceinline__ Granule LoadGranule(const uint8_t *__restrict__ in, uint64_t q, uint32_t mis,
                                               uint64_t qend, uint64_t rend) {
  Granule g{{0, 0, 0, 0}, 0, 0};
  if (q >= rend) return g;
  if (q >= mis && q + 16 <= qend) {
    const uint4 v = *reinterpret_cast<const uint4 *>(in + (q - mis));
    g.w[0] = v.x;
    g.w[1] = v.y;
    g.w[2] = v.z;
    g.w[3] = v.w;
    g.valid = 0xFFFFu;
  } else {
    for (uint32_t j = 0; j < 16; ++j) {
      if (q + j < mis || q + j >= qend) continue;
      g.w[j >> 2] |= static_cast<uint32_t>(in[q + j - mis]) << (8 * (j & 3));
      g.valid |= 1u << j;
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t t = NewlineBits(g.w[k]);
    g.nl |= (((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u)) << (4 * k);
  }
  g.nl &= g.valid;  // a 0 byte is no newline anyway
  return g;
}

__global__ __launch_bounds__(256) void split_kernel(const uint8_t *__restrict__ in, uint64_t nbytes,
                                                    uint8_t *__restrict__ out, uint64_t *__restrict__ off,
                                                    uint64_t line_cap, uint64_t *__restrict__ scratch,
                                                    const uint32_t *__restrict__ status, bool direct) {
  __shared__ uint32_t s_tile;
  __shared__ uint64_t s_w64[4], s_carry;
  __shared__ uint32_t s_w[4];
  __shared__ __align__(16) uint8_t s_img[kSplitTile + 32];
  if (*status) return;  // uniform over the grid: only the finish kernel writes it
  uint64_t *ctl = scratch, *desc = scratch + kTcWords;
  const uint64_t tile = TakeTicket(ctl, &s_tile);
  const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(in) & 15u);
  const uint64_t qend = nbytes ? mis + nbytes : 0;
  const Range r = TextRange(qend, kSplitTile, tile);
  uint64_t sum = 0;
  for (uint64_t q = r.begin + threadIdx.x * 16u; q < r.end; q += kSplitTile)
    sum += __popc(LoadGranule(in, q, mis, qend, r.end).nl);
  sum = BlockSum64(sum, s_w64);
  uint64_t nl_run = BlockBase(desc, tile, sum, &s_carry);  // newlines = lines before the tile
  for (uint64_t s = r.begin; s < r.end; s += kSplitTile) {
    const uint64_t q0 = s + threadIdx.x * 16u;
    const Granule g = LoadGranule(in, q0, mis, qend, r.end);
    uint32_t sub_nl;
    uint64_t nlb = nl_run + BlockExclusiveScan(__popc(g.nl), s_w, &sub_nl);
    // The tile's first valid position and its bytes.
    const uint64_t first = (s < mis ? mis : s) - mis;
    const uint64_t send = s + kSplitTile < r.end ? s + kSplitTile : r.end;
    const uint32_t bytes = send > first + mis ? static_cast<uint32_t>(send - mis - first) : 0u;
    const uint64_t obase = first - nl_run;
    const uint32_t ph = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(out) + obase) & 15u);
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      if (!((g.valid >> j) & 1u)) continue;
      const uint64_t p = q0 + j - mis;
      if ((g.nl >> j) & 1u) {
        if (nlb + 1 <= line_cap) off[nlb + 1] = p - nlb;
        ++nlb;
      } else {
        const uint8_t c = static_cast<uint8_t>(g.w[j >> 2] >> (8 * (j & 3)));
        if (direct) out[p - nlb] = c;
        else s_img[ph + static_cast<uint32_t>(p - nlb - obase)] = c;
      }
    }
    if (!direct) {  // uniform
      __syncthreads();
      FlushImage(out, obase, bytes - sub_nl, ~0ull, s_img, ph);
      __syncthreads();
    }
    nl_run += sub_nl;
  }
}

__global__ void split_finish_kernel(const uint8_t *__restrict__ in, uint64_t nbytes, uint64_t *__restrict__ off,
                                    uint64_t line_cap, uint64_t *__restrict__ counts,
                                    const uint64_t *__restrict__ scratch, uint32_t *__restrict__ status) {
  if (*status) return;
  const uint64_t nl = scratch[kTcWords + kTextBlocks - 1] & kLbValue;
  uint64_t lines = nl;
  off[0] = 0;
  if (nbytes && in[nbytes - 1] != '\n' && ++lines <= line_cap) off[lines] = nbytes - nl;
  if (counts) {
    counts[0] = lines;
    counts[1] = nbytes - nl;
  }
  if (lines > line_cap) *status = SPM_RESOURCE_EXHAUSTED;
}

// ------------------------------------------------------------- row items ----

struct Item {
  bool token;     // else the row's terminator
  bool first;     // first item of its row
  bool last;      // a token: the row's last
  bool empty_row; // a terminator: its row has no token
  uint64_t src;   // a token: index into the row CSR's payload
};

__device__ __forceinline__ Item ItemAt(const TokView &v, uint64_t sent, uint64_t g) {
  const uint64_t s0 = SentStart(v, sent);
  const uint64_t m = SentStart(v, sent + 1) - s0 - 1;
  const uint64_t pos = g - s0;
  Item it;
  it.token = pos < m;
  it.first = pos == 0;
  it.last = pos + 1 == m;
  it.empty_row = m == 0;
  it.src = v.tok_off[sent] + pos;
  return it;
}

__device__ __forceinline__ void RaiseError(uint64_t *ctl, uint32_t code) {
  atomicCAS(reinterpret_cast<uint32_t *>(ctl + kTcError), 0u, code);
}

// row_off[n], exhaustion and the error word, after either row pass.
__global__ void rows_finish_kernel(uint64_t n, uint64_t cap, uint64_t *__restrict__ row_off,
                                   const uint64_t *__restrict__ scratch, uint32_t *__restrict__ status) {
  if (*status) return;
  const uint64_t total = scratch[kTcWords + kTextBlocks - 1] & kLbValue;
  row_off[n] = total;
  const uint32_t err = static_cast<uint32_t>(scratch[kTcError]);
  if (err) *status = err;
  else if (total > cap) *status = SPM_RESOURCE_EXHAUSTED;
}

// --------------------------------------------------------------- id rows ----

// Width of an item of the id pass; *val = the token's id (0 for a bad one).
__device__ __forceinline__ uint32_t IdItemWidth(const TokView &v, const Item &it, uint64_t *ctl, uint32_t *val) {
  *val = 0;
  if (!it.token) return it.empty_row ? 1u : 0u;
  const int32_t id = v.ids[it.src];
  if (id < 0) RaiseError(ctl, SPM_OUT_OF_RANGE);
  else *val = static_cast<uint32_t>(id);
  return DecimalDigits(*val) + 1u;
}

__global__ __launch_bounds__(256) void id_rows_kernel(TokView v, uint8_t *__restrict__ out, uint64_t cap,
                                                      uint64_t *__restrict__ row_off,
                                                      uint64_t *__restrict__ scratch,
                                                      const uint32_t *__restrict__ status, bool direct) {
  __shared__ uint32_t s_tile;
  __shared__ uint64_t s_w64[4], s_carry;
  __shared__ uint32_t s_w[4];
  __shared__ __align__(16) uint8_t s_img[kIdTile * kIdMaxWidth + 32];
  if (*status) return;
  uint64_t *ctl = scratch, *desc = scratch + kTcWords;
  const uint64_t tile = TakeTicket(ctl, &s_tile);
  v.base = v.tok_off[0];
  const Range r = TextRange(SentStart(v, v.n), kIdTile, tile);
  uint64_t sent = 0, sum = 0;
  bool have = false;
  for (uint64_t s = r.begin + threadIdx.x * 4u; s < r.end; s += kIdTile) {
    for (uint32_t j = 0; j < 4 && s + j < r.end; ++j) {
      sent = FindSentence(v, have ? sent : 0, v.n, s + j);
      have = true;
      uint32_t val;
      sum += IdItemWidth(v, ItemAt(v, sent, s + j), ctl, &val);
    }
  }
  sum = BlockSum64(sum, s_w64);
  uint64_t run = BlockBase(desc, tile, sum, &s_carry);
  have = false;
  for (uint64_t s = r.begin; s < r.end; s += kIdTile) {
    const uint64_t g0 = s + threadIdx.x * 4u;
    uint32_t width[4] = {0, 0, 0, 0}, val[4] = {0, 0, 0, 0}, mine = 0;
    Item it[4];
    uint64_t row[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      it[j].token = it[j].first = false;
      if (g0 + j < r.end) {
        sent = FindSentence(v, have ? sent : 0, v.n, g0 + j);
        have = true;
        row[j] = sent;
        it[j] = ItemAt(v, sent, g0 + j);
        width[j] = IdItemWidth(v, it[j], ctl, &val[j]);
        mine += width[j];
      }
    }
    uint32_t sub_total;
    uint32_t at = BlockExclusiveScan(mine, s_w, &sub_total);
    const uint32_t ph = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(out) + run) & 15u);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (g0 + j >= r.end) continue;
      if (it[j].first) row_off[row[j]] = run + at;
      const uint8_t sep = it[j].token && !it[j].last ? ' ' : '\n';
      const uint32_t nd = it[j].token ? width[j] - 1 : 0;
      uint32_t x = val[j];
      if (direct) {  // the lane stores its own bytes
        const uint64_t o = run + at;
        for (uint32_t k = nd; k-- > 0; x /= 10u)
          if (o + k < cap) out[o + k] = static_cast<uint8_t>('0' + x % 10u);
        if (width[j] && o + nd < cap) out[o + nd] = sep;
      } else {
        for (uint32_t k = nd; k-- > 0; x /= 10u) s_img[ph + at + k] = static_cast<uint8_t>('0' + x % 10u);
        if (width[j]) s_img[ph + at + nd] = sep;
      }
      at += width[j];
    }
    if (!direct) {  // uniform
      __syncthreads();
      FlushImage(out, run, sub_total, cap, s_img, ph);
      __syncthreads();
    }
    run += sub_total;
  }
}

// ------------------------------------------------------------ piece rows ----

struct PieceView {
  const spm_hip_piece *pieces;
  const uint8_t *norm;
  const uint64_t *norm_off;
  PieceStrings tab;
};

// Text of a token item: its bytes and their count (0 bytes for a bad record).
__device__ __forceinline__ uint32_t PieceText(const PieceView &pv, const Item &it, uint64_t sent, uint64_t *ctl,
                                              const uint8_t **src) {
  const spm_hip_piece p = pv.pieces[it.src];
  if (p.norm_end > p.norm_begin) {
    const uint64_t b = pv.norm_off[sent];
    if (p.norm_end > pv.norm_off[sent + 1] - b) {
      RaiseError(ctl, SPM_OUT_OF_RANGE);
      return 0;
    }
    *src = pv.norm + b + p.norm_begin;
    return p.norm_end - p.norm_begin;
  }
  if (p.id < 0 || p.id >= pv.tab.num_pieces) {
    RaiseError(ctl, SPM_OUT_OF_RANGE);
    return 0;
  }
  const uint32_t o = pv.tab.off[p.id];
  *src = pv.tab.bytes + o;
  return pv.tab.off[p.id + 1] - o;
}

__global__ __launch_bounds__(256) void piece_rows_kernel(TokView v, PieceView pv, uint8_t *__restrict__ out,
                                                         uint64_t cap, uint64_t *__restrict__ row_off,
                                                         uint64_t *__restrict__ scratch,
                                                         const uint32_t *__restrict__ status, uint32_t wave_over) {
  __shared__ uint32_t s_tile;
  __shared__ uint64_t s_w64[4], s_carry;
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_start[kPieceTile], s_len[kPieceTile];
  __shared__ const uint8_t *s_src[kPieceTile];
  __shared__ uint8_t s_sep[kPieceTile];
  if (*status) return;
  uint64_t *ctl = scratch, *desc = scratch + kTcWords;
  const uint64_t tile = TakeTicket(ctl, &s_tile);
  v.base = v.tok_off[0];
  const Range r = TextRange(SentStart(v, v.n), kPieceTile, tile);
  uint64_t sent = 0, sum = 0;
  bool have = false;
  for (uint64_t g = r.begin + threadIdx.x; g < r.end; g += kPieceTile) {
    sent = FindSentence(v, have ? sent : 0, v.n, g);
    have = true;
    const Item it = ItemAt(v, sent, g);
    const uint8_t *src;
    sum += it.token ? PieceText(pv, it, sent, ctl, &src) + 1u : (it.empty_row ? 1u : 0u);
  }
  sum = BlockSum64(sum, s_w64);
  uint64_t run = BlockBase(desc, tile, sum, &s_carry);
  have = false;
  for (uint64_t s = r.begin; s < r.end; s += kPieceTile) {
    const uint64_t g = s + threadIdx.x;
    uint32_t len = 0, width = 0;
    const uint8_t *src = nullptr;
    uint8_t sep = '\n';
    bool first = false;
    if (g < r.end) {
      sent = FindSentence(v, have ? sent : 0, v.n, g);
      have = true;
      const Item it = ItemAt(v, sent, g);
      first = it.first;
      if (it.token) {
        len = PieceText(pv, it, sent, ctl, &src);
        width = len + 1u;
        if (!it.last) sep = ' ';
      } else {
        width = it.empty_row ? 1u : 0u;
      }
    }
    uint32_t sub_total;
    const uint32_t at = BlockExclusiveScan(width, s_w, &sub_total);
    if (first) row_off[sent] = run + at;
    if (wave_over) {
      // Per lane / per wave: a lane copies its own piece of up to wave_over
      // bytes; a longer one is copied by its wave, 64 bytes a step.
      const uint64_t o = run + at;
      const bool wide = len > wave_over;
      if (!wide)
        for (uint32_t k = 0; k < len; ++k)
          if (o + k < cap) out[o + k] = src[k];
      if (width && o + len < cap) out[o + len] = sep;
      const int lane = threadIdx.x & 63;
      for (uint64_t m = __builtin_amdgcn_ballot_w64(wide); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        const uint64_t sp = reinterpret_cast<uint64_t>(src);
        const uint8_t *from = reinterpret_cast<const uint8_t *>(
            (static_cast<uint64_t>(__shfl(static_cast<uint32_t>(sp >> 32), l)) << 32) |
            __shfl(static_cast<uint32_t>(sp), l));
        const uint64_t to = (static_cast<uint64_t>(__shfl(static_cast<uint32_t>(o >> 32), l)) << 32) |
                            __shfl(static_cast<uint32_t>(o), l);
        const uint32_t n_l = __shfl(len, l);
        for (uint32_t k = lane; k < n_l; k += 64)
          if (to + k < cap) out[to + k] = from[k];
      }
      run += sub_total;
      continue;  // uniform
    }
    s_start[threadIdx.x] = at;
    s_len[threadIdx.x] = len;
    s_src[threadIdx.x] = src;
    s_sep[threadIdx.x] = sep;
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < sub_total && run + o < cap; o += kPieceTile) {
      // The item holding byte o: the last one that starts at or before o
      // (items of no bytes share a start with their successor).
      uint32_t a = 0, b = kPieceTile;
      while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if (s_start[mid] <= o) a = mid;
        else b = mid;
      }
      const uint32_t k = o - s_start[a];
      out[run + o] = k < s_len[a] ? s_src[a][k] : s_sep[a];
    }
    __syncthreads();
    run += sub_total;
  }
}

}  // namespace

// Measurement knobs, read at every call (profiles/pr39_text_rows.txt compares
// the forms): SPM_HIP_TEXT_ROWS_FORM=direct makes every lane of the split and
// of id rows store its own bytes instead of going through the LDS image;
// SPM_HIP_TEXT_ROWS_PIECE_WAVE=N (>= 1) makes piece rows copy a piece of up to
// N bytes by its lane and a longer one by its wave, 0 is the layout over the
// output bytes.
namespace {
bool DirectForm() {
  const char *e = std::getenv("SPM_HIP_TEXT_ROWS_FORM");
  return e ? std::strcmp(e, "direct") == 0 : kTextDirectDefault;
}
uint32_t PieceWaveOver() {
  const char *e = std::getenv("SPM_HIP_TEXT_ROWS_PIECE_WAVE");
  return e ? static_cast<uint32_t>(std::strtoul(e, nullptr, 10)) : kPieceWaveOverDefault;
}
}  // namespace

hipError_t LaunchSplitLines(const uint8_t *in, uint64_t nbytes, uint8_t *out, uint64_t *off, uint64_t line_cap,
                            uint64_t *counts, uint32_t *status, void *scratch, hipStream_t st) {
  uint64_t *sc = static_cast<uint64_t *>(scratch);
  hipLaunchKernelGGL(text_init_kernel, dim3(1), dim3(256), 0, st, sc);
  hipLaunchKernelGGL(split_kernel, dim3(kTextBlocks), dim3(256), 0, st, in, nbytes, out, off, line_cap, sc, status,
                     DirectForm());
  hipLaunchKernelGGL(split_finish_kernel, dim3(1), dim3(1), 0, st, in, nbytes, off, line_cap, counts, sc, status);
  return hipGetLastError();
}

hipError_t LaunchIdRows(const int32_t *ids, const uint64_t *off, uint64_t n, uint8_t *out, uint64_t cap,
                        uint64_t *row_off, uint32_t *status, void *scratch, hipStream_t st) {
  uint64_t *sc = static_cast<uint64_t *>(scratch);
  const TokView v{ids, off, n, 0, 1};
  hipLaunchKernelGGL(text_init_kernel, dim3(1), dim3(256), 0, st, sc);
  hipLaunchKernelGGL(id_rows_kernel, dim3(kTextBlocks), dim3(256), 0, st, v, out, cap, row_off, sc, status,
                     DirectForm());
  hipLaunchKernelGGL(rows_finish_kernel, dim3(1), dim3(1), 0, st, n, cap, row_off, sc, status);
  return hipGetLastError();
}

hipError_t LaunchPieceRows(const spm_hip_piece *pieces, const uint64_t *piece_off, uint64_t n, const uint8_t *norm,
                           const uint64_t *norm_off, PieceStrings tab, uint8_t *out, uint64_t cap,
                           uint64_t *row_off, uint32_t *status, void *scratch, hipStream_t st) {
  uint64_t *sc = static_cast<uint64_t *>(scratch);
  const TokView v{nullptr, piece_off, n, 0, 1};
  const PieceView pv{pieces, norm, norm_off, tab};
  hipLaunchKernelGGL(text_init_kernel, dim3(1), dim3(256), 0, st, sc);
  hipLaunchKernelGGL(piece_rows_kernel, dim3(kTextBlocks), dim3(256), 0, st, v, pv, out, cap, row_off, sc, status,
                     PieceWaveOver());
  hipLaunchKernelGGL(rows_finish_kernel, dim3(1), dim3(1), 0, st, n, cap, row_off, sc, status);
  return hipGetLastError();
}

}  // namespace spm_amd
