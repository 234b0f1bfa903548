// The staged image of one small host call: where the offsets, the input
// bytes, the outputs and the publication words sit in the pinned coherent
// image, and in its device mirror (the same offsets).  Host only.
#pragma once

#include <cstdint>
#include <cstring>

namespace spm_amd {

// kRaw: 1..kCoopSmallMax raw lines (coop_raw_kernel).  kCoop: as many
// normalized sentences (coop_small_kernel).  kLane: up to 256 normalized
// sentences, one tile of the lane kernels, whose zeroed control block
// (ctl_bytes) leads the device mirror.  kBpeRaw / kBpe: the images of kRaw /
// kCoop for a BPE model (bpe_raw_kernel, bpe_small_kernel), which keep no
// per-char tables beside the token slots.
enum class SmallKind { kRaw, kCoop, kLane, kBpeRaw, kBpe };

// Every region starts on a 256-byte boundary.  The kernels read the input in
// 16-byte steps, so 16 bytes of pad follow it; they index token slots and
// scratch rows by the STAGED byte offset (in + off[i]), so `slots` counts from
// the image's start, not from the first input byte.
struct SmallLayout {
  uint64_t off;      // (n + 1) x u64 sentence / line offsets
  uint64_t in;       // input bytes
  uint64_t in_end;   // in + total
  uint64_t tok;      // (n + 1) x u64 token offsets out
  uint64_t ids;      // ids_cap x i32 ids out
  uint64_t len;      // ids_cap x u32 piece lengths out (0: none laid out)
  uint64_t out_end;  // end of the last output region
  uint64_t pub;      // 256 B: publication word, status words, late status copy
  uint64_t ids_cap;  // ids (and lengths) the image has room for
  uint64_t slots;    // raw, coop: rows of the cooperative kernel's device tables (0: lane)
  uint64_t table_slots;  // of them, rows of its per-char tables (w_cpv, w_cnd); 0: lane and the BPE kinds
  uint64_t slot_len_bytes;  // device bytes beside the id slots: coop piece lengths, raw normalized bytes
  uint64_t dev_bytes;  // to reserve for the device mirror
  uint64_t pin_bytes;  // to reserve for the pinned image

  uint32_t stage_words() const { return static_cast<uint32_t>((in_end + 3) / 4); }  // words the kernel copies down
  uint32_t zero_words() const { return static_cast<uint32_t>(off / 4); }  // lane: the control block it zeroes

  // The regions of an image that starts at `b` (pinned, or the device mirror).
  uint64_t *Off(uint8_t *b) const { return reinterpret_cast<uint64_t *>(b + off); }
  uint8_t *In(uint8_t *b) const { return b + in; }
  uint64_t *Tok(uint8_t *b) const { return reinterpret_cast<uint64_t *>(b + tok); }
  int32_t *Ids(uint8_t *b) const { return reinterpret_cast<int32_t *>(b + ids); }
  uint32_t *Len(uint8_t *b) const { return reinterpret_cast<uint32_t *>(b + len); }
  uint32_t *Pub(uint8_t *b) const { return reinterpret_cast<uint32_t *>(b + pub); }
  uint32_t *LateStatus(uint8_t *b) const { return reinterpret_cast<uint32_t *>(b + pub + 128); }

  // The call's input into the pinned image; the publication word cleared.
  void Stage(uint8_t *h, const uint64_t *offsets, const uint8_t *bytes, uint64_t n) const {
    std::memcpy(h + off, offsets, (n + 1) * 8);
    if (in_end > in) std::memcpy(h + in, bytes, in_end - in);
    *static_cast<volatile uint32_t *>(Pub(h)) = 0;
  }
};

constexpr uint64_t SmallAlign(uint64_t x) { return (x + 255) & ~255ull; }

// kCoop lays a `len` region out whether or not the call asks for lengths,
// kLane only with_len.
constexpr SmallLayout MakeSmallLayout(SmallKind kind, uint64_t n, uint64_t total, bool with_len = false,
                                      uint64_t ctl_bytes = 0) {
  const bool bpe = kind == SmallKind::kBpeRaw || kind == SmallKind::kBpe;
  const bool raw = kind == SmallKind::kRaw || kind == SmallKind::kBpeRaw, lane = kind == SmallKind::kLane;
  SmallLayout l{};
  l.off = lane ? SmallAlign(ctl_bytes) : 0;
  l.in = SmallAlign(l.off + (n + 1) * 8);
  l.in_end = l.in + total;
  l.tok = SmallAlign(l.in_end + 16);
  l.ids = SmallAlign(l.tok + (n + 1) * 8);
  // Raw lines: what the normalizer and the encode can make of them at most.
  l.ids_cap = raw ? 4 * total + 8 * n + 64 : (total ? total : 1);
  const bool has_len = kind == SmallKind::kCoop || kind == SmallKind::kBpe || (lane && with_len);
  l.len = has_len ? SmallAlign(l.ids + l.ids_cap * 4) : 0;
  l.out_end = (has_len ? l.len : l.ids) + l.ids_cap * 4;
  l.pub = SmallAlign(l.out_end);
  l.pin_bytes = l.pub + 256;
  l.slots = raw ? l.ids_cap : lane ? 0 : l.in_end + 16;
  l.table_slots = bpe ? 0 : l.slots;
  l.slot_len_bytes = raw ? l.slots : l.slots * 4;
  // The lane kernels address their outputs through the mirror's offsets too.
  l.dev_bytes = lane ? l.out_end : l.in_end + 16;
  return l;
}

// The layout, pinned: the kernels and the host agree on these bytes.
namespace small_layout_pins {
constexpr uint64_t kCtl = 64 + 8 * (1 + 1024);  // status words + one tile count + the scan's look-back tiles
constexpr SmallLayout kL1 = MakeSmallLayout(SmallKind::kLane, 1, 95, true, kCtl);
static_assert(kL1.off == 8448 && kL1.in == 8704 && kL1.tok == 8960 && kL1.ids == 9216 && kL1.len == 9728 &&
              kL1.out_end == 10108 && kL1.pub == 10240 && kL1.pin_bytes == 10496 && kL1.dev_bytes == 10108, "");
constexpr SmallLayout kL2 = MakeSmallLayout(SmallKind::kLane, 1, 95, false, kCtl);
static_assert(kL2.off == 8448 && kL2.in == 8704 && kL2.tok == 8960 && kL2.ids == 9216 && kL2.out_end == 9596 &&
              kL2.pub == 9728 && kL2.pin_bytes == 9984 && kL2.dev_bytes == 9596, "");
constexpr SmallLayout kL3 = MakeSmallLayout(SmallKind::kLane, 256, 0, true, kCtl);
static_assert(kL3.off == 8448 && kL3.in == 10752 && kL3.tok == 11008 && kL3.ids == 13312 && kL3.len == 13568 &&
              kL3.out_end == 13572 && kL3.pub == 13824 && kL3.pin_bytes == 14080, "");
constexpr SmallLayout kL4 = MakeSmallLayout(SmallKind::kLane, 17, 4000, true, kCtl);
static_assert(kL4.in == 8704 && kL4.tok == 12800 && kL4.ids == 13056 && kL4.len == 29184 && kL4.out_end == 45184 &&
              kL4.pub == 45312 && kL4.pin_bytes == 45568, "");
constexpr SmallLayout kC1 = MakeSmallLayout(SmallKind::kCoop, 1, 95);
static_assert(kC1.off == 0 && kC1.in == 256 && kC1.tok == 512 && kC1.ids == 768 && kC1.len == 1280 &&
              kC1.pub == 1792 && kC1.pin_bytes == 2048 && kC1.slots == 367 && kC1.dev_bytes == 367, "");
constexpr SmallLayout kC2 = MakeSmallLayout(SmallKind::kCoop, 16, 0);
static_assert(kC2.in == 256 && kC2.tok == 512 && kC2.ids == 768 && kC2.len == 1024 && kC2.pub == 1280 &&
              kC2.pin_bytes == 1536 && kC2.slots == 272, "");
constexpr SmallLayout kC3 = MakeSmallLayout(SmallKind::kCoop, 16, 3003);
static_assert(kC3.tok == 3328 && kC3.ids == 3584 && kC3.len == 15616 && kC3.pub == 27648 &&
              kC3.pin_bytes == 27904 && kC3.slots == 3275, "");
constexpr SmallLayout kR1 = MakeSmallLayout(SmallKind::kRaw, 1, 95);
static_assert(kR1.off == 0 && kR1.in == 256 && kR1.tok == 512 && kR1.ids == 768 && kR1.ids_cap == 452 &&
              kR1.slots == 452 && kR1.pub == 2816 && kR1.pin_bytes == 3072 && kR1.dev_bytes == 367, "");
constexpr SmallLayout kR2 = MakeSmallLayout(SmallKind::kRaw, 16, 0);
static_assert(kR2.in == 256 && kR2.tok == 512 && kR2.ids == 768 && kR2.ids_cap == 192 && kR2.pub == 1536 &&
              kR2.pin_bytes == 1792, "");
constexpr SmallLayout kR3 = MakeSmallLayout(SmallKind::kRaw, 16, 16384);
static_assert(kR3.tok == 16896 && kR3.ids == 17152 && kR3.ids_cap == 65728 && kR3.pub == 280064 &&
              kR3.pin_bytes == 280320, "");
constexpr SmallLayout kB1 = MakeSmallLayout(SmallKind::kBpe, 1, 95);
static_assert(kB1.off == 0 && kB1.in == 256 && kB1.tok == 512 && kB1.ids == 768 && kB1.len == 1280 &&
              kB1.pub == 1792 && kB1.pin_bytes == 2048 && kB1.slots == 367 && kB1.table_slots == 0 &&
              kB1.slot_len_bytes == 1468 && kB1.dev_bytes == 367 && kC1.table_slots == 367, "");
constexpr SmallLayout kB2 = MakeSmallLayout(SmallKind::kBpeRaw, 1, 95);
static_assert(kB2.off == 0 && kB2.in == 256 && kB2.tok == 512 && kB2.ids == 768 && kB2.ids_cap == 452 &&
              kB2.slots == 452 && kB2.table_slots == 0 && kB2.slot_len_bytes == 452 && kB2.pub == 2816 &&
              kB2.pin_bytes == 3072 && kB2.dev_bytes == 367 && kR1.table_slots == 452, "");
}  // namespace small_layout_pins

}  // namespace spm_amd
