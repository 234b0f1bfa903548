// C-ABI implementation (include/spm_hip.h): model load (ModelFactory::Create +
// InitializePieces + unigram::Model / bpe::Model constructors) and the batched
// encode entry points.
#include <hip/hip_runtime.h>

#include "scratch_cache.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/spm_hip.h"
#include "bpe_tables.h"
#include "dense.h"
#include "device_model.h"
#include "epilogue.h"
#include "host_nbest.h"
#include "kernels.h"
#include "normalize_device.h"
#include "normalizer.h"
#include "piece_table.h"
#include "sample_rng.h"
#include "shard_plan.h"
#include "small_layout.h"
#include "trace.h"

namespace {

thread_local std::string g_last_error;
uint32_t DefaultCoopMinNb();  // (below, with the encode plan)

int Fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

#define SPM_HIP_TRY(expr)                                                              \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return Fail(SPM_INTERNAL, std::string(#expr) + ": " + hipGetErrorString(_e));   \
  } while (0)

int CountChars(const std::string &s) {
  int n = 0;
  for (size_t i = 0; i < s.size();) {
    i += std::min<size_t>(spm_amd::OneCharLen(static_cast<uint8_t>(s[i])), s.size() - i);
    ++n;
  }
  return n;
}

template <typename T>
hipError_t Upload(spm_amd::DevBuf *buf, const std::vector<T> &v) {
  hipError_t e = buf->Reserve(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (e != hipSuccess) return e;
  if (v.empty()) return hipSuccess;
  return hipMemcpy(buf->ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// ModelInterface::InitializePieces (model_interface.cc:101-144).
int InitializePieces(spm_hip_model *m) {
  m->unk_id = -1;
  m->byte_fallback = m->proto.trainer_spec.byte_fallback;
  std::fill(m->byte_ids, m->byte_ids + 256, -1);
  for (size_t i = 0; i < m->proto.pieces.size(); ++i) {
    const auto &sp = m->proto.pieces[i];
    if (sp.piece.empty()) return Fail(SPM_INTERNAL, "piece must not be empty.");
    const bool normal = sp.type == spm_amd::kNormal || sp.type == spm_amd::kUserDefined ||
                        sp.type == spm_amd::kUnused;
    auto &dst = normal ? m->pieces : m->reserved;
    if (!dst.emplace(sp.piece, static_cast<int32_t>(i)).second)
      return Fail(SPM_INTERNAL, sp.piece + " is already defined.");
    if (sp.type == spm_amd::kUserDefined) m->user_defined.push_back(sp.piece);
    if (sp.type == spm_amd::kUnknown) {
      if (m->unk_id >= 0) return Fail(SPM_INTERNAL, "unk is already defined.");
      m->unk_id = static_cast<int32_t>(i);
    }
    // BYTE pieces (byte fallback) are reserved like CONTROL pieces; the byte
    // of a piece is its name's ("<0x41>"), not its position.
    if (sp.type == spm_amd::kBytePiece) {
      if (!m->byte_fallback)
        return Fail(SPM_INTERNAL, "byte piece " + sp.piece + " is found although `byte_fallback` is false.");
      const int byte = spm_amd::PieceToByte(sp.piece);
      if (byte < 0) return Fail(SPM_INTERNAL, "byte piece " + sp.piece + " is invalid.");
      m->byte_ids[byte] = static_cast<int32_t>(i);
    }
  }
  if (m->unk_id == -1) return Fail(SPM_INTERNAL, "unk is not defined.");
  if (m->byte_fallback)
    for (int b = 0; b < 256; ++b)
      if (m->byte_ids[b] < 0)
        return Fail(SPM_INTERNAL, "there are not 256 byte pieces although `byte_fallback` is true.");
  std::sort(m->user_defined.begin(), m->user_defined.end());
  return SPM_OK;
}

// Byte-pass score table: the node score (USER_DEFINED: length * max_score
// + 1.0, unigram_model.cc:589-591, length = the piece's char count), NaN
// for units that are no usable node (inner, empty, UNUSED).
std::vector<float> UsableNodeScores(const spm_hip_model *m, const std::vector<float> &scores) {
  std::vector<float> vbp(m->trie.units.size(), std::numeric_limits<float>::quiet_NaN());
  for (size_t u = 0; u < m->trie.units.size(); ++u) {
    if (!spm_amd::DoubleArray::Leaf(m->trie.units[u])) continue;
    const int32_t v = m->trie.values[u];
    const int32_t kind = v >> spm_amd::kKindShift;
    const int32_t id = v & spm_amd::kIdMask;
    if (kind == 0) {
      vbp[u] = scores[id];
    } else if (kind == spm_amd::kKindUserDefined) {
      const std::string &pc = m->proto.pieces[id].piece;
      const int chars = CountChars(pc.substr(0, pc.find('\0')));
      const float prod = static_cast<float>(chars) * m->max_score;
      vbp[u] = static_cast<float>(static_cast<double>(prod) + 1.0);
    }
  }
  return vbp;
}

// The byte kernel's piece -> (id, node score) table (piece_table.h), built
// from the trie so that a lookup answers exactly what the backtrace's exact
// -match walk answers: every piece's key (up to its first NUL) is walked, and
// the node reached is stored, once, if it is usable (non-NaN in vbp).  Each
// key is placed at one of its two hashed positions (cuckoo insertion; at a
// load of <= 1/2 a seed works with probability > 0.8, so seeds are retried
// and the capacity is doubled once), and the result is checked: every key
// must be found within kPieceProbes entry loads.  Empty on failure (the
// kernel then keeps its walk).
std::vector<uint32_t> BuildPieceTable(const spm_hip_model *m, const std::vector<float> &vbp) {
  using spm_amd::PieceEntry;
  const auto &units = m->trie.units;
  std::vector<PieceEntry> keys;
  std::vector<std::pair<uint32_t, std::string>> nodes;  // (node, key), by node: the order is the trie's
  for (const auto &kv : m->pieces) {
    const std::string key = kv.first.substr(0, kv.first.find('\0'));
    if (key.empty() || key.size() > spm_amd::kPieceKeyBytes) continue;
    uint32_t nbase = m->up.root_base, node = 0;
    bool found = true;
    for (const char ch : key) {
      const uint32_t c = static_cast<uint8_t>(ch);
      node = nbase ^ c;
      if (node >= units.size() || spm_amd::DoubleArray::Label(units[node]) != c) {
        found = false;
        break;
      }
      nbase = spm_amd::DoubleArray::Base(units[node]);
    }
    if (found && !std::isnan(vbp[node])) nodes.emplace_back(node, key);
  }
  std::sort(nodes.begin(), nodes.end());
  nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
  for (const auto &nk : nodes) {
    PieceEntry e{};
    spm_amd::PieceKey(reinterpret_cast<const uint8_t *>(nk.second.data()), static_cast<uint32_t>(nk.second.size()),
                      e.k);
    e.id = m->trie.values[nk.first] & spm_amd::kIdMask;
    e.score = vbp[nk.first];
    keys.push_back(e);
  }
  if (keys.empty()) return {};
  // The kernel loads a key's second position only when the first misses.
  // Keys go in by ascending score and a new key always takes its first
  // position (its holder moves on), so the frequent pieces end up there.
  std::stable_sort(keys.begin(), keys.end(),
                   [](const PieceEntry &x, const PieceEntry &y) { return x.score < y.score; });
  uint32_t cap0 = 16;
  while (cap0 < 2 * keys.size()) cap0 <<= 1;
  constexpr uint32_t kSeeds = 64, kMaxKicks = 512;
  for (uint32_t cap = cap0; cap <= 2 * cap0 && cap <= (1u << 18); cap <<= 1) {
    const uint32_t mask = cap - 1;
    for (uint32_t seed = 1; seed <= kSeeds; ++seed) {
      std::vector<int32_t> slot(cap, -1);
      auto pos_of = [&](int32_t i, uint32_t *p0, uint32_t *p1) {
        spm_amd::PieceHash(keys[i].k[0], keys[i].k[1], keys[i].k[2], keys[i].k[3], seed, mask, p0, p1);
      };
      bool ok = true;
      for (size_t i = 0; i < keys.size() && ok; ++i) {
        int32_t cur = static_cast<int32_t>(i);
        uint32_t p0, p1;
        pos_of(cur, &p0, &p1);
        uint32_t pos = p0;  // a new key takes its first position, whoever holds it
        ok = false;
        for (uint32_t kick = 0; kick < kMaxKicks; ++kick) {
          std::swap(cur, slot[pos]);
          if (cur < 0) {
            ok = true;
            break;
          }
          pos_of(cur, &p0, &p1);  // the evicted key goes to its other position
          pos = pos == p0 ? p1 : p0;
        }
      }
      if (!ok) continue;
      for (size_t i = 0; i < keys.size(); ++i) {  // a free first position is always better
        uint32_t p0, p1;
        pos_of(static_cast<int32_t>(i), &p0, &p1);
        if (slot[p0] < 0 && slot[p1] == static_cast<int32_t>(i)) std::swap(slot[p0], slot[p1]);
      }
      std::vector<uint32_t> img(8 * (static_cast<size_t>(cap) + 1), 0u);
      img[0] = mask;
      img[1] = seed;
      for (uint32_t p = 0; p < cap; ++p) {
        uint32_t *w = &img[8 * (static_cast<size_t>(p) + 1)];
        if (slot[p] < 0) {
          w[3] = spm_amd::kPieceEmpty;
          continue;
        }
        const PieceEntry &e = keys[slot[p]];
        std::memcpy(w, &e, sizeof(e));
      }
      // The probe bound, proven on the finished image with the lookup itself.
      for (const PieceEntry &e : keys) {
        int32_t id;
        float sc;
        if (!spm_amd::PieceTableFind(img.data(), e.k, &id, &sc) || id != e.id || std::memcmp(&sc, &e.score, 4) != 0) ok = false;
      }
      if (ok) return img;
    }
  }
  return {};
}

// Unigram state that follows the piece types (LoadUnigram, and again after
// spm_hip_model_set_piece_types): the piece-length bounds, the kernel tier
// and its switches, tie_mag, the usable-node scores and the byte kernel's
// piece table.  The trie, min_score / max_score and with them up.unk_score
// and up.max_score are the load's and are not touched (the reference keeps
// the model object it built at Load, sentencepiece_processor.cc:203-245).
// vbp: the usable-node scores (empty when the tier has no pair table).
void DeriveUnigram(spm_hip_model *m, std::vector<float> *vbp) {
  int max_chars = 0;
  size_t max_bytes = 0;
  bool split_ok = true;
  float tie_mag = 0.f;
  for (const auto &kv : m->pieces) {
    const int32_t id = kv.second;
    const int32_t type = m->proto.pieces[id].type;
    if (type != spm_amd::kUnused) {
      // C-string key semantics: count chars up to the first NUL.
      std::string k = kv.first.substr(0, kv.first.find('\0'));
      // Byte-position kernel precondition: the lead-byte chain ends exactly
      // at the end of the piece (no char cut by the piece boundary).
      size_t q = 0;
      while (q < k.size()) q += spm_amd::OneCharLen(static_cast<uint8_t>(k[q]));
      if (q != k.size()) split_ok = false;
      max_chars = std::max(max_chars, CountChars(k));
      max_bytes = std::max(max_bytes, k.size());
    }
    if (type == spm_amd::kNormal) tie_mag = std::max(tie_mag, std::fabs(m->proto.pieces[id].score));
  }
  m->max_piece_chars = max_chars;
  m->max_piece_bytes = static_cast<int32_t>(max_bytes);
  tie_mag = std::max(tie_mag, std::fabs(m->up.unk_score));
  tie_mag = std::max(tie_mag, std::fabs(static_cast<float>(max_chars) * m->max_score) + 1.0f);
  m->up.tie_mag = tie_mag + 1.0f;
  // The fast kernel's ring is indexed by byte distance: W > longest piece in bytes.
  m->ring_width = max_bytes < 16 ? 16 : max_bytes < 32 ? 32 : max_bytes < 64 ? 64 : 0;
  const std::vector<float> &scores = m->host_scores;
  bool nan_score = false;
  for (size_t u = 0; u < m->trie.units.size(); ++u) {
    if (!spm_amd::DoubleArray::Leaf(m->trie.units[u])) continue;
    const int32_t v = m->trie.values[u];
    if ((v >> spm_amd::kKindShift) == 0) nan_score |= std::isnan(scores[v & spm_amd::kIdMask]);
  }
  // The byte kernel (W = 16 byte-position pass, unigram_encode.hip) needs
  // pieces of < 16 bytes made of whole chars and no NaN score (NaN tags the
  // per-unit score table); other models with pieces of < 64 bytes run the
  // char kernel (values + scores tables), longer ones the general kernel.
  const bool byte_ok = m->ring_width == 16 && !nan_score && split_ok;
  // Wide-char pass: pieces of whole chars, < 16 chars and < 64 bytes (CJK
  // vocabularies, whose pieces outgrow the byte kernel's 16-byte ring); its
  // ring is indexed by chars (W = 16 chars).
  const bool wide_ok = !byte_ok && split_ok && !nan_score && max_chars < 16 && max_bytes < 64 &&
                       std::getenv("SPM_HIP_NO_WIDE") == nullptr;  // A/B knob
  m->kernel = byte_ok   ? spm_amd::UnigramKernel::kByte
              : wide_ok ? spm_amd::UnigramKernel::kWide
              : m->ring_width ? spm_amd::UnigramKernel::kChar : spm_amd::UnigramKernel::kGeneralOnly;
  if (wide_ok) m->ring_width = 16;
  // The wave-cooperative kernel walks the (unit, score) table, whose NaN
  // marks units without a usable node: models with a NaN score keep the
  // lane kernels' path.
  m->coop_min_nb = (nan_score || max_bytes > 56) ? 0u : DefaultCoopMinNb();
  const bool pair_table = byte_ok || wide_ok || (m->kernel == spm_amd::UnigramKernel::kChar && !nan_score);
  vbp->clear();
  if (pair_table) *vbp = UsableNodeScores(m, scores);
  m->piece_table.clear();
  if (byte_ok) m->piece_table = BuildPieceTable(m, *vbp);
}

// The (unit, score) table of the byte / wide / char / cooperative kernels.
int UploadUnitScores(spm_hip_model *m, const std::vector<float> &vbp) {
  // Empty units get label 0xFF so a walk needs no NUL test: real labels
  // are never 0 (keys stop at NUL) and a 0xFF input byte flags the sentence.
  // The root (unit 0, label 0) gets 0xFF too: a childless node has base 0,
  // so an input NUL after it would otherwise step onto the root and match.
  std::vector<uint32_t> ff = m->trie.units;
  for (size_t u = 1; u < ff.size(); ++u)
    if (ff[u] == 0) ff[u] = 0xFFu;
  if (!ff.empty()) ff[0] |= 0xFFu;
  // One (unit, score) pair per unit: the walk reads both with one 8-byte
  // gather per step.
  std::vector<uint32_t> uvs(2 * ff.size());
  for (size_t u = 0; u < ff.size(); ++u) {
    uvs[2 * u] = ff[u];
    std::memcpy(&uvs[2 * u + 1], &vbp[u], 4);
  }
  SPM_HIP_TRY(Upload(&m->d_uvs, uvs));
  return SPM_OK;
}

// The backtrace's piece table (A/B knob: SPM_HIP_NO_PIECE_TABLE leaves the
// pointer null and the kernel re-walks the trie).
int UploadPieceTable(spm_hip_model *m) {
  if (!m->piece_table.empty() && std::getenv("SPM_HIP_NO_PIECE_TABLE") == nullptr)
    SPM_HIP_TRY(Upload(&m->d_piece_tab, m->piece_table));
  else
    m->d_piece_tab.Release();
  return SPM_OK;
}

// unigram::Model::Model (unigram_model.cc:677-695) + BuildTrie (:624-673).
int LoadUnigram(spm_hip_model *m) {
  m->min_score = FLT_MAX;
  m->max_score = FLT_MIN;
  for (const auto &sp : m->proto.pieces)
    if (sp.type == spm_amd::kNormal) {
      m->min_score = std::min(m->min_score, sp.score);
      m->max_score = std::max(m->max_score, sp.score);
    }
  if (m->proto.pieces.size() >= static_cast<size_t>(spm_amd::kIdMask))
    return Fail(SPM_RESOURCE_EXHAUSTED, "too many pieces for the device trie");
  std::vector<std::pair<std::string, int32_t>> keys;
  keys.reserve(m->pieces.size());
  for (const auto &kv : m->pieces) {
    const int32_t id = kv.second;
    const int32_t type = m->proto.pieces[id].type;
    int32_t kind = 0;
    if (type == spm_amd::kUserDefined) kind = spm_amd::kKindUserDefined;
    if (type == spm_amd::kUnused) kind = spm_amd::kKindUnused;
    keys.emplace_back(kv.first, id | (kind << spm_amd::kKindShift));
  }
  if (keys.empty()) return Fail(SPM_INTERNAL, "no pieces are loaded.");
  std::string err;
  if (!spm_amd::BuildDoubleArray(std::move(keys), &m->trie, &err)) return Fail(SPM_RESOURCE_EXHAUSTED, err);
  if (m->trie.max_prefix_matches == 0) return Fail(SPM_INTERNAL, "no entry is found in the trie.");
  m->up.root_base = spm_amd::DoubleArray::Base(m->trie.units[0]);
  m->up.unk_id = m->unk_id;
  m->up.unk_score = m->min_score - 10.0f;  // kUnkPenalty (unigram_model.cc:563)
  m->up.max_score = m->max_score;
  m->up.trie_results_size = m->trie.max_prefix_matches;
  m->host_scores.resize(m->proto.pieces.size());
  for (size_t i = 0; i < m->host_scores.size(); ++i) m->host_scores[i] = m->proto.pieces[i].score;
  std::vector<float> vbp;
  DeriveUnigram(m, &vbp);
  if (m->host_only) return SPM_OK;
  SPM_HIP_TRY(Upload(&m->d_units, m->trie.units));
  SPM_HIP_TRY(Upload(&m->d_values, m->trie.values));
  SPM_HIP_TRY(Upload(&m->d_scores, m->host_scores));
  if (!vbp.empty()) {
    int rc = UploadUnitScores(m, vbp);
    if (rc == SPM_OK) rc = UploadPieceTable(m);
    if (rc != SPM_OK) return rc;
  }
  return SPM_OK;
}

// word::Model / character::Model (word_model.cc, char_model.cc): nothing but
// InitializePieces.  Encode is a split plus PieceToId, so the device needs
// one exact-match table from piece bytes to PieceToId(piece): reserved pieces
// (CONTROL, UNKNOWN) go in first, then NORMAL / USER_DEFINED / UNUSED ones
// (model_interface.cc:87-97).
int LoadWordChar(spm_hip_model *m) {
  std::vector<std::pair<const std::string *, int32_t>> keys;
  keys.reserve(m->reserved.size() + m->pieces.size());
  for (const auto &kv : m->reserved) keys.emplace_back(&kv.first, kv.second);
  for (const auto &kv : m->pieces)
    if (!m->reserved.count(kv.first)) keys.emplace_back(&kv.first, kv.second);
  // Map order is not deterministic across runs of the standard library; the
  // table image is (by id).
  std::sort(keys.begin(), keys.end(), [](const auto &a, const auto &b) { return a.second < b.second; });
  size_t max_bytes = 0, blob = 0;
  int max_chars = 0;
  for (const auto &k : keys) {
    max_bytes = std::max(max_bytes, k.first->size());
    max_chars = std::max(max_chars, CountChars(*k.first));
    blob += k.first->size();
  }
  if (blob > 0xFFFFFFFFull || keys.size() > (1u << 30))
    return Fail(SPM_RESOURCE_EXHAUSTED, "too many pieces for the device table");
  m->max_piece_chars = max_chars;
  m->max_piece_bytes = static_cast<int32_t>(max_bytes);
  m->wc_user_defined = !m->user_defined.empty();
  uint32_t cap = 16;
  while (cap < 2 * keys.size()) cap <<= 1;
  const uint32_t mask = cap - 1;
  m->wc_tab.assign(cap, spm_amd::WordCharEntry{0, 0, 0, 0});
  m->wc_keys.clear();
  m->wc_keys.reserve(blob + 1);
  for (const auto &k : keys) {
    const auto *s = reinterpret_cast<const uint8_t *>(k.first->data());
    const uint32_t len = static_cast<uint32_t>(k.first->size());
    const uint32_t h = spm_amd::WordCharHash(s, len);
    uint32_t slot = h & mask;
    while (m->wc_tab[slot].key_len != 0) slot = (slot + 1) & mask;
    const bool packed = len <= 4;  // the key itself, no blob bytes
    m->wc_tab[slot] = spm_amd::WordCharEntry{
        h, static_cast<uint32_t>(k.second),
        packed ? spm_amd::WordCharPack(s, len) : static_cast<uint32_t>(m->wc_keys.size()), len};
    if (!packed) m->wc_keys.insert(m->wc_keys.end(), s, s + len);
  }
  // Checked on the finished image with the lookup the kernels use.
  for (const auto &k : keys)
    if (spm_amd::WordCharFind(m->wc_tab.data(), mask, m->wc_keys.data(),
                              reinterpret_cast<const uint8_t *>(k.first->data()),
                              static_cast<uint32_t>(k.first->size()), -1) != k.second)
      return Fail(SPM_INTERNAL, "word/char piece table: a piece is not found");
  if (m->host_only) return SPM_OK;
  SPM_HIP_TRY(Upload(&m->d_wc_tab, m->wc_tab));
  SPM_HIP_TRY(Upload(&m->d_wc_keys, m->wc_keys));
  return SPM_OK;
}

// Fast-kernel timing: begin/end events of the workspace ring (created on
// first use); -1 when timing is off.
int TimedSlot(spm_hip_model *m, spm_amd::EncodeWorkspace *ws) {
  if (!m->timing) return -1;
  const int slot = static_cast<int>(ws->tcount % spm_amd::EncodeWorkspace::kTimingRing);
  for (int k = 0; k < 2; ++k)
    if (!ws->tev[2 * slot + k] && hipEventCreate(&ws->tev[2 * slot + k]) != hipSuccess) return -1;
  for (auto &e : ws->ev)
    if (!e && hipEventCreate(&e) != hipSuccess) return -1;
  ++ws->tcount;
  ws->last_slot = slot;
  return slot;
}

// Status words + look-back descriptors of one encode call, zeroed on the
// stream.  Returns the status pointer.
int PrepareControl(spm_amd::EncodeWorkspace *ws, uint64_t n, hipStream_t st, uint32_t **status) {
  const size_t bytes = spm_amd::kStWords * 4 + 8 * (spm_amd::FastTiles(n) + spm_amd::kScanTiles);
  SPM_HIP_TRY(ws->w_ctl.Reserve(bytes));
  SPM_HIP_TRY(hipMemsetAsync(ws->w_ctl.ptr, 0, bytes, st));
  *status = ws->w_ctl.as<uint32_t>();
  return SPM_OK;
}

constexpr uint32_t kGeneralLanes = 128;     // general-path lanes of the device-count pass
constexpr uint32_t kGeneralSmallNb = 2048;  // per-lane slab: sentences up to this many bytes

// Scratch of the literal-lattice tier (encode and SampleEncode carve the same
// slabs).  Device-count pass: the pool plan of a call of n sentences in `cap`
// bytes, its scratch and overflow list reserved.
int ReserveGeneralPool(const spm_hip_model *m, spm_amd::EncodeWorkspace *ws, uint64_t n, uint64_t cap,
                       spm_amd::GeneralPool *gp) {
  const int K = m->up.trie_results_size;
  *gp = spm_amd::PlanGeneralPool(cap, kGeneralLanes, kGeneralSmallNb,
                                 [&](uint32_t nb) { return spm_amd::UnigramGeneralSlabBytes(nb, K); });
  SPM_HIP_TRY(ws->w_scratch.Reserve(gp->pool));
  const uint64_t ovf_cap = std::min<uint64_t>(n, cap / (gp->small_nb + 1ull) + 1);
  SPM_HIP_TRY(ws->w_ovf.Reserve(ovf_cap * 4));
  return SPM_OK;
}

// Host-sized pass over n >= 1 sentences of <= max_nb bytes: gp->lanes slabs
// of gp->slab bytes, lanes halved while the scratch exceeds 4 GiB; reserved.
int ReserveHostSized(const spm_hip_model *m, spm_amd::EncodeWorkspace *ws, uint64_t n, uint32_t max_nb,
                     const char *too_long, spm_amd::GeneralPool *gp) {
  const uint64_t slab = spm_amd::UnigramGeneralSlabBytes(max_nb, m->up.trie_results_size);
  uint64_t threads = std::min<uint64_t>(n, 16384);
  while (threads > 64 && threads * slab > (4ull << 30)) threads /= 2;
  if (threads * slab > (16ull << 30)) return Fail(SPM_RESOURCE_EXHAUSTED, too_long);
  SPM_HIP_TRY(ws->w_scratch.Reserve(threads * slab));
  // One pass, no overflow pass: small_nb = big_nb = the longest sentence.
  *gp = spm_amd::GeneralPool{static_cast<uint32_t>(threads), max_nb, max_nb, slab, threads * slab};
  return SPM_OK;
}

// ... and its launch: every sentence of the call, no list and no overflow list.
spm_amd::GeneralLaunch HostSizedLaunch(spm_amd::EncodeWorkspace *ws, const spm_amd::GeneralPool &gp, uint64_t n,
                                       uint32_t *status, int32_t *s2, uint32_t *s2l) {
  return spm_amd::GeneralLaunch{nullptr, nullptr, n, ws->w_scratch.as<uint8_t>(), gp.slab, gp.small_nb, gp.lanes,
                                nullptr, nullptr, status + spm_amd::kStError, s2, s2l, ws->w_ntok.as<uint32_t>()};
}

// offsets[n] of a device batch (one small copy and wait).
int BatchBytes(spm_amd::EncodeWorkspace *ws, const uint64_t *d_off, uint64_t n, hipStream_t st, uint64_t *total) {
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned + 8, d_off + n, 8, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(total, ws->pinned + 8, 8);
  if (*total > 0xFFFFFFFFull * 4) return Fail(SPM_OUT_OF_RANGE, "batch too large");
  return SPM_OK;
}

int LongestSentence(const uint64_t *d_off, uint64_t n, hipStream_t st, uint32_t *max_nb) {
  *max_nb = 0;
  if (n == 0) return SPM_OK;
  std::vector<uint64_t> off(n + 1);
  SPM_HIP_TRY(hipMemcpyAsync(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  for (uint64_t i = 0; i < n; ++i) *max_nb = std::max<uint32_t>(*max_nb, static_cast<uint32_t>(off[i + 1] - off[i]));
  return SPM_OK;
}

// The tier counts and kernel times of a blocking call that has been waited
// for: `flagged` sentences left the fast tier, or all n when the call ran
// host-sized.  Publishes the call's stats.
int PublishTierStats(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, uint64_t n, bool host_sized, uint32_t flagged) {
  ws->stats.sentences = n;
  ws->stats.general_path = host_sized ? n : flagged;
  if (m->timing && ws->last_slot >= 0) {
    const int s = ws->last_slot;
    if (!host_sized) SPM_HIP_TRY(hipEventElapsedTime(&ws->stats.fast_kernel_ms, ws->tev[2 * s], ws->tev[2 * s + 1]));
    if (ws->stats.general_path) SPM_HIP_TRY(hipEventElapsedTime(&ws->stats.general_kernel_ms, ws->ev[0], ws->ev[1]));
    ws->tcount = 0;  // consumed here; the ring is for the asynchronous entry point
  }
  spm_amd::PublishStats(m, ws->stats);
  return SPM_OK;
}

// The device-count pass over (list, count): per-lane slabs first, the longer
// sentences then one at a time with the whole pool.  launch(GeneralLaunch)
// is the encode or the sample kernel's launcher.
template <typename Launch>
int LaunchFlaggedPair(spm_amd::EncodeWorkspace *ws, const spm_amd::GeneralPool &gp, const uint32_t *list,
                      const uint32_t *count, uint32_t *status, int32_t *s2, uint32_t *s2l, Launch launch) {
  uint8_t *scratch = ws->w_scratch.as<uint8_t>();
  uint32_t *ovf = ws->w_ovf.as<uint32_t>(), *ntok = ws->w_ntok.as<uint32_t>();
  uint32_t *novf = status + spm_amd::kStOverflow, *err = status + spm_amd::kStError;
  SPM_HIP_TRY(launch(spm_amd::GeneralLaunch{list, count, 0, scratch, gp.slab, gp.small_nb, gp.lanes, ovf, novf, err,
                                            s2, s2l, ntok}));
  SPM_HIP_TRY(launch(spm_amd::GeneralLaunch{ovf, novf, 0, scratch, gp.pool, gp.big_nb, 1, nullptr, nullptr, err, s2,
                                            s2l, ntok}));
  return SPM_OK;
}

// The two tiers of a blocking lattice call (SampleEncode, the entropy, sample
// and score): fast(status) over every sentence, exact(GeneralLaunch) over the
// sentences it flagged (device-count passes, no-ops when none was);
// force_general, or a flagged sentence too long for the device pool, runs
// the exact tier over every sentence with host-sized scratch.  too_long and
// broken: the caller's wording of the two failures.  Waits for the kernels
// and publishes the tier counts; the status words stay in w_ctl.
template <typename Fast, typename Exact>
int LatticeTiers(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint64_t *d_off, uint64_t n, uint64_t cap,
                 int32_t *s2, uint32_t *s2l, const char *too_long, const char *broken, hipStream_t st, Fast fast,
                 Exact exact) {
  bool host_sized = m->force_general;
  uint32_t flagged = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    uint32_t *status = nullptr;
    int rc = PrepareControl(ws, n, st, &status);
    if (rc != SPM_OK) return rc;
    const bool timing = TimedSlot(m, ws) >= 0;
    spm_amd::GeneralPool gp;
    if (host_sized) {
      uint32_t max_nb = 0;
      rc = LongestSentence(d_off, n, st, &max_nb);
      if (rc != SPM_OK) return rc;
      rc = ReserveHostSized(m, ws, n, std::max<uint32_t>(max_nb, 1), too_long, &gp);
      if (rc != SPM_OK) return rc;
      if (timing) SPM_HIP_TRY(hipEventRecord(ws->ev[0], st));
      SPM_HIP_TRY(exact(HostSizedLaunch(ws, gp, n, status, s2, s2l)));
      if (timing) SPM_HIP_TRY(hipEventRecord(ws->ev[1], st));
    } else {
      SPM_HIP_TRY(ws->w_flagged.Reserve(n * 4));
      rc = ReserveGeneralPool(m, ws, n, cap, &gp);
      if (rc != SPM_OK) return rc;
      const int slot = ws->last_slot;
      if (timing) SPM_HIP_TRY(hipEventRecord(ws->tev[2 * slot], st));
      SPM_HIP_TRY(fast(status));
      if (timing) SPM_HIP_TRY(hipEventRecord(ws->tev[2 * slot + 1], st));
      if (timing) SPM_HIP_TRY(hipEventRecord(ws->ev[0], st));
      rc = LaunchFlaggedPair(ws, gp, ws->w_flagged.as<uint32_t>(), status + spm_amd::kStFlagged, status, s2, s2l,
                             exact);
      if (rc != SPM_OK) return rc;
      if (timing) SPM_HIP_TRY(hipEventRecord(ws->ev[1], st));
    }
    SPM_HIP_TRY(hipMemcpyAsync(ws->pinned, status, 4 * (spm_amd::kStError + 1), hipMemcpyDeviceToHost, st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
    flagged = ws->pinned[spm_amd::kStFlagged];
    const uint32_t err = ws->pinned[spm_amd::kStError];
    if (err == 0) break;
    // Bit 0: a flagged sentence outgrew the device pool; anything else is a
    // broken walk, which a second run would only repeat.
    if (host_sized || err != 1u) return Fail(SPM_INTERNAL, broken);
    host_sized = true;
  }
  return PublishTierStats(m, ws, n, host_sized, flagged);
}

// Dense CSR output from the right-aligned slots and w_ntok: LaunchCompact's
// size query, its scan scratch, then the real call.
int CompactSlots(spm_amd::EncodeWorkspace *ws, const uint64_t *off, uint64_t n, const int32_t *slot_ids,
                 const uint32_t *slot_len, int32_t *ids, uint32_t *len, uint64_t *tok, const uint32_t *status,
                 uint32_t *out_status, hipStream_t st) {
  const uint32_t *ntok = ws->w_ntok.as<uint32_t>();
  size_t tmp = 0;
  SPM_HIP_TRY(spm_amd::LaunchCompact(off, n, ntok, slot_ids, slot_len, ids, len, tok, nullptr, &tmp, status,
                                     out_status, st));
  SPM_HIP_TRY(ws->w_scan.Reserve(tmp + 16));
  SPM_HIP_TRY(spm_amd::LaunchCompact(off, n, ntok, slot_ids, slot_len, ids, len, tok, ws->w_scan.ptr, &tmp, status,
                                     out_status, st));
  return SPM_OK;
}

spm_amd::UnigramLaunch UnigramTables(spm_hip_model *m, const spm_amd::EncodeCall &c, uint32_t *status) {
  const bool byte_k = m->kernel == spm_amd::UnigramKernel::kByte || m->kernel == spm_amd::UnigramKernel::kWide;
  spm_amd::UnigramLaunch l{};
  l.bytes = c.bytes;
  l.off = c.off;
  l.n = c.n;
  l.capacity = c.capacity;
  l.units = byte_k ? m->d_uvs.as<uint32_t>() : m->d_units.as<uint32_t>();
  l.gen_units = m->d_units.as<uint32_t>();
  l.values = m->d_values.as<int32_t>();
  l.scores = m->d_scores.as<float>();
  l.num_units = static_cast<uint32_t>(m->trie.units.size());
  l.piece_tab = m->d_piece_tab.as<uint32_t>();
  if (l.piece_tab) {
    l.piece_mask = m->piece_table[0];
    l.piece_seed = m->piece_table[1];
  }
  l.p = m->up;
  l.ids = c.ids;
  l.len = c.len;
  l.tok_off = c.tok;
  l.status = status;
  l.corrupt_bp = m->corrupt_bp.load();
  l.chain = c.out_status;
  return l;
}


// Unigram fast path: no host synchronization.  Fast kernel (dense output),
// then the device-count general passes and the fix-up chain, which do
// nothing unless the fast kernel flagged a sentence.
// One fast-path unigram encode, in two parts: A = the fast kernel (+ the
// tile compaction), B = the general kernel over the flagged sentences + the
// fix-up chain (device no-ops when nothing was flagged).
struct FastPlan {
  spm_amd::UnigramLaunch l;
  spm_amd::GeneralPool gp;
  uint32_t *status = nullptr;
  uint64_t *desc = nullptr;
  int slot = -1;
  bool coop = false;  // long sentences: the wave-cooperative kernel before the general one
  uint64_t slab_chars = 0;  // CoopArgs::slab_chars
  uint32_t coop_blocks = 0;
};

// The wave-cooperative kernel takes the wide / char kernels' sentences of at
// least kCoopMinNb bytes (SPM_HIP_COOP=0 turns it off, SPM_HIP_COOP_MIN_NB
// moves the threshold; A/B knobs).  The byte kernel (short-piece models, the
// c2 path) keeps every sentence.
uint32_t DefaultCoopMinNb() {
  static const bool on = [] {
    const char *e = std::getenv("SPM_HIP_COOP");
    return !(e && std::atoi(e) == 0);
  }();
  static const uint32_t min_nb = [] {
    const char *e = std::getenv("SPM_HIP_COOP_MIN_NB");
    return e ? static_cast<uint32_t>(std::max(1, std::atoi(e))) : 128u;
  }();
  return on ? min_nb : 0u;
}

// Grid cap of the list kernel (SPM_HIP_COOP_BLOCKS: A/B knob, read per call).
uint32_t CoopMaxBlocks() {
  const char *e = std::getenv("SPM_HIP_COOP_BLOCKS");
  const int v = e ? std::atoi(e) : 0;
  return v > 0 ? static_cast<uint32_t>(v) : spm_amd::kCoopMaxBlocks;
}

// The list kernel takes its sentences from a work queue, long ones first
// (SPM_HIP_COOP_QUEUE=0: static grid stride over the flagged list; A/B knob).
bool CoopQueue() {
  static const bool on = [] {
    const char *e = std::getenv("SPM_HIP_COOP_QUEUE");
    return !(e && std::atoi(e) == 0);
  }();
  return on;
}

uint32_t CoopMinNb(const spm_hip_model *m) {
  if (m->kernel != spm_amd::UnigramKernel::kWide && m->kernel != spm_amd::UnigramKernel::kChar) return 0;
  return m->coop_min_nb.load();
}

// SPM_HIP_COOP_PROF (debug): a cooperative kernel's phase cycles to stderr.
// CoopProfiled runs `launch` with zeroed counters on `st` and waits for it.
bool CoopProf() {
  static const bool on = std::getenv("SPM_HIP_COOP_PROF") != nullptr;
  return on;
}

template <typename Launch>
int CoopProfiled(hipStream_t st, Launch launch) {
  uint64_t *prof = nullptr, h[8];
  SPM_HIP_TRY(spm_amd::DevMalloc(&prof, 64));
  SPM_HIP_TRY(hipMemsetAsync(prof, 0, 64, st));
  SPM_HIP_TRY(launch(prof));
  SPM_HIP_TRY(hipMemcpyAsync(h, prof, 64, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  (void)spm_amd::DevFree(prof);
  std::fprintf(stderr, "coop prof: setup %llu lattice %llu viterbi %llu backtrace %llu ids %llu cycles; "
               "bytes %llu chars %llu tokens %llu\n", (unsigned long long)h[0], (unsigned long long)h[1],
               (unsigned long long)h[2], (unsigned long long)h[3], (unsigned long long)h[4],
               (unsigned long long)h[5], (unsigned long long)h[6], (unsigned long long)h[7]);
  return SPM_OK;
}

// Work buffers and launch tables; `status` = a zeroed control block of
// PrepareControl's size (nullptr: PrepareControl zeroes the workspace's).
int FastSetup(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EncodeCall &c, uint32_t *status,
              FastPlan *fp) {
  const uint64_t n = c.n, cap = std::max<uint64_t>(c.capacity, 1), nn = std::max<uint64_t>(n, 1);
  const hipStream_t st = c.st;
  if (!status) {
    int rc = PrepareControl(ws, n, st, &status);
    if (rc != SPM_OK) return rc;
  }
  fp->status = status;
  fp->desc = reinterpret_cast<uint64_t *>(status + spm_amd::kStWords);
  SPM_HIP_TRY(ws->w_bp.Reserve(cap + 16));
  SPM_HIP_TRY(ws->w_flagged.Reserve(nn * 4));
  SPM_HIP_TRY(ws->w_ntok.Reserve(nn * 4));
  SPM_HIP_TRY(ws->w_cnt.Reserve(nn * 4));
  SPM_HIP_TRY(ws->w_slot2_ids.Reserve(cap * 4));
  if (c.len) SPM_HIP_TRY(ws->w_slot2_len.Reserve(cap * 4));
  const int rc = ReserveGeneralPool(m, ws, nn, cap, &fp->gp);
  if (rc != SPM_OK) return rc;
  fp->l = UnigramTables(m, c, status);
  fp->l.bp = ws->w_bp.as<uint8_t>();
  if (m->kernel == spm_amd::UnigramKernel::kWide) {
    SPM_HIP_TRY(ws->w_bpn.Reserve((cap + 16) * 4));
    fp->l.bpn = ws->w_bpn.as<uint32_t>();
  }
  fp->l.flagged = ws->w_flagged.as<uint32_t>();
  fp->l.tile_count = fp->desc;
  SPM_HIP_TRY(ws->w_slot_ids.Reserve(cap * 4));
  if (c.len) SPM_HIP_TRY(ws->w_slot_len.Reserve(cap * 4));
  SPM_HIP_TRY(ws->w_tprefix.Reserve((spm_amd::FastTiles(n) + 1) * 8));
  fp->l.slot_ids = ws->w_slot_ids.as<int32_t>();
  fp->l.slot_len = c.len ? ws->w_slot_len.as<uint32_t>() : nullptr;
  fp->l.coop_min_nb = CoopMinNb(m);
  fp->coop = fp->l.coop_min_nb != 0;
  if (fp->coop) {
    // Cooperative-kernel rows (kCoopSlots x 6 B per char): by byte offset
    // when the call is small, else one slab per wave of the list kernel's
    // grid (bounded whatever the call's size).
    const uint64_t slab = m->coop_slab_chars.load();
    fp->coop_blocks = spm_amd::CoopBlocks(n, CoopMaxBlocks());
    const uint64_t slab_rows = uint64_t{fp->coop_blocks} * 4 * slab;
    const int mode = m->coop_slab_mode.load();
    fp->slab_chars = mode == 1 || (mode == 0 && slab_rows < cap + 64) ? slab : 0;
    const uint64_t rows = fp->slab_chars ? slab_rows : cap + 64;
    SPM_HIP_TRY(ws->w_cpv.Reserve(rows * spm_amd::kCoopSlots * 2));
    SPM_HIP_TRY(ws->w_cnd.Reserve(rows * spm_amd::kCoopSlots * 4));
    SPM_HIP_TRY(ws->w_crest.Reserve(nn * 4));
    if (CoopQueue()) SPM_HIP_TRY(ws->w_cpart.Reserve(nn * 4));
  }
  return SPM_OK;
}

// Part A.  compact = false: one tile whose slots start at byte 0
// (FastTiles(n) == 1 and off[0] == 0) writes the final ids / lengths /
// token offsets itself (slots = the outputs, see EncodeHostSmall).
int FastPartA(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EncodeCall &c, FastPlan *fp,
              bool compact) {
  const hipStream_t st = c.st;
  if (!compact) {
    fp->l.slot_ids = c.ids;
    fp->l.slot_len = c.len;
  }
  fp->slot = TimedSlot(m, ws);
  if (fp->slot >= 0) SPM_HIP_TRY(hipEventRecord(ws->tev[2 * fp->slot], st));
  SPM_HIP_TRY(spm_amd::LaunchUnigramFast(m->kernel, m->ring_width, fp->l, st));
  if (fp->slot >= 0) SPM_HIP_TRY(hipEventRecord(ws->tev[2 * fp->slot + 1], st));
  if (compact) {
    size_t tb = 0;
    SPM_HIP_TRY(spm_amd::LaunchTileCompact(c.off, c.n, fp->desc, ws->w_tprefix.as<uint64_t>(), fp->l.slot_ids,
                                           fp->l.slot_len, c.ids, c.len, c.tok, nullptr, &tb, fp->status, st));
    SPM_HIP_TRY(ws->w_scan.Reserve(tb + 16));
    SPM_HIP_TRY(spm_amd::LaunchTileCompact(c.off, c.n, fp->desc, ws->w_tprefix.as<uint64_t>(), fp->l.slot_ids,
                                           fp->l.slot_len, c.ids, c.len, c.tok, ws->w_scan.ptr, &tb, fp->status,
                                           st));
  }
  return SPM_OK;
}

// Part B.
int FastPartB(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EncodeCall &c, FastPlan *fp) {
  const hipStream_t st = c.st;
  const uint64_t n = c.n;
  uint32_t *status = fp->status;
  int32_t *s2 = ws->w_slot2_ids.as<int32_t>();
  uint32_t *s2l = c.len ? ws->w_slot2_len.as<uint32_t>() : nullptr;
  if (fp->slot >= 0) SPM_HIP_TRY(hipEventRecord(ws->ev[0], st));
  // Flagged sentences first go through the wave-cooperative kernel (the long
  // ones the wide / char kernels routed there, and any other it can take);
  // the general kernel gets what it leaves.
  const uint32_t *glist = fp->l.flagged, *gcount = status + spm_amd::kStFlagged;
  if (fp->coop) {
    spm_amd::CoopArgs ca{c.bytes, c.off, m->d_uvs.as<uint32_t>(), m->d_values.as<int32_t>(),
                         static_cast<uint32_t>(m->trie.units.size()), m->up,
                         fp->l.flagged, status + spm_amd::kStFlagged, 0, s2, s2l, ws->w_ntok.as<uint32_t>(),
                         ws->w_crest.as<uint32_t>(), status + spm_amd::kStCoopRest, ws->w_cpv.as<uint16_t>(),
                         ws->w_cnd.as<uint32_t>(), static_cast<uint32_t>(std::max(m->max_piece_bytes, 4)),
                         fp->l.chain, nullptr, fp->slab_chars};
    if (CoopQueue()) {
      ca.queue = status + spm_amd::kStCoopQueue;
      ca.part = ws->w_cpart.as<uint32_t>();
      ca.part_long = status + spm_amd::kStCoopLong;
      ca.part_n = n;
      SPM_HIP_TRY(spm_amd::LaunchCoopPartition(fp->l.flagged, status + spm_amd::kStFlagged, c.off, n,
                                               ws->w_cpart.as<uint32_t>(), status + spm_amd::kStCoopLong,
                                               status + spm_amd::kStCoopShort, st));
    }
    const uint64_t blocks = fp->coop_blocks;
    if (CoopProf()) {
      const int rc = CoopProfiled(st, [&](uint64_t *prof) {
        ca.prof = prof;
        return spm_amd::LaunchCoopEncode(ca, static_cast<uint32_t>(blocks), st);
      });
      if (rc != SPM_OK) return rc;
    } else {
      SPM_HIP_TRY(spm_amd::LaunchCoopEncode(ca, static_cast<uint32_t>(blocks), st));
    }
    glist = ws->w_crest.as<uint32_t>();
    gcount = status + spm_amd::kStCoopRest;
  }
  const int rc = LaunchFlaggedPair(ws, fp->gp, glist, gcount, status, s2, s2l, [&](const spm_amd::GeneralLaunch &g) {
    return spm_amd::LaunchUnigramGeneral(fp->l, g, st);
  });
  if (rc != SPM_OK) return rc;
  if (fp->slot >= 0) SPM_HIP_TRY(hipEventRecord(ws->ev[1], st));
  spm_amd::FixupLaunch f{c.off, n, c.ids, c.len, c.tok, s2, s2l, ws->w_ntok.as<uint32_t>(),
                         ws->w_cnt.as<uint32_t>(), status, fp->desc + spm_amd::FastTiles(n), c.out_status};
  SPM_HIP_TRY(spm_amd::LaunchEncodeFixup(f, st));
  return SPM_OK;
}

int EncodeUnigramFast(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EncodeCall &c) {
  if (c.n == 0) {
    SPM_HIP_TRY(hipMemsetAsync(c.tok, 0, sizeof(uint64_t), c.st));
    return SPM_OK;
  }
  FastPlan fp;
  int rc = FastSetup(m, ws, c, nullptr, &fp);
  if (rc == SPM_OK) rc = FastPartA(m, ws, c, &fp, true);
  if (rc == SPM_OK) rc = FastPartB(m, ws, c, &fp);
  return rc;
}

// General kernel over every sentence with host-sized scratch (models with
// pieces of >= 64 bytes, force_general, and the re-run after a device-path
// overflow): the reference lattice literally, then scan + compaction.
int EncodeUnigramAll(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EncodeCall &c) {
  const uint64_t n = c.n, cap = std::max<uint64_t>(c.capacity, 1), nn = std::max<uint64_t>(n, 1);
  const hipStream_t st = c.st;
  uint32_t *status = nullptr;
  int rc = PrepareControl(ws, n, st, &status);
  if (rc != SPM_OK) return rc;
  spm_amd::GeneralPool gp;
  rc = ReserveHostSized(m, ws, nn, std::max<uint32_t>(c.max_nb, 1), "sentence too long for the general encode path",
                        &gp);
  if (rc != SPM_OK) return rc;
  SPM_HIP_TRY(ws->w_slot2_ids.Reserve(cap * 4));
  if (c.len) SPM_HIP_TRY(ws->w_slot2_len.Reserve(cap * 4));
  SPM_HIP_TRY(ws->w_ntok.Reserve(nn * 4));
  spm_amd::UnigramLaunch l = UnigramTables(m, c, status);
  int32_t *s2 = ws->w_slot2_ids.as<int32_t>();
  uint32_t *s2l = c.len ? ws->w_slot2_len.as<uint32_t>() : nullptr;
  const bool timing = TimedSlot(m, ws) >= 0;
  if (timing) SPM_HIP_TRY(hipEventRecord(ws->ev[0], st));
  SPM_HIP_TRY(spm_amd::LaunchUnigramGeneral(l, HostSizedLaunch(ws, gp, n, status, s2, s2l), st));
  if (timing) SPM_HIP_TRY(hipEventRecord(ws->ev[1], st));
  return CompactSlots(ws, c.off, n, s2, s2l, c.ids, c.len, c.tok, status, c.out_status, st);
}

bool WordCharModel(const spm_hip_model *m) {
  return m->model_type == spm_amd::kWord || m->model_type == spm_amd::kChar;
}

// The general tier takes every sentence of a CHAR model with USER_DEFINED
// pieces (PrefixMatch is sequential) and everything under force_general.
bool WordCharAllGeneral(const spm_hip_model *m) {
  return m->force_general || (m->model_type == spm_amd::kChar && m->wc_user_defined);
}

int EnsureNormTables(spm_hip_model *m);  // (below)

// WORD / CHAR encode: a pure stream call in both tiers (nothing is sized
// from the sentences; every buffer follows c.capacity and c.n).
int EncodeWordChar(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EncodeCall &c) {
  const hipStream_t st = c.st;
  if (spm_amd::WordCharTiles(c.capacity) >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "batch too large");
  if (c.n == 0) {
    uint32_t *status = nullptr;
    const int rc = PrepareControl(ws, 0, st, &status);
    if (rc != SPM_OK) return rc;
    SPM_HIP_TRY(spm_amd::LaunchWordCharEmpty(c.tok, c.out_status, st));
    return SPM_OK;
  }
  const bool all = WordCharAllGeneral(m);
  const bool ud = m->model_type == spm_amd::kChar && m->wc_user_defined;
  if (ud) {
    const int rc = EnsureNormTables(m);
    if (rc != SPM_OK) return rc;
  }
  uint32_t *status = nullptr;
  int rc = PrepareControl(ws, c.n, st, &status);
  if (rc != SPM_OK) return rc;
  spm_amd::WordCharLaunch l{};
  l.bytes = c.bytes;
  l.off = c.off;
  l.n = c.n;
  l.capacity = c.capacity;
  l.tiles = spm_amd::WordCharTiles(c.capacity);
  l.word = m->model_type == spm_amd::kWord ? 1 : 0;
  l.tab = m->d_wc_tab.as<uint32_t>();
  l.tab_mask = static_cast<uint32_t>(m->wc_tab.size() - 1);
  l.keys = m->d_wc_keys.as<uint8_t>();
  l.max_piece_bytes = static_cast<uint32_t>(m->max_piece_bytes);
  l.unk_id = m->unk_id;
  l.ud_units = ud ? m->d_ud_units.as<uint32_t>() : nullptr;
  l.ud_num_units = ud ? m->ud_units_n : 0;
  SPM_HIP_TRY(ws->w_bp.Reserve(l.tiles * spm_amd::kWcTile));
  SPM_HIP_TRY(ws->w_cnt.Reserve(c.n * 4));
  SPM_HIP_TRY(ws->w_flagged.Reserve(c.n * 4));
  SPM_HIP_TRY(ws->w_wc_count.Reserve(l.tiles * 4));
  SPM_HIP_TRY(ws->w_wc_first.Reserve(l.tiles * 4));
  SPM_HIP_TRY(ws->w_wc_sent.Reserve(l.tiles * 4));
  SPM_HIP_TRY(ws->w_wc_next.Reserve(l.tiles * 8));
  SPM_HIP_TRY(ws->w_tprefix.Reserve((l.tiles + 1) * 8));
  l.mark = ws->w_bp.as<uint8_t>();
  l.sflag = ws->w_cnt.as<uint32_t>();
  l.flagged = ws->w_flagged.as<uint32_t>();
  l.status = status;
  l.tile_count = ws->w_wc_count.as<uint32_t>();
  l.tile_first = ws->w_wc_first.as<uint32_t>();
  l.tile_prefix = ws->w_tprefix.as<uint64_t>();
  l.tile_sent = ws->w_wc_sent.as<uint32_t>();
  l.tile_next = ws->w_wc_next.as<uint64_t>();
  l.ids = c.ids;
  l.len = c.len;
  l.tok_off = c.tok;
  l.chain = c.out_status;
  l.out_status = c.out_status;
  SPM_HIP_TRY(spm_amd::LaunchWordCharSentences(l, st));
  const int slot = TimedSlot(m, ws);
  if (slot >= 0) SPM_HIP_TRY(hipEventRecord(ws->tev[2 * slot], st));
  if (!all) {
    SPM_HIP_TRY(hipMemsetAsync(l.sflag, 0, c.n * 4, st));
    SPM_HIP_TRY(spm_amd::LaunchWordCharTile(l, st));
  }
  if (slot >= 0) {
    SPM_HIP_TRY(hipEventRecord(ws->tev[2 * slot + 1], st));
    SPM_HIP_TRY(hipEventRecord(ws->ev[0], st));
  }
  SPM_HIP_TRY(spm_amd::LaunchWordCharGeneral(l, all, st));
  if (slot >= 0) SPM_HIP_TRY(hipEventRecord(ws->ev[1], st));
  SPM_HIP_TRY(spm_amd::LaunchWordCharOutput(l, st));
  return SPM_OK;
}

// WORD / CHAR models never need host-sized scratch, force_general included.
bool NeedsHostSized(const spm_hip_model *m) {
  if (WordCharModel(m)) return false;
  if (m->force_general) return true;
  if (m->model_type == spm_amd::kUnigram) return m->kernel == spm_amd::UnigramKernel::kGeneralOnly;
  return m->bpe.has_user_defined;
}

// Enqueues one encode (no synchronization unless c.host_sized).
int EncodeEnqueue(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EncodeCall &c) {
  if (WordCharModel(m)) return EncodeWordChar(m, ws, c);
  if (m->model_type == spm_amd::kUnigram)
    return c.host_sized ? EncodeUnigramAll(m, ws, c) : EncodeUnigramFast(m, ws, c);
  return spm_amd::EncodeBpe(m, ws, c, &g_last_error);
}

// Blocking encode on a leased workspace (spm_hip_encode_batch and the host
// and SentencePieceText entry points): reads offsets[n], enqueues the
// encode, waits, and reports the status the reference's Encode would return.
// A flagged sentence too long for the device general pass (kStError) makes
// it re-run the batch with host-sized scratch.
// drop (BPE models): SampleEncode with BPE-dropout instead of Encode.
int EncodeBlocking(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *d_bytes, const uint64_t *d_off,
                   uint64_t n, int32_t *d_ids, uint32_t *d_len, uint64_t *d_tok, hipStream_t st,
                   const spm_amd::BpeDropout *drop = nullptr) {
  uint64_t total = 0;
  int rc = BatchBytes(ws, d_off, n, st, &total);
  if (rc != SPM_OK) return rc;
  spm_amd::EncodeCall c{d_bytes, d_off, n, total, d_ids, d_len, d_tok, nullptr, st, NeedsHostSized(m), 0, drop};
  if (c.host_sized && (rc = LongestSentence(d_off, n, st, &c.max_nb)) != SPM_OK) return rc;
  ws->stats = spm_hip_encode_stats{};
  if ((rc = EncodeEnqueue(m, ws, c)) != SPM_OK) return rc;
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned, ws->w_ctl.ptr, 4 * (spm_amd::kStCoopRest + 1), hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  uint32_t flagged = ws->pinned[spm_amd::kStFlagged], err = ws->pinned[spm_amd::kStError];
  if (err && !c.host_sized) {
    c.host_sized = true;
    rc = LongestSentence(d_off, n, st, &c.max_nb);
    if (rc == SPM_OK) rc = EncodeEnqueue(m, ws, c);
    if (rc != SPM_OK) return rc;
    SPM_HIP_TRY(hipMemcpyAsync(ws->pinned, ws->w_ctl.ptr, 4 * (spm_amd::kStCoopRest + 1), hipMemcpyDeviceToHost,
                               st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
    err = ws->pinned[spm_amd::kStError];
  }
  if (err) return Fail(SPM_INTERNAL, "general encode path: scratch overflow");
  ws->stats.coop_rest = c.host_sized ? 0 : ws->pinned[spm_amd::kStCoopRest];
  return PublishTierStats(m, ws, n, c.host_sized, flagged);
}

// Lazy device tables of the normalizer (charsmap blob, user-defined trie).
int EnsureNormTables(spm_hip_model *m) {
  if (m->norm_ready) return SPM_OK;
  std::lock_guard<std::mutex> g(m->init_mu);
  if (m->norm_ready) return SPM_OK;
  const std::string &blob = m->proto.normalizer_spec.precompiled_charsmap;
  if (!blob.empty()) {
    uint32_t tsize = 0;
    if (blob.size() <= 4) return Fail(SPM_INTERNAL, "Blob for normalization rule is broken.");
    std::memcpy(&tsize, blob.data(), 4);
    if (tsize >= blob.size() || tsize < 4) return Fail(SPM_INTERNAL, "Blob for normalization rule is broken.");
    // The blob plus one NUL: a replacement string the blob leaves
    // unterminated ends there (NormalizePrefix's scan never leaves the copy).
    SPM_HIP_TRY(m->d_charsmap.Reserve(blob.size() + 1));
    SPM_HIP_TRY(hipMemcpy(m->d_charsmap.ptr, blob.data(), blob.size(), hipMemcpyHostToDevice));
    SPM_HIP_TRY(hipMemset(m->d_charsmap.as<uint8_t>() + blob.size(), 0, 1));
  }
  if (!m->user_defined.empty()) {
    std::vector<std::pair<std::string, int32_t>> keys;
    for (const auto &u : m->user_defined) keys.emplace_back(u, 1);
    spm_amd::DoubleArray da;
    std::string err;
    if (!spm_amd::BuildDoubleArray(keys, &da, &err)) return Fail(SPM_INTERNAL, err);
    SPM_HIP_TRY(Upload(&m->d_ud_units, da.units));
    m->ud_units_n = static_cast<uint32_t>(da.units.size());
  }
  m->norm_ready = true;
  return SPM_OK;
}

// The decode table (decode.h) of SentencePieceProcessor::Decode
// (sentencepiece_processor.cc:670-716).  Decode(ids) maps an id to its piece
// and the piece back to an id (PieceToId: reserved pieces first), so the type
// that decides the surface is that of PieceToId(IdToPiece(id)).
int BuildDecodeTable(spm_hip_model *m) {
  static const char kSpace[] = "\xE2\x96\x81";  // U+2581
  const auto &ts = m->proto.trainer_spec;
  const std::string unk_surface = ts.has_unk_surface ? ts.unk_surface : std::string(" \xE2\x81\x87 ");
  spm_amd::DecodeTable &t = m->decode;
  const size_t v = m->proto.pieces.size();
  t.meta.assign(v, 0);
  t.off.assign(v, 0);
  t.bytes.clear();
  t.max_surface = 0;
  t.has_bytes = false;
  for (size_t i = 0; i < v; ++i) {
    const std::string &piece = m->proto.pieces[i].piece;
    int32_t id = static_cast<int32_t>(i);
    auto r = m->reserved.find(piece);
    if (r != m->reserved.end()) id = r->second;
    const int32_t type = m->proto.pieces[id].type;
    std::string surface;
    uint32_t strip = 0;
    if (type == spm_amd::kControl) {
    } else if (type == spm_amd::kBytePiece) {
      // No table surface: it follows from the byte run around the token
      // (decode.h, ByteRunSurface).  At most 4 bytes.
      t.meta[i] = spm_amd::kDecodeByteFlag | static_cast<uint32_t>(spm_amd::PieceToByte(piece));
      t.off[i] = static_cast<uint32_t>(t.bytes.size());
      t.max_surface = std::max<uint32_t>(t.max_surface, 4);
      t.has_bytes = true;
      continue;
    } else if (type == spm_amd::kUnknown) {
      surface = unk_surface;
    } else {
      strip = piece.compare(0, 3, kSpace) == 0 ? 1u : 0u;
      for (size_t k = 0; k < piece.size();) {
        if (piece.compare(k, 3, kSpace) == 0) {
          surface.push_back(' ');
          k += 3;
        } else {
          surface.push_back(piece[k++]);
        }
      }
    }
    if (surface.size() > spm_amd::kDecodeMaxSurface || t.bytes.size() + surface.size() > 0x7FFFFFFFull)
      return Fail(SPM_OUT_OF_RANGE, "piece surfaces too large for the decode table");
    t.off[i] = static_cast<uint32_t>(t.bytes.size());
    t.meta[i] = (static_cast<uint32_t>(surface.size()) << 1) | strip;
    t.bytes.insert(t.bytes.end(), surface.begin(), surface.end());
    t.max_surface = std::max<uint32_t>(t.max_surface, static_cast<uint32_t>(surface.size()));
  }
  if (!m->host_only) {
    SPM_HIP_TRY(Upload(&m->d_dec_meta, t.meta));
    SPM_HIP_TRY(Upload(&m->d_dec_off, t.off));
    SPM_HIP_TRY(Upload(&m->d_dec_bytes, t.bytes));
  }
  return SPM_OK;
}

// Lazy per-piece type bits of the id epilogue.
int EnsureTypes(spm_hip_model *m) {
  if (m->types_ready) return SPM_OK;
  std::lock_guard<std::mutex> g(m->init_mu);
  if (m->types_ready) return SPM_OK;
  std::vector<uint8_t> types(m->proto.pieces.size());
  for (size_t i = 0; i < types.size(); ++i) {
    const int32_t t = m->proto.pieces[i].type;
    types[i] = (t == spm_amd::kUnknown ? spm_amd::kPieceUnknown : 0) |
               (t == spm_amd::kControl ? spm_amd::kPieceControl : 0) |
               (t == spm_amd::kBytePiece ? spm_amd::kPieceByte : 0);
  }
  SPM_HIP_TRY(Upload(&m->d_types, types));
  if (m->byte_fallback)
    SPM_HIP_TRY(Upload(&m->d_byte_ids, std::vector<int32_t>(m->byte_ids, m->byte_ids + 256)));
  m->types_ready = true;
  return SPM_OK;
}

#define SPM_LEASE(lease, call)                                                          \
  do {                                                                                  \
    hipError_t _e = (call);                                                             \
    if (_e != hipSuccess)                                                               \
      return Fail(SPM_INTERNAL, std::string("workspace: ") + hipGetErrorString(_e));   \
  } while (0)

// The device normalizer's tables and switches of a model (after
// EnsureNormTables).
spm_amd::NormTables DeviceNormTables(const spm_hip_model *m) {
  const auto &ns = m->proto.normalizer_spec;
  spm_amd::NormTables t;
  if (!ns.precompiled_charsmap.empty()) {
    uint32_t tsize = 0;
    std::memcpy(&tsize, ns.precompiled_charsmap.data(), 4);
    t.units = reinterpret_cast<const uint32_t *>(m->d_charsmap.as<uint8_t>() + 4);
    t.num_units = tsize / 4;
    t.pool = m->d_charsmap.as<uint8_t>() + 4 + tsize;
    t.pool_size = static_cast<uint32_t>(ns.precompiled_charsmap.size() - 4 - tsize);
  }
  if (!m->user_defined.empty()) {
    t.ud_units = m->d_ud_units.as<uint32_t>();
    t.ud_num_units = m->ud_units_n;
  }
  t.add_dummy_prefix = ns.add_dummy_prefix;
  t.remove_extra_whitespaces = ns.remove_extra_whitespaces;
  t.escape_whitespaces = ns.escape_whitespaces;
  t.suffix = m->proto.trainer_spec.treat_whitespace_as_suffix;
  return t;
}

}  // namespace

namespace spm_amd {
// The unigram trainer E-step's forward pass through the byte kernel of a
// TrainerModel (spm_hip_model_from_pieces): see EStepForwardOut (kernels.h).
// ctl: kStWords zeroed status words (tile tickets); bp: back-pointer scratch
// of bytes_end + 16 bytes, indexed like the input.
bool EStepByteForwardOk(const spm_hip_model *m) {
  return m && m->kernel == UnigramKernel::kByte && m->ring_width == 16;
}
int EStepByteForward(spm_hip_model *m, const uint8_t *bytes, const uint64_t *off, uint64_t n, uint64_t bytes_end,
                     uint8_t *bp, uint32_t *ctl, const EStepForwardOut &e, hipStream_t st) {
  if (!EStepByteForwardOk(m)) return SPM_UNIMPLEMENTED;
  UnigramLaunch l{};
  l.bytes = bytes;
  l.off = off;
  l.n = n;
  l.capacity = bytes_end;
  l.units = m->d_uvs.as<uint32_t>();
  l.gen_units = m->d_units.as<uint32_t>();
  l.values = m->d_values.as<int32_t>();
  l.scores = m->d_scores.as<float>();
  l.num_units = static_cast<uint32_t>(m->trie.units.size());
  l.p = m->up;
  l.bp = bp;
  l.status = ctl;
  return LaunchUnigramEStepForward(l, e, st) == hipSuccess ? SPM_OK : SPM_INTERNAL;
}
}  // namespace spm_amd

namespace spm_amd {

// Ends the resident server (stop flag, then its stream drains: it sees the
// flag within one poll).
void EncodeWorkspace::StopService() {
  if (!svc_running) return;
  __atomic_store_n(&svc_box->stop, 1u, __ATOMIC_RELEASE);
  (void)hipStreamSynchronize(svc_stream);
  __atomic_store_n(&svc_box->stop, 0u, __ATOMIC_RELEASE);
  svc_running = false;
  static const bool kProf = std::getenv("SPM_HIP_SERVICE_PROF") != nullptr;  // debug
  if (kProf && svc_box->served) {
    int khz = 100000, dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
    const double us = 1000.0 / khz;
    std::fprintf(stderr, "service prof: %u requests, seen->copied %.2f us, seen->published %.2f us per request\n",
                 svc_box->served, svc_box->ticks_copy * us / svc_box->served, svc_box->ticks_busy * us / svc_box->served);
  }
  if (kProf && svc_prof) {
    uint64_t h[16];
    if (hipMemcpy(h, svc_prof, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess && h[13]) {
      int khz = 100000, dev = 0;
      (void)hipGetDevice(&dev);
      (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
      const double n = static_cast<double>(h[13]), us = h[14] * (1000.0 / khz) / n;
      std::fprintf(stderr,
                   "raw call prof: %llu calls, %.2f us and %.0f shader cycles per call (%.0f MHz); cycles per call: "
                   "stage %.0f normalize %.0f encode %.0f (setup %.0f lattice %.0f viterbi %.0f backtrace %.0f ids "
                   "%.0f) unknown-merge %.0f outputs+publish %.0f; per call %.1f bytes %.1f chars %.1f tokens\n",
                   (unsigned long long)h[13], us, h[15] / n, h[15] / n / us, h[8] / n, h[9] / n, h[10] / n, h[0] / n,
                   h[1] / n, h[2] / n, h[3] / n, h[4] / n, h[11] / n, h[12] / n, h[5] / n, h[6] / n, h[7] / n);
    }
    (void)hipMemset(svc_prof, 0, 16 * 8);
  }
}

void EncodeWorkspace::Release() {
  StopService();
  if (svc_stream) (void)hipStreamDestroy(svc_stream);
  svc_stream = nullptr;
  if (svc_box) (void)hipHostFree(svc_box);
  svc_box = nullptr;
  if (svc_prof) (void)spm_amd::DevFree(svc_prof);
  svc_prof = nullptr;
  for (DevBuf *b : {&w_ctl, &w_slot_ids, &w_slot_len, &w_tprefix, &w_slot2_ids, &w_slot2_len, &w_ntok, &w_cnt, &w_bp, &w_flagged, &w_ovf, &w_scan,
                    &w_scratch, &w_rest, &w_nlen, &w_nscan, &w_ecount, &w_escan, &w_dfirst, &w_dsum, &w_dctl, &w_bfsum, &w_bfctl, &h_dids, &h_dtok, &h_dout, &h_doff, &h_dbegin, &w_tids, &w_tlen, &w_ttok,
                    &h_in, &h_off, &h_ids, &h_len, &h_tok, &w_small, &w_bpn, &w_cpv, &w_cnd, &w_crest, &w_cpart, &w_salpha, &w_smask, &w_lpath, &w_lscore, &w_llogz,
                    &w_nb_ctl, &w_nb_npaths, &w_nb_stage, &w_nb_ntok, &w_nb_score, &w_nb_ids, &w_nb_len, &w_nb_hids,
                    &w_nb_hlen, &w_nb_ovf2, &w_nb_poff, &w_nb_ptok, &w_nb_toff, &w_nb_oscore, &w_wc_count, &w_wc_first, &w_wc_sent, &w_wc_next, &w_vstat, &w_vcount})
    b->Release();
  if (pinned) (void)hipHostFree(pinned);
  pinned = nullptr;
  if (pin_small) (void)hipHostFree(pin_small);
  pin_small = nullptr;
  pin_small_cap = 0;
  for (auto &e : ev)
    if (e) (void)hipEventDestroy(e);
  for (auto &e : tev)
    if (e) (void)hipEventDestroy(e);
  if (own_stream) (void)hipStreamDestroy(own_stream);
  own_stream = nullptr;
}

static hipError_t NewWorkspace(bool own_stream, std::unique_ptr<EncodeWorkspace> *out) {
  auto ws = std::make_unique<EncodeWorkspace>();
  hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&ws->pinned), 64);
  if (e == hipSuccess && own_stream) e = hipStreamCreateWithFlags(&ws->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    ws->Release();
    return e;
  }
  *out = std::move(ws);
  return hipSuccess;
}

hipError_t WorkspaceLease::ForStream(spm_hip_model *m, hipStream_t st) {
  m_ = m;
  st_ = st;
  std::unique_ptr<EncodeWorkspace> evicted;
  {
    std::lock_guard<std::mutex> g(m->pool_mu);
    auto &slot = m->by_stream[st];
    if (!slot) {
      hipError_t e = NewWorkspace(false, &slot);
      if (e != hipSuccess) {
        m->by_stream.erase(st);
        return e;
      }
    }
    ws_ = slot.get();
    ws_->last_use = ++m->use_clock;
    // Leased under pool_mu: from here until this lease ends the workspace
    // is never an eviction victim, even before its mutex is taken below.
    ++ws_->leases;
    // Bound the pool: callers that create short-lived streams would
    // otherwise grow device memory without limit.  The least recently used
    // unleased workspace goes; its buffers are freed after pool_mu is
    // dropped (hipFree waits for the device work that still uses them, and
    // other threads' leases must not queue behind that).
    if (m->by_stream.size() > kMaxStreamWorkspaces) {
      auto victim = m->by_stream.end();
      for (auto it = m->by_stream.begin(); it != m->by_stream.end(); ++it) {
        if (it->second.get() == ws_ || it->second->leases != 0) continue;
        if (victim == m->by_stream.end() || it->second->last_use < victim->second->last_use) victim = it;
      }
      if (victim != m->by_stream.end()) {
        evicted = std::move(victim->second);
        m->by_stream.erase(victim);
      }
    }
  }
  if (evicted) evicted->Release();
  lock_ = std::unique_lock<std::mutex>(ws_->mu);
  return hipSuccess;
}

hipError_t WorkspaceLease::ForHost(spm_hip_model *m) {
  m_ = m;
  host_ = true;
  std::lock_guard<std::mutex> g(m->pool_mu);
  for (auto &w : m->host_pool)
    if (!w->busy) {
      ws_ = w.get();
      break;
    }
  if (!ws_) {
    std::unique_ptr<EncodeWorkspace> w;
    hipError_t e = NewWorkspace(true, &w);
    if (e != hipSuccess) return e;
    ws_ = w.get();
    m->host_pool.push_back(std::move(w));
  }
  ws_->busy = true;
  st_ = ws_->own_stream;
  return hipSuccess;
}

WorkspaceLease::~WorkspaceLease() {
  if (!ws_) return;
  if (lock_.owns_lock()) lock_.unlock();
  std::lock_guard<std::mutex> g(m_->pool_mu);
  if (host_) ws_->busy = false;
  else --ws_->leases;
}

void PublishStats(spm_hip_model *m, const spm_hip_encode_stats &s) {
  std::lock_guard<std::mutex> g(m->pool_mu);
  m->last_stats = s;
}

}  // namespace spm_amd

// list == nullptr in the general kernel means identity (all sentences).

extern "C" {

const char *spm_hip_last_error(void) { return g_last_error.c_str(); }

int spm_hip_device_bytes(uint64_t *live, uint64_t *peak) {
  if (!live && !peak) return SPM_INVALID_ARGUMENT;
  if (live) *live = spm_amd::DevLiveBytes();
  if (peak) *peak = spm_amd::DevPeakBytes();
  return SPM_OK;
}

void spm_hip_device_peak_reset(void) { spm_amd::DevPeakReset(); }

int spm_hip_estep_shard_plan(uint64_t n, int mode, int num_threads, int world, int rank,
                             uint64_t *segs, uint64_t capacity, uint64_t *num_segments) {
  if (!num_segments || (capacity && !segs) || world < 1 || rank < 0 || rank >= world ||
      (mode != SPM_ESTEP_FAST && mode != SPM_ESTEP_PARITY) || num_threads < 1)
    return SPM_INVALID_ARGUMENT;
  const auto plan = spm_amd::EStepShardPlan(n, mode == SPM_ESTEP_PARITY, num_threads, world, rank);
  *num_segments = plan.size();
  for (uint64_t k = 0; k < plan.size() && k < capacity; ++k) {
    segs[3 * k] = plan[k].index_base;
    segs[3 * k + 1] = plan[k].index_stride;
    segs[3 * k + 2] = plan[k].count;
  }
  return SPM_OK;
}

int spm_hip_estep_bucket_owner(int bucket, int num_threads, int world) {
  if (world < 1 || num_threads < 1 || bucket < 0 || bucket >= num_threads) return -1;
  return spm_amd::EStepBucketOwner(bucket, world);
}

static int LoadImpl(const void *model_proto, size_t len, spm_hip_model **out, bool host_only) {
  if (!out) return Fail(SPM_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!model_proto && len) return Fail(SPM_INVALID_ARGUMENT, "model_proto is null");
  auto *m = new spm_hip_model();
  m->host_only = host_only;
  std::string err;
  if (!spm_amd::ParseModelProto(static_cast<const uint8_t *>(model_proto), len, &m->proto, &err)) {
    delete m;
    return Fail(SPM_INTERNAL, err);
  }
  m->model_type = m->proto.trainer_spec.model_type;
  int rc = InitializePieces(m);
  if (rc == SPM_OK && !host_only) {
    hipError_t e = hipGetDevice(&m->device);
    if (e != hipSuccess) rc = Fail(SPM_INTERNAL, std::string("hipGetDevice: ") + hipGetErrorString(e));
  }
  if (rc == SPM_OK) {
    if (m->model_type == spm_amd::kUnigram) rc = LoadUnigram(m);
    else if (m->model_type == spm_amd::kBpe) rc = spm_amd::LoadBpe(m, &g_last_error);
    else if (WordCharModel(m)) rc = LoadWordChar(m);
    else rc = Fail(SPM_UNIMPLEMENTED, "unknown model type");
  }
  if (rc == SPM_OK) rc = BuildDecodeTable(m);
  if (rc != SPM_OK) {
    spm_hip_model_free(m);
    return rc;
  }
  *out = m;
  return SPM_OK;
}

int spm_hip_model_load(const void *model_proto, size_t len, spm_hip_model **out) {
  return LoadImpl(model_proto, len, out, false);
}

// TrainerModel::SetSentencePieces (unigram_model_trainer.cc:97-119): a unigram
// model over a bare piece list — every piece NORMAL with value = list index,
// no InitializePieces, so unk_id_ keeps its default 0 (model_interface.h:336)
// and UNK nodes carry id 0 with score min_score - 10.
int spm_hip_model_from_pieces(const uint8_t *piece_bytes, const uint64_t *piece_offsets,
                              const float *scores, uint64_t num_pieces, spm_hip_model **out) {
  if (!out) return Fail(SPM_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!piece_offsets || !scores || (num_pieces && !piece_bytes) || num_pieces == 0)
    return Fail(SPM_INVALID_ARGUMENT, "empty piece list");
  auto *m = new spm_hip_model();
  m->model_type = spm_amd::kUnigram;
  m->proto.trainer_spec.model_type = spm_amd::kUnigram;
  m->proto.pieces.resize(num_pieces);
  int rc = SPM_OK;
  for (uint64_t i = 0; i < num_pieces && rc == SPM_OK; ++i) {
    auto &p = m->proto.pieces[i];
    p.piece.assign(reinterpret_cast<const char *>(piece_bytes) + piece_offsets[i],
                   piece_offsets[i + 1] - piece_offsets[i]);
    p.score = scores[i];
    p.type = spm_amd::kNormal;
    if (p.piece.empty() || !m->pieces.emplace(p.piece, static_cast<int32_t>(i)).second)
      rc = Fail(SPM_INTERNAL, "empty or duplicate piece");
  }
  m->unk_id = 0;
  if (rc == SPM_OK) {
    hipError_t e = hipGetDevice(&m->device);
    if (e != hipSuccess) rc = Fail(SPM_INTERNAL, std::string("HIP: ") + hipGetErrorString(e));
  }
  if (rc == SPM_OK) rc = LoadUnigram(m);
  if (rc != SPM_OK) {
    spm_hip_model_free(m);
    return rc;
  }
  *out = m;
  return SPM_OK;
}

int spm_hip_model_load_host_only(const void *model_proto, size_t len, spm_hip_model **out) {
  return LoadImpl(model_proto, len, out, true);
}

void spm_hip_model_free(spm_hip_model *m) {
  if (!m) return;
  // SPM_HIP_SMALL_STATS: what became of the handle's BPE small calls (the
  // processor and the CLIs have no other view of which path served them).
  if (m->model_type == spm_amd::kBpe && std::getenv("SPM_HIP_SMALL_STATS"))
    std::fprintf(stderr, "spm_hip: bpe line calls taken=%llu refused=%llu skipped=%llu\n",
                 static_cast<unsigned long long>(m->bpe_line_taken.load()),
                 static_cast<unsigned long long>(m->bpe_line_refused.load()),
                 static_cast<unsigned long long>(m->bpe_line_skipped.load()));
  for (spm_amd::DevBuf *b : {&m->d_units, &m->d_uvs, &m->d_piece_tab, &m->d_values, &m->d_scores,
                             &m->bpe.pair_keys, &m->bpe.pair_vals, &m->bpe.pair_ent, &m->bpe.rank_piece, &m->bpe.entry_piece,
                             &m->bpe.entry_out, &m->bpe.piece_kind, &m->bpe.piece_out,
                             &m->d_wc_tab, &m->d_wc_keys, &m->d_charsmap, &m->d_ud_units, &m->d_types, &m->d_byte_ids, &m->d_types_kind, &m->d_dec_meta, &m->d_dec_off, &m->d_dec_bytes})
    b->Release();
  for (auto &kv : m->by_stream) kv.second->Release();
  for (auto &w : m->host_pool) w->Release();
  delete m;
}

int spm_hip_model_get_info(const spm_hip_model *m, spm_hip_model_info *info) {
  if (!m || !info) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  info->model_type = m->model_type;
  info->piece_size = static_cast<int32_t>(m->proto.pieces.size());
  info->unk_id = m->unk_id;
  info->max_piece_chars = m->max_piece_chars;
  info->trie_results_size = m->trie.max_prefix_matches;
  info->trie_units = static_cast<int32_t>(m->trie.units.size());
  info->min_score = m->min_score;
  info->max_score = m->max_score;
  info->ring_width = m->model_type == spm_amd::kUnigram ? m->ring_width : 0;
  if (m->model_type == spm_amd::kUnigram) {
    info->fast_variant = static_cast<int32_t>(m->kernel);
  } else if (WordCharModel(m)) {
    // 1: the tile tier runs first; 0: every sentence goes to the general tier.
    info->fast_variant = m->model_type == spm_amd::kChar && m->wc_user_defined ? 0 : 1;
  } else {
    // The BPE encode tier, from what LoadBpe decided (EncodeBpe's branches).
    const auto &b = m->bpe;
    info->fast_variant = b.has_user_defined ? 0 : !b.lane_ok ? 4 : !b.rank_ids ? 3 : b.rank_base >= 0 ? 1 : 2;
  }
  return SPM_OK;
}

int spm_hip_model_piece_lookup(const spm_hip_model *m, const uint8_t *bytes, uint64_t len, int32_t *id,
                               float *score) {
  if (!m || (len && !bytes)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->piece_table.empty()) return Fail(SPM_FAILED_PRECONDITION, "the model has no piece table");
  if (len == 0 || len > spm_amd::kPieceKeyBytes) return SPM_NOT_FOUND;
  uint32_t k[4];
  spm_amd::PieceKey(bytes, static_cast<uint32_t>(len), k);
  int32_t i = 0;
  float s = 0.f;
  if (!spm_amd::PieceTableFind(m->piece_table.data(), k, &i, &s)) return SPM_NOT_FOUND;
  if (id) *id = i;
  if (score) *score = s;
  return SPM_OK;
}

int spm_hip_model_trie_stats(const spm_hip_model *m, const uint8_t *bytes, const uint64_t *off,
                             uint64_t n, int num_threads, spm_hip_trie_stats *out) {
  if (!m || !off || !out || (n && !bytes)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->model_type != spm_amd::kUnigram) return Fail(SPM_UNIMPLEMENTED, "unigram models only");
  const int T = num_threads > 0 ? num_threads : std::max(1u, std::thread::hardware_concurrency());
  std::vector<spm_hip_trie_stats> part(T);
  const std::vector<uint32_t> &units = m->trie.units;
  const uint32_t root = spm_amd::DoubleArray::Base(units[0]);
  // Walk depth (unit loads) of every byte position of sentence i; 0 where no
  // char starts.
  auto walk = [&](uint64_t i, spm_hip_trie_stats *s, std::vector<uint32_t> *dep) {
    const uint8_t *x = bytes + off[i];
    const uint64_t nb = off[i + 1] - off[i];
    dep->assign(nb + 1, 0);
    for (uint64_t p = 0; p < nb;) {
      ++s->char_starts;
      uint32_t base = root;
      uint32_t depth = 0;
      for (uint64_t q = p; q < nb; ++q) {
        const uint32_t c = x[q];
        const uint32_t node = base ^ c;
        ++s->unit_loads;
        ++depth;
        for (int k = 0; k < 8; ++k)
          if (node < (512u << k)) ++s->units_below[k];
        const uint32_t u = node < units.size() ? units[node] : 0u;
        if (c == 0 || spm_amd::DoubleArray::Label(u) != c) break;
        base = spm_amd::DoubleArray::Base(u);
        if (spm_amd::DoubleArray::Leaf(u)) ++s->leaf_loads;
      }
      (*dep)[p] = depth;
      s->max_depth = std::max<uint64_t>(s->max_depth, depth);
      p += std::min<uint64_t>(spm_amd::OneCharLen(x[p]), nb - p);
    }
  };
  const uint64_t nblocks = (n + 255) / 256;
  auto work = [&](int t) {
    spm_hip_trie_stats s{};
    std::vector<std::vector<uint32_t>> dep(256);
    std::vector<uint32_t> order(256);
    for (uint64_t blk = t; blk < nblocks; blk += T) {
      const uint64_t i0 = blk * 256, cnt = std::min<uint64_t>(256, n - i0);
      for (uint64_t k = 0; k < cnt; ++k) {
        walk(i0 + k, &s, &dep[k]);
        order[k] = static_cast<uint32_t>(k);
      }
      std::stable_sort(order.begin(), order.begin() + cnt, [&](uint32_t a, uint32_t b) {
        return std::min<uint64_t>(dep[a].size() - 1, 255) < std::min<uint64_t>(dep[b].size() - 1, 255);
      });
      for (uint64_t w0 = 0; w0 < cnt; w0 += 64) {
        const uint64_t w1 = std::min<uint64_t>(cnt, w0 + 64);
        ++s.waves;
        uint64_t maxlen = 0, dec = 0;
        for (uint64_t k = w0; k < w1; ++k) {
          const auto &d = dep[order[k]];
          maxlen = std::max<uint64_t>(maxlen, d.size() - 1);
          uint64_t tot = 0;
          for (uint32_t v : d) tot += v;
          dec = std::max(dec, (tot + 1) / 2);
        }
        s.decoupled_rounds += dec;
        for (uint64_t p = 0; p < maxlen; p += 2) {
          uint32_t r = 0;
          for (uint64_t k = w0; k < w1; ++k) {
            const auto &d = dep[order[k]];
            for (uint64_t q = p; q < p + 2 && q < d.size(); ++q) r = std::max(r, d[q]);
          }
          s.lockstep_rounds += r;
        }
      }
    }
    part[t] = s;
  };
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back(work, t);
  for (auto &x : th) x.join();
  spm_hip_trie_stats r{};
  for (const auto &s : part) {
    r.char_starts += s.char_starts;
    r.unit_loads += s.unit_loads;
    r.leaf_loads += s.leaf_loads;
    r.max_depth = std::max(r.max_depth, s.max_depth);
    for (int k = 0; k < 8; ++k) r.units_below[k] += s.units_below[k];
    r.lockstep_rounds += s.lockstep_rounds;
    r.decoupled_rounds += s.decoupled_rounds;
    r.waves += s.waves;
  }
  *out = r;
  return SPM_OK;
}

int spm_hip_normalize_batch(const spm_hip_model *m, const uint8_t *in, const uint64_t *in_off,
                            uint64_t n, uint8_t *out, uint64_t *out_off, int num_threads) {
  if (!m || !in_off || !out_off || (n && (!in || !out))) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  spm_amd::PrefixMatcher matcher(m->user_defined);
  spm_amd::Normalizer norm(m->proto.normalizer_spec, m->proto.trainer_spec.treat_whitespace_as_suffix);
  if (!norm.ok()) return Fail(SPM_INTERNAL, norm.error());
  norm.SetPrefixMatcher(&matcher);
  int T = num_threads > 0 ? num_threads : static_cast<int>(std::thread::hardware_concurrency());
  T = std::max(1, std::min<int>(T, static_cast<int>(std::max<uint64_t>(n / 256, 1))));
  // Each thread normalizes a contiguous chunk into its own buffer.
  std::vector<std::string> bufs(T);
  std::vector<std::vector<uint64_t>> lens(T);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      const uint64_t lo = n * t / T, hi = n * (t + 1) / T;
      std::string s;
      std::vector<size_t> n2o;
      for (uint64_t i = lo; i < hi; ++i) {
        norm.Normalize(reinterpret_cast<const char *>(in) + in_off[i], in_off[i + 1] - in_off[i], &s, &n2o);
        bufs[t] += s;
        lens[t].push_back(s.size());
      }
    });
  for (auto &x : th) x.join();
  uint64_t w = 0;
  out_off[0] = 0;
  uint64_t i = 0;
  for (int t = 0; t < T; ++t) {
    std::memcpy(out + w, bufs[t].data(), bufs[t].size());
    for (uint64_t l : lens[t]) {
      w += l;
      out_off[++i] = w;
    }
  }
  return SPM_OK;
}

// Normalizer::Normalize on the device (normalize_kernels.hip).
namespace {

// Device Normalizer::Normalize on a leased workspace; d_n2o (optional)
// receives norm_to_orig (len + 1 entries per sentence at d_out_off[i] + i).
int NormalizeImpl(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *d_in,
                  const uint64_t *d_in_off, uint64_t n, uint8_t *d_out, uint64_t out_capacity,
                  uint64_t *d_out_off, uint64_t *total, uint32_t *d_n2o, hipStream_t st,
                  uint32_t *chain = nullptr) {
  int rc = EnsureNormTables(m);
  if (rc != SPM_OK) return rc;
  const spm_amd::NormTables t = DeviceNormTables(m);
  SPM_HIP_TRY(ws->w_nlen.Reserve(std::max<uint64_t>(n, 1) * sizeof(uint64_t)));
  SPM_HIP_TRY(spm_amd::NormalizeLengths(t, d_in, d_in_off, n, ws->w_nlen.as<uint64_t>(), st, chain));
  size_t tb = 0;
  SPM_HIP_TRY(spm_amd::LengthsToOffsets(ws->w_nlen.as<uint64_t>(), n, d_out_off, nullptr, &tb, st));
  SPM_HIP_TRY(ws->w_nscan.Reserve(std::max<size_t>(tb, 16)));
  SPM_HIP_TRY(spm_amd::LengthsToOffsets(ws->w_nlen.as<uint64_t>(), n, d_out_off, ws->w_nscan.ptr, &tb, st));
  if (chain) {  // asynchronous: the write pass checks the capacity itself
    if (!d_out && out_capacity) return Fail(SPM_INVALID_ARGUMENT, "null output");
    SPM_HIP_TRY(spm_amd::NormalizeWrite(t, d_in, d_in_off, n, d_out, d_out_off, st, d_n2o, out_capacity, chain));
    return SPM_OK;
  }
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned + 2, d_out_off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  uint64_t tot = 0;
  std::memcpy(&tot, ws->pinned + 2, sizeof(uint64_t));
  *total = tot;
  if (tot > out_capacity) return Fail(SPM_RESOURCE_EXHAUSTED, "normalized output exceeds out_capacity");
  if (tot > 0 && !d_out) return Fail(SPM_INVALID_ARGUMENT, "null output");
  SPM_HIP_TRY(spm_amd::NormalizeWrite(t, d_in, d_in_off, n, d_out, d_out_off, st, d_n2o));
  return SPM_OK;
}

}  // namespace

int spm_hip_normalize_batch_device(spm_hip_model *m, const uint8_t *d_in, const uint64_t *d_in_off,
                                   uint64_t n, uint8_t *d_out, uint64_t out_capacity,
                                   uint64_t *d_out_off, uint64_t *total, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_normalize_batch_device");
  return spm_hip_normalize_batch_device_align(m, d_in, d_in_off, n, d_out, out_capacity, d_out_off,
                                              nullptr, total, stream);
}

int spm_hip_normalize_batch_device_align(spm_hip_model *m, const uint8_t *d_in, const uint64_t *d_in_off,
                                         uint64_t n, uint8_t *d_out, uint64_t out_capacity,
                                         uint64_t *d_out_off, uint32_t *d_norm_to_orig, uint64_t *total,
                                         void *stream) {
  if (!m || !d_in_off || !d_out_off || !total || (n && !d_in)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "host-only model handle");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return NormalizeImpl(m, ws.get(), d_in, d_in_off, n, d_out, out_capacity, d_out_off, total,
                       d_norm_to_orig, st);
}

int spm_hip_normalize_batch_device_async(spm_hip_model *m, const uint8_t *d_in, const uint64_t *d_in_off,
                                         uint64_t n, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_out_off,
                                         uint32_t *d_norm_to_orig, uint32_t *d_status, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_normalize_batch_device_async");
  if (!m || !d_in_off || !d_out_off || !d_status || (n && !d_in)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "host-only model handle");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return NormalizeImpl(m, ws.get(), d_in, d_in_off, n, d_out, out_capacity, d_out_off, nullptr, d_norm_to_orig,
                       st, d_status);
}

int spm_hip_model_set_force_general(spm_hip_model *m, int force) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null model");
  m->force_general = force != 0;
  return SPM_OK;
}

int spm_hip_model_set_timing(spm_hip_model *m, int enable) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null model");
  m->timing = enable != 0 && !m->host_only;  // events are created per workspace on first use
  return SPM_OK;
}

int spm_hip_model_last_stats(const spm_hip_model *m, spm_hip_encode_stats *s) {
  if (!m || !s) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  auto *mm = const_cast<spm_hip_model *>(m);
  std::lock_guard<std::mutex> g(mm->pool_mu);
  *s = m->last_stats;
  return SPM_OK;
}

int spm_hip_encode_batch(spm_hip_model *m, const uint8_t *d_bytes, const uint64_t *d_off,
                         uint64_t n, int32_t *d_ids, uint32_t *d_len, uint64_t *d_tok,
                         void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_encode_batch");
  if (!m || (!d_off) || (!d_tok) || (n && !d_ids))
    return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return EncodeBlocking(m, ws.get(), d_bytes, d_off, n, d_ids, d_len, d_tok, st);
}

int spm_hip_encode_batch_async(spm_hip_model *m, const uint8_t *d_bytes, const uint64_t *d_off, uint64_t n,
                               uint64_t capacity, int32_t *d_ids, uint32_t *d_len, uint64_t *d_tok,
                               uint32_t *d_status, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_encode_batch_async");
  if (!m || (!d_off) || (!d_tok) || (n && !d_ids) || !d_status)
    return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  if (capacity > 0xFFFFFFFFull * 4) return Fail(SPM_OUT_OF_RANGE, "batch too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  if (NeedsHostSized(m)) {
    // General kernel over every sentence: its scratch is sized from the
    // longest sentence, which needs the offsets on the host.  A chain that
    // already failed (e.g. a normalize that overflowed its capacity, whose
    // offsets then point past the caller's buffer) launches nothing: the
    // status word keeps its first error, as every kernel of the pure stream
    // path does.
    SPM_HIP_TRY(hipMemcpyAsync(ws->pinned, d_status, 4, hipMemcpyDeviceToHost, st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
    if (ws->pinned[0] != 0) return SPM_OK;
    const int rc = EncodeBlocking(m, ws.get(), d_bytes, d_off, n, d_ids, d_len, d_tok, st);
    if (rc != SPM_OK) SPM_HIP_TRY(spm_amd::LaunchStatusSetFirst(d_status, static_cast<uint32_t>(rc), st));
    return rc;
  }
  spm_amd::EncodeCall c{d_bytes, d_off, n, capacity, d_ids, d_len, d_tok, d_status, st, false, 0};
  return EncodeEnqueue(m, ws.get(), c);
}

int spm_hip_model_drain_kernel_times(spm_hip_model *m, void *stream, float *ms, uint32_t capacity,
                                     uint32_t *count) {
  if (!m || !count || (capacity && !ms)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  const uint32_t ring = spm_amd::EncodeWorkspace::kTimingRing;
  const uint32_t have = ws->tcount < ring ? ws->tcount : ring;
  const uint32_t first = ws->tcount - have;
  uint32_t k = 0;
  for (uint32_t j = 0; j < have && k < capacity; ++j) {
    const uint32_t slot = (first + j) % ring;
    SPM_HIP_TRY(hipEventElapsedTime(&ms[k], ws->tev[2 * slot], ws->tev[2 * slot + 1]));
    ++k;
  }
  *count = k;
  ws->tcount = 0;
  return SPM_OK;
}

int spm_hip_model_set_coop_min_nb(spm_hip_model *m, uint32_t min_nb) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null model");
  if (min_nb && (!m->d_uvs.ptr || m->max_piece_bytes > 56))
    return Fail(SPM_FAILED_PRECONDITION, "model has no cooperative-kernel tables or pieces over 56 bytes");
  m->coop_min_nb = min_nb;
  return SPM_OK;
}

int spm_hip_model_set_coop_slab(spm_hip_model *m, int mode, uint32_t slab_chars) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null model");
  if (mode < 0 || mode > 2) return Fail(SPM_INVALID_ARGUMENT, "coop slab mode must be 0, 1 or 2");
  m->coop_slab_mode = mode;
  m->coop_slab_chars = slab_chars ? slab_chars : static_cast<uint32_t>(spm_amd::kCoopSlabChars);
  return SPM_OK;
}

int spm_hip_model_set_debug_corrupt_bp(spm_hip_model *m, int64_t sentence) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null model");
  m->corrupt_bp = sentence < 0 ? ~0ull : static_cast<uint64_t>(sentence);
  return SPM_OK;
}

int spm_hip_model_release_stream(spm_hip_model *m, void *stream) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null model");
  std::unique_ptr<spm_amd::EncodeWorkspace> w;
  // A call still holding a lease on that stream's workspace finishes first
  // (it may not have taken the workspace mutex yet, so wait on the count).
  for (;;) {
    {
      std::lock_guard<std::mutex> g(m->pool_mu);
      auto it = m->by_stream.find(static_cast<hipStream_t>(stream));
      if (it == m->by_stream.end()) return SPM_OK;
      if (it->second->leases == 0) {
        w = std::move(it->second);
        m->by_stream.erase(it);
        break;
      }
    }
    std::this_thread::yield();
  }
  SPM_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  w->Release();
  return SPM_OK;
}

int spm_hip_abi_version(void) { return SPM_HIP_ABI_VERSION; }

namespace {

// ParseExtraOptions (sentencepiece_processor.cc:981-1010) folded for the
// device epilogues: out = pre · (merged pieces, reversed?) · post.
int FoldExtras(spm_hip_model *m, const char *extra_options, spm_amd::EpilogueExtras *xo) {
  auto piece_to_id = [&](const std::string &s) -> int32_t {
    auto r = m->reserved.find(s);
    if (r != m->reserved.end()) return r->second;
    auto p = m->pieces.find(s);
    if (p != m->pieces.end()) return p->second;
    return m->unk_id;
  };
  // Fold the option list: out = pre · (mid, reversed?) · post.
  std::vector<int32_t> pre, post;
  bool reversed = false;
  const std::string opts = extra_options ? extra_options : "";
  size_t s0 = 0;
  while (s0 <= opts.size()) {
    const size_t e = std::min(opts.find(':', s0), opts.size());
    const std::string o = opts.substr(s0, e - s0);
    s0 = e + 1;
    if (o.empty()) continue;  // SplitPiece drops empty fields
    if (o == "bos" || o == "eos") {
      const std::string &piece = o == "bos" ? m->proto.trainer_spec.bos_piece : m->proto.trainer_spec.eos_piece;
      const int32_t id = piece_to_id(piece);
      if (id == m->unk_id) return Fail(SPM_INTERNAL, "id for `" + piece + "` is not defined.");
      if (o == "bos") pre.insert(pre.begin(), id);
      else post.push_back(id);
    } else if (o == "reverse") {
      std::vector<int32_t> np(post.rbegin(), post.rend()), nq(pre.rbegin(), pre.rend());
      pre.swap(np);
      post.swap(nq);
      reversed = !reversed;
    } else {
      return Fail(SPM_INTERNAL, "option \"" + o + "\" is not available.");
    }
  }
  if (pre.size() > static_cast<size_t>(spm_amd::kMaxExtras) || post.size() > static_cast<size_t>(spm_amd::kMaxExtras))
    return Fail(SPM_OUT_OF_RANGE, "too many bos/eos extra options");
  spm_amd::EpilogueExtras &x = *xo;
  x = spm_amd::EpilogueExtras{};
  for (size_t k = 0; k < pre.size(); ++k) x.ids[k] = pre[k];
  for (size_t k = 0; k < post.size(); ++k) x.ids[spm_amd::kMaxExtras + k] = post[k];
  x.num_pre = static_cast<uint32_t>(pre.size());
  x.num_post = static_cast<uint32_t>(post.size());
  x.reversed = reversed ? 1u : 0u;
  return SPM_OK;
}

}  // namespace

// PopulateSentencePieceText's id part + ApplyExtraOptions on the device
// (epilogue_kernels.hip).  Option parsing follows ParseExtraOptions
// (sentencepiece_processor.cc:981-1010).
static int FinalizeImpl(spm_hip_model *m, const char *extra_options, const int32_t *d_ids,
                        const uint64_t *d_tok_off, uint64_t n, int32_t *d_out_ids, uint64_t out_capacity,
                        uint64_t *d_out_off, uint64_t *total, uint32_t *chain, hipStream_t st) {
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (m->byte_fallback)
    return Fail(SPM_INVALID_ARGUMENT,
                "the model uses byte fallback: unknown tokens expand to their bytes, which needs the normalized "
                "text; call spm_hip_finalize_ids_bytes");
  spm_amd::EpilogueExtras x{};
  {
    const int rc0 = FoldExtras(m, extra_options, &x);
    if (rc0 != SPM_OK) return rc0;
  }
  int rc = EnsureTypes(m);
  if (rc != SPM_OK) return rc;
  const int32_t num_types = static_cast<int32_t>(m->proto.pieces.size());
  if (n == 0) {
    SPM_HIP_TRY(hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), st));
    if (total) *total = 0;
    return SPM_OK;
  }
  if (!d_ids) return Fail(SPM_INVALID_ARGUMENT, "null ids");
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  SPM_HIP_TRY(ws->w_ecount.Reserve(n * sizeof(uint64_t)));
  SPM_HIP_TRY(spm_amd::LaunchEpilogueCount(d_ids, d_tok_off, n, m->d_types.as<uint8_t>(), num_types,
                                            x.num_pre + x.num_post, ws->w_ecount.as<uint64_t>(), st, chain));
  size_t tb = 0;
  SPM_HIP_TRY(spm_amd::LengthsToOffsets(ws->w_ecount.as<uint64_t>(), n, d_out_off, nullptr, &tb, st));
  SPM_HIP_TRY(ws->w_escan.Reserve(std::max<size_t>(tb, 16)));
  SPM_HIP_TRY(spm_amd::LengthsToOffsets(ws->w_ecount.as<uint64_t>(), n, d_out_off, ws->w_escan.ptr, &tb, st));
  if (chain) {  // asynchronous: the write pass checks the capacity itself
    if (!d_out_ids && out_capacity) return Fail(SPM_INVALID_ARGUMENT, "null output");
    SPM_HIP_TRY(spm_amd::LaunchEpilogueWrite(d_ids, d_tok_off, n, m->d_types.as<uint8_t>(), num_types, x,
                                              d_out_off, d_out_ids, st, out_capacity, chain));
    return SPM_OK;
  }
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned + 12, d_out_off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  uint64_t tot = 0;
  std::memcpy(&tot, ws->pinned + 12, sizeof(uint64_t));
  if (total) *total = tot;
  if (tot > out_capacity) return Fail(SPM_RESOURCE_EXHAUSTED, "finalized ids exceed out_capacity");
  if (tot > 0 && !d_out_ids) return Fail(SPM_INVALID_ARGUMENT, "null output");
  SPM_HIP_TRY(spm_amd::LaunchEpilogueWrite(d_ids, d_tok_off, n, m->d_types.as<uint8_t>(), num_types, x,
                                            d_out_off, d_out_ids, st));
  return SPM_OK;
}

// PopulateSentencePieceText's id part + ApplyExtraOptions on the device
// (epilogue_kernels.hip).  Option parsing follows ParseExtraOptions
// (sentencepiece_processor.cc:981-1010).
int spm_hip_finalize_ids(spm_hip_model *m, const char *extra_options, const int32_t *d_ids,
                         const uint64_t *d_tok_off, uint64_t n, int32_t *d_out_ids,
                         uint64_t out_capacity, uint64_t *d_out_off, uint64_t *total, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_finalize_ids");
  if (!m || !d_tok_off || !d_out_off) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  return FinalizeImpl(m, extra_options, d_ids, d_tok_off, n, d_out_ids, out_capacity, d_out_off, total, nullptr,
                      static_cast<hipStream_t>(stream));
}

int spm_hip_finalize_ids_async(spm_hip_model *m, const char *extra_options, const int32_t *d_ids,
                               const uint64_t *d_tok_off, uint64_t n, int32_t *d_out_ids, uint64_t out_capacity,
                               uint64_t *d_out_off, uint32_t *d_status, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_finalize_ids_async");
  if (!m || !d_tok_off || !d_out_off || !d_status) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  return FinalizeImpl(m, extra_options, d_ids, d_tok_off, n, d_out_ids, out_capacity, d_out_off, nullptr, d_status,
                      static_cast<hipStream_t>(stream));
}

// The epilogue of a byte-fallback model (byte_epilogue_kernels.hip).  out_spt
// selects SentencePieceText pieces (then n2o is norm_to_orig).  chain: the
// caller's status word, or null for a blocking call.
static int ByteEpilogueImpl(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EpilogueExtras &x,
                            const int32_t *d_ids, const uint32_t *d_len, const uint64_t *d_tok_off, uint64_t n,
                            const uint8_t *d_norm, const uint64_t *d_norm_off, int32_t *d_out,
                            spm_hip_piece *d_out_spt, const uint32_t *d_n2o, uint64_t out_capacity,
                            uint64_t *d_out_off, uint64_t *total, uint32_t *chain, hipStream_t st) {
  SPM_HIP_TRY(ws->w_bfsum.Reserve(2 * spm_amd::kDecodeBlocks * sizeof(uint64_t)));
  SPM_HIP_TRY(ws->w_bfctl.Reserve(2 * sizeof(uint64_t)));
  uint64_t *ctl = ws->w_bfctl.as<uint64_t>();
  SPM_HIP_TRY(hipMemsetAsync(ctl, 0, 2 * sizeof(uint64_t), st));
  spm_amd::ByteEpilogueLaunch a{};
  a.ids = d_ids;
  a.len = d_len;
  a.tok_off = d_tok_off;
  a.n = n;
  a.norm = d_norm;
  a.norm_off = d_norm_off;
  a.types = m->d_types.as<uint8_t>();
  a.num_types = static_cast<int32_t>(m->proto.pieces.size());
  a.byte_ids = m->d_byte_ids.as<int32_t>();
  a.x = x;
  a.block_sum = ws->w_bfsum.as<uint64_t>();
  a.ctl = ctl;
  a.chain = chain ? chain : reinterpret_cast<uint32_t *>(ctl + 1);  // blocking: a status word of its own
  a.check_capacity = chain != nullptr;
  a.capacity = out_capacity;
  a.out_off = d_out_off;
  a.out = d_out;
  a.out_spt = d_out_spt;
  a.n2o = d_n2o;
  SPM_HIP_TRY(spm_amd::LaunchByteEpilogueCount(a, st));
  if (chain) {  // asynchronous: the fill pass checked the capacity
    if (!d_out && !d_out_spt && out_capacity) return Fail(SPM_INVALID_ARGUMENT, "null output");
    SPM_HIP_TRY(spm_amd::LaunchByteEpilogueWrite(a, st));
    return SPM_OK;
  }
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned + 12, ctl, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  uint64_t tot = 0;
  std::memcpy(&tot, ws->pinned + 12, sizeof(uint64_t));
  if (total) *total = tot;
  if (tot > out_capacity) return Fail(SPM_RESOURCE_EXHAUSTED, "finalized ids exceed out_capacity");
  if (tot > 0 && !d_out && !d_out_spt) return Fail(SPM_INVALID_ARGUMENT, "null output");
  SPM_HIP_TRY(spm_amd::LaunchByteEpilogueWrite(a, st));
  return SPM_OK;
}

static int FinalizeBytesImpl(spm_hip_model *m, const char *extra_options, const int32_t *d_ids,
                             const uint32_t *d_len, const uint64_t *d_tok_off, uint64_t n, const uint8_t *d_norm,
                             const uint64_t *d_norm_off, int32_t *d_out_ids, uint64_t out_capacity,
                             uint64_t *d_out_off, uint64_t *total, uint32_t *chain, hipStream_t st) {
  if (!m->byte_fallback)  // the same result, without reading the text
    return FinalizeImpl(m, extra_options, d_ids, d_tok_off, n, d_out_ids, out_capacity, d_out_off, total, chain, st);
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  spm_amd::EpilogueExtras x{};
  int rc = FoldExtras(m, extra_options, &x);
  if (rc != SPM_OK) return rc;
  rc = EnsureTypes(m);
  if (rc != SPM_OK) return rc;
  if (n == 0) {
    SPM_HIP_TRY(hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), st));
    if (total) *total = 0;
    return SPM_OK;
  }
  if (!d_ids || !d_len || !d_norm || !d_norm_off) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return ByteEpilogueImpl(m, ws.get(), x, d_ids, d_len, d_tok_off, n, d_norm, d_norm_off, d_out_ids, nullptr, nullptr,
                          out_capacity, d_out_off, total, chain, st);
}

int spm_hip_finalize_ids_bytes(spm_hip_model *m, const char *extra_options, const int32_t *d_ids,
                               const uint32_t *d_piece_len, const uint64_t *d_tok_off, uint64_t n,
                               const uint8_t *d_norm_bytes, const uint64_t *d_norm_off, int32_t *d_out_ids,
                               uint64_t out_capacity, uint64_t *d_out_off, uint64_t *total, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_finalize_ids_bytes");
  if (!m || !d_tok_off || !d_out_off) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  return FinalizeBytesImpl(m, extra_options, d_ids, d_piece_len, d_tok_off, n, d_norm_bytes, d_norm_off, d_out_ids,
                           out_capacity, d_out_off, total, nullptr, static_cast<hipStream_t>(stream));
}

int spm_hip_finalize_ids_bytes_async(spm_hip_model *m, const char *extra_options, const int32_t *d_ids,
                                     const uint32_t *d_piece_len, const uint64_t *d_tok_off, uint64_t n,
                                     const uint8_t *d_norm_bytes, const uint64_t *d_norm_off, int32_t *d_out_ids,
                                     uint64_t out_capacity, uint64_t *d_out_off, uint32_t *d_status, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_finalize_ids_bytes_async");
  if (!m || !d_tok_off || !d_out_off || !d_status) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  return FinalizeBytesImpl(m, extra_options, d_ids, d_piece_len, d_tok_off, n, d_norm_bytes, d_norm_off, d_out_ids,
                           out_capacity, d_out_off, nullptr, d_status, static_cast<hipStream_t>(stream));
}

int spm_hip_model_byte_fallback(const spm_hip_model *m, int *enabled, int32_t byte_ids[256]) {
  if (!m || !enabled) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  *enabled = m->byte_fallback ? 1 : 0;
  if (byte_ids)
    for (int b = 0; b < 256; ++b) byte_ids[b] = m->byte_fallback ? m->byte_ids[b] : -1;
  return SPM_OK;
}

// Host buffers: a pooled workspace with a private stream, so concurrent host
// calls on one handle run side by side.
// SentencePieceProcessor::Encode(input, SentencePieceText*) (sentencepiece_
// processor.cc:553-575) on the device: one workspace lease for the whole
// pipeline (normalize + norm_to_orig, Encode, SentencePieceText epilogue).
int spm_hip_encode_spt(spm_hip_model *m, const char *extra_options, const uint8_t *d_raw,
                       const uint64_t *d_raw_off, uint64_t n, uint8_t *d_norm, uint64_t norm_capacity,
                       uint64_t *d_norm_off, uint32_t *d_n2o, spm_hip_piece *d_pieces,
                       uint64_t piece_capacity, uint64_t *d_piece_off, uint64_t *total_norm,
                       uint64_t *total_pieces, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_encode_spt");
  if (!m || !d_raw_off || !d_norm_off || !d_piece_off || !total_norm || !total_pieces || (n && !d_raw))
    return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  *total_norm = *total_pieces = 0;
  spm_amd::EpilogueExtras x{};
  int rc = FoldExtras(m, extra_options, &x);
  if (rc != SPM_OK) return rc;
  rc = EnsureTypes(m);
  if (rc != SPM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  if (n == 0) {
    SPM_HIP_TRY(hipMemsetAsync(d_norm_off, 0, sizeof(uint64_t), st));
    SPM_HIP_TRY(hipMemsetAsync(d_piece_off, 0, sizeof(uint64_t), st));
    return SPM_OK;
  }
  if (!d_n2o) return Fail(SPM_INVALID_ARGUMENT, "null norm_to_orig");
  rc = NormalizeImpl(m, ws.get(), d_raw, d_raw_off, n, d_norm, norm_capacity, d_norm_off, total_norm, d_n2o, st);
  if (rc != SPM_OK) return rc;
  const uint64_t tn = *total_norm;
  SPM_HIP_TRY(ws->w_tids.Reserve(std::max<uint64_t>(tn, 1) * 4));
  SPM_HIP_TRY(ws->w_tlen.Reserve(std::max<uint64_t>(tn, 1) * 4));
  SPM_HIP_TRY(ws->w_ttok.Reserve((n + 1) * 8));
  rc = EncodeBlocking(m, ws.get(), d_norm, d_norm_off, n, ws->w_tids.as<int32_t>(), ws->w_tlen.as<uint32_t>(),
                  ws->w_ttok.as<uint64_t>(), st);
  if (rc != SPM_OK) return rc;
  if (m->byte_fallback) {
    rc = ByteEpilogueImpl(m, ws.get(), x, ws->w_tids.as<int32_t>(), ws->w_tlen.as<uint32_t>(),
                          ws->w_ttok.as<uint64_t>(), n, d_norm, d_norm_off, nullptr, d_pieces, d_n2o, piece_capacity,
                          d_piece_off, total_pieces, nullptr, st);
    if (rc == SPM_RESOURCE_EXHAUSTED) return Fail(SPM_RESOURCE_EXHAUSTED, "pieces exceed piece_capacity");
    if (rc == SPM_INVALID_ARGUMENT) return Fail(SPM_INVALID_ARGUMENT, "null pieces output");
    return rc;
  }
  const int32_t num_types = static_cast<int32_t>(m->proto.pieces.size());
  SPM_HIP_TRY(ws->w_ecount.Reserve(n * sizeof(uint64_t)));
  SPM_HIP_TRY(spm_amd::LaunchEpilogueCount(ws->w_tids.as<int32_t>(), ws->w_ttok.as<uint64_t>(), n,
                                            m->d_types.as<uint8_t>(), num_types, x.num_pre + x.num_post,
                                            ws->w_ecount.as<uint64_t>(), st));
  size_t tb = 0;
  SPM_HIP_TRY(spm_amd::LengthsToOffsets(ws->w_ecount.as<uint64_t>(), n, d_piece_off, nullptr, &tb, st));
  SPM_HIP_TRY(ws->w_escan.Reserve(std::max<size_t>(tb, 16)));
  SPM_HIP_TRY(spm_amd::LengthsToOffsets(ws->w_ecount.as<uint64_t>(), n, d_piece_off, ws->w_escan.ptr, &tb, st));
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned + 12, d_piece_off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  uint64_t tot = 0;
  std::memcpy(&tot, ws->pinned + 12, sizeof(uint64_t));
  *total_pieces = tot;
  if (tot > piece_capacity) return Fail(SPM_RESOURCE_EXHAUSTED, "pieces exceed piece_capacity");
  if (tot > 0 && !d_pieces) return Fail(SPM_INVALID_ARGUMENT, "null pieces output");
  SPM_HIP_TRY(spm_amd::LaunchSptWrite(ws->w_tids.as<int32_t>(), ws->w_tlen.as<uint32_t>(),
                                       ws->w_ttok.as<uint64_t>(), n, m->d_types.as<uint8_t>(), num_types, x,
                                       d_n2o, d_norm_off, d_piece_off, d_pieces, st));
  return SPM_OK;
}

namespace {

constexpr uint64_t kSmallMaxSentences = 256;    // one fast-kernel tile
constexpr uint64_t kSmallMaxBytes = 1ull << 20;  // pinned staging bound

// The resident small-call server (coop_service_kernel, CoopServiceBox):
// on by default; SPM_HIP_SERVICE=0 launches one kernel per call instead.
// SPM_HIP_SERVICE_IDLE_US: wall-clock microseconds without a request after
// which the server exits (default 2000; the next call relaunches it).  While
// it runs it holds one CU and its stream's hardware queue.
bool ServiceOn() {
  static const bool on = [] {
    const char *e = std::getenv("SPM_HIP_SERVICE");
    return !(e && std::atoi(e) == 0);
  }();
  return on;
}

uint64_t ServiceIdleTicks() {
  static const uint64_t ticks = [] {
    int khz = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) !=
                                                  hipSuccess || khz <= 0)
      khz = 100000;  // 100 MHz
    const char *e = std::getenv("SPM_HIP_SERVICE_IDLE_US");
    const uint64_t us = e ? std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)) : 2000;
    return static_cast<uint64_t>(khz) * us / 1000;
  }();
  return ticks;
}

// The pinned image and the device buffers of one small call, of any kind.
// The server's launch tables point into all of them (svc_key) and a buffer
// that grows is reallocated, so the server is stopped first whenever one
// must.  pin_small is always coherent (fine-grained): the kernels read the
// input image from it and write the outputs and the publication word into it
// directly, and the host polls that word.
int ReserveSmall(spm_amd::EncodeWorkspace *ws, const spm_amd::SmallLayout &l) {
  // The lane kind has no slots: FastSetup reserves its work buffers, nothing of these four.
  // The BPE kinds have slots and no per-char tables.
  const uint64_t rows = l.table_slots ? (l.table_slots + 64) * spm_amd::kCoopSlots : 0;
  const std::pair<spm_amd::DevBuf *, uint64_t> want[] = {{&ws->w_small, l.dev_bytes},
                                                         {&ws->w_slot2_ids, l.slots * 4},
                                                         {&ws->w_slot2_len, l.slot_len_bytes},
                                                         {&ws->w_cpv, rows * 2},
                                                         {&ws->w_cnd, rows * 4}};
  bool grows = ws->pin_small_cap < l.pin_bytes;
  for (const auto &w : want) grows |= w.first->cap < w.second;
  if (grows) ws->StopService();
  for (const auto &w : want) SPM_HIP_TRY(w.first->Reserve(w.second));
  if (ws->pin_small_cap < l.pin_bytes) {
    if (ws->pin_small) SPM_HIP_TRY(hipHostFree(ws->pin_small));
    ws->pin_small = nullptr;
    ws->pin_small_cap = 0;
    const size_t want_pin = std::max<uint64_t>(l.pin_bytes, 64 << 10);
    SPM_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ws->pin_small), want_pin, hipHostMallocCoherent));
    ws->pin_small_cap = want_pin;
  }
  return SPM_OK;
}

// The call's publication sequence number: 30 bits (the server's request word
// keeps the call kind above them), never 0 (a cleared publication word).
uint32_t NextPubSeq(spm_amd::EncodeWorkspace *ws) {
  if ((++ws->pub_seq & 0x3FFFFFFFu) == 0) ++ws->pub_seq;
  return ws->pub_seq & 0x3FFFFFFFu;
}

// What a one-block kernel is told of the staged call: its sizes, the input's
// place in the image and the outputs' in pinned memory.
spm_amd::CoopCall SmallCoopCall(spm_amd::EncodeWorkspace *ws, const spm_amd::SmallLayout &l, uint64_t n,
                                bool with_len) {
  uint8_t *h = ws->pin_small;
  spm_amd::CoopCall c{};
  c.n = static_cast<uint32_t>(n);
  c.stage_words = l.stage_words();
  c.pub_seq = NextPubSeq(ws);
  c.in_at = l.in;
  c.ids_cap = l.ids_cap;
  c.tok = l.Tok(h);
  c.ids = l.Ids(h);
  c.len = with_len ? l.Len(h) : nullptr;
  c.host_pub = l.Pub(h);
  return c;
}

// Completion: the kernel's publication word, polled until pub[0] == seq; the
// stream is queried now and then so that a kernel that ended without
// publishing (an early exit: *published = false) or failed (the stream is
// synchronized, the HIP error returned) is noticed.
int WaitPublished(volatile const uint32_t *pub, uint32_t seq, hipStream_t st, bool *published) {
  *published = false;
  for (uint32_t spin = 1; pub[0] != seq; ++spin) {
    if ((spin & 1023) != 0) continue;
    const hipError_t q = hipStreamQuery(st);
    if (q == hipSuccess) {
      if (pub[0] != seq) return SPM_OK;
      break;
    }
    if (q != hipErrorNotReady) {
      (void)hipStreamSynchronize(st);
      return Fail(SPM_INTERNAL, std::string("HIP: ") + hipGetErrorString(q));
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  *published = true;
  return SPM_OK;
}

// The tail of a normalized small call: tok, then tok[n] ids and lengths out
// of the pinned image, and the call's stats (slot >= 0: the lane kernels'
// timed ring slot).
int FinishSmall(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::SmallLayout &l, uint64_t n,
                uint32_t flagged, int slot, int32_t *ids, uint32_t *len, uint64_t *tok) {
  uint8_t *h = ws->pin_small;
  std::memcpy(tok, l.Tok(h), (n + 1) * 8);
  const uint64_t ntok = tok[n];
  if (ntok) {
    std::memcpy(ids, l.Ids(h), ntok * 4);
    if (len) std::memcpy(len, l.Len(h), ntok * 4);
  }
  ws->stats = spm_hip_encode_stats{};
  ws->stats.sentences = n;
  ws->stats.general_path = flagged;
  ws->stats.tokens = ntok;
  if (m->timing && slot >= 0) {
    SPM_HIP_TRY(hipEventSynchronize(ws->tev[2 * slot + 1]));
    SPM_HIP_TRY(hipEventElapsedTime(&ws->stats.fast_kernel_ms, ws->tev[2 * slot], ws->tev[2 * slot + 1]));
    if (flagged) SPM_HIP_TRY(hipEventElapsedTime(&ws->stats.general_kernel_ms, ws->ev[0], ws->ev[1]));
    ws->tcount = 0;
  }
  spm_amd::PublishStats(m, ws->stats);
  return SPM_OK;
}

// One small call through the server (kind 1: normalized batch with `sa`,
// 2: raw lines with `ra`), or, with the server off, one launch on `st`; then
// the wait for host_pub[0] == c.pub_seq.  A server that has exited meanwhile
// (idle timeout before it saw the request) is relaunched once to serve it.
int RunSmallCall(spm_amd::EncodeWorkspace *ws, int kind, const spm_amd::CoopSmallArgs *sa,
                 const spm_amd::CoopRawArgs *ra, const spm_amd::CoopCall &c, hipStream_t st, const char *what) {
  const bool svc = ServiceOn();
  hipStream_t wait_st = st;
  uint32_t prev = 0;
  auto launch = [&](uint32_t last) -> hipError_t {
    ws->svc_args.box = ws->svc_box;
    ws->svc_args.last = last;
    ws->svc_args.idle_ticks = ServiceIdleTicks();
    hipError_t e = spm_amd::LaunchCoopService(ws->svc_args, ws->svc_stream);
    if (e == hipSuccess) ws->svc_running = true;
    return e;
  };
  if (svc) {
    if (!ws->svc_stream) SPM_HIP_TRY(hipStreamCreateWithFlags(&ws->svc_stream, hipStreamNonBlocking));
    if (!ws->svc_box) {
      SPM_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ws->svc_box), sizeof(spm_amd::CoopServiceBox),
                                hipHostMallocCoherent));
      std::memset(ws->svc_box, 0, sizeof(spm_amd::CoopServiceBox));
    }
    if (ws->svc_running && hipStreamQuery(ws->svc_stream) == hipSuccess) ws->svc_running = false;  // idled out
    // The call's tables are a function of the workspace buffers (and the
    // model): a server launched with other buffers is restarted.
    const void *key[6] = {ws->w_small.ptr, ws->w_slot2_ids.ptr, ws->w_slot2_len.ptr, ws->w_cpv.ptr, ws->w_cnd.ptr,
                          ws->pin_small};
    const bool same = std::memcmp(ws->svc_key[kind - 1], key, sizeof(key)) == 0;
    if (ws->svc_running && !same) ws->StopService();
    std::memcpy(ws->svc_key[kind - 1], key, sizeof(key));
    if (kind == 1) ws->svc_args.small = *sa;
    else ws->svc_args.raw = *ra;
    prev = __atomic_load_n(&ws->svc_box->seq, __ATOMIC_ACQUIRE);
    if (!ws->svc_running) SPM_HIP_TRY(launch(prev));
    std::memcpy(const_cast<spm_amd::CoopCall *>(&ws->svc_box->call), &c, sizeof(c));
    __atomic_store_n(&ws->svc_box->seq, (c.pub_seq & 0x3FFFFFFFu) | static_cast<uint32_t>(kind) << 30,
                     __ATOMIC_RELEASE);
    wait_st = ws->svc_stream;
  } else if (kind == 1) {
    SPM_HIP_TRY(spm_amd::LaunchCoopSmall(*sa, c, st));
  } else {
    SPM_HIP_TRY(spm_amd::LaunchCoopRaw(*ra, c, st));
  }
  bool published = false;
  int rc = WaitPublished(c.host_pub, c.pub_seq, wait_st, &published);
  if (rc == SPM_OK && !published && svc) {
    // The server exited (idle) before it saw this request: serve it.
    ws->svc_running = false;
    SPM_HIP_TRY(launch(prev));
    rc = WaitPublished(c.host_pub, c.pub_seq, wait_st, &published);
  }
  if (rc != SPM_OK) {
    ws->svc_running = false;
    return rc;
  }
  if (!published) return Fail(SPM_INTERNAL, std::string(what) + " ended without publishing");
  return SPM_OK;
}

// Raw lines -> final ids of Encode(line, &ids) without extra options, in one
// launch (coop_raw_kernel): the raw image goes up through pinned coherent
// memory, ids and offsets come back there, the host polls the completion
// word.  *done = false: a line the fused path does not take (general-kernel
// lattice, a line past kRawMaxBytes, an output past its capacity).
int EncodeRawCoop(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *raw, const uint64_t *raw_off,
                  uint64_t n, int32_t *ids, uint64_t ids_cap, uint64_t *out_off, hipStream_t st, bool *done) {
  *done = false;
  const spm_amd::SmallLayout l = spm_amd::MakeSmallLayout(spm_amd::SmallKind::kRaw, n, raw_off[n]);
  int rc = ReserveSmall(ws, l);
  if (rc != SPM_OK) return rc;
  uint8_t *h = ws->pin_small;
  uint8_t *d = ws->w_small.as<uint8_t>();
  l.Stage(h, raw_off, raw, n);
  spm_amd::CoopArgs a{ws->w_slot2_len.as<uint8_t>(), nullptr, m->d_uvs.as<uint32_t>(),  // normalized bytes
                      m->d_values.as<int32_t>(), static_cast<uint32_t>(m->trie.units.size()), m->up,
                      nullptr, nullptr, 0, ws->w_slot2_ids.as<int32_t>(), nullptr, nullptr, nullptr, nullptr,
                      ws->w_cpv.as<uint16_t>(), ws->w_cnd.as<uint32_t>(),
                      static_cast<uint32_t>(std::max(m->max_piece_bytes, 4)), nullptr};
  static const bool kSvcProf = std::getenv("SPM_HIP_SERVICE_PROF") != nullptr;  // debug: phase cycles at stop
  if (kSvcProf) {
    if (!ws->svc_prof) {
      SPM_HIP_TRY(spm_amd::DevMalloc(&ws->svc_prof, 16 * 8));
      SPM_HIP_TRY(hipMemset(ws->svc_prof, 0, 16 * 8));
    }
    a.prof = ws->svc_prof;
  }
  spm_amd::CoopRawArgs ra{a,
                          DeviceNormTables(m),
                          reinterpret_cast<const uint32_t *>(h),
                          reinterpret_cast<uint32_t *>(d),
                          m->d_types.as<uint8_t>(),
                          static_cast<int32_t>(m->proto.pieces.size())};
  const spm_amd::CoopCall c = SmallCoopCall(ws, l, n, false);
  rc = RunSmallCall(ws, 2, nullptr, &ra, c, st, "raw-line encode");
  if (rc != SPM_OK) return rc;
  if (static_cast<volatile uint32_t *>(c.host_pub)[1] != 0) {  // not taken
    ws->StopService();  // the caller's fallback may share the server's hardware queue
    return SPM_OK;
  }
  std::memcpy(out_off, l.Tok(h), (n + 1) * 8);
  const uint64_t nt = out_off[n];
  if (nt > ids_cap) return Fail(SPM_RESOURCE_EXHAUSTED, "ids exceed ids_cap");
  if (nt) std::memcpy(ids, l.Ids(h), nt * 4);
  *done = true;
  return SPM_OK;
}

// Host API, very small batches (n <= kCoopSmallMax, unigram models with the
// cooperative kernel's tables): ONE launch of coop_small_kernel, one block
// whose waves encode a sentence each (its trie walks 64 at a time, the
// latency a one-sentence call is made of), with the input read from and the
// outputs written to pinned host memory and completion polled on a host
// word.  *done = false: the caller takes the lane-kernel small path.
int EncodeHostCoop(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *bytes, const uint64_t *off,
                   uint64_t n, int32_t *ids, uint32_t *len, uint64_t *tok, hipStream_t st, bool *done) {
  *done = false;
  const spm_amd::SmallLayout l = spm_amd::MakeSmallLayout(spm_amd::SmallKind::kCoop, n, off[n]);
  int rc = ReserveSmall(ws, l);
  if (rc != SPM_OK) return rc;
  uint8_t *h = ws->pin_small;
  uint8_t *d = ws->w_small.as<uint8_t>();
  l.Stage(h, off, bytes, n);
  spm_amd::CoopArgs a{d, reinterpret_cast<const uint64_t *>(d), m->d_uvs.as<uint32_t>(),
                      m->d_values.as<int32_t>(), static_cast<uint32_t>(m->trie.units.size()), m->up,
                      nullptr, nullptr, 0, ws->w_slot2_ids.as<int32_t>(), ws->w_slot2_len.as<uint32_t>(),
                      nullptr, nullptr, nullptr, ws->w_cpv.as<uint16_t>(), ws->w_cnd.as<uint32_t>(),
                      static_cast<uint32_t>(std::max(m->max_piece_bytes, 4)), nullptr};
  spm_amd::CoopSmallArgs sa{a, reinterpret_cast<const uint32_t *>(h), reinterpret_cast<uint32_t *>(d)};
  const spm_amd::CoopCall c = SmallCoopCall(ws, l, n, len != nullptr);
  volatile uint32_t *pub = c.host_pub;
  if (CoopProf()) {  // this call's phase cycles: one launch on `st`, not through the server
    rc = CoopProfiled(st, [&](uint64_t *prof) {
      spm_amd::CoopSmallArgs sp = sa;
      sp.a.prof = prof;
      return spm_amd::LaunchCoopSmall(sp, c, st);
    });
    if (rc != SPM_OK) return rc;
    if (pub[0] != c.pub_seq) return Fail(SPM_INTERNAL, "cooperative encode ended without publishing");
  } else {
    rc = RunSmallCall(ws, 1, &sa, nullptr, c, st, "cooperative encode");
    if (rc != SPM_OK) return rc;
  }
  if (pub[1] != 0) {  // a sentence it does not take: not done
    ws->StopService();  // the lane-kernel re-run may share the server's hardware queue
    return SPM_OK;
  }
  rc = FinishSmall(m, ws, l, n, 0, -1, ids, len, tok);
  *done = rc == SPM_OK;
  return rc;
}

// The model's tables for the BPE line kernels (bpe_line.hip).
spm_amd::BpeLineArgs BpeLineTables(const spm_hip_model *m) {
  spm_amd::BpeLineArgs a{};
  a.units = m->d_units.as<uint32_t>();
  a.values = m->d_values.as<int32_t>();
  a.entry_piece = m->bpe.entry_piece.as<int32_t>();
  a.entry_out = m->bpe.entry_out.as<int32_t>();
  a.piece_out = m->bpe.piece_out.as<int32_t>();
  a.pair_ent = m->bpe.pair_ent.as<uint4>();
  a.pair_mask = m->bpe.pair_mask;
  a.root_base = m->up.root_base;
  a.unk_id = m->unk_id;
  a.irregular = m->bpe.irregular ? 1 : 0;
  return a;
}

// Whether a BPE handle's small call tries the line kernel: the back-off of
// the unigram small calls (coop_small_rejects).  A vocabulary-restricted
// model, whose merges keep pushing UNUSED pieces, would otherwise pay two
// round trips on every call: after 8 refusals in a row the kernel is skipped,
// every 64th call tries again, and a call it takes resets the count.
bool BpeLineTry(spm_hip_model *m) {
  const uint32_t rejects = m->coop_small_rejects.load(std::memory_order_relaxed);
  if (rejects < 8 || rejects % 64 == 0) return true;
  m->coop_small_rejects.fetch_add(1, std::memory_order_relaxed);
  m->bpe_line_skipped.fetch_add(1, std::memory_order_relaxed);
  return false;
}

// SPM_HIP_BPE_SMALL_HOST=1 (read per call): spm_hip_encode_batch_host sends a
// BPE model's calls of <= kCoopSmallMax sentences to bpe_small_kernel first.
bool BpeSmallHostOn() {
  const char *e = std::getenv("SPM_HIP_BPE_SMALL_HOST");
  return e && std::atoi(e) != 0;
}

void BpeLineTried(spm_hip_model *m, bool taken) {
  if (taken) {
    m->coop_small_rejects.store(0, std::memory_order_relaxed);
    m->bpe_line_taken.fetch_add(1, std::memory_order_relaxed);
  } else {
    m->coop_small_rejects.fetch_add(1, std::memory_order_relaxed);
    m->bpe_line_refused.fetch_add(1, std::memory_order_relaxed);
  }
}

// One BPE small call: its single launch is on `st` already; the wait for
// host_pub[0] == c.pub_seq.  *taken = false: the kernel published "not taken".
int WaitBpeCall(const spm_amd::CoopCall &c, hipStream_t st, const char *what, bool *taken) {
  bool published = false;
  const int rc = WaitPublished(c.host_pub, c.pub_seq, st, &published);
  if (rc != SPM_OK) return rc;
  if (!published) return Fail(SPM_INTERNAL, std::string(what) + " ended without publishing");
  *taken = static_cast<volatile uint32_t *>(c.host_pub)[1] == 0;
  return SPM_OK;
}

// Raw lines -> final ids of Encode(line, &ids) on a BPE model, in one launch
// (bpe_raw_kernel) on the workspace's stream: the staging of EncodeRawCoop,
// no server.  *done = false: a line the kernel does not take (more than
// kBpeLineMaxBytes normalized bytes, a pushed UNUSED piece, on an irregular
// model a char outside the vocabulary).  The call's stats say which it was:
// coop_rest = n when the kernel handed the call back.
int EncodeRawBpe(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *raw, const uint64_t *raw_off,
                 uint64_t n, int32_t *ids, uint64_t ids_cap, uint64_t *out_off, hipStream_t st, bool *done) {
  *done = false;
  const spm_amd::SmallLayout l = spm_amd::MakeSmallLayout(spm_amd::SmallKind::kBpeRaw, n, raw_off[n]);
  int rc = ReserveSmall(ws, l);
  if (rc != SPM_OK) return rc;
  uint8_t *h = ws->pin_small;
  uint8_t *d = ws->w_small.as<uint8_t>();
  l.Stage(h, raw_off, raw, n);
  spm_amd::BpeLineArgs a = BpeLineTables(m);
  a.bytes = ws->w_slot2_len.as<uint8_t>();  // normalized bytes
  a.slot_ids = ws->w_slot2_ids.as<int32_t>();
  a.stage_src = reinterpret_cast<const uint32_t *>(h);
  a.stage_dst = reinterpret_cast<uint32_t *>(d);
  const spm_amd::BpeRawArgs ra{a, DeviceNormTables(m), m->d_types.as<uint8_t>(),
                               static_cast<int32_t>(m->proto.pieces.size())};
  const spm_amd::CoopCall c = SmallCoopCall(ws, l, n, false);
  SPM_HIP_TRY(spm_amd::LaunchBpeRaw(ra, c, st));
  bool taken = false;
  if ((rc = WaitBpeCall(c, st, "BPE raw-line encode", &taken)) != SPM_OK) return rc;
  ws->stats = spm_hip_encode_stats{};
  ws->stats.sentences = n;
  if (!taken) {
    ws->stats.coop_rest = n;
    spm_amd::PublishStats(m, ws->stats);
    return SPM_OK;
  }
  std::memcpy(out_off, l.Tok(h), (n + 1) * 8);
  const uint64_t nt = out_off[n];
  if (nt > ids_cap) return Fail(SPM_RESOURCE_EXHAUSTED, "ids exceed ids_cap");
  if (nt) std::memcpy(ids, l.Ids(h), nt * 4);
  ws->stats.tokens = nt;
  spm_amd::PublishStats(m, ws->stats);
  *done = true;
  return SPM_OK;
}

// Host API, very small batches of a BPE model (n <= kCoopSmallMax): ONE launch
// of bpe_small_kernel, the image and the outputs as in EncodeHostCoop.
// *done = false: the caller takes the staged blocking path.
int EncodeHostBpe(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *bytes, const uint64_t *off,
                  uint64_t n, int32_t *ids, uint32_t *len, uint64_t *tok, hipStream_t st, bool *done) {
  *done = false;
  const spm_amd::SmallLayout l = spm_amd::MakeSmallLayout(spm_amd::SmallKind::kBpe, n, off[n]);
  int rc = ReserveSmall(ws, l);
  if (rc != SPM_OK) return rc;
  uint8_t *h = ws->pin_small;
  uint8_t *d = ws->w_small.as<uint8_t>();
  l.Stage(h, off, bytes, n);
  spm_amd::BpeLineArgs a = BpeLineTables(m);
  a.bytes = d;
  a.slot_ids = ws->w_slot2_ids.as<int32_t>();
  a.slot_len = ws->w_slot2_len.as<uint32_t>();
  a.stage_src = reinterpret_cast<const uint32_t *>(h);
  a.stage_dst = reinterpret_cast<uint32_t *>(d);
  const spm_amd::CoopCall c = SmallCoopCall(ws, l, n, len != nullptr);
  SPM_HIP_TRY(spm_amd::LaunchBpeSmall(a, c, st));
  bool taken = false;
  if ((rc = WaitBpeCall(c, st, "BPE small encode", &taken)) != SPM_OK) return rc;
  if (!taken) return SPM_OK;
  rc = FinishSmall(m, ws, l, n, 0, -1, ids, len, tok);
  *done = rc == SPM_OK;
  return rc;
}

// Host API, small batches (one fast-kernel tile: n <= 256; unigram fast
// kernels; offsets start at 0).  The reference calls Encode once per line
// (spm_encode_main.cc:189-191, model_interface.h:117); the blocking path
// costs that four synchronizations, pageable copies and a dozen launches.
// Here the fast kernel's single tile reads the offsets and the bytes straight
// from the pinned image, zeroes the control block itself, and writes the
// final ids / lengths / token offsets into the image (its slots are the
// outputs: one tile whose slots start at byte 0, no tile compaction); the
// status words come back with the publication word the host polls.  Only a
// batch the fast kernel flagged runs the general kernel and the fix-up chain,
// with a second round trip.  *done = false: the caller takes the general
// blocking path (a device-path overflow).
int EncodeHostSmall(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *bytes, const uint64_t *off,
                    uint64_t n, int32_t *ids, uint32_t *len, uint64_t *tok, hipStream_t st, bool *done) {
  *done = false;
  const uint64_t total = off[n];
  const uint64_t ctl_bytes = spm_amd::kStWords * 4 + 8 * (spm_amd::FastTiles(n) + spm_amd::kScanTiles);
  const auto l = spm_amd::MakeSmallLayout(spm_amd::SmallKind::kLane, n, total, len != nullptr, ctl_bytes);
  int rc = ReserveSmall(ws, l);
  if (rc != SPM_OK) return rc;
  uint8_t *h = ws->pin_small;
  uint8_t *d = ws->w_small.as<uint8_t>();
  l.Stage(h, off, bytes, n);
  volatile uint32_t *pub = l.Pub(h);
  const uint32_t seq = NextPubSeq(ws);
  spm_amd::EncodeCall c{l.In(d), l.Off(d), n, total, l.Ids(h), len ? l.Len(h) : nullptr, l.Tok(h), nullptr,
                        st, false, 0};
  FastPlan fp;
  rc = FastSetup(m, ws, c, reinterpret_cast<uint32_t *>(d), &fp);
  if (rc != SPM_OK) return rc;
  fp.l.stage_src = reinterpret_cast<const uint32_t *>(h);
  fp.l.stage_dst = reinterpret_cast<uint32_t *>(d);
  fp.l.stage_zero = l.zero_words();
  fp.l.stage_words = l.stage_words();
  fp.l.host_pub = l.Pub(h);
  fp.l.pub_seq = seq;
  rc = FastPartA(m, ws, c, &fp, false);
  if (rc != SPM_OK) {
    (void)hipStreamSynchronize(st);  // nothing may still read h when it is reused
    return rc;
  }
  bool published = false;
  if ((rc = WaitPublished(pub, seq, st, &published)) != SPM_OK) return rc;
  uint32_t sw[spm_amd::kStWords];
  if (published) {
    for (int k = 0; k < spm_amd::kStWords; ++k) sw[k] = pub[1 + k];
  } else {  // the kernel ended early: the status words say why
    SPM_HIP_TRY(hipMemcpy(sw, d, sizeof(sw), hipMemcpyDeviceToHost));
  }
  const uint32_t flagged = sw[spm_amd::kStFlagged];
  if (sw[spm_amd::kStError]) {
    SPM_HIP_TRY(hipStreamSynchronize(st));
    return SPM_OK;  // not done: the blocking path
  }
  if (flagged) {
    // Rare: the general kernel and the fix-up chain over the flagged
    // sentences (they update the outputs in h), then one synchronization.
    if ((rc = FastPartB(m, ws, c, &fp)) != SPM_OK) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    SPM_HIP_TRY(hipMemcpyAsync(l.LateStatus(h), d, 16, hipMemcpyDeviceToHost, st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
    if (l.LateStatus(h)[spm_amd::kStError]) return SPM_OK;
  }
  rc = FinishSmall(m, ws, l, n, flagged, fp.slot, ids, len, tok);
  *done = rc == SPM_OK;
  return rc;
}

// Blocking SampleEncode on a leased workspace: LatticeTiers' two tiers leave
// the draws in the right-aligned slots, then scan + compaction.
int SampleBlocking(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *d_bytes, const uint64_t *d_off,
                   uint64_t n, float theta, uint64_t seed, uint64_t index_base, int32_t *d_ids, uint32_t *d_len,
                   uint64_t *d_tok, hipStream_t st) {
  uint64_t total = 0;
  int rc = BatchBytes(ws, d_off, n, st, &total);
  if (rc != SPM_OK) return rc;
  ws->stats = spm_hip_encode_stats{};
  if (n == 0) {
    SPM_HIP_TRY(hipMemsetAsync(d_tok, 0, sizeof(uint64_t), st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
    spm_amd::PublishStats(m, ws->stats);
    return SPM_OK;
  }
  const uint64_t cap = std::max<uint64_t>(total, 1);
  SPM_HIP_TRY(ws->w_slot2_ids.Reserve(cap * 4));
  if (d_len) SPM_HIP_TRY(ws->w_slot2_len.Reserve(cap * 4));
  SPM_HIP_TRY(ws->w_ntok.Reserve(n * 4));
  int32_t *s2 = ws->w_slot2_ids.as<int32_t>();
  uint32_t *s2l = d_len ? ws->w_slot2_len.as<uint32_t>() : nullptr;
  const uint32_t num_units = static_cast<uint32_t>(m->trie.units.size());
  if (!m->force_general) {
    SPM_HIP_TRY(ws->w_salpha.Reserve((cap + n + 1) * 4));
    SPM_HIP_TRY(ws->w_smask.Reserve((cap + n + 1) * 8));
  }
  auto fast = [&](uint32_t *status) {
    const spm_amd::SampleFastArgs f{d_bytes, d_off, n, total, m->d_units.as<uint32_t>(), m->d_values.as<int32_t>(),
                                    m->d_scores.as<float>(), num_units, m->up, theta, seed, index_base,
                                    ws->w_salpha.as<float>(), ws->w_smask.as<uint64_t>(), s2, s2l,
                                    ws->w_ntok.as<uint32_t>(), ws->w_flagged.as<uint32_t>(), status};
    return spm_amd::LaunchUnigramSampleFast(f, st);
  };
  // The exact tier over the sentences of g (SampleExactArgs ends with GeneralLaunch's fields).
  auto exact = [&](const spm_amd::GeneralLaunch &g) {
    const spm_amd::SampleExactArgs x{d_bytes, d_off, m->d_units.as<uint32_t>(), m->d_values.as<int32_t>(),
                                     m->d_scores.as<float>(), num_units, m->up, theta, seed, index_base,
                                     g.slot_ids, g.slot_len, g.ntok, g.list, g.count, g.list_n, g.scratch,
                                     g.slab_bytes, g.max_nb, g.ovf_list, g.ovf_count, g.error, g.threads};
    return spm_amd::LaunchUnigramSampleExact(x, st);
  };
  rc = LatticeTiers(m, ws, d_off, n, cap, s2, s2l, "sentence too long for the exact sampling path",
                    "exact sampling path: scratch overflow or broken walk", st, fast, exact);
  if (rc != SPM_OK) return rc;
  rc = CompactSlots(ws, d_off, n, s2, s2l, d_ids, d_len, d_tok, ws->w_ctl.as<uint32_t>(), nullptr, st);
  if (rc != SPM_OK) return rc;
  SPM_HIP_TRY(hipStreamSynchronize(st));
  return SPM_OK;
}

int SampleArgsCheck(const spm_hip_model *m, float theta) {
  if (!std::isfinite(theta)) return Fail(SPM_INVALID_ARGUMENT, "theta must be finite");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (m->model_type != spm_amd::kUnigram)
    return Fail(SPM_UNIMPLEMENTED, "SampleEncode is implemented for unigram models only");
  return SPM_OK;
}

// Host batch entry points: offsets that start at 0 and never decrease.
int HostOffsetsCheck(const uint64_t *off, uint64_t n) {
  if (off[0] != 0) return Fail(SPM_INVALID_ARGUMENT, "offsets must start at 0");
  for (uint64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return Fail(SPM_INVALID_ARGUMENT, "offsets must not decrease");
  return SPM_OK;
}

// The workspace's device copies of a host batch (h_in, h_off), uploaded.
int StageHostInput(spm_amd::EncodeWorkspace *ws, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                   uint64_t total, hipStream_t st) {
  SPM_HIP_TRY(ws->h_in.Reserve(std::max<uint64_t>(total, 1)));
  SPM_HIP_TRY(ws->h_off.Reserve((n + 1) * 8));
  if (total) SPM_HIP_TRY(hipMemcpyAsync(ws->h_in.ptr, bytes, total, hipMemcpyHostToDevice, st));
  SPM_HIP_TRY(hipMemcpyAsync(ws->h_off.ptr, off, (n + 1) * 8, hipMemcpyHostToDevice, st));
  return SPM_OK;
}

// ... and the output buffers of an encode or a SampleEncode (h_ids, h_len,
// h_tok) sized.
int StageHostBatch(spm_amd::EncodeWorkspace *ws, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                   uint64_t total, bool with_len, hipStream_t st) {
  const int rc = StageHostInput(ws, bytes, off, n, total, st);
  if (rc != SPM_OK) return rc;
  SPM_HIP_TRY(ws->h_ids.Reserve(std::max<uint64_t>(total, 1) * 4));
  if (with_len) SPM_HIP_TRY(ws->h_len.Reserve(std::max<uint64_t>(total, 1) * 4));
  SPM_HIP_TRY(ws->h_tok.Reserve((n + 1) * 8));
  return SPM_OK;
}

// ... and the results back: token offsets first, then tok[n] ids / lengths;
// publishes the call's stats.
int FetchHostBatch(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, uint64_t n, int32_t *ids, uint32_t *len,
                   uint64_t *tok, hipStream_t st) {
  SPM_HIP_TRY(hipMemcpyAsync(tok, ws->h_tok.ptr, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  const uint64_t ntok = tok[n];
  if (ntok) {
    SPM_HIP_TRY(hipMemcpyAsync(ids, ws->h_ids.ptr, ntok * 4, hipMemcpyDeviceToHost, st));
    if (len) SPM_HIP_TRY(hipMemcpyAsync(len, ws->h_len.ptr, ntok * 4, hipMemcpyDeviceToHost, st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
  }
  ws->stats.tokens = ntok;
  spm_amd::PublishStats(m, ws->stats);
  return SPM_OK;
}


// ---- NBestEncode --------------------------------------------------------
constexpr uint32_t kNBestSmallNb = 256;       // first tier: sentences up to this many bytes
constexpr uint32_t kNBestLanes = 131072;      // first tier lanes, halved while the pool exceeds kNBestPool
constexpr uint64_t kNBestPool = 4ull << 30;
constexpr uint32_t kNBestLanes2 = 4096;       // second tier: at most this many lanes
constexpr uint64_t kNBestMaxSlab = 4ull << 30;  // a longer sentence's lattice goes to the host
constexpr uint64_t kNBestStageFull = 32ull << 20;  // token staging up to this many entries is sized by its bound

spm_amd::HostNBestTables HostTables(const spm_hip_model *m, const std::vector<float> &scores) {
  return spm_amd::HostNBestTables{m->trie.units.data(), static_cast<uint32_t>(m->trie.units.size()),
                                  m->trie.values.data(), scores.data(), m->up};
}

int NBestArgsCheck(const spm_hip_model *m) {
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (m->model_type != spm_amd::kUnigram)
    return Fail(SPM_UNIMPLEMENTED, "NBestEncode is implemented for unigram models only");
  return SPM_OK;
}

// The search of one n-best call on a leased workspace: the two device tiers
// and the host tier, then the two offset scans.  Leaves npaths / stage /
// per-path counts and scores / token staging in the workspace, path offsets
// in w_nb_poff and token offsets in w_nb_toff, and returns the totals.
// h_bytes: the batch's bytes on the host when the caller has them (else the
// host tier copies its sentences from the device).
int NBestSearch(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *d_bytes, const uint64_t *d_off,
                const uint8_t *h_bytes, uint64_t n, int N, bool with_len, uint64_t *total_paths,
                uint64_t *total_tokens, hipStream_t st) {
  *total_paths = *total_tokens = 0;
  std::vector<uint64_t> off(n + 1);
  SPM_HIP_TRY(hipMemcpyAsync(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  uint32_t max_nb = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (off[i + 1] < off[i]) return Fail(SPM_INVALID_ARGUMENT, "offsets must not decrease");
    if (off[i + 1] - off[i] > 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "sentence too long");
    max_nb = std::max<uint32_t>(max_nb, static_cast<uint32_t>(off[i + 1] - off[i]));
  }
  const uint64_t total = off[n] - off[0];
  if (n * static_cast<uint64_t>(N) >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many paths in one batch");
  const int K = m->up.trie_results_size;
  // Plan.  First tier: every sentence of <= nb1 bytes, hyps1 hypotheses each.
  const uint32_t nb1 = std::max<uint32_t>(std::min(max_nb, kNBestSmallNb), 1);
  const uint32_t knob1 = m->nbest_hyps1.load(), knob2 = m->nbest_hyps2.load();
  uint32_t hyps1 = 2, hyps2 = 2;
  if (N > 1) {
    hyps1 = knob1 ? std::max(knob1, 2u) : 40u * N + 4u * nb1 + 64u;
    hyps2 = knob2 ? std::max(knob2, 2u) : 16u * hyps1;
  }
  const uint64_t slab1 = spm_amd::UnigramNBestSlabBytes(nb1, K, hyps1);
  uint32_t lanes1 = static_cast<uint32_t>(std::min<uint64_t>((n + 63) / 64 * 64, kNBestLanes));
  while (lanes1 > 64 && lanes1 * slab1 > kNBestPool) lanes1 /= 2;
  // Second tier: the longest sentence when its slab can be had, with the
  // pool split among as many lanes as fit.
  uint32_t nb2 = std::max<uint32_t>(max_nb, 1);
  uint64_t slab2 = spm_amd::UnigramNBestSlabBytes(nb2, K, hyps2);
  if (slab2 > kNBestMaxSlab) {
    nb2 = nb1;
    slab2 = spm_amd::UnigramNBestSlabBytes(nb2, K, hyps2);
  }
  if (slab2 > kNBestMaxSlab) return Fail(SPM_RESOURCE_EXHAUSTED, "n-best hypothesis arena too large");
  const uint64_t pool = std::max<uint64_t>(lanes1 * slab1, slab2);
  const uint32_t lanes2 = static_cast<uint32_t>(std::min<uint64_t>(pool / slab2, kNBestLanes2));
  SPM_HIP_TRY(ws->w_scratch.Reserve(pool));
  SPM_HIP_TRY(ws->w_ovf.Reserve(n * 4));
  SPM_HIP_TRY(ws->w_nb_ovf2.Reserve(n * 4));
  SPM_HIP_TRY(ws->w_nb_ctl.Reserve(16));
  SPM_HIP_TRY(ws->w_nb_npaths.Reserve(n * 4));
  SPM_HIP_TRY(ws->w_nb_stage.Reserve(n * 8));
  SPM_HIP_TRY(ws->w_nb_ntok.Reserve(n * N * 4));
  SPM_HIP_TRY(ws->w_nb_score.Reserve(n * N * 4));
  SPM_HIP_TRY(ws->w_nb_poff.Reserve((n + 1) * 8));
  SPM_HIP_TRY(hipMemsetAsync(ws->w_nb_npaths.ptr, 0, n * 4, st));
  // Token staging: at most one token per byte per path; large batches start
  // with a third of that bound and run again when the cursor passes it.
  const uint64_t full = std::max<uint64_t>(total * N, 1);
  uint64_t stage_cap = full <= kNBestStageFull ? full : std::max<uint64_t>(kNBestStageFull, full / 3);
  uint32_t *ctl = ws->w_nb_ctl.as<uint32_t>();
  uint32_t second = 0, host = 0;
  const bool timing = TimedSlot(m, ws) >= 0;
  for (int attempt = 0;; ++attempt) {
    SPM_HIP_TRY(ws->w_nb_ids.Reserve(stage_cap * 4));
    if (with_len) SPM_HIP_TRY(ws->w_nb_len.Reserve(stage_cap * 4));
    SPM_HIP_TRY(hipMemsetAsync(ctl, 0, 16, st));
    spm_amd::NBestLaunch a{d_bytes, d_off, m->d_units.as<uint32_t>(), m->d_values.as<int32_t>(),
                           m->d_scores.as<float>(), static_cast<uint32_t>(m->trie.units.size()), m->up, N,
                           nullptr, nullptr, n, ws->w_scratch.as<uint8_t>(), slab1, nb1, hyps1, lanes1,
                           ws->w_ovf.as<uint32_t>(), ctl, ws->w_nb_npaths.as<uint32_t>(),
                           ws->w_nb_stage.as<uint64_t>(), ws->w_nb_ntok.as<uint32_t>(), ws->w_nb_score.as<float>(),
                           ws->w_nb_ids.as<int32_t>(), with_len ? ws->w_nb_len.as<uint32_t>() : nullptr, stage_cap,
                           reinterpret_cast<unsigned long long *>(ctl + 2)};
    if (timing) SPM_HIP_TRY(hipEventRecord(ws->ev[0], st));
    SPM_HIP_TRY(spm_amd::LaunchUnigramNBest(a, st));
    // The overflow list with the pool split among fewer lanes (a device no-op
    // when the list is empty).
    a.list = ws->w_ovf.as<uint32_t>();
    a.count = ctl;
    a.list_n = 0;
    a.slab_bytes = slab2;
    a.max_nb = nb2;
    a.max_hyps = hyps2;
    a.lanes = lanes2;
    a.ovf_list = ws->w_nb_ovf2.as<uint32_t>();
    a.ovf_count = ctl + 1;
    SPM_HIP_TRY(spm_amd::LaunchUnigramNBest(a, st));
    if (timing) SPM_HIP_TRY(hipEventRecord(ws->ev[1], st));
    SPM_HIP_TRY(hipMemcpyAsync(ws->pinned, ctl, 16, hipMemcpyDeviceToHost, st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
    second = ws->pinned[0];
    host = ws->pinned[1];
    uint64_t cursor = 0;
    std::memcpy(&cursor, ws->pinned + 2, 8);
    if (cursor <= stage_cap) break;
    if (attempt == 1) return Fail(SPM_INTERNAL, "n-best token staging overflow");
    stage_cap = cursor;
  }
  if (second > n || host > second) return Fail(SPM_INTERNAL, "n-best overflow lists are inconsistent");
  // Host tier: the same search over the host tables, its tokens in a staging
  // buffer of their own (kNBestHostStage in stage[i]).  Sized for the few
  // sentences expected there: one thread, four small uploads per sentence and,
  // for a device-pointer call, one download of its bytes.
  if (host) {
    std::vector<uint32_t> list(host);
    SPM_HIP_TRY(hipMemcpyAsync(list.data(), ws->w_nb_ovf2.ptr, host * 4ull, hipMemcpyDeviceToHost, st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
    const spm_amd::HostNBestTables t = HostTables(m, m->host_scores);
    std::vector<int32_t> hids;
    std::vector<uint32_t> hlen;
    std::vector<std::vector<uint32_t>> rows_ntok(host);
    std::vector<std::vector<float>> rows_score(host);
    std::vector<uint32_t> npaths(host);
    std::vector<uint64_t> stage(host);
    std::vector<uint8_t> sent;
    std::vector<spm_amd::HostNBestPath> paths;
    for (uint32_t j = 0; j < host; ++j) {
      const uint32_t i = list[j];
      if (i >= n) return Fail(SPM_INTERNAL, "n-best overflow list is out of range");
      const uint32_t nb = static_cast<uint32_t>(off[i + 1] - off[i]);
      const uint8_t *s = h_bytes ? h_bytes + off[i] : nullptr;
      if (!s) {
        sent.resize(nb);
        SPM_HIP_TRY(hipMemcpyAsync(sent.data(), d_bytes + off[i], nb, hipMemcpyDeviceToHost, st));
        SPM_HIP_TRY(hipStreamSynchronize(st));
        s = sent.data();
      }
      spm_amd::HostNBest(t, s, nb, N, spm_amd::kNBestMaxAgenda, &paths, nullptr);
      npaths[j] = static_cast<uint32_t>(paths.size());
      stage[j] = spm_amd::kNBestHostStage | hids.size();
      for (const auto &p : paths) {
        rows_ntok[j].push_back(static_cast<uint32_t>(p.ids.size()));
        rows_score[j].push_back(p.score);
        hids.insert(hids.end(), p.ids.begin(), p.ids.end());
        hlen.insert(hlen.end(), p.lens.begin(), p.lens.end());
      }
    }
    SPM_HIP_TRY(ws->w_nb_hids.Reserve(std::max<size_t>(hids.size(), 1) * 4));
    if (with_len) SPM_HIP_TRY(ws->w_nb_hlen.Reserve(std::max<size_t>(hids.size(), 1) * 4));
    if (!hids.empty()) {
      SPM_HIP_TRY(hipMemcpyAsync(ws->w_nb_hids.ptr, hids.data(), hids.size() * 4, hipMemcpyHostToDevice, st));
      if (with_len)
        SPM_HIP_TRY(hipMemcpyAsync(ws->w_nb_hlen.ptr, hlen.data(), hlen.size() * 4, hipMemcpyHostToDevice, st));
    }
    for (uint32_t j = 0; j < host; ++j) {
      const uint64_t i = list[j];
      SPM_HIP_TRY(hipMemcpyAsync(ws->w_nb_npaths.as<uint32_t>() + i, &npaths[j], 4, hipMemcpyHostToDevice, st));
      SPM_HIP_TRY(hipMemcpyAsync(ws->w_nb_stage.as<uint64_t>() + i, &stage[j], 8, hipMemcpyHostToDevice, st));
      SPM_HIP_TRY(hipMemcpyAsync(ws->w_nb_ntok.as<uint32_t>() + i * N, rows_ntok[j].data(), npaths[j] * 4ull,
                                 hipMemcpyHostToDevice, st));
      SPM_HIP_TRY(hipMemcpyAsync(ws->w_nb_score.as<float>() + i * N, rows_score[j].data(), npaths[j] * 4ull,
                                 hipMemcpyHostToDevice, st));
    }
    SPM_HIP_TRY(hipStreamSynchronize(st));  // the copies read these vectors
  }
  // path_off = scan of npaths; tok_off = scan of the paths' token counts.
  size_t tmp = 0;
  SPM_HIP_TRY(spm_amd::LaunchNBestPathOffsets(ws->w_nb_npaths.as<uint32_t>(), n, ws->w_nb_poff.as<uint64_t>(), nullptr,
                                              &tmp, st));
  SPM_HIP_TRY(ws->w_scan.Reserve(tmp + 16));
  SPM_HIP_TRY(spm_amd::LaunchNBestPathOffsets(ws->w_nb_npaths.as<uint32_t>(), n, ws->w_nb_poff.as<uint64_t>(),
                                              ws->w_scan.ptr, &tmp, st));
  uint64_t P = 0, T = 0;
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned + 4, ws->w_nb_poff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(&P, ws->pinned + 4, 8);
  if (P > n * static_cast<uint64_t>(N)) return Fail(SPM_INTERNAL, "n-best path count out of range");
  SPM_HIP_TRY(ws->w_nb_ptok.Reserve(std::max<uint64_t>(P, 1) * 4));
  SPM_HIP_TRY(ws->w_nb_toff.Reserve((P + 1) * 8));
  SPM_HIP_TRY(spm_amd::LaunchNBestTokOffsets(n, N, ws->w_nb_npaths.as<uint32_t>(), ws->w_nb_poff.as<uint64_t>(),
                                             ws->w_nb_ntok.as<uint32_t>(), P, ws->w_nb_ptok.as<uint32_t>(),
                                             ws->w_nb_toff.as<uint64_t>(), nullptr, &tmp, st));
  SPM_HIP_TRY(ws->w_scan.Reserve(tmp + 16));
  SPM_HIP_TRY(spm_amd::LaunchNBestTokOffsets(n, N, ws->w_nb_npaths.as<uint32_t>(), ws->w_nb_poff.as<uint64_t>(),
                                             ws->w_nb_ntok.as<uint32_t>(), P, ws->w_nb_ptok.as<uint32_t>(),
                                             ws->w_nb_toff.as<uint64_t>(), ws->w_scan.ptr, &tmp, st));
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned + 6, ws->w_nb_toff.as<uint64_t>() + P, 8, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(&T, ws->pinned + 6, 8);
  *total_paths = P;
  *total_tokens = T;
  ws->stats = spm_hip_encode_stats{};
  ws->stats.sentences = n;
  ws->stats.tokens = T;
  ws->stats.general_path = n;
  if (timing) {
    SPM_HIP_TRY(hipEventElapsedTime(&ws->stats.general_kernel_ms, ws->ev[0], ws->ev[1]));
    ws->tcount = 0;
  }
  spm_amd::PublishStats(m, ws->stats);
  {
    std::lock_guard<std::mutex> lk(m->pool_mu);
    m->nbest_second = second;
    m->nbest_host = host;
  }
  return SPM_OK;
}

// The searched call's blocks to their final places (device pointers).
int NBestGatherTo(spm_amd::EncodeWorkspace *ws, uint64_t n, int N, int32_t *d_ids, uint32_t *d_len, float *d_scores,
                  hipStream_t st) {
  const spm_amd::NBestGather g{n, static_cast<uint32_t>(N), ws->w_nb_poff.as<uint64_t>(),
                               ws->w_nb_toff.as<uint64_t>(), ws->w_nb_stage.as<uint64_t>(),
                               ws->w_nb_score.as<float>(), ws->w_nb_ids.as<int32_t>(), ws->w_nb_len.as<uint32_t>(),
                               ws->w_nb_hids.as<int32_t>(), ws->w_nb_hlen.as<uint32_t>(), d_ids, d_len, d_scores};
  SPM_HIP_TRY(spm_amd::LaunchNBestGather(g, st));
  return SPM_OK;
}

}  // namespace

int spm_hip_encode_raw_small_host(spm_hip_model *m, const uint8_t *raw, const uint64_t *raw_off, uint64_t n,
                                  int32_t *ids, uint64_t ids_cap, uint64_t *out_off) {
  spm_amd::TraceRange trace_range_("spm_hip_encode_raw_small_host");
  if (!m || !raw_off || !out_off || (n && !raw && raw_off[n])) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  // The fused launch merges unknown runs; under byte fallback they expand
  // instead (spm_hip_finalize_ids_bytes), so the caller takes the batch path.
  // NeedsHostSized: force_general, a unigram model without a fast kernel, a
  // BPE model with USER_DEFINED pieces.
  const bool bpe = m->model_type == spm_amd::kBpe;
  if (n == 0 || n > spm_amd::kCoopSmallMax || raw_off[0] != 0 || raw_off[n] > kSmallMaxBytes / 8 ||
      m->byte_fallback || (m->model_type != spm_amd::kUnigram && !bpe) || NeedsHostSized(m) ||
      (!bpe && (!m->d_uvs.ptr || m->max_piece_bytes > 56)))
    return SPM_UNIMPLEMENTED;
  for (uint64_t i = 0; i < n; ++i)
    if (raw_off[i + 1] < raw_off[i]) return Fail(SPM_INVALID_ARGUMENT, "offsets must not decrease");
  int rc = EnsureNormTables(m);
  if (rc == SPM_OK) rc = EnsureTypes(m);
  if (rc != SPM_OK) return rc;
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  bool done = false;
  if (bpe) {
    if (!BpeLineTry(m)) {
      ws->stats = spm_hip_encode_stats{};
      ws->stats.sentences = n;
      spm_amd::PublishStats(m, ws->stats);
      return SPM_UNIMPLEMENTED;
    }
    rc = EncodeRawBpe(m, ws.get(), raw, raw_off, n, ids, ids_cap, out_off, ws.stream(), &done);
    if (rc != SPM_OK) return rc;
    BpeLineTried(m, done);
    return done ? SPM_OK : SPM_UNIMPLEMENTED;
  }
  rc = EncodeRawCoop(m, ws.get(), raw, raw_off, n, ids, ids_cap, out_off, ws.stream(), &done);
  if (rc != SPM_OK) return rc;
  return done ? SPM_OK : SPM_UNIMPLEMENTED;
}

int spm_hip_encode_batch_host(spm_hip_model *m, const uint8_t *bytes, const uint64_t *off,
                              uint64_t n, int32_t *ids, uint32_t *len, uint64_t *tok) {
  spm_amd::TraceRange trace_range_("spm_hip_encode_batch_host");
  if (!m || !off || !tok) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  const uint64_t total = off[n] - off[0];
  if (off[0] != 0) return Fail(SPM_INVALID_ARGUMENT, "offsets must start at 0");
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  hipStream_t st = ws.stream();
  if (n >= 1 && n <= kSmallMaxSentences && total <= kSmallMaxBytes && m->model_type == spm_amd::kUnigram &&
      m->kernel != spm_amd::UnigramKernel::kGeneralOnly && !NeedsHostSized(m)) {
    bool done = false;
    // A model whose small calls the cooperative kernel keeps handing back
    // (broken UTF-8, > 8 nodes at a position: each costs a second round
    // trip) skips it after 8 rejections in a row, trying again every 64th
    // call; a call it takes resets the count.
    const uint32_t rejects = m->coop_small_rejects.load(std::memory_order_relaxed);
    const bool try_coop = rejects < 8 || rejects % 64 == 0;
    if (!try_coop) m->coop_small_rejects.fetch_add(1, std::memory_order_relaxed);
    if (try_coop && n <= spm_amd::kCoopSmallMax && m->d_uvs.ptr && m->max_piece_bytes <= 56 &&
        !m->force_general) {
      const int rc = EncodeHostCoop(m, ws.get(), bytes, off, n, ids, len, tok, st, &done);
      if (rc != SPM_OK) return rc;
      if (done) {
        m->coop_small_rejects.store(0, std::memory_order_relaxed);
        return rc;
      }
      m->coop_small_rejects.fetch_add(1, std::memory_order_relaxed);
    }
    const int rc = EncodeHostSmall(m, ws.get(), bytes, off, n, ids, len, tok, st, &done);
    if (rc != SPM_OK || done) return rc;
  }
  // BPE, with SPM_HIP_BPE_SMALL_HOST=1: n <= kCoopSmallMax sentences through
  // bpe_small_kernel first (one launch); a call it does not take falls to the
  // staged path below, and the call's stats then carry coop_rest = n.  Off by
  // default: through this entry the batch tiers' routing (general_path) is
  // pinned down to batches of one sentence.
  uint64_t bpe_refused = 0;
  if (n >= 1 && n <= spm_amd::kCoopSmallMax && total <= kSmallMaxBytes && m->model_type == spm_amd::kBpe &&
      !NeedsHostSized(m) && BpeSmallHostOn() && BpeLineTry(m)) {
    bool done = false;
    const int rc = EncodeHostBpe(m, ws.get(), bytes, off, n, ids, len, tok, st, &done);
    if (rc != SPM_OK) return rc;
    BpeLineTried(m, done);
    if (done) return rc;
    bpe_refused = n;
  }
  int rc = StageHostBatch(ws.get(), bytes, off, n, total, len != nullptr, st);
  if (rc != SPM_OK) return rc;
  rc = EncodeBlocking(m, ws.get(), ws->h_in.as<uint8_t>(), ws->h_off.as<uint64_t>(), n,
                      ws->h_ids.as<int32_t>(), len ? ws->h_len.as<uint32_t>() : nullptr,
                      ws->h_tok.as<uint64_t>(), st);
  if (rc != SPM_OK) return rc;
  rc = FetchHostBatch(m, ws.get(), n, ids, len, tok, st);
  if (rc == SPM_OK && bpe_refused) {
    ws->stats.coop_rest = bpe_refused;
    spm_amd::PublishStats(m, ws->stats);
  }
  return rc;
}

int spm_hip_sample_encode_batch(spm_hip_model *m, const uint8_t *d_bytes, const uint64_t *d_off, uint64_t n,
                                float theta, uint64_t seed, uint64_t index_base, int32_t *d_ids, uint32_t *d_len,
                                uint64_t *d_tok, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_sample_encode_batch");
  if (!m || (!d_off) || (!d_tok) || (n && !d_ids)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  const int rc = SampleArgsCheck(m, theta);
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return SampleBlocking(m, ws.get(), d_bytes, d_off, n, theta, seed, index_base, d_ids, d_len, d_tok, st);
}

int spm_hip_sample_encode_batch_host(spm_hip_model *m, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                                     float theta, uint64_t seed, uint64_t index_base, int32_t *ids, uint32_t *len,
                                     uint64_t *tok) {
  spm_amd::TraceRange trace_range_("spm_hip_sample_encode_batch_host");
  if (!m || !off || !tok) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  int rc = SampleArgsCheck(m, theta);
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  if ((rc = HostOffsetsCheck(off, n)) != SPM_OK) return rc;
  const uint64_t total = off[n];
  if (total && (!bytes || !ids)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  hipStream_t st = ws.stream();
  rc = StageHostBatch(ws.get(), bytes, off, n, total, len != nullptr, st);
  if (rc != SPM_OK) return rc;
  rc = SampleBlocking(m, ws.get(), ws->h_in.as<uint8_t>(), ws->h_off.as<uint64_t>(), n, theta, seed, index_base,
                      ws->h_ids.as<int32_t>(), len ? ws->h_len.as<uint32_t>() : nullptr, ws->h_tok.as<uint64_t>(),
                      st);
  if (rc != SPM_OK) return rc;
  return FetchHostBatch(m, ws.get(), n, ids, len, tok, st);
}

// ---------------------------------------------------------------------------
// BPE-dropout (bpe_dropout.hip, bpe_general_kernel<true>): EncodeBlocking's
// tiers with every popped pair masked by the sentence's draw stream.
namespace {

// ceil(alpha * 2^53) clamped to [0, 2^53]: a draw's 53 bits are below it
// exactly when SampleDraw < (double) alpha (alpha * 2^53 is exact in double).
bool BpeDropoutThreshold(float alpha, uint64_t *t) {
  if (std::isnan(alpha)) return false;
  const double a = static_cast<double>(alpha);
  *t = a <= 0.0 ? 0ull : a >= 1.0 ? (1ull << 53) : static_cast<uint64_t>(std::ceil(a * 0x1.0p53));
  return true;
}

int BpeDropoutArgsCheck(const spm_hip_model *m, float alpha, spm_amd::BpeDropout *drop) {
  if (!BpeDropoutThreshold(alpha, &drop->threshold)) return Fail(SPM_INVALID_ARGUMENT, "alpha must not be NaN");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (m->model_type != spm_amd::kBpe)
    return Fail(SPM_UNIMPLEMENTED, "BPE-dropout is implemented for BPE models only");
  return SPM_OK;
}

}  // namespace

int spm_hip_bpe_dropout_threshold(float alpha, uint64_t *threshold) {
  if (!threshold) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (!BpeDropoutThreshold(alpha, threshold)) return Fail(SPM_INVALID_ARGUMENT, "alpha must not be NaN");
  return SPM_OK;
}

int spm_hip_bpe_dropout_encode_batch(spm_hip_model *m, const uint8_t *d_bytes, const uint64_t *d_off, uint64_t n,
                                     float alpha, uint64_t seed, uint64_t index_base, int32_t *d_ids,
                                     uint32_t *d_len, uint64_t *d_tok, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_bpe_dropout_encode_batch");
  if (!m || (!d_off) || (!d_tok) || (n && !d_ids)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  spm_amd::BpeDropout drop{0, seed, index_base};
  const int rc = BpeDropoutArgsCheck(m, alpha, &drop);
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return EncodeBlocking(m, ws.get(), d_bytes, d_off, n, d_ids, d_len, d_tok, st, &drop);
}

int spm_hip_bpe_dropout_encode_batch_host(spm_hip_model *m, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                                          float alpha, uint64_t seed, uint64_t index_base, int32_t *ids,
                                          uint32_t *len, uint64_t *tok) {
  spm_amd::TraceRange trace_range_("spm_hip_bpe_dropout_encode_batch_host");
  if (!m || !off || !tok) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  spm_amd::BpeDropout drop{0, seed, index_base};
  int rc = BpeDropoutArgsCheck(m, alpha, &drop);
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  if ((rc = HostOffsetsCheck(off, n)) != SPM_OK) return rc;
  const uint64_t total = off[n];
  if (total && (!bytes || !ids)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  hipStream_t st = ws.stream();
  rc = StageHostBatch(ws.get(), bytes, off, n, total, len != nullptr, st);
  if (rc != SPM_OK) return rc;
  rc = EncodeBlocking(m, ws.get(), ws->h_in.as<uint8_t>(), ws->h_off.as<uint64_t>(), n, ws->h_ids.as<int32_t>(),
                      len ? ws->h_len.as<uint32_t>() : nullptr, ws->h_tok.as<uint64_t>(), st, &drop);
  if (rc != SPM_OK) return rc;
  return FetchHostBatch(m, ws.get(), n, ids, len, tok, st);
}

// ---------------------------------------------------------------------------
// Lattice scores (unigram_lattice_score.hip): CalculateEntropy and
// SampleEncodeAndScore.
namespace {

int LatticeScoreArgsCheck(const spm_hip_model *m, float theta, const char *what) {
  if (!std::isfinite(theta)) return Fail(SPM_INVALID_ARGUMENT, "theta must be finite");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  if (m->model_type != spm_amd::kUnigram)
    return Fail(SPM_UNIMPLEMENTED, std::string(what) + " is implemented for unigram models only");
  return SPM_OK;
}

int EntropyBlocking(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *d_bytes, const uint64_t *d_off,
                    uint64_t n, float theta, float *d_entropy, float *d_log_z, hipStream_t st) {
  uint64_t total = 0;
  int rc = BatchBytes(ws, d_off, n, st, &total);
  if (rc != SPM_OK) return rc;
  ws->stats = spm_hip_encode_stats{};
  if (n == 0) {
    spm_amd::PublishStats(m, ws->stats);
    return SPM_OK;
  }
  const uint64_t cap = std::max<uint64_t>(total, 1);
  const uint32_t num_units = static_cast<uint32_t>(m->trie.units.size());
  if (!m->force_general) {
    SPM_HIP_TRY(ws->w_salpha.Reserve((cap + n + 1) * 4));
    SPM_HIP_TRY(ws->w_lpath.Reserve((cap + n + 1) * 4));
  }
  auto fast = [&](uint32_t *status) {
    const spm_amd::EntropyFastArgs f{d_bytes, d_off, n, total, m->d_units.as<uint32_t>(), m->d_values.as<int32_t>(),
                                     m->d_scores.as<float>(), num_units, m->up, theta, ws->w_salpha.as<float>(),
                                     ws->w_lpath.as<float>(), d_entropy, d_log_z, ws->w_flagged.as<uint32_t>(),
                                     status};
    return spm_amd::LaunchUnigramEntropyFast(f, st);
  };
  auto exact = [&](const spm_amd::GeneralLaunch &g) {
    const spm_amd::EntropyExactArgs x{d_bytes, d_off, m->d_units.as<uint32_t>(), m->d_values.as<int32_t>(),
                                      m->d_scores.as<float>(), num_units, m->up, theta, d_entropy, d_log_z, g.list,
                                      g.count, g.list_n, g.scratch, g.slab_bytes, g.max_nb, g.ovf_list, g.ovf_count,
                                      g.error, g.threads};
    return spm_amd::LaunchUnigramEntropyExact(x, st);
  };
  return LatticeTiers(m, ws, d_off, n, cap, nullptr, nullptr, "sentence too long for the exact entropy path",
                      "exact lattice path: scratch overflow or broken walk", st, fast, exact);
}

// Sample and score on a leased workspace: the rows' token offsets go to
// d_tok and the scores to d_scores; *tokens = the rows' token total.  The
// tokens wait in the workspace's slots for ScoreGatherTo.
int ScoreBlocking(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const uint8_t *d_bytes, const uint64_t *d_off,
                  uint64_t n, uint32_t ns, float theta, uint64_t seed, uint64_t index_base, bool with_len,
                  uint64_t *d_tok, float *d_scores, uint64_t *tokens, hipStream_t st) {
  uint64_t total = 0;
  int rc = BatchBytes(ws, d_off, n, st, &total);
  if (rc != SPM_OK) return rc;
  ws->stats = spm_hip_encode_stats{};
  *tokens = 0;
  if (n == 0) {
    SPM_HIP_TRY(hipMemsetAsync(d_tok, 0, sizeof(uint64_t), st));
    SPM_HIP_TRY(hipStreamSynchronize(st));
    spm_amd::PublishStats(m, ws->stats);
    return SPM_OK;
  }
  const uint64_t rows = n * ns;
  const uint64_t cap = std::max<uint64_t>(total, 1);
  SPM_HIP_TRY(ws->w_slot2_ids.Reserve(cap * ns * 4));
  if (with_len) SPM_HIP_TRY(ws->w_slot2_len.Reserve(cap * ns * 4));
  SPM_HIP_TRY(ws->w_ntok.Reserve(rows * 4));
  int32_t *s2 = ws->w_slot2_ids.as<int32_t>();
  uint32_t *s2l = with_len ? ws->w_slot2_len.as<uint32_t>() : nullptr;
  const uint32_t num_units = static_cast<uint32_t>(m->trie.units.size());
  if (!m->force_general) {
    SPM_HIP_TRY(ws->w_salpha.Reserve((cap + n + 1) * 4));
    SPM_HIP_TRY(ws->w_smask.Reserve((cap + n + 1) * 8));
    SPM_HIP_TRY(ws->w_lpath.Reserve((cap + n + 1) * 8));
  }
  auto fast = [&](uint32_t *status) {
    const spm_amd::ScoreFastArgs f{
        spm_amd::SampleFastArgs{d_bytes, d_off, n, total, m->d_units.as<uint32_t>(), m->d_values.as<int32_t>(),
                                m->d_scores.as<float>(), num_units, m->up, theta, seed, index_base,
                                ws->w_salpha.as<float>(), ws->w_smask.as<uint64_t>(), s2, s2l,
                                ws->w_ntok.as<uint32_t>(), ws->w_flagged.as<uint32_t>(), status},
        ns, ws->w_lpath.as<uint64_t>(), d_scores};
    return spm_amd::LaunchUnigramScoreFast(f, st);
  };
  auto exact = [&](const spm_amd::GeneralLaunch &g) {
    const spm_amd::ScoreExactArgs x{
        spm_amd::SampleExactArgs{d_bytes, d_off, m->d_units.as<uint32_t>(), m->d_values.as<int32_t>(),
                                 m->d_scores.as<float>(), num_units, m->up, theta, seed, index_base, g.slot_ids,
                                 g.slot_len, g.ntok, g.list, g.count, g.list_n, g.scratch, g.slab_bytes, g.max_nb,
                                 g.ovf_list, g.ovf_count, g.error, g.threads},
        ns, d_scores};
    return spm_amd::LaunchUnigramScoreExact(x, st);
  };
  rc = LatticeTiers(m, ws, d_off, n, cap, s2, s2l, "sentence too long for the exact sampling path",
                    "exact lattice path: scratch overflow or broken walk", st, fast, exact);
  if (rc != SPM_OK) return rc;
  size_t tmp = 0;
  SPM_HIP_TRY(spm_amd::LaunchScoreScan(ws->w_ntok.as<uint32_t>(), rows, d_tok, nullptr, &tmp, st));
  SPM_HIP_TRY(ws->w_scan.Reserve(tmp + 16));
  SPM_HIP_TRY(spm_amd::LaunchScoreScan(ws->w_ntok.as<uint32_t>(), rows, d_tok, ws->w_scan.ptr, &tmp, st));
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned + 8, d_tok + rows, 8, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(tokens, ws->pinned + 8, 8);
  ws->stats.tokens = *tokens;
  spm_amd::PublishStats(m, ws->stats);
  return SPM_OK;
}

int ScoreGatherTo(spm_amd::EncodeWorkspace *ws, const uint64_t *d_off, uint64_t n, uint32_t ns, const uint64_t *d_tok,
                  int32_t *d_ids, uint32_t *d_len, hipStream_t st) {
  SPM_HIP_TRY(spm_amd::LaunchScoreGather(d_off, n, ns, ws->w_slot2_ids.as<int32_t>(),
                                         d_len ? ws->w_slot2_len.as<uint32_t>() : nullptr, d_tok, d_ids, d_len, st));
  return SPM_OK;
}

int ScoreArgsCheck(const spm_hip_model *m, uint64_t n, uint32_t ns, float theta) {
  if (ns == 0) return Fail(SPM_INVALID_ARGUMENT, "num_samples must be positive");
  const int rc = LatticeScoreArgsCheck(m, theta, "SampleEncodeAndScore");
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull || n * static_cast<uint64_t>(ns) >= 0x7FFFFFFFull)
    return Fail(SPM_OUT_OF_RANGE, "too many sample rows in one batch");
  return SPM_OK;
}

}  // namespace

int spm_hip_entropy_batch(spm_hip_model *m, const uint8_t *d_bytes, const uint64_t *d_off, uint64_t n, float theta,
                          float *d_entropy, float *d_log_z, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_entropy_batch");
  if (!m || !d_off || (n && !d_entropy)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  const int rc = LatticeScoreArgsCheck(m, theta, "CalculateEntropy");
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return EntropyBlocking(m, ws.get(), d_bytes, d_off, n, theta, d_entropy, d_log_z, st);
}

int spm_hip_entropy_batch_host(spm_hip_model *m, const uint8_t *bytes, const uint64_t *off, uint64_t n, float theta,
                               float *entropy, float *log_z) {
  spm_amd::TraceRange trace_range_("spm_hip_entropy_batch_host");
  if (!m || !off || (n && !entropy)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  int rc = LatticeScoreArgsCheck(m, theta, "CalculateEntropy");
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  if ((rc = HostOffsetsCheck(off, n)) != SPM_OK) return rc;
  const uint64_t total = off[n];
  if (total && !bytes) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  hipStream_t st = ws.stream();
  SPM_HIP_TRY(ws->w_lscore.Reserve(std::max<uint64_t>(n, 1) * 4));
  if (log_z) SPM_HIP_TRY(ws->w_llogz.Reserve(std::max<uint64_t>(n, 1) * 4));
  if ((rc = StageHostInput(ws.get(), bytes, off, n, total, st)) != SPM_OK) return rc;
  rc = EntropyBlocking(m, ws.get(), ws->h_in.as<uint8_t>(), ws->h_off.as<uint64_t>(), n, theta,
                       ws->w_lscore.as<float>(), log_z ? ws->w_llogz.as<float>() : nullptr, st);
  if (rc != SPM_OK || n == 0) return rc;
  SPM_HIP_TRY(hipMemcpyAsync(entropy, ws->w_lscore.ptr, n * 4, hipMemcpyDeviceToHost, st));
  if (log_z) SPM_HIP_TRY(hipMemcpyAsync(log_z, ws->w_llogz.ptr, n * 4, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  return SPM_OK;
}

int spm_hip_sample_encode_and_score_batch(spm_hip_model *m, const uint8_t *d_bytes, const uint64_t *d_off, uint64_t n,
                                          uint32_t num_samples, float theta, uint64_t seed, uint64_t index_base,
                                          int32_t *d_ids, uint64_t token_capacity, uint32_t *d_len, uint64_t *d_tok,
                                          float *d_scores, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_sample_encode_and_score_batch");
  if (!m || !d_off || !d_tok || (n && !d_scores)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  int rc = ScoreArgsCheck(m, n, num_samples, theta);
  if (rc != SPM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  uint64_t T = 0;
  rc = ScoreBlocking(m, ws.get(), d_bytes, d_off, n, num_samples, theta, seed, index_base, d_len != nullptr, d_tok,
                     d_scores, &T, st);
  if (rc != SPM_OK) return rc;
  if (T > token_capacity) return Fail(SPM_RESOURCE_EXHAUSTED, "sampled tokens exceed the caller's capacity");
  if (T && !d_ids) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (T == 0) return SPM_OK;
  rc = ScoreGatherTo(ws.get(), d_off, n, num_samples, d_tok, d_ids, d_len, st);
  if (rc != SPM_OK) return rc;
  SPM_HIP_TRY(hipStreamSynchronize(st));
  return SPM_OK;
}

int spm_hip_sample_encode_and_score_batch_host(spm_hip_model *m, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                                               uint32_t num_samples, float theta, uint64_t seed, uint64_t index_base,
                                               int32_t *ids, uint64_t token_capacity, uint32_t *len, uint64_t *tok,
                                               float *scores) {
  spm_amd::TraceRange trace_range_("spm_hip_sample_encode_and_score_batch_host");
  if (!m || !off || !tok || (n && !scores)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  int rc = ScoreArgsCheck(m, n, num_samples, theta);
  if (rc != SPM_OK) return rc;
  if ((rc = HostOffsetsCheck(off, n)) != SPM_OK) return rc;
  const uint64_t total = off[n];
  if (total && !bytes) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  const uint64_t rows = n * num_samples;
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  hipStream_t st = ws.stream();
  SPM_HIP_TRY(ws->h_tok.Reserve((rows + 1) * 8));
  SPM_HIP_TRY(ws->w_lscore.Reserve(std::max<uint64_t>(rows, 1) * 4));
  if ((rc = StageHostInput(ws.get(), bytes, off, n, total, st)) != SPM_OK) return rc;
  uint64_t T = 0;
  rc = ScoreBlocking(m, ws.get(), ws->h_in.as<uint8_t>(), ws->h_off.as<uint64_t>(), n, num_samples, theta, seed,
                     index_base, len != nullptr, ws->h_tok.as<uint64_t>(), ws->w_lscore.as<float>(), &T, st);
  if (rc != SPM_OK) return rc;
  SPM_HIP_TRY(hipMemcpyAsync(tok, ws->h_tok.ptr, (rows + 1) * 8, hipMemcpyDeviceToHost, st));
  if (rows) SPM_HIP_TRY(hipMemcpyAsync(scores, ws->w_lscore.ptr, rows * 4, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  if (T > token_capacity) return Fail(SPM_RESOURCE_EXHAUSTED, "sampled tokens exceed the caller's capacity");
  if (T && !ids) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (T == 0) return SPM_OK;
  SPM_HIP_TRY(ws->h_ids.Reserve(T * 4));
  if (len) SPM_HIP_TRY(ws->h_len.Reserve(T * 4));
  rc = ScoreGatherTo(ws.get(), ws->h_off.as<uint64_t>(), n, num_samples, ws->h_tok.as<uint64_t>(),
                     ws->h_ids.as<int32_t>(), len ? ws->h_len.as<uint32_t>() : nullptr, st);
  if (rc != SPM_OK) return rc;
  SPM_HIP_TRY(hipMemcpyAsync(ids, ws->h_ids.ptr, T * 4, hipMemcpyDeviceToHost, st));
  if (len) SPM_HIP_TRY(hipMemcpyAsync(len, ws->h_len.ptr, T * 4, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  return SPM_OK;
}

int spm_hip_sample_seed(uint64_t seed, uint64_t sample, uint64_t *seed_out) {
  if (!seed_out) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  *seed_out = spm_amd::SampleSeedAt(seed, sample);
  return SPM_OK;
}

int spm_hip_nbest_encode_batch(spm_hip_model *m, const uint8_t *d_bytes, const uint64_t *d_off, uint64_t n,
                               int32_t nbest_size, int32_t *d_ids, uint32_t *d_len, uint64_t token_capacity,
                               uint64_t *d_tok, float *d_scores, uint64_t path_capacity, uint64_t *d_path_off,
                               uint64_t *total_paths, uint64_t *total_tokens, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_nbest_encode_batch");
  if (!m || !d_off || !d_tok || !d_path_off) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  int rc = NBestArgsCheck(m);
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  const int N = spm_amd::NBestClamp(nbest_size);
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  uint64_t P = 0, T = 0;
  rc = NBestSearch(m, ws.get(), d_bytes, d_off, nullptr, n, N, d_len != nullptr, &P, &T, st);
  if (rc != SPM_OK) return rc;
  if (total_paths) *total_paths = P;
  if (total_tokens) *total_tokens = T;
  if (P > path_capacity || T > token_capacity)
    return Fail(SPM_RESOURCE_EXHAUSTED, "n-best output exceeds the caller's capacities");
  if ((T && !d_ids) || (P && !d_scores)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  SPM_HIP_TRY(hipMemcpyAsync(d_path_off, ws->w_nb_poff.ptr, (n + 1) * 8, hipMemcpyDeviceToDevice, st));
  SPM_HIP_TRY(hipMemcpyAsync(d_tok, ws->w_nb_toff.ptr, (P + 1) * 8, hipMemcpyDeviceToDevice, st));
  rc = NBestGatherTo(ws.get(), n, N, d_ids, d_len, d_scores, st);
  if (rc != SPM_OK) return rc;
  SPM_HIP_TRY(hipStreamSynchronize(st));
  return SPM_OK;
}

int spm_hip_nbest_encode_batch_host(spm_hip_model *m, const uint8_t *bytes, const uint64_t *off, uint64_t n,
                                    int32_t nbest_size, int32_t *ids, uint32_t *len, uint64_t token_capacity,
                                    uint64_t *tok, float *scores, uint64_t path_capacity, uint64_t *path_off,
                                    uint64_t *total_paths, uint64_t *total_tokens) {
  spm_amd::TraceRange trace_range_("spm_hip_nbest_encode_batch_host");
  if (!m || !off || !tok || !path_off) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  int rc = NBestArgsCheck(m);
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  if ((rc = HostOffsetsCheck(off, n)) != SPM_OK) return rc;
  const uint64_t total = off[n];
  if (total && !bytes) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  const int N = spm_amd::NBestClamp(nbest_size);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  hipStream_t st = ws.stream();
  if ((rc = StageHostInput(ws.get(), bytes, off, n, total, st)) != SPM_OK) return rc;
  uint64_t P = 0, T = 0;
  rc = NBestSearch(m, ws.get(), ws->h_in.as<uint8_t>(), ws->h_off.as<uint64_t>(), bytes, n, N, len != nullptr, &P, &T,
                   st);
  if (rc != SPM_OK) return rc;
  if (total_paths) *total_paths = P;
  if (total_tokens) *total_tokens = T;
  if (P > path_capacity || T > token_capacity)
    return Fail(SPM_RESOURCE_EXHAUSTED, "n-best output exceeds the caller's capacities");
  if ((T && !ids) || (P && !scores)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  SPM_HIP_TRY(ws->h_ids.Reserve(std::max<uint64_t>(T, 1) * 4));
  if (len) SPM_HIP_TRY(ws->h_len.Reserve(std::max<uint64_t>(T, 1) * 4));
  SPM_HIP_TRY(ws->w_nb_oscore.Reserve(std::max<uint64_t>(P, 1) * 4));
  rc = NBestGatherTo(ws.get(), n, N, ws->h_ids.as<int32_t>(), len ? ws->h_len.as<uint32_t>() : nullptr,
                     ws->w_nb_oscore.as<float>(), st);
  if (rc != SPM_OK) return rc;
  SPM_HIP_TRY(hipMemcpyAsync(path_off, ws->w_nb_poff.ptr, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipMemcpyAsync(tok, ws->w_nb_toff.ptr, (P + 1) * 8, hipMemcpyDeviceToHost, st));
  if (T) SPM_HIP_TRY(hipMemcpyAsync(ids, ws->h_ids.ptr, T * 4, hipMemcpyDeviceToHost, st));
  if (T && len) SPM_HIP_TRY(hipMemcpyAsync(len, ws->h_len.ptr, T * 4, hipMemcpyDeviceToHost, st));
  if (P) SPM_HIP_TRY(hipMemcpyAsync(scores, ws->w_nb_oscore.ptr, P * 4, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  return SPM_OK;
}

int spm_hip_model_set_nbest_max_hyps(spm_hip_model *m, uint32_t first, uint32_t second) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  m->nbest_hyps1 = first;
  m->nbest_hyps2 = second;
  return SPM_OK;
}

int spm_hip_nbest_last_stats(const spm_hip_model *m, uint64_t *second_pass, uint64_t *host_path) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  std::lock_guard<std::mutex> lk(const_cast<spm_hip_model *>(m)->pool_mu);
  if (second_pass) *second_pass = m->nbest_second;
  if (host_path) *host_path = m->nbest_host;
  return SPM_OK;
}

int spm_hip_sample_uniform(uint64_t seed, uint64_t index, uint64_t draw, double *u) {
  if (!u) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  *u = spm_amd::SampleDraw(spm_amd::SampleKey(seed, index), draw);
  return SPM_OK;
}

// ---------------------------------------------------------------------------
// Decode (sentencepiece_processor.cc:670-733) on the device: decode_kernels.hip.
namespace {

int FailDecodeRange(uint64_t sentence, int64_t id, size_t pieces) {
  return Fail(SPM_OUT_OF_RANGE, "decode: sentence " + std::to_string(sentence) + " holds id " + std::to_string(id) +
                                    ", outside [0, " + std::to_string(pieces) + ")");
}

int DecodeImpl(spm_hip_model *m, spm_amd::EncodeWorkspace *ws, const spm_amd::EpilogueExtras &x,
               const int32_t *d_ids, const uint64_t *d_tok_off, uint64_t n, uint8_t *d_out, uint64_t out_capacity,
               uint64_t *d_out_off, uint32_t *d_piece_begin, uint64_t *total, uint32_t *chain, hipStream_t st) {
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  if (n == 0) {
    SPM_HIP_TRY(hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), st));
    if (total) *total = 0;
    return SPM_OK;
  }
  SPM_HIP_TRY(ws->w_dfirst.Reserve(n * sizeof(uint32_t)));
  SPM_HIP_TRY(ws->w_dsum.Reserve(spm_amd::kDecodeBlocks * sizeof(uint64_t)));
  SPM_HIP_TRY(ws->w_dctl.Reserve(spm_amd::kDcWords * sizeof(uint64_t)));
  uint64_t *ctl = ws->w_dctl.as<uint64_t>();
  SPM_HIP_TRY(hipMemsetAsync(ctl, 0, spm_amd::kDcWords * sizeof(uint64_t), st));
  SPM_HIP_TRY(hipMemsetAsync(ctl + spm_amd::kDcBadKey, 0xFF, sizeof(uint64_t), st));
  SPM_HIP_TRY(hipMemsetAsync(ws->w_dfirst.ptr, 0xFF, n * sizeof(uint32_t), st));
  spm_amd::DecodeLaunch a{};
  a.ids = d_ids;
  a.tok_off = d_tok_off;
  a.n = n;
  a.meta = m->d_dec_meta.as<uint32_t>();
  a.off = m->d_dec_off.as<uint32_t>();
  a.bytes = m->d_dec_bytes.as<uint8_t>();
  a.num_pieces = static_cast<int32_t>(m->decode.meta.size());
  a.has_bytes = m->decode.has_bytes;
  a.x = x;
  a.first = ws->w_dfirst.as<uint32_t>();
  a.block_sum = ws->w_dsum.as<uint64_t>();
  a.ctl = ctl;
  // Blocking call: the call's own status word lives in the control block.
  a.chain = chain ? chain : reinterpret_cast<uint32_t *>(ctl + spm_amd::kDcStatus);
  a.out = d_out;
  a.capacity = out_capacity;
  a.out_off = d_out_off;
  a.piece_begin = d_piece_begin;
  SPM_HIP_TRY(spm_amd::LaunchDecode(a, chain == nullptr, st));
  if (chain) return SPM_OK;
  uint64_t h[spm_amd::kDcWords];
  static_assert(sizeof(h) <= 48, "read-back fits the pinned slots below the epilogue's");
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(h, ws->pinned, sizeof(h));
  const uint32_t status = static_cast<uint32_t>(h[spm_amd::kDcStatus]);
  if (status == SPM_OUT_OF_RANGE)
    return FailDecodeRange(h[spm_amd::kDcBadSentence], static_cast<int64_t>(h[spm_amd::kDcBadId]),
                           m->decode.meta.size());
  if (total) *total = h[spm_amd::kDcTotal];
  if (status == SPM_RESOURCE_EXHAUSTED) return Fail(SPM_RESOURCE_EXHAUSTED, "decoded text exceeds out_capacity");
  if (status != 0) return Fail(static_cast<int>(status), "decode failed");
  return SPM_OK;
}

int DecodeArgs(spm_hip_model *m, const char *extra_options, const uint64_t *tok_off, uint64_t *out_off,
               spm_amd::EpilogueExtras *x) {
  if (!m || !tok_off || !out_off) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->decode.meta.empty()) return Fail(SPM_FAILED_PRECONDITION, "model has no decode table");
  return FoldExtras(m, extra_options, x);
}

}  // namespace

int spm_hip_decode_batch(spm_hip_model *m, const char *extra_options, const int32_t *d_ids,
                         const uint64_t *d_tok_off, uint64_t n, uint8_t *d_out, uint64_t out_capacity,
                         uint64_t *d_out_off, uint32_t *d_piece_begin, uint64_t *total, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_decode_batch");
  spm_amd::EpilogueExtras x{};
  const int rc = DecodeArgs(m, extra_options, d_tok_off, d_out_off, &x);
  if (rc != SPM_OK) return rc;
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return DecodeImpl(m, ws.get(), x, d_ids, d_tok_off, n, d_out, out_capacity, d_out_off, d_piece_begin, total,
                    nullptr, st);
}

int spm_hip_decode_batch_async(spm_hip_model *m, const char *extra_options, const int32_t *d_ids,
                               const uint64_t *d_tok_off, uint64_t n, uint8_t *d_out, uint64_t out_capacity,
                               uint64_t *d_out_off, uint32_t *d_piece_begin, uint32_t *d_status, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_decode_batch_async");
  if (!d_status) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  spm_amd::EpilogueExtras x{};
  const int rc = DecodeArgs(m, extra_options, d_tok_off, d_out_off, &x);
  if (rc != SPM_OK) return rc;
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "model was loaded host-only");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  return DecodeImpl(m, ws.get(), x, d_ids, d_tok_off, n, d_out, out_capacity, d_out_off, d_piece_begin, nullptr,
                    d_status, st);
}

int spm_hip_decode_batch_host(spm_hip_model *m, const char *extra_options, const int32_t *ids,
                              const uint64_t *tok_off, uint64_t n, uint8_t *out, uint64_t out_capacity,
                              uint64_t *out_off, uint32_t *piece_begin, uint64_t *total) {
  spm_amd::TraceRange trace_range_("spm_hip_decode_batch_host");
  spm_amd::EpilogueExtras x{};
  int rc = DecodeArgs(m, extra_options, tok_off, out_off, &x);
  if (rc != SPM_OK) return rc;
  if (n >= 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  if (tok_off[0] != 0) return Fail(SPM_INVALID_ARGUMENT, "offsets must start at 0");
  for (uint64_t i = 0; i < n; ++i)
    if (tok_off[i + 1] < tok_off[i]) return Fail(SPM_INVALID_ARGUMENT, "offsets must not decrease");
  const uint64_t tokens = tok_off[n];
  if (tokens && !ids) return Fail(SPM_INVALID_ARGUMENT, "null ids");
  if (total) *total = 0;
  if (m->host_only) {
    uint64_t bad_sentence = 0;
    int32_t bad_id = 0;
    // Offsets go to a scratch first: an out-of-range id must leave no output.
    std::vector<uint64_t> off(n + 1);
    rc = spm_amd::DecodeHostLoop(m->decode, x, ids, tok_off, n, out, out_capacity, off.data(), piece_begin,
                                 &bad_sentence, &bad_id);
    if (rc != SPM_OK) return FailDecodeRange(bad_sentence, bad_id, m->decode.meta.size());
    std::memcpy(out_off, off.data(), (n + 1) * sizeof(uint64_t));
    if (total) *total = off[n];
    if (out && off[n] > out_capacity) return Fail(SPM_RESOURCE_EXHAUSTED, "decoded text exceeds out_capacity");
    return SPM_OK;
  }
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  hipStream_t st = ws.stream();
  const uint64_t final_tokens = tokens + n * (x.num_pre + x.num_post);
  SPM_HIP_TRY(ws->h_dids.Reserve(std::max<uint64_t>(tokens, 1) * sizeof(int32_t)));
  SPM_HIP_TRY(ws->h_dtok.Reserve((n + 1) * sizeof(uint64_t)));
  SPM_HIP_TRY(ws->h_doff.Reserve((n + 1) * sizeof(uint64_t)));
  if (out) SPM_HIP_TRY(ws->h_dout.Reserve(std::max<uint64_t>(out_capacity, 1)));
  if (out && piece_begin) SPM_HIP_TRY(ws->h_dbegin.Reserve(std::max<uint64_t>(final_tokens, 1) * sizeof(uint32_t)));
  if (tokens) SPM_HIP_TRY(hipMemcpyAsync(ws->h_dids.ptr, ids, tokens * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SPM_HIP_TRY(hipMemcpyAsync(ws->h_dtok.ptr, tok_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  uint64_t tot = 0;
  rc = DecodeImpl(m, ws.get(), x, ws->h_dids.as<int32_t>(), ws->h_dtok.as<uint64_t>(), n,
                  out ? ws->h_dout.as<uint8_t>() : nullptr, out_capacity, ws->h_doff.as<uint64_t>(),
                  out && piece_begin ? ws->h_dbegin.as<uint32_t>() : nullptr, &tot, nullptr, st);
  if (rc != SPM_OK && rc != SPM_RESOURCE_EXHAUSTED) return rc;
  if (total) *total = tot;
  SPM_HIP_TRY(hipMemcpyAsync(out_off, ws->h_doff.ptr, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (rc == SPM_OK && out) {
    if (tot) SPM_HIP_TRY(hipMemcpyAsync(out, ws->h_dout.ptr, tot, hipMemcpyDeviceToHost, st));
    if (piece_begin && final_tokens)
      SPM_HIP_TRY(hipMemcpyAsync(piece_begin, ws->h_dbegin.ptr, final_tokens * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, st));
  }
  SPM_HIP_TRY(hipStreamSynchronize(st));
  return rc;
}

int spm_hip_model_decode_bound(const spm_hip_model *m, uint32_t *max_surface_bytes) {
  if (!m || !max_surface_bytes) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->decode.meta.empty()) return Fail(SPM_FAILED_PRECONDITION, "model has no decode table");
  *max_surface_bytes = m->decode.max_surface;
  return SPM_OK;
}

// ---- Vocabulary restriction (sentencepiece_processor.cc:203-245) ----

int spm_hip_model_get_piece_types(const spm_hip_model *m, uint8_t *types, uint64_t n) {
  if (!m || !types) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (n != m->proto.pieces.size()) return Fail(SPM_INVALID_ARGUMENT, "n is not the model's piece_size");
  for (uint64_t i = 0; i < n; ++i) types[i] = static_cast<uint8_t>(m->proto.pieces[i].type);
  return SPM_OK;
}

int spm_hip_model_set_piece_types(spm_hip_model *m, const uint8_t *types, uint64_t n) {
  spm_amd::TraceRange trace_range_("spm_hip_model_set_piece_types");
  if (!m || !types) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  auto &pieces = m->proto.pieces;
  if (n != pieces.size()) return Fail(SPM_INVALID_ARGUMENT, "n is not the model's piece_size");
  bool changed = false;
  for (uint64_t i = 0; i < n; ++i) {
    const int32_t was = pieces[i].type, now = types[i];
    if (was == now) continue;
    const bool free_was = was == spm_amd::kNormal || was == spm_amd::kUnused;
    const bool free_now = now == spm_amd::kNormal || now == spm_amd::kUnused;
    if (!free_was || !free_now)
      return Fail(SPM_INVALID_ARGUMENT, "piece " + std::to_string(i) + ": only NORMAL and UNUSED may be exchanged");
    changed = true;
  }
  if (!changed) return SPM_OK;
  // Quiesce: the resident small-call servers end (their arguments were
  // captured at launch; the next small call restarts them with the new
  // state), then every stream this handle has work on drains.
  if (!m->host_only) {
    std::vector<spm_amd::EncodeWorkspace *> all;
    std::vector<hipStream_t> streams;
    {
      std::lock_guard<std::mutex> g(m->pool_mu);
      for (auto &kv : m->by_stream) {
        all.push_back(kv.second.get());
        streams.push_back(kv.first);
      }
      for (auto &w : m->host_pool) {
        all.push_back(w.get());
        streams.push_back(w->own_stream);
      }
    }
    for (size_t k = 0; k < all.size(); ++k) {
      std::lock_guard<std::mutex> g(all[k]->mu);
      all[k]->StopService();
      std::memset(all[k]->svc_key, 0, sizeof(all[k]->svc_key));
      SPM_HIP_TRY(hipStreamSynchronize(streams[k]));
    }
  }
  // What the small calls' one-wave kernels handed back so far says nothing
  // about the new vocabulary: their back-off starts over.
  m->coop_small_rejects.store(0, std::memory_order_relaxed);
  std::vector<uint8_t> kind(n, 0);
  for (uint64_t i = 0; i < n; ++i) {
    pieces[i].type = types[i];
    kind[i] = types[i] == spm_amd::kUserDefined ? spm_amd::kKindUserDefined
              : types[i] == spm_amd::kUnused    ? spm_amd::kKindUnused
                                                : 0;
  }
  const hipStream_t st = nullptr;
  if (m->model_type == spm_amd::kUnigram) {
    const bool had_uvs = m->d_uvs.ptr != nullptr;
    for (size_t u = 0; u < m->trie.units.size(); ++u) {
      if (!spm_amd::DoubleArray::Leaf(m->trie.units[u])) continue;
      const int32_t id = m->trie.values[u] & spm_amd::kIdMask;
      m->trie.values[u] = id | (static_cast<int32_t>(kind[id]) << spm_amd::kKindShift);
    }
    std::vector<float> vbp;
    DeriveUnigram(m, &vbp);
    if (m->host_only) return SPM_OK;
    SPM_HIP_TRY(Upload(&m->d_types_kind, kind));
    SPM_HIP_TRY(spm_amd::LaunchVocabRetagUnigram(m->d_units.as<uint32_t>(), m->d_values.as<int32_t>(),
                                                 had_uvs ? m->d_uvs.as<uint32_t>() : nullptr,
                                                 m->d_scores.as<float>(), m->d_types_kind.as<uint8_t>(),
                                                 static_cast<uint32_t>(m->trie.units.size()),
                                                 static_cast<uint32_t>(n), st));
    // A tier that had no (unit, score) table at load and needs one now gets
    // it built on the host, as at load.
    int rc = SPM_OK;
    if (!had_uvs && !vbp.empty()) rc = UploadUnitScores(m, vbp);
    if (rc == SPM_OK) rc = UploadPieceTable(m);
    if (rc != SPM_OK) return rc;
  } else if (m->model_type == spm_amd::kBpe) {
    if (m->host_only) return SPM_OK;
    SPM_HIP_TRY(Upload(&m->bpe.piece_kind, kind));
    SPM_HIP_TRY(spm_amd::LaunchVocabRetagBpe(m->bpe.pair_ent.ptr, m->bpe.pair_mask + 1, m->bpe.piece_kind.as<uint8_t>(),
                                             static_cast<uint32_t>(n), st));
  } else {
    return SPM_OK;  // WORD / CHAR encode does not look at NORMAL against UNUSED
  }
  SPM_HIP_TRY(hipStreamSynchronize(st));
  return SPM_OK;
}

int spm_hip_model_set_vocabulary(spm_hip_model *m, const uint8_t *piece_bytes, const uint64_t *piece_offsets,
                                 uint64_t num_pieces) {
  if (!m || (num_pieces && (!piece_bytes || !piece_offsets))) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->model_type != spm_amd::kUnigram && m->model_type != spm_amd::kBpe)
    return Fail(SPM_INTERNAL, "Vocabulary constraint is only enabled in subword units.");
  std::vector<uint8_t> types(m->proto.pieces.size());
  for (size_t i = 0; i < types.size(); ++i) types[i] = static_cast<uint8_t>(m->proto.pieces[i].type);
  std::vector<char> keep(types.size(), 0);
  for (uint64_t k = 0; k < num_pieces; ++k) {
    const std::string p(reinterpret_cast<const char *>(piece_bytes) + piece_offsets[k],
                        piece_offsets[k + 1] - piece_offsets[k]);
    auto it = m->pieces.find(p);
    if (it != m->pieces.end()) keep[it->second] = 1;
    auto r = m->reserved.find(p);
    if (r != m->reserved.end()) keep[r->second] = 1;
  }
  for (size_t i = 0; i < types.size(); ++i) {
    if (types[i] != spm_amd::kNormal && types[i] != spm_amd::kUnused) continue;
    const std::string &p = m->proto.pieces[i].piece;
    // string_util::OneCharLen(piece.c_str()) == piece.size()
    const bool one_char = spm_amd::OneCharLen(static_cast<uint8_t>(p.c_str()[0])) == p.size();
    types[i] = keep[i] || one_char ? spm_amd::kNormal : spm_amd::kUnused;
  }
  return spm_hip_model_set_piece_types(m, types.data(), types.size());
}

int spm_hip_model_reset_vocabulary(spm_hip_model *m) {
  if (!m) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  std::vector<uint8_t> types(m->proto.pieces.size());
  for (size_t i = 0; i < types.size(); ++i) {
    types[i] = static_cast<uint8_t>(m->proto.pieces[i].type);
    if (types[i] == spm_amd::kUnused) types[i] = spm_amd::kNormal;
  }
  return spm_hip_model_set_piece_types(m, types.data(), types.size());
}

// ---- Piece counting ----

int spm_hip_count_ids(spm_hip_model *m, const int32_t *d_ids, uint64_t num_tokens, uint64_t *d_counts,
                      uint32_t *d_status, void *stream) {
  spm_amd::TraceRange trace_range_("spm_hip_count_ids");
  if (!m || !d_counts || (num_tokens && !d_ids)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "host-only model handle");
  hipStream_t st = static_cast<hipStream_t>(stream);
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForStream(m, st));
  if (!d_status) {
    SPM_HIP_TRY(ws->w_vstat.Reserve(4));
    d_status = ws->w_vstat.as<uint32_t>();
    SPM_HIP_TRY(hipMemsetAsync(d_status, 0, 4, st));
  }
  // The LDS bins are 32 bits wide: at most 2^31 tokens per launch.
  const uint32_t v = static_cast<uint32_t>(m->proto.pieces.size());
  for (uint64_t at = 0; at < num_tokens; at += 1ull << 31)
    SPM_HIP_TRY(spm_amd::LaunchVocabCount(d_ids + at, std::min<uint64_t>(num_tokens - at, 1ull << 31), d_counts, v,
                                          d_status, st));
  return SPM_OK;
}

int spm_hip_count_ids_host(spm_hip_model *m, const int32_t *ids, uint64_t num_tokens, uint64_t *counts,
                           uint32_t *status) {
  spm_amd::TraceRange trace_range_("spm_hip_count_ids_host");
  if (!m || !counts || (num_tokens && !ids)) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (m->host_only) return Fail(SPM_FAILED_PRECONDITION, "host-only model handle");
  const uint64_t v = m->proto.pieces.size();
  spm_amd::WorkspaceLease ws;
  SPM_LEASE(ws, ws.ForHost(m));
  hipStream_t st = ws.stream();
  SPM_HIP_TRY(ws->h_ids.Reserve(std::max<uint64_t>(num_tokens, 1) * sizeof(int32_t)));
  SPM_HIP_TRY(ws->w_vcount.Reserve(v * sizeof(uint64_t) + 8));
  uint64_t *d_counts = ws->w_vcount.as<uint64_t>();
  uint32_t *d_status = reinterpret_cast<uint32_t *>(d_counts + v);
  if (num_tokens) SPM_HIP_TRY(hipMemcpyAsync(ws->h_ids.ptr, ids, num_tokens * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (v) SPM_HIP_TRY(hipMemcpyAsync(d_counts, counts, v * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  SPM_HIP_TRY(hipMemsetAsync(d_status, 0, 8, st));
  for (uint64_t at = 0; at < num_tokens; at += 1ull << 31)
    SPM_HIP_TRY(spm_amd::LaunchVocabCount(ws->h_ids.as<int32_t>() + at, std::min<uint64_t>(num_tokens - at, 1ull << 31),
                                          d_counts, static_cast<uint32_t>(v), d_status, st));
  if (v) SPM_HIP_TRY(hipMemcpyAsync(counts, d_counts, v * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipMemcpyAsync(ws->pinned, d_status, 4, hipMemcpyDeviceToHost, st));
  SPM_HIP_TRY(hipStreamSynchronize(st));
  if (status) *status = ws->pinned[0];
  return SPM_OK;
}

// ---- Dense id batches (dense.h) ----

namespace {

// The argument checks the device and the host entries share; nothing here
// touches HIP.
int DenseArgs(const uint64_t *off, uint32_t row_len, uint32_t flags, const int32_t *out) {
  if (!off || !out) return Fail(SPM_INVALID_ARGUMENT, "null argument");
  if (row_len == 0 || row_len > 0x7FFFFFFFu) return Fail(SPM_INVALID_ARGUMENT, "row_len must be in [1, INT32_MAX]");
  if (flags & ~spm_amd::kDenseFlagMask) return Fail(SPM_INVALID_ARGUMENT, "unknown dense flag bit");
  return SPM_OK;
}

int PadArgs(const uint64_t *off, uint64_t n, uint32_t row_len, uint32_t flags, const int32_t *out) {
  const int rc = DenseArgs(off, row_len, flags, out);
  if (rc != SPM_OK) return rc;
  if (n > std::numeric_limits<uint64_t>::max() / row_len) return Fail(SPM_OUT_OF_RANGE, "n * row_len exceeds 64 bits");
  return SPM_OK;
}

int PackArgs(const uint64_t *off, uint64_t n, uint32_t row_len, const int32_t *out, uint64_t *rows_capacity) {
  const int rc = DenseArgs(off, row_len, 0, out);
  if (rc != SPM_OK) return rc;
  if (n > 0x7FFFFFFFull) return Fail(SPM_OUT_OF_RANGE, "too many sentences in one batch");
  // More rows than 64-bit slots cannot be written anyway.
  *rows_capacity = std::min(*rows_capacity, std::numeric_limits<uint64_t>::max() / row_len);
  return SPM_OK;
}

}  // namespace

int spm_hip_pad_ids(const int32_t *d_ids, const uint64_t *d_off, uint64_t n, uint32_t row_len, int32_t pad_id,
                    uint32_t flags, int32_t *d_out, int32_t *d_lengths, uint8_t *d_mask, uint64_t *d_stats,
                    void *stream) {
  const int rc = PadArgs(d_off, n, row_len, flags, d_out);
  if (rc != SPM_OK) return rc;
  spm_amd::TraceRange trace_range_("spm_hip_pad_ids");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (d_stats) SPM_HIP_TRY(hipMemsetAsync(d_stats, 0, 2 * sizeof(uint64_t), st));
  SPM_HIP_TRY(spm_amd::LaunchDensePad(d_ids, d_off, n, row_len, pad_id, flags, d_out, d_lengths, d_mask, d_stats, st));
  return SPM_OK;
}

int spm_hip_pack_ids(const int32_t *d_ids, const uint64_t *d_off, uint64_t n, uint32_t row_len, int32_t pad_id,
                     uint64_t rows_capacity, int32_t *d_out, int32_t *d_seq, int32_t *d_pos, uint64_t *d_stats,
                     void *stream) {
  const int rc = PackArgs(d_off, n, row_len, d_out, &rows_capacity);
  if (rc != SPM_OK) return rc;
  spm_amd::TraceRange trace_range_("spm_hip_pack_ids");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0 && d_stats) SPM_HIP_TRY(hipMemsetAsync(d_stats, 0, 2 * sizeof(uint64_t), st));
  SPM_HIP_TRY(spm_amd::LaunchDensePack(d_ids, d_off, n, row_len, pad_id, rows_capacity, d_out, d_seq, d_pos, d_stats,
                                       st));
  return SPM_OK;
}

int spm_hip_pad_ids_host(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t row_len, int32_t pad_id,
                         uint32_t flags, int32_t *out, int32_t *lengths, uint8_t *mask, uint64_t *stats) {
  const int rc = PadArgs(off, n, row_len, flags, out);
  if (rc != SPM_OK) return rc;
  spm_amd::DensePadHostLoop(ids, off, n, row_len, pad_id, flags, out, lengths, mask, stats);
  return SPM_OK;
}

int spm_hip_pack_ids_host(const int32_t *ids, const uint64_t *off, uint64_t n, uint32_t row_len, int32_t pad_id,
                          uint64_t rows_capacity, int32_t *out, int32_t *seq, int32_t *pos, uint64_t *stats) {
  const int rc = PackArgs(off, n, row_len, out, &rows_capacity);
  if (rc != SPM_OK) return rc;
  spm_amd::DensePackHostLoop(ids, off, n, row_len, pad_id, rows_capacity, out, seq, pos, stats);
  return SPM_OK;
}

}  // extern "C"
