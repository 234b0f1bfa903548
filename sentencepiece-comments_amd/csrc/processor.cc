// SentencePieceProcessor mirror (see processor.h).
#include "processor.h"

#include <hip/hip_runtime.h>

#include "decode.h"
#include "scratch_cache.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <random>
#include <sstream>

namespace spm_amd {
namespace {

Status Err(int code, const std::string &msg) { return Status{code, msg}; }

Status FromC(int rc) {
  if (rc == SPM_OK) return Status::Ok();
  return Err(rc, spm_hip_last_error());
}

}  // namespace

SentencePieceProcessor::~SentencePieceProcessor() { spm_hip_model_free(model_); }

void *SentencePieceProcessor::Staging::Get(int k, size_t bytes) {
  bytes = std::max<size_t>(bytes, 16);
  if (bytes > cap[k]) {
    if (ptr[k]) (void)DevFree(ptr[k]);
    ptr[k] = nullptr;
    cap[k] = 0;
    const size_t c = bytes + bytes / 4;
    if (DevMalloc(&ptr[k], c) != hipSuccess) return nullptr;
    cap[k] = c;
  }
  return ptr[k];
}

SentencePieceProcessor::Staging::~Staging() {
  for (void *p : ptr)
    if (p) (void)DevFree(p);
}

SentencePieceProcessor::SmallPath::~SmallPath() {
  if (stream) (void)hipStreamDestroy(static_cast<hipStream_t>(stream));
  if (pin) (void)hipHostFree(pin);
}

Status SentencePieceProcessor::Load(const std::string &filename) {
  std::ifstream in(filename, std::ios::binary);
  if (!in) return Err(SPM_NOT_FOUND, "\"" + filename + "\": No such file or directory");
  std::string proto((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  return LoadFromSerializedProto(proto);
}

Status SentencePieceProcessor::LoadFromSerializedProto(const std::string &serialized) {
  return LoadImpl(serialized, false);
}

Status SentencePieceProcessor::LoadHostOnly(const std::string &serialized) { return LoadImpl(serialized, true); }

Status SentencePieceProcessor::LoadImpl(const std::string &serialized, bool host_only) {
  host_only_ = host_only;
  spm_hip_model_free(model_);
  model_ = nullptr;
  proto_ = ModelProtoView();
  pieces_.clear();
  reserved_.clear();
  std::fill(byte_ids_, byte_ids_ + 256, -1);
  std::string err;
  if (!ParseModelProto(reinterpret_cast<const uint8_t *>(serialized.data()), serialized.size(),
                       &proto_, &err))
    return status_ = Err(SPM_INTERNAL, err);
  Status st = FromC(host_only ? spm_hip_model_load_host_only(serialized.data(), serialized.size(), &model_)
                              : spm_hip_model_load(serialized.data(), serialized.size(), &model_));
  if (!st.ok()) return status_ = st;
  for (size_t i = 0; i < proto_.pieces.size(); ++i) {
    const auto &p = proto_.pieces[i];
    const bool normal = p.type == kNormal || p.type == kUserDefined || p.type == kUnused;
    (normal ? pieces_ : reserved_).emplace(p.piece, static_cast<int>(i));
    if (p.type == kBytePiece && PieceToByte(p.piece) >= 0) byte_ids_[PieceToByte(p.piece)] = static_cast<int>(i);
  }
  status_ = Status::Ok();
  // Self-test samples (sentencepiece_processor.cc:135-153).
  std::vector<std::string> inputs;
  for (const auto &s : proto_.self_test) inputs.push_back(s.first);
  if (!inputs.empty() && !host_only) {
    std::vector<std::vector<std::string>> got;
    Status e = EncodeBatch(inputs, nullptr, &got);
    if (!e.ok()) return status_ = e;
    int fails = 0;
    for (size_t i = 0; i < inputs.size(); ++i) {
      std::string joined;
      for (size_t k = 0; k < got[i].size(); ++k) joined += (k ? " " : "") + got[i][k];
      if (joined != proto_.self_test[i].second) ++fails;
    }
    if (fails) return status_ = Err(SPM_INTERNAL, "Self-test failures. See LOG(INFO).");
  }
  return status_;
}

Status SentencePieceProcessor::status() const { return status_; }

int SentencePieceProcessor::GetPieceSize() const { return static_cast<int>(proto_.pieces.size()); }

// ModelInterface::PieceToId (model_interface.cc:87-97).
int SentencePieceProcessor::PieceToId(const std::string &piece) const {
  auto r = reserved_.find(piece);
  if (r != reserved_.end()) return r->second;
  auto p = pieces_.find(piece);
  if (p != pieces_.end()) return p->second;
  return unk_id();
}

const std::string &SentencePieceProcessor::IdToPiece(int id) const {
  static const std::string kEmpty;
  if (id < 0 || id >= GetPieceSize()) return kEmpty;
  return proto_.pieces[id].piece;
}
float SentencePieceProcessor::GetScore(int id) const { return proto_.pieces[id].score; }
bool SentencePieceProcessor::IsUnknown(int id) const {
  return id >= 0 && id < GetPieceSize() && proto_.pieces[id].type == kUnknown;
}
bool SentencePieceProcessor::IsControl(int id) const {
  return id >= 0 && id < GetPieceSize() && proto_.pieces[id].type == kControl;
}
bool SentencePieceProcessor::IsByte(int id) const {
  return id >= 0 && id < GetPieceSize() && proto_.pieces[id].type == kBytePiece;
}
bool SentencePieceProcessor::IsUnused(int id) const {
  return id >= 0 && id < GetPieceSize() && proto_.pieces[id].type == kUnused;
}
int SentencePieceProcessor::unk_id() const {
  for (size_t i = 0; i < proto_.pieces.size(); ++i)
    if (proto_.pieces[i].type == kUnknown) return static_cast<int>(i);
  return -1;
}
int SentencePieceProcessor::bos_id() const {
  const int id = PieceToId(proto_.trainer_spec.bos_piece);
  return IsControl(id) ? id : -1;
}
int SentencePieceProcessor::eos_id() const {
  const int id = PieceToId(proto_.trainer_spec.eos_piece);
  return IsControl(id) ? id : -1;
}
int SentencePieceProcessor::pad_id() const {
  const int id = PieceToId(proto_.trainer_spec.pad_piece);
  return IsControl(id) ? id : -1;
}

// ParseExtraOptions (sentencepiece_processor.cc:981-1023).
Status SentencePieceProcessor::ParseExtraOptions(const std::string &opts, std::vector<ExtraOption> *out) const {
  out->clear();
  if (opts.empty()) return Status::Ok();
  if (!status_.ok()) return status_;
  std::vector<std::string> parts;
  size_t st = 0;
  while (true) {
    const size_t e = opts.find(':', st);
    parts.push_back(opts.substr(st, e == std::string::npos ? std::string::npos : e - st));
    if (e == std::string::npos) break;
    st = e + 1;
  }
  for (const auto &s : parts) {
    if (s.empty()) continue;  // SplitPiece drops empty fields
    if (s == "bos") {
      if (IsUnknown(PieceToId(proto_.trainer_spec.bos_piece)))
        return Err(SPM_INTERNAL, "id for `" + proto_.trainer_spec.bos_piece + "` is not defined.");
      out->push_back(BOS);
    } else if (s == "eos") {
      if (IsUnknown(PieceToId(proto_.trainer_spec.eos_piece)))
        return Err(SPM_INTERNAL, "id for `" + proto_.trainer_spec.eos_piece + "` is not defined.");
      out->push_back(EOS);
    } else if (s == "reverse") {
      out->push_back(REVERSE);
    } else {
      return Err(SPM_INTERNAL, "option \"" + s + "\" is not available.");
    }
  }
  return Status::Ok();
}

Status SentencePieceProcessor::SetEncodeExtraOptions(const std::string &opts) {
  extra_str_.clear();
  const Status st = ParseExtraOptions(opts, &extra_);
  if (!st.ok()) return st;  // like the reference, the options parsed so far stay
  extra_str_ = opts;
  return Status::Ok();
}

Status SentencePieceProcessor::SetDecodeExtraOptions(const std::string &opts) {
  decode_extra_str_.clear();
  const Status st = ParseExtraOptions(opts, &decode_extra_);
  if (!st.ok()) return st;
  decode_extra_str_ = opts;
  return Status::Ok();
}

namespace {
constexpr uint64_t kSmallLines = 4096;
constexpr uint64_t kSmallBytes = 64 << 10;
inline uint64_t Al256(uint64_t x) { return (x + 255) & ~255ull; }
}  // namespace

// Encode(ids) of a small batch — the reference's per-line plugin point
// (sentencepiece_processor.cc:319-330) — as ONE stream-ordered chain: the
// zeroed status word, offsets and raw bytes go up in one copy from pinned
// memory, spm_hip_normalize_batch_device_async -> spm_hip_encode_batch_async
// -> spm_hip_finalize_ids_async run back to back on a private stream, and
// the status word and the final ids come back with one synchronization.
// The normalized size is bounded by a guess (4 bytes per raw byte + 8 per
// line); a batch that exceeds it reports RESOURCE_EXHAUSTED in the status
// word and takes the general path.
Status SentencePieceProcessor::EncodeIdsSmall(const std::vector<std::string> &inputs,
                                              std::vector<std::vector<int>> *ids, bool *done) const {
  *done = false;
  const uint64_t n = inputs.size();
  uint64_t raw = 0;
  for (const auto &s : inputs) raw += s.size();
  const bool bf = proto_.trainer_spec.byte_fallback;
  if (extra_.empty() && n <= 16) {
    // One launch: normalize + encode + unknown-run merge (coop_raw_kernel).
    // (A byte-fallback model gets SPM_UNIMPLEMENTED and takes the chain below.)
    std::vector<uint64_t> roff(n + 1, 0);
    std::string rb;
    rb.reserve(raw);
    for (uint64_t i = 0; i < n; ++i) {
      rb += inputs[i];
      roff[i + 1] = rb.size();
    }
    std::vector<int32_t> out(4 * raw + 8 * n + 64);
    std::vector<uint64_t> ooff(n + 1);
    const int rc = spm_hip_encode_raw_small_host(model_, reinterpret_cast<const uint8_t *>(rb.data()), roff.data(),
                                                 n, out.data(), out.size(), ooff.data());
    if (rc == SPM_OK) {
      ids->assign(n, {});
      for (uint64_t i = 0; i < n; ++i) (*ids)[i].assign(out.begin() + ooff[i], out.begin() + ooff[i + 1]);
      *done = true;
      return Status::Ok();
    }
    if (rc != SPM_UNIMPLEMENTED) return FromC(rc);
  }
  uint64_t n_extra = 0;
  for (ExtraOption opt : extra_) n_extra += opt != REVERSE;
  const uint64_t cap_norm = 4 * raw + 8 * n + 64, cap_out = cap_norm + n * n_extra;
  // Device block: [status | in_off | in bytes] (uploaded) [norm | norm_off |
  // ids | tok] (device only) [out_off | out ids] (downloaded).
  const uint64_t o_inoff = 256, o_in = Al256(o_inoff + (n + 1) * 8), up_end = o_in + raw;
  const uint64_t o_norm = Al256(up_end + 16), o_noff = Al256(o_norm + cap_norm);
  // (byte fallback: the piece lengths follow the ids, for spm_hip_finalize_ids_bytes_async)
  const uint64_t o_ids = Al256(o_noff + (n + 1) * 8), o_len = Al256(o_ids + cap_norm * 4);
  const uint64_t o_tok = bf ? Al256(o_len + cap_norm * 4) : o_len;
  const uint64_t o_oo = Al256(o_tok + (n + 1) * 8), o_out = Al256(o_oo + (n + 1) * 8);
  const uint64_t end = o_out + cap_out * 4;
  enum { kSmallBlock = 9 };
  uint8_t *d = static_cast<uint8_t *>(dev_.Get(kSmallBlock, end));
  if (!d) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
  auto fail_hip = [](hipError_t e) { return Err(SPM_INTERNAL, hipGetErrorString(e)); };
  hipError_t he;
  if (!small_.stream) {
    hipStream_t s;
    if ((he = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) return fail_hip(he);
    small_.stream = s;
  }
  if (small_.pin_cap < end) {
    if (small_.pin) (void)hipHostFree(small_.pin);
    small_.pin = nullptr;
    small_.pin_cap = 0;
    const size_t want = std::max<uint64_t>(end + end / 4, 1 << 20);
    if ((he = hipHostMalloc(reinterpret_cast<void **>(&small_.pin), want)) != hipSuccess) return fail_hip(he);
    small_.pin_cap = want;
  }
  hipStream_t st = static_cast<hipStream_t>(small_.stream);
  uint8_t *h = small_.pin;
  std::memset(h, 0, 256);
  uint64_t *in_off = reinterpret_cast<uint64_t *>(h + o_inoff);
  in_off[0] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    std::memcpy(h + o_in + in_off[i], inputs[i].data(), inputs[i].size());
    in_off[i + 1] = in_off[i] + inputs[i].size();
  }
  if ((he = hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, st)) != hipSuccess) return fail_hip(he);
  uint32_t *d_status = reinterpret_cast<uint32_t *>(d);
  int rc = spm_hip_normalize_batch_device_async(model_, d + o_in, reinterpret_cast<uint64_t *>(d + o_inoff), n,
                                                d + o_norm, cap_norm, reinterpret_cast<uint64_t *>(d + o_noff),
                                                nullptr, d_status, st);
  if (rc == SPM_OK)
    rc = spm_hip_encode_batch_async(model_, d + o_norm, reinterpret_cast<uint64_t *>(d + o_noff), n, cap_norm,
                                    reinterpret_cast<int32_t *>(d + o_ids),
                                    bf ? reinterpret_cast<uint32_t *>(d + o_len) : nullptr,
                                    reinterpret_cast<uint64_t *>(d + o_tok), d_status, st);
  if (rc == SPM_OK && bf)
    rc = spm_hip_finalize_ids_bytes_async(model_, extra_str_.c_str(), reinterpret_cast<int32_t *>(d + o_ids),
                                          reinterpret_cast<uint32_t *>(d + o_len),
                                          reinterpret_cast<uint64_t *>(d + o_tok), n, d + o_norm,
                                          reinterpret_cast<uint64_t *>(d + o_noff),
                                          reinterpret_cast<int32_t *>(d + o_out), cap_out,
                                          reinterpret_cast<uint64_t *>(d + o_oo), d_status, st);
  else if (rc == SPM_OK)
    rc = spm_hip_finalize_ids_async(model_, extra_str_.c_str(), reinterpret_cast<int32_t *>(d + o_ids),
                                    reinterpret_cast<uint64_t *>(d + o_tok), n, reinterpret_cast<int32_t *>(d + o_out),
                                    cap_out, reinterpret_cast<uint64_t *>(d + o_oo), d_status, st);
  if (rc != SPM_OK) return FromC(rc);
  if ((he = hipMemcpyAsync(h, d, 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (he = hipMemcpyAsync(h + o_oo, d + o_oo, end - o_oo, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (he = hipStreamSynchronize(st)) != hipSuccess)
    return fail_hip(he);
  uint32_t code;
  std::memcpy(&code, h, 4);
  if (code == SPM_RESOURCE_EXHAUSTED) return Status::Ok();  // not done: the general path
  if (code != SPM_OK) return Err(static_cast<int>(code), "device encode failed");
  const uint64_t *oo = reinterpret_cast<const uint64_t *>(h + o_oo);
  const int32_t *out = reinterpret_cast<const int32_t *>(h + o_out);
  ids->resize(n);
  for (uint64_t i = 0; i < n; ++i) (*ids)[i].assign(out + oo[i], out + oo[i + 1]);
  *done = true;
  return Status::Ok();
}

Status SentencePieceProcessor::EncodeBatch(const std::vector<std::string> &inputs,
                                           std::vector<std::vector<int>> *ids,
                                           std::vector<std::vector<std::string>> *pieces) const {
  return RunBatch(inputs, ids, pieces, nullptr);
}

void SentencePieceProcessor::SetRandomSeed(uint64_t seed) {
  sample_seed_ = seed;
  sample_count_ = 0;
  sample_seeded_ = true;
}

Status SentencePieceProcessor::SampleEncodeBatch(const std::vector<std::string> &inputs, int nbest_size, float alpha,
                                                 std::vector<std::vector<int>> *ids,
                                                 std::vector<std::vector<std::string>> *pieces) const {
  if (!status_.ok()) return status_;
  if (nbest_size > 512) return Err(SPM_INTERNAL, "nbest_size must be nbest_size <= 512");
  if (nbest_size == 0 || nbest_size == 1) return RunBatch(inputs, ids, pieces, nullptr);
  // A BPE model samples by BPE-dropout with probability alpha, whatever
  // nbest_size is (the package ignores it there).
  const bool bpe = proto_.trainer_spec.model_type == kBpe;
  if (nbest_size > 1 && !bpe)
    return Err(SPM_UNIMPLEMENTED,
               "SampleEncode among the n best (nbest_size > 1) is not implemented on the device; "
               "use nbest_size=-1 to sample from the whole lattice");
  if (!sample_seeded_) {
    std::random_device rd;
    sample_seed_ = (static_cast<uint64_t>(rd()) << 32) | rd();
    sample_seeded_ = true;
  }
  const SampleSpec spec{alpha, sample_seed_, sample_count_};
  Status st = RunBatch(inputs, ids, pieces, &spec);
  if (st.ok()) sample_count_ += inputs.size();
  return st;
}

Status SentencePieceProcessor::SampleEncode(const std::string &input, int nbest_size, float alpha,
                                            std::vector<int> *ids) const {
  if (!ids) return Err(SPM_INTERNAL, "output container is null");
  std::vector<std::vector<int>> out;
  Status st = SampleEncodeBatch({input}, nbest_size, alpha, &out, nullptr);
  if (st.ok()) *ids = std::move(out[0]);
  return st;
}

Status SentencePieceProcessor::SampleEncode(const std::string &input, int nbest_size, float alpha,
                                            std::vector<std::string> *pieces) const {
  if (!pieces) return Err(SPM_INTERNAL, "output container is null");
  std::vector<std::vector<std::string>> out;
  Status st = SampleEncodeBatch({input}, nbest_size, alpha, nullptr, &out);
  if (st.ok()) *pieces = std::move(out[0]);
  return st;
}

namespace {
enum {
  kIn, kInOff, kNorm, kNormOff, kIds, kLen, kTok, kOut, kOutOff, kSmallBlockSlot, kCounts,
  kDenseIds, kDenseAux0, kDenseAux1, kDenseStats
};
}  // namespace

// CalculateEntropy of the `sentencepiece` package, batched: the device
// normalizer, then spm_hip_entropy_batch.
Status SentencePieceProcessor::CalculateEntropy(const std::vector<std::string> &inputs, float alpha,
                                                std::vector<float> *entropy) const {
  if (!status_.ok()) return status_;
  if (!entropy) return Err(SPM_INTERNAL, "output container is null");
  if (host_only_) return Err(SPM_FAILED_PRECONDITION, "host-only processor");
  if (proto_.trainer_spec.model_type != kUnigram)
    return Err(SPM_INTERNAL, "CalculateEntropy is not available for the current model.");
  const uint64_t n = inputs.size();
  entropy->assign(n, 0.f);
  if (n == 0) return Status::Ok();
  uint8_t *d_norm = nullptr;
  uint64_t *d_norm_off = nullptr;
  uint64_t total = 0;
  Status st = DeviceNormalize(inputs, &d_norm, &d_norm_off, &total);
  if (!st.ok()) return st;
  float *d_h = static_cast<float *>(dev_.Get(kOut, n * 4));
  if (!d_h) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
  st = FromC(spm_hip_entropy_batch(model_, d_norm, d_norm_off, n, alpha, d_h, nullptr, nullptr));
  if (!st.ok()) return st;
  const hipError_t he = hipMemcpy(entropy->data(), d_h, n * 4, hipMemcpyDeviceToHost);
  return he == hipSuccess ? Status::Ok() : Err(SPM_INTERNAL, hipGetErrorString(he));
}

Status SentencePieceProcessor::CalculateEntropy(const std::string &input, float alpha, float *entropy) const {
  if (!entropy) return Err(SPM_INTERNAL, "output container is null");
  std::vector<float> out;
  const Status st = CalculateEntropy(std::vector<std::string>{input}, alpha, &out);
  if (st.ok()) *entropy = out[0];
  return st;
}

// SampleEncodeAndScore of the package with wor = false, batched: the device
// normalizer, spm_hip_sample_encode_and_score_batch, then
// PopulateSentencePieceText on every sample.
Status SentencePieceProcessor::SampleEncodeAndScoreBatch(
    const std::vector<std::string> &inputs, int num_samples, float alpha, bool wor, bool include_best,
    std::vector<std::vector<std::pair<std::vector<int>, float>>> *ids,
    std::vector<std::vector<std::pair<std::vector<std::string>, float>>> *pieces) const {
  if (!status_.ok()) return status_;
  if (host_only_) return Err(SPM_FAILED_PRECONDITION, "host-only processor");
  if (proto_.trainer_spec.model_type != kUnigram)
    return Err(SPM_INTERNAL, "SampleEncodeAndScore is not available for the current model.");
  if (wor || include_best)
    return Err(SPM_UNIMPLEMENTED,
               "SampleEncodeAndScore without replacement (wor, include_best) is not implemented on the device; "
               "use wor=false, include_best=false");
  if (num_samples <= 0) return Err(SPM_INTERNAL, "SampleEncodeAndScore returns empty result.");
  const uint64_t n = inputs.size(), ns = static_cast<uint64_t>(num_samples), rows = n * ns;
  if (ids) ids->assign(n, {});
  if (pieces) pieces->assign(n, {});
  if (n == 0) return Status::Ok();
  if (!sample_seeded_) {
    std::random_device rd;
    sample_seed_ = (static_cast<uint64_t>(rd()) << 32) | rd();
    sample_seeded_ = true;
  }
  uint8_t *d_norm = nullptr;
  uint64_t *d_norm_off = nullptr;
  uint64_t total = 0;
  Status st = DeviceNormalize(inputs, &d_norm, &d_norm_off, &total);
  if (!st.ok()) return st;
  const uint64_t cap = std::max<uint64_t>(total * ns, 1);
  int32_t *d_ids = static_cast<int32_t *>(dev_.Get(kIds, cap * 4));
  uint32_t *d_len = static_cast<uint32_t *>(dev_.Get(kLen, cap * 4));
  uint64_t *d_tok = static_cast<uint64_t *>(dev_.Get(kTok, (rows + 1) * 8));
  float *d_sc = static_cast<float *>(dev_.Get(kOut, rows * 4));
  if (!d_ids || !d_len || !d_tok || !d_sc) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
  st = FromC(spm_hip_sample_encode_and_score_batch(model_, d_norm, d_norm_off, n, static_cast<uint32_t>(ns), alpha,
                                                   sample_seed_, sample_count_, d_ids, cap, d_len, d_tok, d_sc,
                                                   nullptr));
  if (!st.ok()) return st;
  sample_count_ += n;
  auto fail_hip = [](hipError_t e) { return Err(SPM_INTERNAL, hipGetErrorString(e)); };
  hipError_t he;
  std::vector<uint64_t> norm_off(n + 1), tok_off(rows + 1);
  std::vector<float> sc(rows);
  if ((he = hipMemcpy(norm_off.data(), d_norm_off, (n + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (he = hipMemcpy(tok_off.data(), d_tok, (rows + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (he = hipMemcpy(sc.data(), d_sc, rows * 4, hipMemcpyDeviceToHost)) != hipSuccess)
    return fail_hip(he);
  const uint64_t ntok = tok_off[rows];
  std::vector<int32_t> tok_ids(std::max<uint64_t>(ntok, 1));
  std::vector<uint32_t> tok_len(std::max<uint64_t>(ntok, 1));
  const bool need_norm = pieces || proto_.trainer_spec.byte_fallback;
  std::vector<uint8_t> norm(need_norm ? std::max<uint64_t>(total, 1) : 0);
  if ((he = hipMemcpy(tok_ids.data(), d_ids, ntok * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (he = hipMemcpy(tok_len.data(), d_len, ntok * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (need_norm && (he = hipMemcpy(norm.data(), d_norm, total, hipMemcpyDeviceToHost)) != hipSuccess))
    return fail_hip(he);
  std::vector<std::pair<std::string, int>> spt;
  for (uint64_t i = 0; i < n; ++i) {
    // The package's model returns no sample for an empty normalized text.
    if (norm_off[i + 1] == norm_off[i]) return Err(SPM_INTERNAL, "SampleEncodeAndScore returns empty result.");
    const char *normalized = need_norm ? reinterpret_cast<const char *>(norm.data()) + norm_off[i] : nullptr;
    for (uint64_t j = 0; j < ns; ++j) {
      const uint64_t r = i * ns + j;
      Status ps = PopulateText(normalized, norm_off[i + 1] - norm_off[i], tok_ids.data() + tok_off[r],
                               tok_len.data() + tok_off[r], tok_off[r + 1] - tok_off[r], &spt);
      if (!ps.ok()) return ps;
      if (ids) {
        (*ids)[i].emplace_back(std::vector<int>(), sc[r]);
        for (auto &p : spt) (*ids)[i].back().first.push_back(p.second);
      }
      if (pieces) {
        (*pieces)[i].emplace_back(std::vector<std::string>(), sc[r]);
        for (auto &p : spt) (*pieces)[i].back().first.push_back(std::move(p.first));
      }
    }
  }
  return Status::Ok();
}

Status SentencePieceProcessor::SampleEncodeAndScore(const std::string &input, int num_samples, float alpha, bool wor,
                                                    bool include_best,
                                                    std::vector<std::pair<std::vector<int>, float>> *ids) const {
  if (!ids) return Err(SPM_INTERNAL, "output container is null");
  std::vector<std::vector<std::pair<std::vector<int>, float>>> out;
  Status st = SampleEncodeAndScoreBatch({input}, num_samples, alpha, wor, include_best, &out, nullptr);
  if (st.ok()) *ids = std::move(out[0]);
  return st;
}

Status SentencePieceProcessor::SampleEncodeAndScore(
    const std::string &input, int num_samples, float alpha, bool wor, bool include_best,
    std::vector<std::pair<std::vector<std::string>, float>> *pieces) const {
  if (!pieces) return Err(SPM_INTERNAL, "output container is null");
  std::vector<std::vector<std::pair<std::vector<std::string>, float>>> out;
  Status st = SampleEncodeAndScoreBatch({input}, num_samples, alpha, wor, include_best, nullptr, &out);
  if (st.ok()) *pieces = std::move(out[0]);
  return st;
}

// Raw lines -> device; Normalizer::Normalize and ModelInterface::Encode (or
// the sampler) run on the device over the whole batch.  *b: the device
// buffers of the normalized bytes and the model-level tokens.
Status SentencePieceProcessor::DeviceEncode(const std::vector<std::string> &inputs, const SampleSpec *sample,
                                            DeviceBatch *b) const {
  const uint64_t n = inputs.size();
  uint8_t *d_norm = nullptr;
  uint64_t *d_norm_off = nullptr;
  uint64_t total = 0;
  Status st = DeviceNormalize(inputs, &d_norm, &d_norm_off, &total);
  if (!st.ok()) return st;
  uint64_t *d_tok = static_cast<uint64_t *>(dev_.Get(kTok, (n + 1) * 8));
  int32_t *d_ids = static_cast<int32_t *>(dev_.Get(kIds, std::max<uint64_t>(total, 1) * 4));
  uint32_t *d_len = static_cast<uint32_t *>(dev_.Get(kLen, std::max<uint64_t>(total, 1) * 4));
  if (!d_tok || !d_ids || !d_len) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
  if (sample && proto_.trainer_spec.model_type == kBpe)  // BPE-dropout: theta is the drop probability
    st = FromC(spm_hip_bpe_dropout_encode_batch(model_, d_norm, d_norm_off, n, sample->theta, sample->seed,
                                                sample->index_base, d_ids, d_len, d_tok, nullptr));
  else
    st = FromC(sample ? spm_hip_sample_encode_batch(model_, d_norm, d_norm_off, n, sample->theta, sample->seed,
                                                    sample->index_base, d_ids, d_len, d_tok, nullptr)
                      : spm_hip_encode_batch(model_, d_norm, d_norm_off, n, d_ids, d_len, d_tok, nullptr));
  if (!st.ok()) return st;
  *b = DeviceBatch{d_norm, d_norm_off, d_ids, d_len, d_tok, total};
  return Status::Ok();
}

// Raw lines -> device and Normalizer::Normalize over the whole batch: the
// normalized bytes, their offsets (dev_'s buffers) and their number.
Status SentencePieceProcessor::DeviceNormalize(const std::vector<std::string> &inputs, uint8_t **d_norm_out,
                                               uint64_t **d_norm_off_out, uint64_t *total_out) const {
  const uint64_t n = inputs.size();
  std::vector<uint64_t> in_off(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) in_off[i + 1] = in_off[i] + inputs[i].size();
  std::string in_bytes;
  in_bytes.reserve(in_off[n]);
  for (const auto &s : inputs) in_bytes += s;
  auto fail_hip = [](hipError_t e) { return Err(SPM_INTERNAL, hipGetErrorString(e)); };
  uint8_t *d_in = static_cast<uint8_t *>(dev_.Get(kIn, in_off[n]));
  uint64_t *d_in_off = static_cast<uint64_t *>(dev_.Get(kInOff, (n + 1) * 8));
  uint64_t *d_norm_off = static_cast<uint64_t *>(dev_.Get(kNormOff, (n + 1) * 8));
  if (!d_in || !d_in_off || !d_norm_off) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
  hipError_t he;
  if ((he = hipMemcpy(d_in, in_bytes.data(), in_off[n], hipMemcpyHostToDevice)) != hipSuccess ||
      (he = hipMemcpy(d_in_off, in_off.data(), (n + 1) * 8, hipMemcpyHostToDevice)) != hipSuccess)
    return fail_hip(he);
  uint64_t total = 0;
  uint64_t ncap = dev_.cap[kNorm];
  uint8_t *d_norm = static_cast<uint8_t *>(dev_.Get(kNorm, std::max<uint64_t>(ncap, 1)));
  int rc = spm_hip_normalize_batch_device(model_, d_in, d_in_off, n, d_norm, dev_.cap[kNorm],
                                          d_norm_off, &total, nullptr);
  if (rc == SPM_RESOURCE_EXHAUSTED) {
    d_norm = static_cast<uint8_t *>(dev_.Get(kNorm, total));
    if (!d_norm) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
    rc = spm_hip_normalize_batch_device(model_, d_in, d_in_off, n, d_norm, dev_.cap[kNorm], d_norm_off,
                                        &total, nullptr);
  }
  Status st = FromC(rc);
  if (!st.ok()) return st;
  *d_norm_out = d_norm;
  *d_norm_off_out = d_norm_off;
  *total_out = total;
  return Status::Ok();
}

// The id epilogue of Encode(ids) on the device (spm_hip_finalize_ids: unknown
// -run merge + extra options): the final ids, their offsets and their number.
Status SentencePieceProcessor::DeviceFinalize(const DeviceBatch &b, uint64_t n, int32_t **d_out, uint64_t **d_out_off,
                                              uint64_t *fin) const {
  uint64_t n_extra = 0;
  for (ExtraOption opt : extra_) n_extra += opt != REVERSE;
  const uint64_t cap = b.total + n * n_extra;
  *d_out_off = static_cast<uint64_t *>(dev_.Get(kOutOff, (n + 1) * 8));
  *d_out = static_cast<int32_t *>(dev_.Get(kOut, std::max<uint64_t>(cap, 1) * 4));
  if (!*d_out_off || !*d_out) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
  if (proto_.trainer_spec.byte_fallback)  // unknown tokens expand to their bytes: at most b.total ids
    return FromC(spm_hip_finalize_ids_bytes(model_, extra_str_.c_str(), b.d_ids, b.d_len, b.d_tok, n, b.d_norm,
                                            b.d_norm_off, *d_out, cap, *d_out_off, fin, nullptr));
  return FromC(spm_hip_finalize_ids(model_, extra_str_.c_str(), b.d_ids, b.d_tok, n, *d_out, cap, *d_out_off, fin,
                                    nullptr));
}

Status SentencePieceProcessor::RunBatch(const std::vector<std::string> &inputs, std::vector<std::vector<int>> *ids,
                                        std::vector<std::vector<std::string>> *pieces,
                                        const SampleSpec *sample) const {
  if (!status_.ok()) return status_;
  if (host_only_) return Err(SPM_FAILED_PRECONDITION, "host-only processor");
  const uint64_t n = inputs.size();
  // A WORD / CHAR model can return a CONTROL piece's id for a token (a word
  // that spells it: PieceToId searches the reserved pieces first).  Such a
  // token consumes no surface, so the reference fails the line ("all
  // normalized characters are not consumed.").  The device id epilogue does
  // not carry that check, so these models' ids take the host epilogue below.
  const bool word_char = proto_.trainer_spec.model_type == kWord || proto_.trainer_spec.model_type == kChar;
  if (!sample && !pieces && ids && !word_char && n >= 1 && n <= kSmallLines) {
    uint64_t raw = 0;
    for (const auto &s : inputs) raw += s.size();
    if (raw <= kSmallBytes) {
      bool done = false;
      Status st = EncodeIdsSmall(inputs, ids, &done);
      if (!st.ok() || done) return st;
    }
  }
  auto fail_hip = [](hipError_t e) { return Err(SPM_INTERNAL, hipGetErrorString(e)); };
  hipError_t he;
  DeviceBatch b;
  Status st = DeviceEncode(inputs, sample, &b);
  if (!st.ok()) return st;
  uint8_t *d_norm = b.d_norm;
  uint64_t *d_norm_off = b.d_norm_off, *d_tok = b.d_tok;
  int32_t *d_ids = b.d_ids;
  uint32_t *d_len = b.d_len;
  const uint64_t total = b.total;
  if (!pieces && !word_char) {
    // Encode(ids): the id epilogue (unk-run merge + extra options) runs on the
    // device as well (spm_hip_finalize_ids); only the final ids come back.
    int32_t *d_out = nullptr;
    uint64_t *d_out_off = nullptr;
    uint64_t fin = 0;
    st = DeviceFinalize(b, n, &d_out, &d_out_off, &fin);
    if (!st.ok()) return st;
    std::vector<uint64_t> out_off(n + 1);
    std::vector<int32_t> out(std::max<uint64_t>(fin, 1));
    if ((he = hipMemcpy(out_off.data(), d_out_off, (n + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
        (fin && (he = hipMemcpy(out.data(), d_out, fin * 4, hipMemcpyDeviceToHost)) != hipSuccess))
      return fail_hip(he);
    if (ids) {
      ids->resize(n);
      for (uint64_t i = 0; i < n; ++i) (*ids)[i].assign(out.begin() + out_off[i], out.begin() + out_off[i + 1]);
    }
    return Status::Ok();
  }
  std::vector<uint64_t> norm_off(n + 1), tok_off(n + 1);
  if ((he = hipMemcpy(norm_off.data(), d_norm_off, (n + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
      (he = hipMemcpy(tok_off.data(), d_tok, (n + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess)
    return fail_hip(he);
  const uint64_t ntok = tok_off[n];
  std::vector<int32_t> tok_ids(std::max<uint64_t>(ntok, 1));
  std::vector<uint32_t> tok_len(std::max<uint64_t>(ntok, 1));
  const bool need_norm = pieces || proto_.trainer_spec.byte_fallback;  // byte pieces come from the text
  std::vector<uint8_t> norm(need_norm ? std::max<uint64_t>(total, 1) : 0);
  if ((he = hipMemcpy(tok_ids.data(), d_ids, ntok * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (he = hipMemcpy(tok_len.data(), d_len, ntok * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (need_norm && (he = hipMemcpy(norm.data(), d_norm, total, hipMemcpyDeviceToHost)) != hipSuccess))
    return fail_hip(he);
  if (ids) ids->assign(n, {});
  if (pieces) pieces->assign(n, {});
  std::vector<std::pair<std::string, int>> spt;
  for (uint64_t i = 0; i < n; ++i) {
    const char *normalized = need_norm ? reinterpret_cast<const char *>(norm.data()) + norm_off[i] : nullptr;
    Status ps = PopulateText(normalized, norm_off[i + 1] - norm_off[i], tok_ids.data() + tok_off[i],
                             tok_len.data() + tok_off[i], tok_off[i + 1] - tok_off[i], &spt);
    if (!ps.ok()) return ps;
    if (ids)
      for (auto &p : spt) (*ids)[i].push_back(p.second);
    if (pieces)
      for (auto &p : spt) (*pieces)[i].push_back(std::move(p.first));
  }
  return Status::Ok();
}

// Dense id batches: the final id CSR of the batch (device encode + device id
// epilogue; WORD / CHAR: RunBatch's host epilogue, uploaded) through
// spm_hip_pad_ids / spm_hip_pack_ids into dev_'s buffers.
Status SentencePieceProcessor::RunDense(const std::vector<std::string> &inputs, const SampleSpec *sample,
                                        const DenseOptions &o, DenseBatch *out,
                                        std::vector<int32_t> *host_ids) const {
  if (!status_.ok()) return status_;
  if (host_only_) return Err(SPM_FAILED_PRECONDITION, "host-only processor");
  if (!out) return Err(SPM_INTERNAL, "output container is null");
  if (o.row_len == 0 || o.row_len > 0x7FFFFFFFu) return Err(SPM_INVALID_ARGUMENT, "row_len must be in [1, INT32_MAX]");
  if (o.flags & ~(o.pack ? 0u : SPM_DENSE_PAD_LEFT | SPM_DENSE_TRUNCATE_LEFT | SPM_DENSE_KEEP_END))
    return Err(SPM_INVALID_ARGUMENT, "unknown dense flag bit");
  *out = DenseBatch();
  out->row_len = o.row_len;
  if (host_ids) host_ids->clear();
  const uint64_t n = inputs.size(), L = o.row_len;
  if (n == 0) return Status::Ok();
  auto fail_hip = [](hipError_t e) { return Err(SPM_INTERNAL, hipGetErrorString(e)); };
  hipError_t he;
  int32_t *d_csr = nullptr;
  uint64_t *d_csr_off = nullptr;
  uint64_t fin = 0;
  const bool word_char = proto_.trainer_spec.model_type == kWord || proto_.trainer_spec.model_type == kChar;
  if (word_char) {
    std::vector<std::vector<int>> rows;
    Status st = RunBatch(inputs, &rows, nullptr, sample);
    if (!st.ok()) return st;
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<int32_t> flat;
    for (uint64_t i = 0; i < n; ++i) {
      flat.insert(flat.end(), rows[i].begin(), rows[i].end());
      off[i + 1] = flat.size();
    }
    fin = flat.size();
    d_csr_off = static_cast<uint64_t *>(dev_.Get(kOutOff, (n + 1) * 8));
    d_csr = static_cast<int32_t *>(dev_.Get(kOut, std::max<uint64_t>(fin, 1) * 4));
    if (!d_csr_off || !d_csr) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
    if ((he = hipMemcpy(d_csr_off, off.data(), (n + 1) * 8, hipMemcpyHostToDevice)) != hipSuccess ||
        (fin && (he = hipMemcpy(d_csr, flat.data(), fin * 4, hipMemcpyHostToDevice)) != hipSuccess))
      return fail_hip(he);
  } else {
    DeviceBatch b;
    Status st = DeviceEncode(inputs, sample, &b);
    if (!st.ok()) return st;
    st = DeviceFinalize(b, n, &d_csr, &d_csr_off, &fin);
    if (!st.ok()) return st;
  }
  // Pack: the row count comes from the id count the epilogue returned.
  const uint64_t rows = o.pack ? (fin + L - 1) / L : n;
  if (rows > std::numeric_limits<uint64_t>::max() / (4 * L)) return Err(SPM_OUT_OF_RANGE, "rows * row_len is too large");
  const uint64_t slots = rows * L;
  int32_t *d_ids = static_cast<int32_t *>(dev_.Get(kDenseIds, slots * 4));
  void *d_a0 = dev_.Get(kDenseAux0, o.pack ? slots * 4 : n * 4);  // seq | lengths
  void *d_a1 = dev_.Get(kDenseAux1, o.pack ? slots * 4 : slots);  // pos | mask
  uint64_t *d_stats = static_cast<uint64_t *>(dev_.Get(kDenseStats, 16));
  if (!d_ids || !d_a0 || !d_a1 || !d_stats) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
  Status st = FromC(o.pack ? spm_hip_pack_ids(d_csr, d_csr_off, n, o.row_len, o.pad_id, rows, d_ids,
                                              static_cast<int32_t *>(d_a0), static_cast<int32_t *>(d_a1), d_stats,
                                              nullptr)
                           : spm_hip_pad_ids(d_csr, d_csr_off, n, o.row_len, o.pad_id, o.flags, d_ids,
                                             static_cast<int32_t *>(d_a0), static_cast<uint8_t *>(d_a1), d_stats,
                                             nullptr));
  if (!st.ok()) return st;
  out->ids = d_ids;
  (o.pack ? out->seq : out->lengths) = static_cast<const int32_t *>(d_a0);
  if (o.pack) out->pos = static_cast<const int32_t *>(d_a1);
  else out->mask = static_cast<const uint8_t *>(d_a1);
  out->stats = d_stats;
  out->rows = rows;
  out->tokens = fin;
  if (host_ids) {
    host_ids->resize(slots);
    uint64_t stats[2] = {0, 0};
    if ((slots && (he = hipMemcpy(host_ids->data(), d_ids, slots * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
        (he = hipMemcpy(stats, d_stats, 16, hipMemcpyDeviceToHost)) != hipSuccess)
      return fail_hip(he);
    if (!o.pack) {
      out->cut = stats[0];
      out->dropped = stats[1];
    }
  }
  return Status::Ok();
}

Status SentencePieceProcessor::EncodeDense(const std::vector<std::string> &inputs, const DenseOptions &options,
                                           DenseBatch *out, std::vector<int32_t> *host_ids) const {
  return RunDense(inputs, nullptr, options, out, host_ids);
}

Status SentencePieceProcessor::SampleEncodeDense(const std::vector<std::string> &inputs, int nbest_size, float alpha,
                                                 const DenseOptions &options, DenseBatch *out,
                                                 std::vector<int32_t> *host_ids) const {
  if (!status_.ok()) return status_;
  // The rules of SampleEncodeBatch.
  if (nbest_size > 512) return Err(SPM_INTERNAL, "nbest_size must be nbest_size <= 512");
  if (nbest_size == 0 || nbest_size == 1) return RunDense(inputs, nullptr, options, out, host_ids);
  const bool bpe = proto_.trainer_spec.model_type == kBpe;
  if (nbest_size > 1 && !bpe)
    return Err(SPM_UNIMPLEMENTED,
               "SampleEncode among the n best (nbest_size > 1) is not implemented on the device; "
               "use nbest_size=-1 to sample from the whole lattice");
  if (!sample_seeded_) {
    std::random_device rd;
    sample_seed_ = (static_cast<uint64_t>(rd()) << 32) | rd();
    sample_seeded_ = true;
  }
  const SampleSpec spec{alpha, sample_seed_, sample_count_};
  Status st = RunDense(inputs, &spec, options, out, host_ids);
  if (st.ok()) sample_count_ += inputs.size();
  return st;
}

// SetVocabulary / ResetVocabulary / LoadVocabulary (sentencepiece_processor.cc:
// 203-274).  The rule runs in the C-ABI over the handle's pieces, which are
// this proto's; the resulting types come back into proto_, so IsUnused and
// Encode agree.
Status SentencePieceProcessor::SyncTypes() {
  std::vector<uint8_t> types(proto_.pieces.size());
  const Status st = FromC(spm_hip_model_get_piece_types(model_, types.data(), types.size()));
  if (!st.ok()) return st;
  for (size_t i = 0; i < types.size(); ++i) proto_.pieces[i].type = types[i];
  return Status::Ok();
}

Status SentencePieceProcessor::SetVocabulary(const std::vector<std::string> &valid_vocab) {
  if (!status_.ok()) return status_;
  std::vector<uint64_t> off(valid_vocab.size() + 1, 0);
  std::string bytes;
  for (size_t i = 0; i < valid_vocab.size(); ++i) {
    bytes += valid_vocab[i];
    off[i + 1] = bytes.size();
  }
  const Status st = FromC(spm_hip_model_set_vocabulary(model_, reinterpret_cast<const uint8_t *>(bytes.data()),
                                                       off.data(), valid_vocab.size()));
  return st.ok() ? SyncTypes() : st;
}

Status SentencePieceProcessor::ResetVocabulary() {
  if (!status_.ok()) return status_;
  const Status st = FromC(spm_hip_model_reset_vocabulary(model_));
  return st.ok() ? SyncTypes() : st;
}

Status SentencePieceProcessor::LoadVocabulary(const std::string &filename, int threshold) {
  std::ifstream in(filename, std::ios::binary);
  if (!in) return Err(SPM_NOT_FOUND, "\"" + filename + "\": No such file or directory");
  std::vector<std::string> vocab;
  std::string line;
  while (std::getline(in, line)) {
    // string_util::Split(line, "\t") (util.cc:32-49): empty fields are
    // dropped, so an empty line (or one of tabs only) has no field at all.
    std::vector<std::string> v;
    for (size_t at = 0; at <= line.size();) {
      const size_t e = std::min(line.find('\t', at), line.size());
      if (e > at) v.push_back(line.substr(at, e - at));
      at = e + 1;
    }
    if (v.empty()) return Err(SPM_INTERNAL, "[(v.size()) >= (1)] ");
    if (v[0].empty()) return Err(SPM_INTERNAL, "[!v[0].empty()] ");
    int freq = 1;
    if (v.size() >= 2) freq = std::atoi(v[1].c_str());
    if (freq >= threshold) vocab.push_back(v[0]);
  }
  return SetVocabulary(vocab);
}

// Piece frequencies of a batch: normalize, encode, the id epilogue and the
// count (spm_hip_count_ids) run on the device; only the counters come back.
Status SentencePieceProcessor::CountPieces(const std::vector<std::string> &inputs,
                                           std::vector<uint64_t> *counts) const {
  if (!status_.ok()) return status_;
  if (!counts) return Err(SPM_INTERNAL, "output container is null");
  const uint64_t n = inputs.size(), v = proto_.pieces.size();
  counts->resize(v, 0);
  if (n == 0) return Status::Ok();
  std::vector<uint64_t> add(v, 0);
  const bool word_char = proto_.trainer_spec.model_type == kWord || proto_.trainer_spec.model_type == kChar;
  if (word_char) {
    // These models' ids take the host epilogue (RunBatch); their ids go back up.
    std::vector<std::vector<int>> ids;
    Status st = RunBatch(inputs, &ids, nullptr, nullptr);
    if (!st.ok()) return st;
    std::vector<int32_t> flat;
    for (const auto &row : ids) flat.insert(flat.end(), row.begin(), row.end());
    st = FromC(spm_hip_count_ids_host(model_, flat.data(), flat.size(), add.data(), nullptr));
    if (!st.ok()) return st;
  } else {
    DeviceBatch b;
    Status st = DeviceEncode(inputs, nullptr, &b);
    if (!st.ok()) return st;
    int32_t *d_out = nullptr;
    uint64_t *d_out_off = nullptr;
    uint64_t fin = 0;
    st = DeviceFinalize(b, n, &d_out, &d_out_off, &fin);
    if (!st.ok()) return st;
    uint64_t *d_counts = static_cast<uint64_t *>(dev_.Get(kCounts, v * 8));
    if (!d_counts) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
    hipError_t he;
    if ((he = hipMemset(d_counts, 0, v * 8)) != hipSuccess) return Err(SPM_INTERNAL, hipGetErrorString(he));
    st = FromC(spm_hip_count_ids(model_, d_out, fin, d_counts, nullptr, nullptr));
    if (!st.ok()) return st;
    if ((he = hipMemcpy(add.data(), d_counts, v * 8, hipMemcpyDeviceToHost)) != hipSuccess)
      return Err(SPM_INTERNAL, hipGetErrorString(he));
  }
  for (uint64_t i = 0; i < v; ++i) (*counts)[i] += add[i];
  return Status::Ok();
}

// PopulateSentencePieceText (sentencepiece_processor.cc:488-551) +
// ApplyExtraOptions (:945-979) over one path's model-level tokens: (piece,
// id) pairs with unknown runs merged (byte fallback: expanded to BYTE pieces,
// which needs the text).  normalized == nullptr: ids only.
Status SentencePieceProcessor::PopulateText(const char *normalized, uint64_t nlen, const int32_t *tok_ids,
                                            const uint32_t *tok_len, uint64_t count,
                                            std::vector<std::pair<std::string, int>> *out) const {
  std::vector<std::pair<std::string, int>> &spt = *out;
  spt.clear();
  uint64_t consumed = 0;
  bool prev_unk = false;
  for (uint64_t k = 0; k < count; ++k) {
    const int id = tok_ids[k];
    const uint32_t len = tok_len[k];
    if (len == 0) return Err(SPM_INTERNAL, "Empty piece is not allowed.");
    std::string w = normalized ? std::string(normalized + consumed, len) : std::string();
    const bool is_unk = IsUnknown(id);
    if (IsControl(id)) {
      spt.emplace_back(std::move(w), id);
    } else if (is_unk && proto_.trainer_spec.byte_fallback) {
      // One BYTE piece per byte of the token, no merge with its neighbours.
      for (const char c : w) {
        const int bid = byte_ids_[static_cast<uint8_t>(c)];
        spt.emplace_back(IdToPiece(bid), bid);
      }
      consumed += len;
    } else {
      if (prev_unk && is_unk) spt.back().first += w;
      else spt.emplace_back(std::move(w), id);
      consumed += len;
    }
    prev_unk = is_unk;
  }
  if (consumed != nlen) return Err(SPM_INTERNAL, "all normalized characters are not consumed.");
  const std::string &bos = proto_.trainer_spec.bos_piece, &eos = proto_.trainer_spec.eos_piece;
  for (ExtraOption opt : extra_) {
    if (opt == REVERSE) std::reverse(spt.begin(), spt.end());
    else if (opt == EOS) spt.emplace_back(eos, PieceToId(eos));
    else spt.insert(spt.begin(), {bos, PieceToId(bos)});
  }
  return Status::Ok();
}

// NBestEncode (sentencepiece_processor.cc:588-609), batched: the device
// normalizer, spm_hip_nbest_encode_batch over the chunk, then
// PopulateSentencePieceText on every path.  Ids alone finish on the device
// (spm_hip_finalize_ids with every path passed as a "sentence"); pieces and
// scores are put together on the host.
Status SentencePieceProcessor::NBestEncodeBatch(const std::vector<std::string> &inputs, int nbest_size,
                                                std::vector<std::vector<std::vector<int>>> *ids,
                                                std::vector<std::vector<std::vector<std::string>>> *pieces,
                                                std::vector<std::vector<float>> *scores) const {
  if (!status_.ok()) return status_;
  // The reference's non-unigram models return no path at all (:598-599).
  if (proto_.trainer_spec.model_type != kUnigram) return Err(SPM_INTERNAL, "NBestEncode returns empty result.");
  const uint64_t n_all = inputs.size();
  const uint64_t N = static_cast<uint64_t>(std::max(1, std::min(nbest_size, 1024)));
  if (ids) ids->assign(n_all, {});
  if (pieces) pieces->assign(n_all, {});
  if (scores) scores->assign(n_all, {});
  // Chunks of at most 2^20 paths and 2^26 path bytes, so staging stays bounded.
  const uint64_t max_lines = std::max<uint64_t>(1, (1ull << 20) / N);
  const uint64_t max_bytes = std::max<uint64_t>(1, (1ull << 26) / N);
  enum { kIn, kInOff, kNorm, kNormOff, kIds, kLen, kTok, kOut, kOutOff, kSmallBlock };
  // (kSmallBlock doubles as the path-level arrays: EncodeIdsSmall is not running.)
  auto fail_hip = [](hipError_t e) { return Err(SPM_INTERNAL, hipGetErrorString(e)); };
  hipError_t he;
  std::vector<std::pair<std::string, int>> spt;
  for (uint64_t c0 = 0; c0 < n_all;) {
    uint64_t c1 = c0, raw = 0;
    while (c1 < n_all && c1 - c0 < max_lines && (c1 == c0 || raw + inputs[c1].size() <= max_bytes))
      raw += inputs[c1++].size();
    const uint64_t n = c1 - c0;
    std::vector<uint64_t> in_off(n + 1, 0);
    std::string in_bytes;
    in_bytes.reserve(raw);
    for (uint64_t i = 0; i < n; ++i) {
      in_bytes += inputs[c0 + i];
      in_off[i + 1] = in_bytes.size();
    }
    uint8_t *d_in = static_cast<uint8_t *>(dev_.Get(kIn, std::max<uint64_t>(raw, 1)));
    uint64_t *d_in_off = static_cast<uint64_t *>(dev_.Get(kInOff, (n + 1) * 8));
    uint64_t *d_norm_off = static_cast<uint64_t *>(dev_.Get(kNormOff, (n + 1) * 8));
    uint64_t *d_path_off = static_cast<uint64_t *>(dev_.Get(kOutOff, (n + 1) * 8));
    if (!d_in || !d_in_off || !d_norm_off || !d_path_off)
      return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
    if ((raw && (he = hipMemcpy(d_in, in_bytes.data(), raw, hipMemcpyHostToDevice)) != hipSuccess) ||
        (he = hipMemcpy(d_in_off, in_off.data(), (n + 1) * 8, hipMemcpyHostToDevice)) != hipSuccess)
      return fail_hip(he);
    uint64_t total = 0;
    uint8_t *d_norm = static_cast<uint8_t *>(dev_.Get(kNorm, std::max<uint64_t>(dev_.cap[kNorm], 1)));
    int rc = spm_hip_normalize_batch_device(model_, d_in, d_in_off, n, d_norm, dev_.cap[kNorm], d_norm_off, &total,
                                            nullptr);
    if (rc == SPM_RESOURCE_EXHAUSTED) {
      d_norm = static_cast<uint8_t *>(dev_.Get(kNorm, total));
      if (!d_norm) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
      rc = spm_hip_normalize_batch_device(model_, d_in, d_in_off, n, d_norm, dev_.cap[kNorm], d_norm_off, &total,
                                          nullptr);
    }
    Status st = FromC(rc);
    if (!st.ok()) return st;
    // First try: capacities for 16 tokens per path, then the returned totals.
    uint64_t P = n * N, T = std::min<uint64_t>(std::max<uint64_t>(total, 1) * N, n * N * 16 + 1024);
    int32_t *d_ids = nullptr;
    uint32_t *d_len = nullptr;
    uint64_t *d_tok = nullptr;
    float *d_scores = nullptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
      d_ids = static_cast<int32_t *>(dev_.Get(kIds, std::max<uint64_t>(T, 1) * 4));
      d_len = static_cast<uint32_t *>(dev_.Get(kLen, std::max<uint64_t>(T, 1) * 4));
      d_tok = static_cast<uint64_t *>(dev_.Get(kTok, (P + 1) * 8));
      d_scores = static_cast<float *>(dev_.Get(kSmallBlock, std::max<uint64_t>(P, 1) * 4));
      if (!d_ids || !d_len || !d_tok || !d_scores) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
      const uint64_t pcap = P, tcap = T;
      rc = spm_hip_nbest_encode_batch(model_, d_norm, d_norm_off, n, static_cast<int32_t>(N), d_ids, d_len, tcap, d_tok,
                                      d_scores, pcap, d_path_off, &P, &T, nullptr);
      if (rc != SPM_RESOURCE_EXHAUSTED) break;
    }
    st = FromC(rc);
    if (!st.ok()) return st;
    std::vector<uint64_t> path_off(n + 1);
    if ((he = hipMemcpy(path_off.data(), d_path_off, (n + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess)
      return fail_hip(he);
    if (scores) {
      std::vector<float> sc(std::max<uint64_t>(P, 1));
      if (P && (he = hipMemcpy(sc.data(), d_scores, P * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(he);
      for (uint64_t i = 0; i < n; ++i) (*scores)[c0 + i].assign(sc.begin() + path_off[i], sc.begin() + path_off[i + 1]);
    }
    // (Byte fallback expands a path's unknown tokens from the line's text: its
    // ids come from the host epilogue below, like the pieces.)
    if (!pieces && !(ids && proto_.trainer_spec.byte_fallback)) {
      if (ids) {
        uint64_t n_extra = 0;
        for (ExtraOption opt : extra_) n_extra += opt != REVERSE;
        const uint64_t cap = T + P * n_extra;
        uint64_t *d_out_off = static_cast<uint64_t *>(dev_.Get(kInOff, (P + 1) * 8));
        int32_t *d_out = static_cast<int32_t *>(dev_.Get(kOut, std::max<uint64_t>(cap, 1) * 4));
        if (!d_out_off || !d_out) return Err(SPM_RESOURCE_EXHAUSTED, "device allocation failed");
        uint64_t fin = 0;
        st = FromC(spm_hip_finalize_ids(model_, extra_str_.c_str(), d_ids, d_tok, P, d_out, cap, d_out_off, &fin,
                                        nullptr));
        if (!st.ok()) return st;
        std::vector<uint64_t> out_off(P + 1);
        std::vector<int32_t> out(std::max<uint64_t>(fin, 1));
        if ((he = hipMemcpy(out_off.data(), d_out_off, (P + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
            (fin && (he = hipMemcpy(out.data(), d_out, fin * 4, hipMemcpyDeviceToHost)) != hipSuccess))
          return fail_hip(he);
        for (uint64_t i = 0; i < n; ++i)
          for (uint64_t p = path_off[i]; p < path_off[i + 1]; ++p)
            (*ids)[c0 + i].emplace_back(out.begin() + out_off[p], out.begin() + out_off[p + 1]);
      }
      c0 = c1;
      continue;
    }
    std::vector<uint64_t> norm_off(n + 1), tok_off(P + 1);
    std::vector<int32_t> tok_ids(std::max<uint64_t>(T, 1));
    std::vector<uint32_t> tok_len(std::max<uint64_t>(T, 1));
    std::vector<uint8_t> norm(std::max<uint64_t>(total, 1));
    if ((he = hipMemcpy(norm_off.data(), d_norm_off, (n + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
        (he = hipMemcpy(tok_off.data(), d_tok, (P + 1) * 8, hipMemcpyDeviceToHost)) != hipSuccess ||
        (T && (he = hipMemcpy(tok_ids.data(), d_ids, T * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
        (T && (he = hipMemcpy(tok_len.data(), d_len, T * 4, hipMemcpyDeviceToHost)) != hipSuccess) ||
        (total && (he = hipMemcpy(norm.data(), d_norm, total, hipMemcpyDeviceToHost)) != hipSuccess))
      return fail_hip(he);
    for (uint64_t i = 0; i < n; ++i)
      for (uint64_t p = path_off[i]; p < path_off[i + 1]; ++p) {
        const char *normalized = reinterpret_cast<const char *>(norm.data()) + norm_off[i];
        Status ps = PopulateText(normalized, norm_off[i + 1] - norm_off[i], tok_ids.data() + tok_off[p],
                                 tok_len.data() + tok_off[p], tok_off[p + 1] - tok_off[p], &spt);
        if (!ps.ok()) return ps;
        if (ids) {
          (*ids)[c0 + i].emplace_back();
          for (auto &q : spt) (*ids)[c0 + i].back().push_back(q.second);
        }
        if (!pieces) continue;
        (*pieces)[c0 + i].emplace_back();
        for (auto &q : spt) (*pieces)[c0 + i].back().push_back(std::move(q.first));
      }
    c0 = c1;
  }
  return Status::Ok();
}

Status SentencePieceProcessor::NBestEncode(const std::string &input, int nbest_size,
                                           std::vector<std::vector<int>> *ids) const {
  if (!ids) return Err(SPM_INTERNAL, "output container is null");
  std::vector<std::vector<std::vector<int>>> out;
  Status st = NBestEncodeBatch({input}, nbest_size, &out, nullptr, nullptr);
  if (st.ok()) *ids = std::move(out[0]);
  return st;
}

Status SentencePieceProcessor::NBestEncode(const std::string &input, int nbest_size,
                                           std::vector<std::vector<std::string>> *pieces) const {
  if (!pieces) return Err(SPM_INTERNAL, "output container is null");
  std::vector<std::vector<std::vector<std::string>>> out;
  Status st = NBestEncodeBatch({input}, nbest_size, nullptr, &out, nullptr);
  if (st.ok()) *pieces = std::move(out[0]);
  return st;
}

Status SentencePieceProcessor::Encode(const std::string &input, std::vector<int> *ids) const {
  if (!ids) return Err(SPM_INTERNAL, "output container is null");
  std::vector<std::vector<int>> out;
  Status st = EncodeBatch({input}, &out, nullptr);
  if (st.ok()) *ids = std::move(out[0]);
  return st;
}

Status SentencePieceProcessor::Encode(const std::string &input,
                                      std::vector<std::string> *pieces) const {
  if (!pieces) return Err(SPM_INTERNAL, "output container is null");
  std::vector<std::vector<std::string>> out;
  Status st = EncodeBatch({input}, nullptr, &out);
  if (st.ok()) *pieces = std::move(out[0]);
  return st;
}

// ---------------------------------------------------------------------------
// Decode (sentencepiece_processor.cc:341-370, :670-733).

namespace {

const char kSpaceSymbol[] = "\xE2\x96\x81";  // U+2581

SentencePieceProcessor::DecodePath DecodePathFromEnv() {
  static const SentencePieceProcessor::DecodePath kPath = [] {
    const char *e = std::getenv("SPM_HIP_DECODE_PATH");
    const std::string v = e ? e : "";
    if (v == "host") return SentencePieceProcessor::kDecodeHost;
    if (v == "device") return SentencePieceProcessor::kDecodeDevice;
    return SentencePieceProcessor::kDecodeAuto;
  }();
  return kPath;
}

}  // namespace

// ApplyExtraOptions (:945-979) over (piece, id) rows, then the surface loop of
// Decode (:678-713).
void SentencePieceProcessor::DecodeLineHost(std::vector<std::pair<std::string, int>> *row, std::string *text,
                                            std::vector<DecodedPiece> *spt) const {
  const auto &ts = proto_.trainer_spec;
  for (const ExtraOption o : decode_extra_) {
    if (o == REVERSE) std::reverse(row->begin(), row->end());
    else if (o == EOS) row->emplace_back(ts.eos_piece, PieceToId(ts.eos_piece));
    else row->insert(row->begin(), std::make_pair(ts.bos_piece, PieceToId(ts.bos_piece)));
  }
  if (!text) return;  // options only
  text->clear();
  std::string surface;
  for (size_t at = 0; at < row->size(); ++at) {
    const auto &pi = (*row)[at];
    const std::string &piece = pi.first;
    const int id = pi.second;
    surface.clear();
    if (IsControl(id)) {
    } else if (IsByte(id)) {
      // The byte run around the token, at most 3 tokens each way (decode.h).
      uint8_t w[7] = {}, lit[4];
      w[3] = static_cast<uint8_t>(PieceToByte(IdToPiece(id)));
      uint32_t lo = 0, hi = 0;
      while (lo < 3 && at > lo && IsByte((*row)[at - lo - 1].second)) {
        ++lo;
        w[3 - lo] = static_cast<uint8_t>(PieceToByte(IdToPiece((*row)[at - lo].second)));
      }
      while (hi < 3 && at + hi + 1 < row->size() && IsByte((*row)[at + hi + 1].second)) {
        ++hi;
        w[3 + hi] = static_cast<uint8_t>(PieceToByte(IdToPiece((*row)[at + hi].second)));
      }
      surface.assign(reinterpret_cast<const char *>(lit), ByteRunSurface(w, lo, hi, lit));
    } else if (IsUnknown(id)) {
      surface = IdToPiece(id) == piece ? ts.unk_surface : piece;
    } else {
      size_t k = text->empty() && piece.compare(0, 3, kSpaceSymbol) == 0 ? 3 : 0;
      while (k < piece.size()) {
        if (piece.compare(k, 3, kSpaceSymbol) == 0) {
          surface.push_back(' ');
          k += 3;
        } else {
          surface.push_back(piece[k++]);
        }
      }
    }
    if (spt) {
      DecodedPiece d;
      d.piece = piece;
      d.id = id;
      d.surface = surface;
      d.begin = static_cast<uint32_t>(text->size());
      d.end = static_cast<uint32_t>(text->size() + surface.size());
      spt->push_back(std::move(d));
    }
    *text += surface;
  }
}

Status SentencePieceProcessor::DecodeRows(std::vector<std::vector<std::pair<std::string, int>>> *rows,
                                          const std::vector<char> &oov, std::vector<std::string> *texts,
                                          std::vector<std::vector<DecodedPiece>> *spt) const {
  const size_t n = rows->size();
  const int v = GetPieceSize();
  uint64_t tokens = 0;
  for (size_t i = 0; i < n; ++i) {
    for (const auto &pi : (*rows)[i])
      if (pi.second < 0 || pi.second >= v)
        return Err(SPM_OUT_OF_RANGE, "decode: sentence " + std::to_string(i) + " holds id " +
                                         std::to_string(pi.second) + ", outside [0, " + std::to_string(v) + ")");
    tokens += (*rows)[i].size();
  }
  texts->assign(n, std::string());
  if (spt) spt->assign(n, std::vector<DecodedPiece>());
  DecodePath path = decode_path_ != kDecodeAuto ? decode_path_ : DecodePathFromEnv();
  if (path == kDecodeAuto) path = tokens >= kDecodeDeviceMinTokens ? kDecodeDevice : kDecodeHost;
  std::vector<char> done(n, 0);
  if (path == kDecodeDevice) {
    // Every line whose pieces are all in the vocabulary goes up as one id CSR.
    std::vector<size_t> lines;
    std::vector<int32_t> ids;
    std::vector<uint64_t> off(1, 0);
    Status st = Status::Ok();
    uint64_t extras = 0;
    for (const ExtraOption o : decode_extra_) extras += o != REVERSE;
    for (size_t i = 0; i < n; ++i) {
      if (oov[i]) continue;
      lines.push_back(i);
      for (const auto &pi : (*rows)[i]) ids.push_back(pi.second);
      off.push_back(ids.size());
    }
    const uint64_t nd = lines.size();
    if (nd) {
      std::vector<uint64_t> out_off(nd + 1);
      uint64_t total = 0;
      // Size the text by the model's bound when that stays small, else by a
      // count call: a batch that large amortizes it, and tokens * bound would
      // be many times the text.
      uint32_t bound = 0;
      st = FromC(spm_hip_model_decode_bound(model_, &bound));
      if (!st.ok()) return st;
      total = (ids.size() + nd * extras) * static_cast<uint64_t>(bound);
      if (total > (16u << 20)) {
        st = FromC(spm_hip_decode_batch_host(model_, decode_extra_str_.c_str(), ids.data(), off.data(), nd, nullptr,
                                             0, out_off.data(), nullptr, &total));
        if (!st.ok()) return st;
      }
      std::string out(total, '\0');
      std::vector<uint32_t> begins(spt ? ids.size() + nd * extras : 0);
      st = FromC(spm_hip_decode_batch_host(model_, decode_extra_str_.c_str(), ids.data(), off.data(), nd,
                                           reinterpret_cast<uint8_t *>(&out[0]), out.size(), out_off.data(),
                                           spt ? begins.data() : nullptr, &total));
      if (!st.ok()) return st;
      uint64_t g = 0;
      for (uint64_t k = 0; k < nd; ++k) {
        const size_t i = lines[k];
        std::string &text = (*texts)[i];
        text.assign(out, out_off[k], out_off[k + 1] - out_off[k]);
        done[i] = 1;
        if (!spt) continue;
        auto &row = (*rows)[i];
        DecodeLineHost(&row, nullptr, nullptr);  // the piece list in final order
        auto &dst = (*spt)[i];
        dst.resize(row.size());
        for (size_t t = 0; t < row.size(); ++t, ++g) {
          DecodedPiece &d = dst[t];
          d.piece = row[t].first;
          d.id = row[t].second;
          d.begin = begins[g];
          d.end = t + 1 < row.size() ? begins[g + 1] : static_cast<uint32_t>(text.size());
          d.surface.assign(text, d.begin, d.end - d.begin);
        }
      }
    }
  }
  for (size_t i = 0; i < n; ++i)
    if (!done[i]) DecodeLineHost(&(*rows)[i], &(*texts)[i], spt ? &(*spt)[i] : nullptr);
  return Status::Ok();
}

Status SentencePieceProcessor::DecodeBatch(const std::vector<std::vector<int>> &ids, std::vector<std::string> *texts,
                                           std::vector<std::vector<DecodedPiece>> *spt) const {
  if (!status_.ok()) return status_;
  if (!texts) return Err(SPM_INTERNAL, "output container is null");
  texts->clear();
  std::vector<std::vector<std::pair<std::string, int>>> rows(ids.size());
  for (size_t i = 0; i < ids.size(); ++i) {
    rows[i].reserve(ids[i].size());
    for (const int id : ids[i]) {
      const bool in_range = id >= 0 && id < GetPieceSize();  // DecodeRows rejects the others
      rows[i].emplace_back(IdToPiece(id), in_range ? PieceToId(IdToPiece(id)) : id);
    }
  }
  return DecodeRows(&rows, std::vector<char>(ids.size(), 0), texts, spt);
}

Status SentencePieceProcessor::DecodeBatch(const std::vector<std::vector<std::string>> &pieces,
                                           std::vector<std::string> *texts,
                                           std::vector<std::vector<DecodedPiece>> *spt) const {
  if (!status_.ok()) return status_;
  if (!texts) return Err(SPM_INTERNAL, "output container is null");
  texts->clear();
  std::vector<std::vector<std::pair<std::string, int>>> rows(pieces.size());
  std::vector<char> oov(pieces.size(), 0);
  for (size_t i = 0; i < pieces.size(); ++i) {
    rows[i].reserve(pieces[i].size());
    for (const std::string &w : pieces[i]) {
      const int id = PieceToId(w);
      if (IsUnknown(id) && IdToPiece(id) != w) oov[i] = 1;
      rows[i].emplace_back(w, id);
    }
  }
  return DecodeRows(&rows, oov, texts, spt);
}

Status SentencePieceProcessor::Decode(const std::vector<int> &ids, std::string *detokenized) const {
  if (!status_.ok()) return status_;
  if (!detokenized) return Err(SPM_INTERNAL, "output container is null");
  detokenized->clear();
  std::vector<std::string> out;
  Status st = DecodeBatch(std::vector<std::vector<int>>{ids}, &out);
  if (st.ok()) *detokenized = std::move(out[0]);
  return st;
}

Status SentencePieceProcessor::Decode(const std::vector<std::string> &pieces, std::string *detokenized) const {
  if (!status_.ok()) return status_;
  if (!detokenized) return Err(SPM_INTERNAL, "output container is null");
  detokenized->clear();
  std::vector<std::string> out;
  Status st = DecodeBatch(std::vector<std::vector<std::string>>{pieces}, &out);
  if (st.ok()) *detokenized = std::move(out[0]);
  return st;
}

}  // namespace spm_amd
