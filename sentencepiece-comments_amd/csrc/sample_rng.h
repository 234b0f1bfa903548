// Random stream of the unigram sampler (host and device): stateless and
// counter based, so a draw depends only on (seed, global sentence index, draw
// number), never on the batch shape, the launch geometry or the tier that ran
// the sentence.  Spelled out in include/spm_hip.h (spm_hip_sample_uniform).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SPM_RNG_FN __host__ __device__ inline
#else
#define SPM_RNG_FN inline
#endif

namespace spm_amd {

constexpr uint64_t kSampleGolden = 0x9E3779B97F4A7C15ull;

// splitmix64's finalizer.
SPM_RNG_FN uint64_t SampleMix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Key of the sentence with global index g.
SPM_RNG_FN uint64_t SampleKey(uint64_t seed, uint64_t g) { return SampleMix(seed + kSampleGolden * (g + 1)); }

// Seed of sample j of a sample-and-score call: sample 0 keeps the caller's
// seed (so it is SampleEncode's draw), sample j > 0 takes a seed of its own;
// its key is SampleKey(SampleSeedAt(seed, j), g).
constexpr uint64_t kSampleStride = 0xD1B54A32D192ED03ull;
SPM_RNG_FN uint64_t SampleSeedAt(uint64_t seed, uint64_t j) {
  return j == 0 ? seed : SampleMix(seed + kSampleStride * j);
}

// Draw k of a sentence: a multiple of 2^-53 in [0, 1).
SPM_RNG_FN double SampleDraw(uint64_t key, uint64_t k) {
  return static_cast<double>(SampleMix(key + kSampleGolden * (k + 1)) >> 11) * 0x1.0p-53;
}

}  // namespace spm_amd
