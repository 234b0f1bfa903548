// Agenda of the n-best A* search (host and device): a binary heap of
// (fx, hypothesis index) keys moved exactly as libstdc++'s push_heap /
// pop_heap move the elements of the reference's std::priority_queue
// <Hypothesis *> ordered by fx < (unigram_model.cc:391-401), so hypotheses of
// equal fx pop in the reference's order.  The key travels with the index: a
// sift compares values it has already loaded.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SPM_NBEST_FN __host__ __device__ inline
#else
#define SPM_NBEST_FN inline
#endif

namespace spm_amd {

constexpr int kNBestMax = 1024;              // nbest_size clamp (unigram_model.cc:735)
constexpr uint32_t kNBestMaxAgenda = 100000; // kMaxAgendaSize (:462)
constexpr uint32_t kNBestMinAgenda = 512;    // kMinAgendaSize (:463)

SPM_NBEST_FN int NBestClamp(int nbest_size) {
  return nbest_size < 1 ? 1 : nbest_size > kNBestMax ? kNBestMax : nbest_size;
}

struct NBestKey {
  float fx;
  int32_t hyp;
};

// std::__push_heap with top index 0: v rises from `hole`.
SPM_NBEST_FN void NBestSiftUp(NBestKey *heap, uint32_t hole, NBestKey v) {
  while (hole > 0) {
    const uint32_t parent = (hole - 1) / 2;
    const NBestKey pk = heap[parent];
    if (!(pk.fx < v.fx)) break;
    heap[hole] = pk;
    hole = parent;
  }
  heap[hole] = v;
}

// push_back + push_heap.
SPM_NBEST_FN void NBestPush(NBestKey *heap, uint32_t *size, NBestKey v) { NBestSiftUp(heap, (*size)++, v); }

// top + pop_heap (std::__adjust_heap over the first size - 1 keys with the
// last key as the value) + pop_back.  *size >= 1.
SPM_NBEST_FN NBestKey NBestPop(NBestKey *heap, uint32_t *size) {
  const NBestKey top = heap[0];
  const uint32_t len = --*size;
  if (len > 0) {
    const NBestKey v = heap[len];
    uint32_t hole = 0, child = 0;
    while (child < (len - 1) / 2) {
      child = 2 * (child + 1);
      NBestKey ck = heap[child];
      const NBestKey lk = heap[child - 1];
      if (ck.fx < lk.fx) {
        --child;
        ck = lk;
      }
      heap[hole] = ck;
      hole = child;
    }
    if ((len & 1u) == 0 && child == (len - 2) / 2) {
      child = 2 * (child + 1);
      heap[hole] = heap[child - 1];
      hole = child - 1;
    }
    NBestSiftUp(heap, hole, v);
  }
  return top;
}

}  // namespace spm_amd
