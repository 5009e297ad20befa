// oatk_amd/csrc/count_onepass_core.hpp -- the part of the count's one-pass check (count.hpp: gather_verify_kernel) that touches no device memory
// model: which records of a strip are compared and which k-mers a strip loads for it, and where a difference is reported.  Plain functions, shared
// with the stand-alone check tests/c/count_onepass_check.cpp.
//
// Sorted records that are not the head of their equal-hash group ("live") are compared with their PREDECESSOR in sorted order, not with the head:
// equality is transitive, so "every live record equals the one in front of it" says the same as "every live record equals its head", and the
// predecessor's locator and s-mer sit in the neighbouring lane of the pass that gathered them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OATK_OP_FN __host__ __device__ __forceinline__
#else
#define OATK_OP_FN static inline
#endif

namespace oatk {

// A strip is `strip` consecutive sorted records starting at s0; bit r of `live` says that record s0 + r is in range and no head.  The strip's
// k-mers are numbered 0 .. strip: k-mer j belongs to record s0 + j - 1 (k-mer 0 is the record in front of the strip).  Record r is compared
// with record r - 1, that is k-mer r + 1 with k-mer r, so the k-mers a strip loads are those of its live records and of their predecessors.
OATK_OP_FN uint32_t onepass_need_mask(uint32_t live) { return live | live << 1; }

// bit r of the result: live record r differs from its predecessor in this 32-base word (w[j]: the word of k-mer j; words of k-mers that
// were not loaded may hold anything)
template <int STRIP>
OATK_OP_FN uint32_t onepass_diff_mask(const uint64_t (&w)[STRIP + 1], uint32_t live)
{
    uint32_t d = 0;
#pragma unroll
    for (int r = 0; r < STRIP; ++r) d |= (uint32_t) (w[r + 1] != w[r]) << r;
    return d & live;
}

// does the tile that starts at sorted record t0 need the record in front of it?  (only when its first record is compared with it)
OATK_OP_FN bool onepass_tile_needs_pred(const uint32_t *newclus, uint32_t n_rec, uint32_t t0) { return t0 > 0 && t0 < n_rec && !newclus[t0]; }

// the head of the group of sorted record i: back from i while the records are no heads (record 0 is always one)
OATK_OP_FN uint32_t onepass_head_of(const uint32_t *newclus, uint32_t i)
{
    while (i > 0 && !newclus[i]) --i;
    return i;
}

}  // namespace oatk
