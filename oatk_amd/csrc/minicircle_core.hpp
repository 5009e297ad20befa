// oatk_amd/csrc/minicircle_core.hpp -- what decides whether an alignment record walks round the anchor unitig periodically, which repeat unit it gives
// and how that unit reads as a canonical path: minicircle_analysis_thread (path_finder.c:545-607) and the path collection of
// extract_minicircles_with_anchor (:657-671, order :620-638).  Decided here and nowhere else: the device kernels (minicircle.hpp) and the CPU check
// (tests/c/minicircle_core_check.cpp, under ASan + UBSan) run these functions.  Like cons_str_core.hpp it compiles for host and device alike.
//
// The rule, in the reference's words: a HIT is a fragment whose uid >> 1 is the anchor.  A record of fewer than two fragments or fewer than two hits gives
// nothing, and so does one with two hits of different orientation -- any two, wherever they are.  beg = the first hit, end = the second hit - 1, rev = the hits'
// orientation.  Unless the unit is the record's head and reaches its last fragment but one (beg == 0 && end >= n - 2), the WHOLE record must repeat it:
// with r = end - beg, beg <= r and uid[j] == uid[beg + ((j + r + 1 - beg) mod (r + 1))] for every j, on the full 64-bit uid.  None of this depends on the
// order the fragments are looked at, which is what lets a wave take them 64 at a time (Hits, hits_add_chunk).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OATK_MC_HD __host__ __device__ __forceinline__
#else
#define OATK_MC_HD inline
#endif

namespace oatk_mc {

constexpr uint64_t NONE = ~0ULL;                                           // UINT64_MAX: the record gives no unit
enum { SHORT = 32, CHUNK = 64 };                                           // SHORT: the longest record / path a single lane walks (minicircle.hpp)

OATK_MC_HD bool hit(uint64_t uid, uint64_t anchor) { return (uid >> 1) == anchor; }
OATK_MC_HD uint64_t pack(uint32_t beg, uint32_t end, uint32_t rev) { return (uint64_t) beg << 33 | (uint64_t) end << 1 | rev; }       // :606; beg < 2^31
OATK_MC_HD uint32_t unit_beg(uint64_t u) { return (uint32_t) (u >> 33); }
OATK_MC_HD uint32_t unit_end(uint64_t u) { return (uint32_t) (u >> 1); }
OATK_MC_HD uint32_t unit_rev(uint64_t u) { return (uint32_t) (u & 1); }
OATK_MC_HD uint32_t unit_nv(uint64_t u) { return unit_end(u) - unit_beg(u) + 1; }

// what a pass over a record's fragments collects about its hits (:564-579)
struct Hits {
    uint32_t n_hit, first, second;                                         // second: valid from two hits on
    bool fwd, rev;                                                         // a hit of either orientation was seen
};
OATK_MC_HD void hits_init(Hits &h) { h.n_hit = 0, h.first = 0, h.second = 0, h.fwd = false, h.rev = false; }
// fragment j, in ascending order of j
OATK_MC_HD void hits_add(Hits &h, uint32_t j, uint64_t uid, uint64_t anchor)
{
    const bool is = hit(uid, anchor);                                      // (selects, not branches: as two guarded stores hipcc made an indexed store to scratch of them)
    h.first = is && h.n_hit == 0? j : h.first;
    h.second = is && h.n_hit == 1? j : h.second;
    h.n_hit += is;
    h.rev |= is && (uid & 1), h.fwd |= is && !(uid & 1);
}
// fragments base .. base + 63 at once, in ascending order of base: bit l of hit_mask = fragment base + l is a hit, of rev_mask = it is one with uid & 1
OATK_MC_HD void hits_add_chunk(Hits &h, uint32_t base, uint64_t hit_mask, uint64_t rev_mask)
{
    if (!hit_mask) return;
    uint64_t m = hit_mask;
    if (h.n_hit == 0) { h.first = base + (uint32_t) __builtin_ctzll(m); m &= m - 1; }
    if (h.n_hit <= 1 && m) h.second = base + (uint32_t) __builtin_ctzll(m);
    h.n_hit += (uint32_t) __builtin_popcountll(hit_mask);
    if (rev_mask) h.rev = true;
    if (hit_mask & ~rev_mask) h.fwd = true;
}
// The verdict on a record of n fragments from its hits (:557-592): NONE, or the unit.  *period: the unit stands only if period_ok holds for every j in [0, n)
OATK_MC_HD uint64_t verdict(const Hits &h, uint64_t n, bool *period)
{
    *period = false;
    if (n < 2 || h.n_hit < 2 || (h.fwd && h.rev)) return NONE;
    const uint32_t beg = h.first, end = h.second - 1;
    if (beg > 0 || (uint64_t) end + 2 < n) {
        if (beg > end - beg) return NONE;
        *period = true;
    }
    return pack(beg, end, h.rev? 1u : 0u);
}
// the fragment that fragment j must equal (:594-601): the one a whole number of periods away inside the unit; beg <= r = end - beg
OATK_MC_HD uint32_t period_src(uint32_t j, uint32_t beg, uint32_t r) { return beg + (uint32_t) (((uint64_t) j + r + 1 - beg) % ((uint64_t) r + 1)); }
OATK_MC_HD bool period_ok(const uint64_t *uid, uint32_t j, uint32_t beg, uint32_t r) { return uid[j] == uid[period_src(j, beg, r)]; }

// the whole rule for one record, a fragment at a time; n < 2^31
OATK_MC_HD uint64_t unit_of(const uint64_t *uid, uint32_t n, uint64_t anchor)
{
    Hits h;
    hits_init(h);
    for (uint32_t j = 0; j < n; ++j) hits_add(h, j, uid[j], anchor);
    bool period;
    const uint64_t u = verdict(h, n, &period);
    if (u == NONE || !period) return u;
    const uint32_t beg = unit_beg(u), r = unit_end(u) - beg;
    for (uint32_t j = 0; j < n; ++j) if (!period_ok(uid, j, beg, r)) return NONE;
    return u;
}

// Element t (0 <= t < nv) of the canonical path of unit u (:661-668): uid[beg .. end] truncated to 32 bits; for a reverse unit elements 1 .. nv - 1 in reverse
// order and every element's strand flipped, so that every path starts with anchor << 1.  path_uid is the fragment's full uid: the reference drops its upper
// half without a word, the device call refuses (OATK_E_ARG) when it is not zero.
OATK_MC_HD uint64_t path_uid(const uint64_t *uid, uint64_t u, uint32_t t) { return uid[!unit_rev(u) || t == 0? unit_beg(u) + t : unit_end(u) + 1 - t]; }
OATK_MC_HD uint32_t path_elem(uint64_t full_uid, uint64_t u) { return (uint32_t) full_uid ^ unit_rev(u); }

// path_cmpfunc (:620-638): by length, then element by element; < 0, 0, > 0
OATK_MC_HD int path_cmp(const uint32_t *x, uint64_t nx, const uint32_t *y, uint64_t ny)
{
    if (nx != ny) return nx > ny? 1 : -1;
    for (uint64_t i = 0; i < nx; ++i) if (x[i] != y[i]) return x[i] > y[i]? 1 : -1;
    return 0;
}

// The 64-bit key under which equal paths meet: hash_seed(nv) + the sum of hash_term(t, v[t]) over the path, modulo 2^64 -- a sum, so that the lanes of a wave can
// each add their share in any order.  Only a grouping: every member of a group is compared with its head element by element (minicircle.hpp).
OATK_MC_HD uint64_t mix64(uint64_t x)
{
    x ^= x >> 33, x *= 0xFF51AFD7ED558CCDULL;
    x ^= x >> 33, x *= 0xC4CEB9FE1A85EC53ULL;
    return x ^ x >> 33;
}
OATK_MC_HD uint64_t hash_seed(uint64_t nv) { return mix64(nv); }
OATK_MC_HD uint64_t hash_term(uint32_t t, uint32_t elem) { return mix64(((uint64_t) t << 32 | elem) + 0x9E3779B97F4A7C15ULL); }
OATK_MC_HD uint64_t hash_mask(unsigned bits) { return bits == 0 || bits >= 64? ~0ULL : (1ULL << bits) - 1; }      // oatk_hip_debug_mc_hash_bits

}  // namespace oatk_mc
