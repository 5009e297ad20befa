// oatk_amd/csrc/count.hpp -- syncmer count / ID assignment on the device.
//
// Replaces `collect_syncmer_from_reads` + `process_kmer_cluster` (syncmer.c:1397-1451, :1270-1393).
// The reference sorts 128-bit (hash, sid<<32|idx<<1|rev) records, walks equal-hash groups, splits true
// 64-bit collisions by comparing the k-mer sequences, and hands out dense IDs in that order.  Here:
//   1. placement: scan records are unordered but carry (sid, ordinal), and the per-read counts are
//      known, so each record has an exact slot scm_off[read] + ordinal.  Scattering them there yields the
//      per-read arrays (m_pos, s_mer, hash) AND a sequence already ordered by the low 64 key bits.  The
//      scan's k-mer hash kernel does it as it finishes a record (kmer_hash.hpp).
//   2. one stable 64-bit radix sort of (hash -> slot) finishes the 128-bit order.
//   3. gather_verify: equal-hash neighbours are compared base-for-base (half a wave per strip of eight records,
//      one 32-base word per lane) -- the collision check the reference performs -- in the pass that writes the table.
//   4. split_collisions: groups that really hold different k-mers (never seen in practice; forced in tests
//      by masking hash bits) are partitioned in first-seen order by one lane per group.
//   5. IDs = prefix sum of new-cluster flags; coverage, CSR occurrence lists, s-mer consistency
//      (syncmer.c:1365-1376) and the per-read k_mer = id << 1 rewrite (:1378) are one pass each.
#pragma once
#include "common.hpp"
#include "count_onepass_core.hpp"

namespace oatk {

// 32 oriented k-mer bases [32*wd, 32*wd+32) MSB-first, zero beyond K, straight from the hoco string in HBM
__device__ __forceinline__ uint64_t kmer_word_global(const uint32_t *hs32, uint32_t pos, uint32_t rev, int K, int wd)
{
    int32_t t = rev? (int32_t) pos + K - 32 - 32 * wd : (int32_t) pos + 32 * wd;
    int nb = K - 32 * wd;
    nb = nb > 32? 32 : nb;
    int32_t wi = t >> 4;
    uint32_t sh = ((uint32_t) t & 15u) * 2u;
    uint32_t w0, w1, w2;
    if (wi >= 0) {                // one 12-byte load (the lanes of a comparison sit 8 bytes apart: three dword loads look up every cache line three times)
        struct __attribute__((packed, aligned(4))) W3 { uint32_t a, b, c; };
        const W3 v = *(const W3 *) (hs32 + wi);
        w0 = __builtin_bswap32(v.a), w1 = __builtin_bswap32(v.b), w2 = __builtin_bswap32(v.c);
    } else {                      // (the first bases of a slab's first read, reverse strand: what lies in front is masked)
        w0 = 0u;
        w1 = wi + 1 >= 0? __builtin_bswap32(hs32[wi + 1]) : 0u;
        w2 = wi + 2 >= 0? __builtin_bswap32(hs32[wi + 2]) : 0u;
    }
    uint64_t hi = (uint64_t) w0 << 32 | w1;
    uint64_t V = sh? (hi << sh) | ((uint64_t) w2 >> (32u - sh)) : hi;
    if (rev) V = revcomp32(V);
    if (nb < 32) V &= ~0ULL << (64 - 2 * nb);
    return V;
}

struct GroupArgs {
    const uint64_t *sorted_key;   // masked hash, ascending
    const uint32_t *perm;         // sorted index -> slot
    uint32_t n_rec;
    const uint64_t *pos_lo;
    const uint32_t *pos_mpos;
    const uint8_t *hoco_s;
    const uint64_t *off;
    uint64_t sid0;
    int K;
    uint32_t *head;               // 1 where a new equal-hash group starts
    uint32_t *newclus;            // 1 where a new syncmer (cluster) starts; starts as a copy of head
    uint32_t *flags;              // [0] some group holds different k-mers, [1] s-mer mismatch, [2] too many clusters
    uint64_t *loc;                // where the k-mer of sorted record i lives: (32-bit word index of its read's hoco string) << 32 | pos << 1 | rev
                                  // (loc and smer_sorted exist in the pessimistic order only: regather_kernel)
    // what else the sort permutation is followed for, fetched while it is followed the first time: the occurrence word (sid | index | strand)
    // and the s-mer of every sorted record -- finish_heads and check_smer then read them in order instead of gathering them again
    const uint64_t *pos_smer;
    uint64_t *occ_sorted, *smer_sorted;
    // ... and fetched as ONE 32-byte record per slot (kmer_hash_kernel; pack_slots_kernel for a batch assembled from pieces): occurrence word, s-mer, k-mer locator.  Three arrays indexed by the same
    // random slot cost three 64-byte fetches and the locator a fourth, dependent one (the read's offset); packed side by side in slot order -- a
    // streaming pass -- they cost one
    uint4 *slot_rec;
};

// (only for per-slot arrays that did not come out of kmer_hash_kernel, which writes the same records: oatk_hip_scan_append)
__global__ void pack_slots_kernel(GroupArgs a)
{
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_rec) return;
    const uint64_t lo = a.pos_lo[p], sm = a.pos_smer[p];
    const uint64_t loc = ((a.off[(lo >> 32) - a.sid0] >> 4) << 32) | a.pos_mpos[p];      // (slots are in read order: the offsets stream too)
    a.slot_rec[2 * (size_t) p] = make_uint4((uint32_t) lo, (uint32_t) (lo >> 32), (uint32_t) sm, (uint32_t) (sm >> 32));
    a.slot_rec[2 * (size_t) p + 1] = make_uint4((uint32_t) loc, (uint32_t) (loc >> 32), 0u, 0u);
}

// The sort of the k-mer hashes looks at their top 40 bits only (five radix passes instead of eight: 42 M records at config 3, 0.36 ms per pass).
// Two DIFFERENT hashes share 40 bits about n_distinct^2 / 2^41 times per batch -- a handful of runs -- and then their records sit interleaved,
// in slot order.  These two kernels finish the order there: every position where the hash changes inside a run of equal top bits reports to
// the run's start, and the smallest such position of a run sorts it (stable insertion sort of keys and permutation; runs are a few coverages
// long).  A run longer than OATK_SORT_REPAIR_MAX sets flags[3] and the host sorts again on all 64 bits.
#define OATK_SORT_LOW_BITS 24
#define OATK_SORT_REPAIR_MAX 4096u
__device__ __forceinline__ bool sort_repair_boundary(const uint64_t *key, uint32_t n, uint32_t i, uint32_t &start, uint32_t *flags)
{
    if (i == 0 || i >= n) return false;
    const uint64_t k = key[i], kp = key[i - 1];
    if ((k >> OATK_SORT_LOW_BITS) != (kp >> OATK_SORT_LOW_BITS) || k == kp) return false;
    uint32_t s = i - 1;
    while (s > 0 && (key[s - 1] >> OATK_SORT_LOW_BITS) == (k >> OATK_SORT_LOW_BITS)) {
        --s;
        if (i - s > OATK_SORT_REPAIR_MAX) { flags[3] = 1u; return false; }
    }
    start = s;
    return true;
}
__global__ void sort_repair_find_kernel(const uint64_t *key, uint32_t n, uint32_t *owner, uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s;
    if (sort_repair_boundary(key, n, i, s, flags)) atomicMin(&owner[s], i);       // owner[] starts as all ones
    // (nothing is taken on trust: rocPRIM's small-size paths were seen to leave the top bits of a bit-range sort out of order -- tools/ubench/sort_repair_test.hip,
    //  2000 - 100 000 keys -- and any inversion sends the count to the sort on all 64 bits)
    if (i > 0 && i < n && (key[i] >> OATK_SORT_LOW_BITS) < (key[i - 1] >> OATK_SORT_LOW_BITS)) flags[3] = 1u;
}
__global__ void sort_repair_kernel(uint64_t *key, uint32_t *perm, uint32_t n, uint32_t *owner, uint32_t *flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s;
    if (!sort_repair_boundary(key, n, i, s, flags) || owner[s] != i) return;     // (only a run's owner writes, and nobody reads what it writes: the others leave at once)
    const uint64_t top = key[i] >> OATK_SORT_LOW_BITS;
    uint32_t e = i + 1;
    while (e < n && (key[e] >> OATK_SORT_LOW_BITS) == top) {
        ++e;
        if (e - s > OATK_SORT_REPAIR_MAX) { flags[3] = 1u; return; }
    }
    for (uint32_t a = i; a < e; ++a) {                    // [s, i) holds one hash: sorted already
        const uint64_t kk = key[a];
        const uint32_t pp = perm[a];
        uint32_t b = a;
        while (b > s && key[b - 1] > kk) { key[b] = key[b - 1], perm[b] = perm[b - 1]; --b; }
        key[b] = kk, perm[b] = pp;
    }
}

// The sort is a library call whose paths differ by size and version: what comes back is CHECKED to be the input, permuted and in order.  Two independent
// 64-bit sums over a mix of every (hash, slot) pair are taken of the sort's input and of its output (after the repair); equal sums = the same multiset of
// pairs (up to 2^-128), so perm is a permutation and every hash sits beside its own slot; the order is compared directly.
// flags[8..11] hold the input's sums, flags[12..15] the output's, flags[4] an inversion.  Grid-stride with a fixed grid and one pair of atomics per
// workgroup: a first version with a pair per WAVE of a one-thread-per-record kernel cost 16 ms at config 3 -- 1.3 M atomics on two addresses.
__device__ __forceinline__ void pair_sums(uint64_t key, uint32_t slot, uint64_t &s0, uint64_t &s1)
{
    uint64_t x = key ^ ((uint64_t) slot * 0x9E3779B97F4A7C15ULL);
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ULL; x ^= x >> 32;
    s0 = x;
    x *= 0xD6E8FEB86659FD93ULL; x ^= x >> 29; x += key;
    s1 = x;
}
// perm == nullptr: the pairs are (key[i], i) -- the sort's input; otherwise (key[i], perm[i]) and the keys are checked to ascend.
// HEADS (the sort's output only): the pass that compares every sorted key with the one in front of it also says where an equal-hash group starts -- head
// and newclus as the optimistic order wants them (round 4: with the ids known from a scan of these flags BEFORE the verification -- on the
// assumption, checked in the same pass, that no hash group holds two k-mers -- one pass through the permutation gathers, writes what finish_heads_kernel
// writes and verifies (gather_verify_kernel); a collision falls back to the passes below).  The two arrays are only touched when HEADS is set.
template <bool HEADS>
__global__ __launch_bounds__(256) void pair_sum_kernel(const uint64_t *key, const uint32_t *perm, uint32_t n, uint32_t *flags, int at,
                                                       uint32_t *head, uint32_t *newclus)
{
    __shared__ uint64_t part[2][4];
    uint64_t s0 = 0, s1 = 0;
    bool inv = false;
    // (four independent elements per turn: the loads of a turn are in flight together)
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += 4 * stride) {
        uint64_t k[4], kp[4];
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t i = i0 + u * stride;
            const bool in = i < n;
            k[u] = in? key[i] : 0, v[u] = in? (perm? perm[i] : (uint32_t) i) : 0, kp[u] = in && perm && i? key[i - 1] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u * stride >= n) continue;
            uint64_t a, b;
            pair_sums(k[u], v[u], a, b);
            s0 += a, s1 += b;
            if (k[u] < kp[u]) inv = true;
            if (HEADS) {
                const uint32_t i = (uint32_t) (i0 + u * stride), h = i == 0 || k[u] != kp[u];
                head[i] = h, newclus[i] = h;
            }
        }
    }
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1) s0 += __shfl_xor(s0, d), s1 += __shfl_xor(s1, d);
    if ((threadIdx.x & 63u) == 0) part[0][threadIdx.x >> 6] = s0, part[1][threadIdx.x >> 6] = s1;
    if (inv) flags[4] = 1u;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd((unsigned long long *) (flags + at), (unsigned long long) (part[0][0] + part[0][1] + part[0][2] + part[0][3]));
        atomicAdd((unsigned long long *) (flags + at + 2), (unsigned long long) (part[1][0] + part[1][1] + part[1][2] + part[1][3]));
    }
}

// after a split of colliding groups the permutation has changed inside them: fetch what finish_heads and check_smer read in order
__global__ void regather_kernel(GroupArgs a)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_rec) return;
    const uint32_t p = a.perm[i];
    const uint4 r0 = a.slot_rec[2 * (size_t) p], r1 = a.slot_rec[2 * (size_t) p + 1];
    a.loc[i] = (uint64_t) r1.y << 32 | r1.x;
    a.occ_sorted[i] = (uint64_t) r0.y << 32 | r0.x, a.smer_sorted[i] = (uint64_t) r0.w << 32 | r0.z;
}

// one lane per colliding group: first-seen clustering, then a stable partition of the group's slice of perm
#define OATK_MAX_SPLIT 16
__global__ void split_collisions_kernel(GroupArgs a, const uint32_t *bad_head, uint32_t *perm_rw, uint32_t *tag, uint32_t *tmp_perm)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_rec || !a.head[i] || !bad_head[i]) return;
    uint32_t e = i + 1;
    while (e < a.n_rec && !a.head[e]) ++e;
    const int nw = (a.K + 31) / 32;
    uint32_t rep[OATK_MAX_SPLIT], nclus = 0;
    for (uint32_t t = i; t < e; ++t) {
        uint32_t p = perm_rw[t];
        uint64_t lo_p = a.pos_lo[p];
        const uint32_t *hs_p = (const uint32_t *) (a.hoco_s + (a.off[(lo_p >> 32) - a.sid0] >> 2));
        uint32_t mp = a.pos_mpos[p], c;
        for (c = 0; c < nclus; ++c) {
            uint32_t q = perm_rw[rep[c]];
            uint64_t lo_q = a.pos_lo[q];
            const uint32_t *hs_q = (const uint32_t *) (a.hoco_s + (a.off[(lo_q >> 32) - a.sid0] >> 2));
            uint32_t mq = a.pos_mpos[q];
            bool same = true;
            for (int wd = 0; wd < nw && same; ++wd)
                same = kmer_word_global(hs_p, mp >> 1, mp & 1u, a.K, wd) == kmer_word_global(hs_q, mq >> 1, mq & 1u, a.K, wd);
            if (same) break;
        }
        if (c == nclus) {
            if (nclus == OATK_MAX_SPLIT) { a.flags[2] = 1u; return; }
            rep[nclus++] = t;
        }
        tag[t] = c;
    }
    // stable partition by cluster; clusters keep first-seen order (syncmer.c:1324-1334, :1353-1360)
    uint32_t w = i;
    for (uint32_t c = 0; c < nclus; ++c) {
        bool first = true;
        for (uint32_t t = i; t < e; ++t)
            if (tag[t] == c) {
                tmp_perm[w] = perm_rw[t];
                a.newclus[w] = first? 1u : 0u;
                first = false;
                ++w;
            }
    }
    for (uint32_t t = i; t < e; ++t) perm_rw[t] = tmp_perm[t];
}

struct FinishArgs {
    const uint32_t *perm;
    const uint32_t *newclus;
    const uint32_t *clus_id1;     // inclusive scan of newclus: id + 1
    uint32_t n_rec;
    const uint64_t *sorted_key, *smer_sorted;     // smer_sorted: the s-mer of every sorted record (regather_kernel)
    uint64_t *scm_h, *scm_s;
    uint64_t *scm_occ_off;        // [n_scm + 1]
    uint64_t *scm_occ;            // [n_rec]: written by gather_verify_kernel / regather_kernel (GroupArgs::occ_sorted)
    const uint64_t *loc;          // k-mer locator of every sorted record (regather_kernel)
    uint64_t *scm_loc;            // [n_scm] where a syncmer's k-mer can be read: the locator of its first occurrence (what the EC graph's vertices need)
    uint64_t *pos_kid;            // id << 1 per slot
    uint32_t *flags;
};

__global__ void finish_heads_kernel(FinishArgs a, uint32_t n_scm)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_rec) return;
    uint32_t p = a.perm[i], id = a.clus_id1[i] - 1u;
    a.pos_kid[p] = (uint64_t) id << 1;
    if (a.newclus[i]) {
        a.scm_h[id] = a.sorted_key[i];
        a.scm_s[id] = a.smer_sorted[i];
        a.scm_occ_off[id] = i;
        a.scm_loc[id] = a.loc[i];
    }
    if (i == a.n_rec - 1) a.scm_occ_off[n_scm] = a.n_rec;
}

// The optimistic order in ONE pass over the sorted records (clus_id1 = id + 1, straight from the inclusive scan of the head flags): a tile of
// OATK_OP_TILE records per workgroup, in two halves.
//   Gather and finish, a lane per record: follow perm into the 32-byte slot record, write the occurrence word, the read's id, and at a head the
//   table's row.  The record's k-mer locator and s-mer go to LDS and nowhere else; lane 0 also fetches the record in front of the tile when the
//   tile's first record is no head.
//   Check: is every record that is no head identical to its PREDECESSOR in sorted order -- k-mer and s-mer?  Equality is transitive, so that says
//   the same as "identical to its group head", and the predecessor's locator and s-mer lie one LDS slot to the left (count_onepass_core.hpp).
//   The s-mers are compared by the lane that gathered the record.  The k-mers go by STRIPs of eight consecutive records, half a wave per strip
//   (32 lanes x 32 bases cover k <= 1024 in one step, one 32-base word per lane): a strip inside one group -- the usual case: a solid syncmer
//   occurs once per read that covers it, tens of records at HiFi depth -- loads nine k-mers, the eight records' and the one in front, all
//   in flight together before the first comparison.  A strip of heads (singletons, most of the error k-mers) does nothing.
// The check is a chain of dependent gathers and its rate is (bytes in flight) / (HBM latency); what it needs from the gather half arrives through
// LDS instead of through three per-record arrays in HBM (locator, s-mer, head index: 40 B written and 60 B read per record) and one max-scan.
// A k-mer that differs sets flags[0] and bad_head at the head of its group, found by walking back over newclus (forced-collision tests only: the
// host then takes the pessimistic order below, which decides flags[1] again on its final clusters); an s-mer that differs sets flags[1].
#ifndef OATK_VG_STRIP
#define OATK_VG_STRIP 8
#endif
#ifndef OATK_VFY_WAVES
#define OATK_VFY_WAVES 1
#endif
#define OATK_OP_TILE 256
static_assert(64 % OATK_VG_STRIP == 0 && OATK_VG_STRIP <= 31 && OATK_OP_TILE % 64 == 0, "a wave's 64 head flags hold whole strips");
__global__ __launch_bounds__(OATK_OP_TILE, OATK_VFY_WAVES) void gather_verify_kernel(GroupArgs g, FinishArgs a, const uint32_t *clus_id1, uint32_t n_scm, uint32_t *bad_head)
{
    __shared__ uint64_t s_loc[OATK_OP_TILE + 1], s_sm[OATK_OP_TILE + 1];      // [1 + t]: record t0 + t; [0]: the record in front of the tile
    __shared__ uint64_t s_live[OATK_OP_TILE / 64];                            // bit t: record t0 + t is in range and no head
    const uint32_t t = threadIdx.x, t0 = blockIdx.x * (uint32_t) OATK_OP_TILE, i = t0 + t;
    uint64_t loc = 0, smer = 0;
    bool live = false;
    if (i < a.n_rec) {
        const uint32_t p = g.perm[i], id = clus_id1[i] - 1u, nc = g.newclus[i];
        const uint32_t pp = t == 0 && i > 0? g.perm[i - 1] : 0u;
        const uint4 r0 = g.slot_rec[2 * (size_t) p], r1 = g.slot_rec[2 * (size_t) p + 1];
        live = !nc && i > 0;
        if (t == 0 && live) {                  // (both gathers of this lane are in flight together)
            const uint4 q0 = g.slot_rec[2 * (size_t) pp], q1 = g.slot_rec[2 * (size_t) pp + 1];
            s_loc[0] = (uint64_t) q1.y << 32 | q1.x, s_sm[0] = (uint64_t) q0.w << 32 | q0.z;
        }
        loc = (uint64_t) r1.y << 32 | r1.x, smer = (uint64_t) r0.w << 32 | r0.z;
        g.occ_sorted[i] = (uint64_t) r0.y << 32 | r0.x;
        a.pos_kid[p] = (uint64_t) id << 1;
        if (nc) {
            a.scm_h[id] = a.sorted_key[i];
            a.scm_s[id] = smer;
            a.scm_occ_off[id] = i;
            a.scm_loc[id] = loc;
        }
        if (i == a.n_rec - 1) a.scm_occ_off[n_scm] = a.n_rec;
    }
    s_loc[1 + t] = loc, s_sm[1 + t] = smer;
    const uint64_t wave_live = __ballot(live);
    if ((t & 63u) == 0) s_live[t >> 6] = wave_live;
    __syncthreads();
    // identical k-mers must carry the same s-mer (fatal in the reference, syncmer.c:1370-1376); only meaningful where the k-mers ARE identical
    if (live && s_sm[t] != smer) g.flags[1] = 1u;

    const uint32_t hl = t & 31u, half0 = t & 32u;                             // lane in the half wave; first lane of the half wave within the wave
    const uint32_t *hs32 = (const uint32_t *) g.hoco_s;
    const int nw = (g.K + 31) / 32;
    constexpr uint32_t PER_HALF = OATK_OP_TILE / OATK_VG_STRIP / (OATK_OP_TILE / 32);       // strips per half wave: those of the records its wave gathered
#pragma unroll 1
    for (uint32_t u = 0; u < PER_HALF; ++u) {
        const uint32_t s0 = ((t >> 5) * PER_HALF + u) * OATK_VG_STRIP;        // the strip's first record within the tile
        const uint32_t live_mask = (uint32_t) (s_live[s0 >> 6] >> (s0 & 63u)) & ((1u << OATK_VG_STRIP) - 1u);
        if (live_mask == 0) continue;
        const uint32_t need = onepass_need_mask(live_mask);
        uint32_t diff = 0;                                                    // bit r: this lane saw record s0 + r differ from the one in front of it
        for (int w0 = 0; w0 < nw; w0 += 32) {
            const int wd = w0 + (int) hl;
            const bool in = wd < nw;
            uint64_t w[OATK_VG_STRIP + 1];
#pragma unroll
            for (int j = 0; j <= OATK_VG_STRIP; ++j) {                        // every load of the strip is issued before the first comparison
                const uint64_t lp = s_loc[s0 + j];
                w[j] = in && ((need >> j) & 1u)? kmer_word_global(hs32 + (lp >> 32), (uint32_t) lp >> 1, (uint32_t) lp & 1u, g.K, wd) : 0;
            }
            diff |= onepass_diff_mask<OATK_VG_STRIP>(w, live_mask);
        }
        if (((__ballot(diff != 0) >> half0) & 0xFFFFFFFFULL) == 0) continue;
#pragma unroll
        for (int r = 0; r < OATK_VG_STRIP; ++r) {
            const uint64_t bad = (__ballot((diff >> r) & 1u) >> half0) & 0xFFFFFFFFULL;
            if (bad && hl == (uint32_t) r) g.flags[0] = 1u, bad_head[onepass_head_of(g.newclus, t0 + s0 + r)] = 1u;
        }
    }
}

// identical k-mers must carry the same s-mer (fatal in the reference, syncmer.c:1370-1376): on the final clusters of the pessimistic order
__global__ void check_smer_kernel(FinishArgs a)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_rec) return;
    uint32_t id = a.clus_id1[i] - 1u;
    if (a.smer_sorted[i] != a.scm_s[id]) a.flags[1] = 1u;
}

__global__ void cov_kernel(const uint64_t *occ_off, uint32_t *cov, uint32_t n_scm)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_scm) cov[i] = (uint32_t) (occ_off[i + 1] - occ_off[i]);
}

}  // namespace oatk
