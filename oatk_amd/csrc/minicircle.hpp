// oatk_amd/csrc/minicircle.hpp -- the repeat units of the mini-circle path finder (extract_minicircles_with_anchor, path_finder.c:640-693) from the read
// alignments: per record its unit, the valid records' canonical paths back to back, and the distinct paths with the number of records behind each.  The rule and
// the path element are minicircle_core.hpp's; C ABI in api_minicircle.inc, include/oatk_hip_racov.h.
//
// Records and paths come in two LENGTH CLASSES.  Almost every record has 1-4 fragments: a lane takes a whole record of up to SHORT fragments
// and runs the rule a fragment at a time, and puts the index of a longer one on a list.  A wave then takes each listed record 64 fragments at a time: the hits of
// a chunk are two ballots, the period check a third, so a record of any length costs ceil(n / 64) steps per pass and nothing is held per fragment.  The paths are
// written the same way.  Which lane or wave handles a record never shows in the result: every record's unit, path and key are functions of the record alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "minicircle_core.hpp"

namespace oatk {

enum { MC_ERR_LONG = 1, MC_ERR_UID = 2 };

struct McArgs {
    uint64_t n_aln;                // below 2^32
    const uint64_t *off;           // [n_aln + 1]
    const uint64_t *uid;
    uint64_t anchor;
    unsigned int *err;
};

__device__ __forceinline__ uint32_t mc_wave_id() { return (uint32_t) __builtin_amdgcn_readfirstlane((int) ((blockIdx.x * blockDim.x + threadIdx.x) >> 6)); }

// ---- (a) MC_UNIT ----
__global__ void mc_unit_short_kernel(McArgs a, uint64_t *unit, uint32_t *long_idx, unsigned int *n_long)
{
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_aln; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t f0 = a.off[i], n = a.off[i + 1] - f0;
        if (n > oatk_mc::SHORT) { long_idx[atomicAdd(n_long, 1u)] = (uint32_t) i; continue; }
        unit[i] = oatk_mc::unit_of(a.uid + f0, (uint32_t) n, a.anchor);
    }
}
__global__ void mc_unit_long_kernel(McArgs a, uint64_t *unit, const uint32_t *long_idx, const unsigned int *n_long)
{
    const uint32_t lane = threadIdx.x & 63, n_waves = (gridDim.x * blockDim.x) >> 6, n_list = *n_long;
    for (uint32_t w = mc_wave_id(); w < n_list; w += n_waves) {
        const uint64_t i = long_idx[w], f0 = a.off[i], n64 = a.off[i + 1] - f0;
        if (n64 >> 31) {                                                   // (the reference counts a record's fragments in 32 bits, and beg takes 31 of the unit's)
            if (lane == 0) unit[i] = oatk_mc::NONE, atomicOr(a.err, (unsigned) MC_ERR_LONG);
            continue;
        }
        const uint32_t n = (uint32_t) n64;
        const uint64_t *p = a.uid + f0;
        oatk_mc::Hits h;
        oatk_mc::hits_init(h);
        for (uint32_t base = 0; base < n; base += oatk_mc::CHUNK) {
            const uint32_t j = base + lane;
            const uint64_t u = j < n? p[j] : 0;
            const bool is = j < n && oatk_mc::hit(u, a.anchor);
            oatk_mc::hits_add_chunk(h, base, __ballot(is), __ballot(is && (u & 1)));
            if (h.fwd && h.rev) break;                                     // both orientations: nothing, whatever follows
        }
        bool period;
        uint64_t v = oatk_mc::verdict(h, n, &period);
        if (v != oatk_mc::NONE && period) {
            const uint32_t beg = oatk_mc::unit_beg(v), r = oatk_mc::unit_end(v) - beg;
            for (uint32_t base = 0; base < n; base += oatk_mc::CHUNK) {
                const uint32_t j = base + lane;
                if (__ballot(j < n && !oatk_mc::period_ok(p, j, beg, r))) { v = oatk_mc::NONE; break; }
            }
        }
        if (lane == 0) unit[i] = v;
    }
}

// ---- (b) the valid records, and their paths back to back ----
// flag / nv [n_aln + 1] for the two scans (entry n_aln = 0)
__global__ void mc_nv_kernel(uint64_t n_aln, const uint64_t *unit, uint64_t *flag, uint64_t *nv)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_aln) return;
    const bool valid = i < n_aln && unit[i] != oatk_mc::NONE;
    flag[i] = valid, nv[i] = valid? oatk_mc::unit_nv(unit[i]) : 0;
}
// rec[k] = the k-th valid record, p_off[k] = where its path starts (p_off[n_valid] = all paths' elements)
__global__ void mc_place_kernel(uint64_t n_aln, const uint64_t *unit, const uint64_t *pos, const uint64_t *voff, uint32_t *rec, uint64_t *p_off)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_aln) return;
    if (i == n_aln) p_off[pos[i]] = voff[i];
    else if (unit[i] != oatk_mc::NONE) rec[pos[i]] = (uint32_t) i, p_off[pos[i]] = voff[i];
}
// v[p_off[k] ..) = the canonical path of valid record k, key[k] = its hash under `mask`, val[k] = k
__global__ void mc_path_short_kernel(McArgs a, const uint64_t *unit, uint64_t n_valid, const uint32_t *rec, const uint64_t *p_off, uint32_t *v, uint64_t *key,
                                     uint32_t *val, uint64_t mask, uint32_t *long_idx, unsigned int *n_long)
{
    for (uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; k < n_valid; k += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t i = rec[k], u = unit[i];
        const uint32_t nv = oatk_mc::unit_nv(u);
        val[k] = (uint32_t) k;
        if (nv > oatk_mc::SHORT) { long_idx[atomicAdd(n_long, 1u)] = (uint32_t) k; continue; }
        const uint64_t *p = a.uid + a.off[i];
        uint32_t *out = v + p_off[k];
        uint64_t h = oatk_mc::hash_seed(nv), high = 0;
        for (uint32_t t = 0; t < nv; ++t) {
            const uint64_t full = oatk_mc::path_uid(p, u, t);
            const uint32_t e = oatk_mc::path_elem(full, u);
            high |= full >> 32, out[t] = e, h += oatk_mc::hash_term(t, e);
        }
        if (high) atomicOr(a.err, (unsigned) MC_ERR_UID);
        key[k] = h & mask;
    }
}
__global__ void mc_path_long_kernel(McArgs a, const uint64_t *unit, const uint32_t *rec, const uint64_t *p_off, uint32_t *v, uint64_t *key, uint64_t mask,
                                    const uint32_t *long_idx, const unsigned int *n_long)
{
    const uint32_t lane = threadIdx.x & 63, n_waves = (gridDim.x * blockDim.x) >> 6, n_list = *n_long;
    for (uint32_t w = mc_wave_id(); w < n_list; w += n_waves) {
        const uint64_t k = long_idx[w], i = rec[k], u = unit[i];
        const uint32_t nv = oatk_mc::unit_nv(u);
        const uint64_t *p = a.uid + a.off[i];
        uint32_t *out = v + p_off[k];
        uint64_t h = 0, high = 0;
        for (uint32_t t = lane; t < nv; t += oatk_mc::CHUNK) {
            const uint64_t full = oatk_mc::path_uid(p, u, t);
            const uint32_t e = oatk_mc::path_elem(full, u);
            high |= full >> 32, out[t] = e, h += oatk_mc::hash_term(t, e);
        }
        for (int d = 32; d; d >>= 1) h += (uint64_t) __shfl_xor((long long) h, d);
        if (__ballot(high != 0) && lane == 0) atomicOr(a.err, (unsigned) MC_ERR_UID);
        if (lane == 0) key[k] = (oatk_mc::hash_seed(nv) + h) & mask;
    }
}

// ---- (c) distinct paths ----
// (key, val)[0 .. n): valid records sorted by key, a key's records in ascending order (a stable sort, and what is left of one after a stable selection).  Every
// member of a run of one key is compared, element by element, with the run's first member, the HEAD: an equal path gets rep[its record] = the head's record and
// leaves; a different one (two paths under one key) stays, left[j] = 1, and meets the first of those that stayed in the next round.  The head equals itself,
// so every round settles at least one record per key.
__global__ void mc_verify_kernel(uint64_t n, const uint64_t *key, const uint32_t *val, const uint64_t *p_off, const uint32_t *v, uint32_t *rep, uint8_t *left)
{
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t K = key[j];
    uint64_t lo = 0, hi = j;                                               // the first entry with this key
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (key[mid] < K) lo = mid + 1; else hi = mid; }
    const uint32_t k = val[j], kh = val[lo];
    const uint64_t nv = p_off[k + 1] - p_off[k];
    bool same = nv == p_off[kh + 1] - p_off[kh];
    const uint32_t *x = v + p_off[k], *y = v + p_off[kh];
    for (uint64_t t = 0; same && t < nv; ++t) same = x[t] == y[t];
    if (same) rep[k] = kh;
    left[j] = !same;
}
// cnt[k] = records whose path is valid record k's, for the k that stand for a path (rep[k] == k); flag / nv [n_valid + 1] for the scans over those
__global__ void mc_count_kernel(uint64_t n_valid, const uint32_t *rep, const uint64_t *p_off, unsigned long long *cnt, uint64_t *flag, uint64_t *nv)
{
    const uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_valid) return;
    const bool head = k < n_valid && rep[k] == k;
    flag[k] = head, nv[k] = head? p_off[k + 1] - p_off[k] : 0;
    if (k < n_valid) atomicAdd(&cnt[rep[k]], 1ull);
}
// the distinct paths back to back, in the order of their first records
__global__ void mc_gather_kernel(uint64_t n_valid, const uint32_t *rep, const uint64_t *pos, const uint64_t *doff, const uint64_t *p_off, const uint32_t *v,
                                 const unsigned long long *cnt, uint64_t *o_off, uint32_t *o_v, uint64_t *o_cnt)
{
    const uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_valid) return;
    if (k == n_valid) { o_off[pos[k]] = doff[k]; return; }
    if (rep[k] != k) return;
    const uint64_t d = pos[k], nv = p_off[k + 1] - p_off[k];
    o_off[d] = doff[k], o_cnt[d] = cnt[k];
    for (uint64_t t = 0; t < nv; ++t) o_v[doff[k] + t] = v[p_off[k] + t];
}

}  // namespace oatk
