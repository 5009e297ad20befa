// oatk_amd/csrc/triplet.hpp -- the spanning-triplet table of scg_multiplex (syncasm.c:1110-1166) from the read alignments.  C ABI in
// api_multiplex.inc, include/oatk_hip_racov.h.
//
// A triplet is keyed by a pair of arc ids (l0, l1); every event puts its key A = (l0, l1) and then the mirror A' = (c1, c0).  Both keys
// of an event lie in one GROUP: the unordered pair of their link ids {l0 >> 1, l1 >> 1} (c is l or l ^ 1).  A group has eight keys at the
// most -- which link comes first, and the two comp bits -- and they live side by side in val8 / have8[8 * group + slot].  Identity is by
// key value alone, like kh_dbl's: whatever the link ids, two events meet in a slot exactly when the reference's table would hand them one
// bucket.  The groups are those of the (in, out) arc pairs scg_multiplex looks up (:1240); events of other groups are dropped, they can
// touch no key that is read.  The doubles are formed like the reference forms them: per slot its additions in record order, runs of 1.0
// bundled where that rounds the same, FP contraction off.
#pragma once
#include "racov.hpp"

namespace oatk {

// where key (k0, k1) lives in its group (lo = the smaller link id of the two)
__host__ __device__ __forceinline__ uint32_t rc_tri_slot(uint64_t k0, uint64_t k1, uint64_t lo)
{
    return (uint32_t) (((k0 >> 1) != lo? 4 : 0) | (k0 & 1) << 1 | (k1 & 1));
}
__host__ __device__ __forceinline__ uint64_t rc_tri_group(uint64_t k0, uint64_t k1)
{
    const uint64_t a = k0 >> 1, b = k1 >> 1;
    return a < b? a << 32 | b : b << 32 | a;
}

// flag[p] = the syncmer at unitig position p lies on this one position only (scm_utg_n == 1).  Its exclusive prefix sums answer "has
// fragment [u_beg, u_end] a unique syncmer" with two loads, however long the fragment
__global__ void rc_tri_uniq_kernel(RcArgs a, uint64_t m_scm, uint64_t *flag)
{
    const uint64_t p = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m_scm) return;
    const uint64_t x = a.utg_a[p] >> 1;
    flag[p] = x < a.n_scm && a.su_off[x + 1] - a.su_off[x] == 1;
}

__device__ __forceinline__ uint64_t rc_tri_arc(const RcArcArgs &g, uint64_t v, uint64_t w)           // asmg_arc: deleted arcs too
{
    for (uint64_t t = g.idx_p[v], e = t + g.idx_n[v]; t < e && t < g.n_arc; ++t) if (g.arc_w[t] == w) return t;
    return g.n_arc;
}

// One event per slot j >= 2 of a record of three or more fragments whose fragments j - 2, j - 1, j are all unique (:1145-1164).  Slot f
// is the event's rank in the reference's order.  An event makes two CONTRIBUTIONS, one to the slot of its key A (key[2f]) and one to the
// slot of its mirror A' (key[2f + 1]), a slot being 8 * group + rc_tri_slot; both stay ~0 when there is no event or nobody reads the group.
// first[slot] = the first event that touches the slot.  A missing arc between ANY two consecutive fragments of such a record is an error
// (the reference dereferences NULL), and so is a fragment outside the graph.
__global__ void rc_triplet_kernel(RcArgs a, RcArcArgs g, const uint64_t *uq, const uint64_t *grp, uint64_t n_grp, uint32_t *key, uint32_t *val,
                                  uint32_t *first, double *score_out)
{
#pragma clang fp contract(off)
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_aln; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t f0 = a.off[i], m = a.off[i + 1] - f0;
        if (m < 3) continue;
        double score = rc_frac(a.s[i]);
        if (score < DBL_EPSILON) score = 1.0;
        const bool look = score < .99;                                      // not uniquely mapped: fragment by fragment
        bool ok = true;
        for (uint64_t f = f0; f < f0 + m; ++f) {
            const uint64_t u = a.uid[f] >> 1;
            if (u >= a.n_utg || (look && a.ubeg[f] <= a.uend[f] && a.uend[f] >= a.utg_n[u])) ok = false;
        }
        if (!ok) { atomicOr(a.err, (unsigned) RC_ERR_FRG); continue; }
        auto uniq = [&](uint64_t f) -> bool {
            if (!look) return true;
            if (a.ubeg[f] > a.uend[f]) return false;
            const uint64_t b = a.utg_off[a.uid[f] >> 1];
            return uq[b + a.uend[f] + 1] > uq[b + a.ubeg[f]];
        };
        uint64_t x0 = rc_tri_arc(g, a.uid[f0], a.uid[f0 + 1]);
        if (x0 == g.n_arc) atomicOr(a.err, (unsigned) RC_ERR_ARC);
        bool u0 = uniq(f0), u1 = uniq(f0 + 1);
        for (uint64_t j = 2; j < m; ++j) {
            const uint64_t x1 = rc_tri_arc(g, a.uid[f0 + j - 1], a.uid[f0 + j]);
            const bool u2 = uniq(f0 + j);
            if (x1 == g.n_arc) atomicOr(a.err, (unsigned) RC_ERR_ARC);
            else if (x0 != g.n_arc && u0 && u1 && u2) {
                const uint64_t l0 = g.arc_link[x0] << 1 | g.arc_comp[x0], l1 = g.arc_link[x1] << 1 | g.arc_comp[x1];
                const uint64_t c0 = (g.arc_v[x0] ^ 1) != g.arc_w[x0]? l0 ^ 1 : l0, c1 = (g.arc_v[x1] ^ 1) != g.arc_w[x1]? l1 ^ 1 : l1;   // asmg_comp_arc_id
                const uint64_t gk = rc_tri_group(l0, l1), lo = gk >> 32;
                uint64_t b = 0, e = n_grp;
                while (b < e) { const uint64_t mid = b + (e - b) / 2; if (grp[mid] < gk) b = mid + 1; else e = mid; }
                if (b < n_grp && grp[b] == gk) {
                    const uint64_t f = f0 + j;
                    const uint32_t p = (uint32_t) (8 * b) + rc_tri_slot(l0, l1, lo), q = (uint32_t) (8 * b) + rc_tri_slot(c1, c0, lo);
                    key[2 * f] = p, key[2 * f + 1] = q, val[2 * f] = (uint32_t) (2 * f), val[2 * f + 1] = (uint32_t) (2 * f + 1);
                    atomicMin(&first[p], (uint32_t) f), atomicMin(&first[q], (uint32_t) f);
                    score_out[f] = score;
                }
            }
            x0 = x1, u0 = u1, u1 = u2;
        }
    }
}

// kh_dbl's puts (:1151-1160): an event whose key A is absent SETS val[A] = val[A'] = score, any other ADDS the score to both (a mirror that
// is absent then starts from 0, which is what an absent slot holds here).  A slot is present once any event has touched it, so the events
// that set are those that are the first to touch the slot of their key, where the table they go on from (zeros, or what the previous rank
// left) does not have it: at most eight per group.  last[slot] = 1 + the last such event that wrote the slot, 0 = none.
__global__ void rc_tri_assign_kernel(uint64_t n_frg, const uint32_t *key, const uint32_t *first, const uint8_t *have8, uint32_t *last)
{
    const uint64_t f = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frg || key[2 * f] == 0xFFFFFFFFu) return;
    const uint32_t p = key[2 * f], q = key[2 * f + 1];
    if (first[p] == (uint32_t) f && !have8[p]) atomicMax(&last[p], (uint32_t) f + 1), atomicMax(&last[q], (uint32_t) f + 1);
}
// per contribution in (slot, order) order: w = 1 for a score of 1.0 (the uniquely mapped reads), fl = 1 for a fractional one
__global__ void rc_tri_prep_kernel(uint64_t n, const uint32_t *key, const uint32_t *ord, const double *score, uint64_t *w, uint64_t *fl)
{
    const uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const bool valid = key[c] != 0xFFFFFFFFu, one = valid && score[ord[c] >> 1] == 1.0;
    w[c] = one, fl[c] = valid && !one;
}
// One lane per slot: its value is what its last setting event left (or what the table held), plus the contributions behind that event in
// the reference's order -- the fractional ones one by one, the runs of 1.0 between them by rc_add_run, which rounds like the sequential
// additions do (racov.hpp).  An event whose key is its own mirror contributes twice to the one slot: set once, or added twice.
__global__ void rc_tri_replay_kernel(uint64_t n, const uint32_t *key, const uint32_t *ord, const double *score, const uint32_t *last, const uint64_t *E,
                                     const uint64_t *ef, const uint64_t *fpos, double *val8, uint8_t *have8)
{
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || key[i] == 0xFFFFFFFFu || (i > 0 && key[i - 1] == key[i])) return;
    const uint32_t S = key[i];
    uint64_t c0 = i, c1 = i + 1;
    { uint64_t hi = n; while (c1 < hi) { const uint64_t mid = c1 + (hi - c1) / 2; if (key[mid] == S) c1 = mid + 1; else hi = mid; } }     // the slot's contributions: [c0, c1)
    double s = val8[S];
    if (last[S]) {
        const uint32_t e = last[S] - 1;
        s = score[e];
        uint64_t lo = c0, hi = c1;                                            // behind the setting event's own contributions
        while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if ((ord[mid] >> 1) <= e) lo = mid + 1; else hi = mid; }
        c0 = lo;
    }
    uint64_t cur = c0;
    for (uint64_t x = ef[c0], xe = ef[c1]; x < xe; ++x) {
        const uint64_t p = fpos[x];
        s = rc_add_run(s, cur, p, E);
        s += score[ord[p] >> 1];
        cur = p + 1;
    }
    s = rc_add_run(s, cur, c1, E);
    val8[S] = s, have8[S] = 1;
}

// the pairs in the reference's lookup order: pslot[p] = 8 * group + slot of the pair's key
__global__ void rc_tri_out_kernel(uint64_t n_pair, const uint32_t *pslot, const double *val8, const uint8_t *have8, double *score, uint8_t *have)
{
    const uint64_t p = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pair) return;
    have[p] = have8[pslot[p]];
    score[p] = have[p]? val8[pslot[p]] : 0.;
}

}  // namespace oatk
