// oatk_amd/csrc/racov.hpp -- unitig and arc coverage from read alignments: scg_ra_utg_coverage (syncasm.c:1882-2065) with make_ma_block /
// find_lcs (:1652-1878), and the duplet sums of scg_ra_arc_coverage (:2067-2138).  C ABI in api_racov.inc, include/oatk_hip_racov.h.
//
// Every double these kernels form is formed like the reference forms it: FP contraction is off inside each kernel that touches one
// (`#pragma clang fp contract(off)`: gcc for baseline x86-64 never fuses a * b + c), and every sum whose addends may be fractional is
// a sequential replay in the reference's order -- per unitig (EM, IQR means) or per link (duplets).  Only the first round's counts are
// summed by atomics: integral addends, partial sums far below 2^53.  With reads sharded by record the replays are chained
// through the ranks: the EM's sums and the duplet table start from what the previous rank left (a carry-in, zeros for one handle).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

namespace oatk {

enum { RC_ERR_FRG = 1, RC_ERR_ARC = 2, RC_ERR_ROOM = 4 };

struct RcArgs {
    // alignments (flat scg_ra_v): records in ra_v order, fragments back to back
    uint64_t n_aln;
    const uint32_t *sid;           // read index into the chains
    const uint64_t *off;           // [n_aln + 1]
    const double *s;
    const uint64_t *uid;
    const uint32_t *ubeg, *uend, *sbeg, *send;
    // chains (sr_db->a[sid].k_mer)
    uint64_t n_reads;
    const uint64_t *chain_off, *k_mer;
    // graph
    uint64_t n_scm, n_utg;
    const uint64_t *su_off, *su_uid;
    const uint32_t *su_pos, *utg_n, *scm_cov;
    const uint64_t *utg_off, *utg_a;  // [n_utg + 1], vtx[].a back to back
    // reads = runs of records with one sid
    uint64_t n_rd;
    const uint64_t *rd_beg;        // [n_rd + 1]
    // make_ma_block's working room, per read at the scanned offsets
    const uint64_t *cell_off, *lcs_off, *blk_off, *u_off;
    int32_t *cells;
    uint64_t *lcs;
    uint32_t *rec_lb, *rec_ln;     // per record: its LCS blocks in lcs[]
    uint32_t *st_frg, *st_lcsb, *st_uid;
    uint64_t *st_beg, *st_len;
    // multiple-alignment blocks: ma_n[blk_off[r] + k], ma_u[u_off[r] + k * a + i], nb[r] = b
    uint32_t *ma_n, *ma_u, *nb;
    unsigned int *err;
};

__device__ __forceinline__ double rc_frac(double x)
{
    double ip;
    return modf(x, &ip);
}

// ---- reads: runs of equal sid in ra_v order (:1966-1977) ----
__global__ void rc_head_kernel(RcArgs a, uint64_t *flag)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_aln) flag[i] = i == 0 || a.sid[i] != a.sid[i - 1];
}
__global__ void rc_runs_kernel(RcArgs a, const uint64_t *flag, const uint64_t *pos, uint64_t *rd_beg)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_aln && flag[i]) rd_beg[pos[i]] = i;
    if (i == a.n_aln) rd_beg[a.n_rd] = a.n_aln;
}

// ---- first round (:1932-1942): uniquely mapped records add 1 to every syncmer position they cover ----
__global__ void rc_r1_count_kernel(RcArgs a, unsigned int *cnt)
{
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_aln; i += (uint64_t) gridDim.x * blockDim.x) {
        if (rc_frac(a.s[i]) > DBL_EPSILON) continue;
        for (uint64_t f = a.off[i]; f < a.off[i + 1]; ++f) {
            const uint64_t u = a.uid[f] >> 1;
            if (u >= a.n_utg || (a.ubeg[f] <= a.uend[f] && a.uend[f] >= a.utg_n[u])) { atomicOr(a.err, (unsigned) RC_ERR_FRG); continue; }
            const uint64_t base = a.utg_off[u];
            for (uint64_t k = a.ubeg[f]; k <= a.uend[f]; ++k) atomicAdd(&cnt[base + k], 1u);
        }
    }
}
__global__ void rc_u2d_kernel(const unsigned int *in, double *out, uint64_t n)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double) in[i];
}

// quantile(a, n, q, sorted = 1) and average_IQR(a, n, sorted) (syncasm.c:584-628) on an ascending array
__device__ double rc_quantile(const double *a, int n, double q)
{
#pragma clang fp contract(off)
    if (n == 1) return a[0];
    double ip;
    const double fp = modf(q * (n - 1), &ip);
    const int i = (int) lround(ip);
    if (i == n - 1) return a[i];
    return a[i] + (a[i + 1] - a[i]) * fp;
}
__device__ double rc_average_iqr(const double *a, int n)
{
#pragma clang fp contract(off)
    if (n == 0) return 0.;
    double q1 = rc_quantile(a, n, 0.25), q3 = rc_quantile(a, n, 0.75);
    const double iqr = q3 - q1;
    q1 -= 1.5 * iqr;
    q3 += 1.5 * iqr;
    int n0 = 0;
    double s = 0.;
    for (int i = 0; i < n; ++i)
        if (a[i] >= q1 && a[i] <= q3) ++n0, s += a[i];
    return n0? s / n0 : 0.;
}
// per unitig, its sorted values: MAX(1., average_IQR(...)), skipping the leading values below DBL_EPSILON when drop_zero (:1944-1951, :2040-2043)
__global__ void rc_iqr_kernel(uint64_t n_utg, const uint64_t *utg_off, const double *v, int drop_zero, double *avg)
{
#pragma clang fp contract(off)
    const uint64_t u = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_utg) return;
    const double *c = v + utg_off[u];
    const int n = (int) (utg_off[u + 1] - utg_off[u]);
    int m = 0;
    if (drop_zero) while (m < n && c[m] < DBL_EPSILON) ++m;
    const double x = rc_average_iqr(c + m, n - m);
    avg[u] = 1. > x? 1. : x;            // MAX(1., x) of the reference's macro: (1.) > (x)? (1.) : (x)
}

// ---- make_ma_block (:1756-1878), a lane per read ----
struct RcFrag {
    const uint64_t *s;             // the read's syncmers from s_beg
    const uint64_t *u;             // the unitig's from u_beg
    int64_t s_n, u_n;
    int rev;
    __device__ uint64_t S(int64_t t) const { return s[t] >> 1; }
    __device__ uint64_t U(int64_t t) const { return (rev? u[u_n - 1 - t] : u[t]) >> 1; }
};
__device__ __forceinline__ bool rc_frag(const RcArgs &a, uint64_t r, uint64_t f, RcFrag *g)
{
    const uint64_t sid = a.sid[r], u = a.uid[f] >> 1;
    if (sid >= a.n_reads || u >= a.n_utg) return false;
    const uint64_t rn = a.chain_off[sid + 1] - a.chain_off[sid];
    if (a.sbeg[f] > a.send[f] || a.send[f] >= rn || a.ubeg[f] > a.uend[f] || a.uend[f] >= a.utg_n[u]) return false;
    g->s = a.k_mer + a.chain_off[sid] + a.sbeg[f];
    g->u = a.utg_a + a.utg_off[u] + a.ubeg[f];
    g->s_n = (int64_t) a.send[f] - a.sbeg[f] + 1, g->u_n = (int64_t) a.uend[f] - a.ubeg[f] + 1;
    g->rev = (int) (a.uid[f] & 1);
    return true;
}
// find_lcs's trimming (:1693-1695): start, and the core's sizes
__device__ __forceinline__ void rc_trim(const RcFrag &g, int64_t *start, int64_t *cs, int64_t *cu)
{
    int64_t st = 0, se = g.s_n - 1, ue = g.u_n - 1;
    while (st < g.s_n && st < g.u_n && g.S(st) == g.U(st)) ++st;
    while (st <= se && st <= ue && g.S(se) == g.U(ue)) --se, --ue;
    *start = st, *cs = se - st + 1, *cu = ue - st + 1;
}

// sizes: [0] cells of the largest LCS matrix, [1] LCS blocks at most (prefix + one per match + tail, per fragment), which also bounds the
// multiple-alignment blocks (every step of the sweep moves at least one record to its next LCS block), [2] that times the records
__global__ void rc_ma_size_kernel(RcArgs a, uint64_t *need_cells, uint64_t *need_lcs, uint64_t *need_u)
{
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rd) return;
    uint64_t cells = 0, nl = 0;
    for (uint64_t i = a.rd_beg[r]; i < a.rd_beg[r + 1]; ++i)
        for (uint64_t f = a.off[i]; f < a.off[i + 1]; ++f) {
            RcFrag g;
            if (!rc_frag(a, i, f, &g)) { atomicOr(a.err, (unsigned) RC_ERR_FRG); continue; }
            int64_t st, cs, cu;
            rc_trim(g, &st, &cs, &cu);
            if (cs > 0 && cu > 0) { const uint64_t c = (uint64_t) (cs + 1) * (uint64_t) (cu + 1); if (c > cells) cells = c; }
            nl += 2 + (uint64_t) (cs < cu? (cs > 0? cs : 0) : (cu > 0? cu : 0));
        }
    need_cells[r] = cells, need_lcs[r] = nl, need_u[r] = nl * (a.rd_beg[r + 1] - a.rd_beg[r]);
}

// find_lcs (:1681-1745) of one fragment: its merged blocks (read position << 32 | length) appended at out[*n]; false if that would pass out[lim]
__device__ bool rc_find_lcs(const RcFrag &g, uint64_t offset, int32_t *L, uint64_t *out, uint64_t *n, uint64_t lim)
{
    int64_t start, cs, cu;
    rc_trim(g, &start, &cs, &cu);
    const uint64_t p0 = *n;
    uint64_t p = p0;
    if (start > 0) { if (p >= lim) return false; out[p++] = offset << 32 | (uint64_t) start; }
    if (cs > 0 && cu > 0) {
        const int64_t w = cu + 1;
        for (int64_t j = 0; j <= cu; ++j) L[j] = 0;
        for (int64_t i = 1; i <= cs; ++i) {
            int32_t *Li = L + i * w, *Lp = Li - w;
            Li[0] = 0;
            const uint64_t si = g.S(start + i - 1);
            for (int64_t j = 1; j <= cu; ++j)
                Li[j] = si == g.U(start + j - 1)? Lp[j - 1] + 1 : (Lp[j] > Li[j - 1]? Lp[j] : Li[j - 1]);
        }
        // lcs_backtrace (:1652-1663), then array_reverse of what it pushed
        const uint64_t b0 = p;
        int64_t i = cs, j = cu;
        while (i > 0 && j > 0) {
            if (g.S(start + i - 1) == g.U(start + j - 1)) { if (p >= lim) return false; out[p++] = (uint64_t) (i - 1 + (int64_t) offset + start) << 32 | 1; --i, --j; }
            else if (L[i * w + j - 1] > L[(i - 1) * w + j]) --j;
            else --i;
        }
        for (uint64_t x = b0, y = p; x + 1 < y; ++x, --y) { const uint64_t t = out[x]; out[x] = out[y - 1]; out[y - 1] = t; }
    }
    if (start + (cs > 0? cs : 0) < g.s_n) {
        const int64_t ce = cs > 0? cs : 0;
        if (p >= lim) return false;
        out[p++] = (uint64_t) ((int64_t) offset + start + ce) << 32 | (uint64_t) (g.s_n - start - ce);
    }
    // lcs_block_merge (:1665-1678)
    if (p - p0 > 1) {
        uint64_t q = p0;
        for (uint64_t k = p0 + 1; k < p; ++k) {
            if ((out[q] >> 32) + (uint32_t) out[q] == (out[k] >> 32)) out[q] += (uint32_t) out[k];
            else out[++q] = out[k];
        }
        p = q + 1;
    }
    *n = p;
    return true;
}

__device__ __forceinline__ bool rc_shift(const RcArgs &a, uint64_t i)
{
    const uint64_t x = a.lcs[a.rec_lb[i] + a.st_lcsb[i]];
    a.st_beg[i] = x >> 32, a.st_len[i] = (uint32_t) x;
    const uint64_t f0 = a.off[i], nf = a.off[i + 1] - f0;
    while (a.st_frg[i] < nf && a.send[f0 + a.st_frg[i]] < a.st_beg[i]) ++a.st_frg[i];
    if (a.st_frg[i] >= nf) return false;
    a.st_uid[i] = (uint32_t) (a.uid[f0 + a.st_frg[i]] >> 1);
    return true;
}

__global__ void rc_ma_kernel(RcArgs a)
{
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rd) return;
    const uint64_t r0 = a.rd_beg[r], r1 = a.rd_beg[r + 1], n = r1 - r0;
    uint64_t nl = a.lcs_off[r];
    a.nb[r] = 0;
    for (uint64_t i = r0; i < r1; ++i) {
        a.rec_lb[i] = (uint32_t) nl;
        for (uint64_t f = a.off[i]; f < a.off[i + 1]; ++f) {
            RcFrag g;
            if (!rc_frag(a, i, f, &g)) { atomicOr(a.err, (unsigned) RC_ERR_FRG); return; }
            if (!rc_find_lcs(g, a.sbeg[f], a.cells + a.cell_off[r], a.lcs, &nl, a.lcs_off[r + 1])) { atomicOr(a.err, (unsigned) RC_ERR_ROOM); return; }
        }
        a.rec_ln[i] = (uint32_t) (nl - a.rec_lb[i]);
    }
    // the sweep (:1812-1858)
    for (uint64_t i = r0; i < r1; ++i) {
        if (a.rec_ln[i] == 0) return;                                   // goto ma_done: b = 0
        a.st_lcsb[i] = 0, a.st_frg[i] = 0;
        if (!rc_shift(a, i)) { atomicOr(a.err, (unsigned) RC_ERR_FRG); return; }
    }
    const uint64_t b_cap = a.blk_off[r + 1] - a.blk_off[r];
    uint32_t *mn = a.ma_n + a.blk_off[r], *mu = a.ma_u + a.u_off[r];
    uint64_t b = 0;
    while (1) {
        uint64_t s_beg = 0;
        for (uint64_t i = r0; i < r1; ++i) s_beg = s_beg > a.st_beg[i]? s_beg : a.st_beg[i];
        int m_ext = INT32_MAX;
        for (uint64_t i = r0; i < r1; ++i) {
            const int ext = (int) (a.st_len[i] - s_beg + a.st_beg[i]);
            m_ext = m_ext < ext? m_ext : ext;
        }
        if (m_ext > 0) {
            if (b >= b_cap) { atomicOr(a.err, (unsigned) RC_ERR_ROOM); a.nb[r] = (uint32_t) b; return; }
            mn[b] = (uint32_t) m_ext;
            for (uint64_t i = r0; i < r1; ++i) mu[b * n + (i - r0)] = a.st_uid[i];
            ++b;
            a.nb[r] = (uint32_t) b;
            for (uint64_t i = r0; i < r1; ++i) {
                const int ext = (int) (a.st_len[i] - s_beg + a.st_beg[i]);
                if (ext == m_ext) {
                    if (++a.st_lcsb[i] == a.rec_ln[i]) return;
                    if (!rc_shift(a, i)) { atomicOr(a.err, (unsigned) RC_ERR_FRG); return; }
                } else {
                    a.st_beg[i] = s_beg + (uint64_t) m_ext;
                    a.st_len[i] = (uint64_t) (int64_t) (ext - m_ext);
                }
            }
        } else {
            uint64_t i = r0;
            for (uint64_t j = r0 + 1; j < r1; ++j) if (a.st_beg[j] < a.st_beg[i]) i = j;
            if (++a.st_lcsb[i] == a.rec_ln[i]) return;
            if (!rc_shift(a, i)) { atomicOr(a.err, (unsigned) RC_ERR_FRG); return; }
        }
    }
}

// ---- the EM (:1983-2009) ----
// the contributions in the reference's order (read, block, member): key = unitig (n_utg for the unused slots), value = block
__global__ void rc_contrib_kernel(RcArgs a, uint32_t *key, uint32_t *val, uint32_t *blk_a)
{
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rd) return;
    const uint64_t n = a.rd_beg[r + 1] - a.rd_beg[r], b = a.nb[r];
    for (uint64_t k = 0; k < b; ++k) {
        blk_a[a.blk_off[r] + k] = (uint32_t) n;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t x = a.u_off[r] + k * n + i;
            key[x] = a.ma_u[x], val[x] = (uint32_t) (a.blk_off[r] + k);
        }
    }
}
// per contribution in unitig order: w = n[k] of a block with one member (its addend x / x * n == n is integral whenever x is positive and
// finite), 0 otherwise; fl = 1 for the others (members of blocks of two or more: fractional addends)
__global__ void rc_em_prep_kernel(uint64_t n, uint64_t n_utg, const uint32_t *key, const uint32_t *blk, const uint32_t *blk_a, const uint32_t *ma_n,
                                  uint64_t *w, uint64_t *fl)
{
    const uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const bool valid = key[c] < n_utg, single = valid && blk_a[blk[c]] == 1;
    w[c] = single? ma_n[blk[c]] : 0, fl[c] = valid && !single;
}
__global__ void rc_fpos_kernel(uint64_t n, const uint64_t *fl, const uint64_t *ef, uint64_t *fpos)
{
    const uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n && fl[c]) fpos[ef[c]] = c;
}
// s + the integral addends w[i..j) (E = exclusive prefix sums of w), each addition rounded like the reference's sequential one.  A run is
// added at once when no partial sum can round: s integral and s + I <= 2^53, or s in [2^e, 2^(e+1)) and s + I < 2^(e+1) (every partial
// sum is then a multiple of ulp(s) inside the binade).  Otherwise the longest prefix that fits is added at once, the next addend alone
// (the one rounding), and so on: a run crosses at most one binade per step.
__device__ __forceinline__ bool rc_fits(double s, uint64_t I)
{
#pragma clang fp contract(off)
    if (I == 0) return true;
    if (I >= (1ull << 53)) return false;
    if (s == floor(s)) return s <= 9007199254740992.0 && (double) I <= 9007199254740992.0 - s;
    const double lim = ldexp(1.0, ilogb(s) + 1);
    return (double) I < lim - s;
}
__device__ double rc_add_run(double s, uint64_t i, uint64_t j, const uint64_t *E)
{
#pragma clang fp contract(off)
    while (i < j) {
        if (rc_fits(s, E[j] - E[i])) return s + (double) (E[j] - E[i]);
        uint64_t lo = i, hi = j;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (rc_fits(s, E[mid] - E[i])) lo = mid; else hi = mid;
        }
        s = s + (double) (E[lo] - E[i]);
        s = s + (double) (E[lo + 1] - E[lo]);
        i = lo + 1;
    }
    return s;
}
__global__ void rc_segments_kernel(uint64_t n, uint64_t n_utg, const uint32_t *key, uint64_t *seg_beg, uint64_t *seg_end)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || key[i] >= n_utg) return;
    if (i == 0 || key[i - 1] != key[i]) seg_beg[key[i]] = i;
    if (i + 1 == n || key[i + 1] != key[i]) seg_end[key[i]] = i + 1;
}
// covt of every block: the sum over its members in order (:1990-1992)
__global__ void rc_covt_kernel(RcArgs a, const double *avg, double *covt)
{
#pragma clang fp contract(off)
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rd) return;
    const uint64_t n = a.rd_beg[r + 1] - a.rd_beg[r], b = a.nb[r];
    for (uint64_t k = 0; k < b; ++k) {
        const uint32_t *m = a.ma_u + a.u_off[r] + k * n;
        double c = 0.;
        for (uint64_t i = 0; i < n; ++i) c += avg[m[i]];
        covt[a.blk_off[r] + k] = c;
    }
}
// covs[u]: u's contributions in the reference's order (:1994-1995) -- the fractional ones one by one, the runs of integral ones between
// them by rc_add_run; x not positive and finite: all one by one.  carry (may be NULL = zeros): where every unitig's sum starts -- with reads
// sharded by record a rank's contributions are a stretch of the reference's order, and its sums go on from the previous rank's
__global__ void rc_em_kernel(uint64_t n_utg, const uint64_t *seg_beg, const uint64_t *seg_end, const uint32_t *blk, const double *covt,
                             const uint32_t *ma_n, const double *avg, const uint64_t *E, const uint64_t *ef, const uint64_t *fpos, const double *carry,
                             double *covs)
{
#pragma clang fp contract(off)
    const uint64_t u = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_utg) return;
    const double x = avg[u];
    const uint64_t c0 = seg_beg[u], c1 = seg_end[u];
    double s = carry? carry[u] : 0.;
    if (!(x > 0. && x <= DBL_MAX)) {
        for (uint64_t c = c0; c < c1; ++c) {
            const uint32_t b = blk[c];
            const double t = covt[b];
            if (t == 0.) continue;
            s += x / t * (double) ma_n[b];
        }
    } else {
        uint64_t cur = c0;
        for (uint64_t q = ef[c0], qe = ef[c1]; q < qe; ++q) {
            const uint64_t p = fpos[q];
            s = rc_add_run(s, cur, p, E);
            const uint32_t b = blk[p];
            const double t = covt[b];
            if (t != 0.) s += x / t * (double) ma_n[b];
            cur = p + 1;
        }
        s = rc_add_run(s, cur, c1, E);
    }
    covs[u] = s;
}
// the update and diff (:1998-2003), in unitig order: one workgroup, the sum by lane 0
__global__ void rc_diff_kernel(uint64_t n_utg, const uint32_t *utg_n, const double *covs, double *avg, double *diff_out)
{
#pragma clang fp contract(off)
    __shared__ double d[256];
    double diff = 0.;
    for (uint64_t j0 = 0; j0 < n_utg; j0 += 256) {
        const uint64_t j = j0 + threadIdx.x;
        if (j < n_utg) {
            const double c = covs[j] / (double) utg_n[j];
            d[threadIdx.x] = fabs(c - avg[j]);
            avg[j] = c;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint64_t m = n_utg - j0 < 256? n_utg - j0 : 256;
            for (uint64_t t = 0; t < m; ++t) diff += d[t];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *diff_out = diff;
}

// ---- third round (:2028-2039) ----
__global__ void rc_r3_kernel(RcArgs a, const double *avg, double *C)
{
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_scm) return;
    const uint64_t b = a.su_off[i], e = a.su_off[i + 1];
    if (b == e) return;
    for (uint64_t j = b; j < e; ++j) if ((a.su_uid[j] >> 1) >= a.n_utg) { atomicOr(a.err, (unsigned) RC_ERR_FRG); return; }
    double covt = 0.;
    for (uint64_t j = b; j < e; ++j) covt += avg[a.su_uid[j] >> 1];
    if (covt < DBL_EPSILON) return;
    for (uint64_t j = b; j < e; ++j) {
        const uint64_t u = a.su_uid[j] >> 1;
        if (a.su_pos[j] >= a.utg_n[u]) { atomicOr(a.err, (unsigned) RC_ERR_FRG); continue; }
        C[a.utg_off[u] + a.su_pos[j]] = avg[u] / covt * (double) a.scm_cov[i];
    }
}

// ---- scg_ra_arc_coverage's duplets (:2083-2129) ----
struct RcArcArgs {
    const uint64_t *idx_p, *idx_n, *arc_v, *arc_w, *arc_link;
    const uint8_t *arc_comp, *arc_del;
    uint64_t n_arc, n_link;
};
__device__ __forceinline__ bool rc_uniq(const RcArgs &a, uint64_t f)
{
    const uint64_t u = a.uid[f] >> 1;
    const uint64_t *v = a.utg_a + a.utg_off[u];
    const uint64_t lim = a.utg_off[u + 1] - a.utg_off[u];
    for (uint64_t s = a.ubeg[f]; s <= a.uend[f] && s < lim; ++s) {
        const uint64_t x = v[s] >> 1;
        if (x < a.n_scm && a.su_off[x + 1] - a.su_off[x] == 1) return true;
    }
    return false;
}
// event at slot f (the record's j-th fragment, j >= 1): key = link id of the arc (n_link when none), bits = l0 & 1 | (c0 == l0) << 1
__global__ void rc_duplet_kernel(RcArgs a, RcArcArgs g, uint64_t *key, uint32_t *val, uint8_t *bits, double *score_out)
{
#pragma clang fp contract(off)
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_aln; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t f0 = a.off[i], m = a.off[i + 1] - f0;
        if (m < 2) continue;
        double score = rc_frac(a.s[i]);
        if (score < DBL_EPSILON) score = 1.0;
        bool ok = true;
        for (uint64_t f = f0; f < f0 + m; ++f) if ((a.uid[f] >> 1) >= a.n_utg) ok = false;
        if (!ok) { atomicOr(a.err, (unsigned) RC_ERR_FRG); continue; }
        bool prev = score < .99? rc_uniq(a, f0) : true;
        for (uint64_t j = 1; j < m; ++j) {
            const bool cur = score < .99? rc_uniq(a, f0 + j) : true;
            const uint64_t v = a.uid[f0 + j - 1], w = a.uid[f0 + j];
            uint64_t x = g.n_arc;
            for (uint64_t t = g.idx_p[v], e = t + g.idx_n[v]; t < e && t < g.n_arc; ++t) if (g.arc_w[t] == w) { x = t; break; }   // asmg_arc
            if (x == g.n_arc) { atomicOr(a.err, (unsigned) RC_ERR_ARC); prev = cur; continue; }
            if (prev && cur) {
                const uint64_t l0 = g.arc_link[x] << 1 | g.arc_comp[x];
                const bool self = !((g.arc_v[x] ^ 1) != g.arc_w[x] || (g.arc_w[x] ^ 1) != g.arc_v[x]);      // asmg_comp_arc_id
                key[f0 + j] = g.arc_link[x], val[f0 + j] = (uint32_t) (f0 + j), bits[f0 + j] = (uint8_t) ((l0 & 1) | (self? 2 : 0));
                score_out[f0 + j] = score;
            }
            prev = cur;
        }
    }
}
// kh_dbl's puts replayed per link in read order: both keys of a link (link << 1 | 0/1) live in val2[2 * link + b], have2 says which were put.
// The replay goes on from what val2 / have2 hold: zeros, or with reads sharded by record the table as the previous rank left it
__global__ void rc_link_kernel(uint64_t n, uint64_t n_link, const uint64_t *key, const uint32_t *ev, const uint8_t *bits, const double *score,
                               double *val2, uint8_t *have2)
{
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || key[i] >= n_link || (i > 0 && key[i - 1] == key[i])) return;
    const uint64_t L = key[i];
    double v[2] = {val2[2 * L], val2[2 * L + 1]};
    bool h[2] = {have2[2 * L] != 0, have2[2 * L + 1] != 0};
    for (uint64_t c = i; c < n && key[c] == L; ++c) {
        const uint32_t e = ev[c];
        const int l = bits[e] & 1, k = (bits[e] & 2)? l : l ^ 1;
        const double sc = score[e];
        if (!h[l]) { h[l] = true, v[l] = sc; h[k] = true, v[k] = sc; }
        else { v[l] += sc; if (!h[k]) h[k] = true, v[k] = 0.; v[k] += sc; }
    }
    val2[2 * L] = v[0], val2[2 * L + 1] = v[1], have2[2 * L] = h[0], have2[2 * L + 1] = h[1];
}
// :2131-2138 before the (uint32_t): every live arc gets its l0 value or 0
__global__ void rc_arc_out_kernel(RcArcArgs g, const double *val2, const uint8_t *have2, double *out)
{
    const uint64_t x = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= g.n_arc) return;
    if (g.arc_del[x]) { out[x] = 0.; return; }
    const uint64_t l0 = g.arc_link[x] << 1 | g.arc_comp[x];
    out[x] = have2[l0]? val2[l0] : 0.;
}

}  // namespace oatk
