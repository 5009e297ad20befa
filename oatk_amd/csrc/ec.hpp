// oatk_amd/csrc/ec.hpp -- per-read syncmer-chain error correction on the device.
//
// Replaces, on flat arrays that stay resident in HBM:
//   find_error_syncmers            syncerr.c:679-757   -> ec_mark_kernel, ec_arc_del_kernel
//   error blocks of a read         syncerr.c:339-612   -> ec_blocks, ec_blocks_wave (device functions)
//   dfs_search + wf_ed_core        syncerr.c:144-286, levdist.c:75-310 -> ec_wave_kernel (ec_wave.hpp)
//   update_syncmer_db              syncerr.c:769-814   -> a stable radix sort of (syncmer, occurrence) pairs + ec_cov_runs_kernel, ec_del_kernel (api_ec.inc)
//
// The graph is the reference's asmg_t in arc-array order (sorted (v,w), graph.c:70-83) as CSR over oriented vertices.
// Every vertex is one syncmer (utg id == syncmer id, syncerr.c:421-423) and its hoco consensus is the oriented k-mer of
// the syncmer's first occurrence (scg_syncmer_consensus in hoco mode, syncasm.c:910-940) -- so no 1002-byte string per
// vertex is materialised: bases are read in place from the resident hoco strings of the reads.
//
// Mapping: error blocks of one read are independent (they are delimited on the ORIGINAL chain), so the unit of work is
// one block: a depth-first search over the good-syncmer graph that extends a consensus string arc by arc and re-aligns
// it to the read segment with a resumable Landau-Vishkin wavefront.  One WAVE solves one block (ec_wave.hpp).
#pragma once
#include "common.hpp"

namespace oatk {

#define EC_FAILURE 0
#define EC_SUCCESS 1
#define EC_AMBISNQ 2
#define EC_AMBISEQ 3
#define EC_MAX_DFS_PATH 10000
#define EC_MIN_ERR_SEQ_LEN 10
#define EC_MIN_ERR_BASE 6
#define EC_NONE 0xFFFFFFFFFFFFFFFFULL

struct EcGraph {
    uint64_t n_vtx, n_arc;
    const uint64_t *idx_p;        // [2 n_vtx] first arc of an oriented vertex
    const uint32_t *idx_n;        // [2 n_vtx] arc count
    const uint64_t *arc_v, *arc_w;
    const uint32_t *arc_ls, *arc_cov;
    uint8_t *arc_del;
    uint8_t *scm_del;             // [n_vtx]
    const uint32_t *scm_cov;
    const uint64_t *scm_s;
    // where the bases of a vertex live: byte offset of the read's hoco string, and pos << 1 | rev on it
    const uint64_t *vtx_hs_off;
    const uint32_t *vtx_mpos;
    const uint8_t *other;         // light graph (ecgraph.hpp): [2 n_vtx] the oriented vertex has arcs that were never materialised; else null
};

struct EcReads {
    uint64_t n_reads, sid0;
    int K;
    const uint8_t *hoco_s;
    const uint64_t *off;          // packed-stream offsets; hoco string of read r at off[r] / 4
    const uint32_t *hoco_l;
    const uint64_t *scm_off;      // [n_reads + 1] slots of the per-read chains
    const uint64_t *k_mer;        // id << 1 (| corrected)
    const uint32_t *m_pos;
};

// ---- find_error_syncmers, first loop (syncerr.c:690-718) ----
__global__ void ec_mark_kernel(EcGraph g, uint32_t err_mer_c, uint32_t max_err_c, uint32_t err_arc_c, double max_arc_f)
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n_vtx) return;
    if (g.scm_del[i] || g.scm_cov[i] >= max_err_c) return;
    if (g.scm_cov[i] < err_mer_c) { g.scm_del[i] = 1; return; }
    const uint32_t nv = g.scm_cov[i];
    int b[2] = {-1, -1};
    for (int k = 0; k < 2; ++k) {
        const uint64_t v = i << 1 | (uint64_t) k, p = g.idx_p[v];
        const uint32_t na = g.idx_n[v];
        uint32_t live = 0;
        for (uint32_t j = 0; j < na; ++j) live += !g.arc_del[p + j];
        if (!live && !(g.other && g.other[v])) continue;
        b[k] = 0;
        for (uint32_t j = 0; j < na; ++j) {
            if (g.arc_del[p + j]) continue;
            const uint32_t nw = g.scm_cov[g.arc_w[p + j] >> 1], mn = nv < nw? nv : nw, ac = g.arc_cov[p + j];
            if (ac >= err_arc_c && (double) ac >= (double) mn * max_arc_f) { b[k] = 1; break; }
        }
    }
    if (!b[0] || !b[1]) g.scm_del[i] = 1;
}

// asmg_vtx_del for every marked syncmer (syncerr.c:748-752, graph.h:101-122): in a symmetric graph that is every arc
// with a deleted endpoint.  Runs after ec_mark_kernel has finished (the marking reads the ORIGINAL arc flags).
__global__ void ec_arc_del_kernel(EcGraph g)
{
    uint64_t a = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= g.n_arc) return;
    if (g.scm_del[g.arc_v[a] >> 1] || g.scm_del[g.arc_w[a] >> 1]) g.arc_del[a] = 1;
}

// where each vertex's k-mer can be read: its first occurrence (syncasm.c:910-926; nothing is corrected yet)
// (sharded reads: `l2g` maps the shard's syncmer ids to the global ids the graph is built on; vertices this shard never saw
// keep EC_NO_SRC until their k-mer is imported)
#define EC_NO_SRC 0xFFFFFFFFFFFFFFFFULL
__global__ void ec_vtx_src_kernel(uint64_t n_local, const uint64_t *scm_loc, const uint32_t *l2g, uint64_t *vtx_hs_off, uint32_t *vtx_mpos)
{
    // scm_loc (count.hpp: the locator of a syncmer's first occurrence) = (32-bit word index of the read's hoco string) << 32 | pos << 1 | rev
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_local) return;
    const uint64_t loc = scm_loc[i], v = l2g? l2g[i] : i;
    vtx_hs_off[v] = (loc >> 32) << 2;
    vtx_mpos[v] = (uint32_t) loc;
}
__global__ void ec_remap_kernel(uint64_t n, const uint64_t *k_mer, const uint32_t *l2g, uint64_t *out)
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint64_t) l2g[k_mer[i] >> 1] << 1 | (k_mer[i] & 1ULL);
}

__device__ __forceinline__ uint32_t hoco_base(const uint8_t *hs, uint32_t p)
{
    return (hs[p >> 2] >> (((p & 3u) ^ 3u) << 1)) & 3u;
}

// ---- one error block of a read ----
struct EcBlock {
    uint64_t beg_utg, end_utg;    // source / sink oriented vertices (EC_NONE = open end)
    uint32_t beg_pos;             // first base of the read segment (hoco)
    int32_t l;                    // its length
    int32_t beg, end;             // chain indices: left anchor (after adjustment) and right anchor
    int32_t r;                    // 1 = leading block, solved on the reverse complement
};

// Walks the blocks of one read exactly like the loop at syncerr.c:394-598 and calls
//   on_block(k, blk)                 for the k-th block that has an anchor, and
//   on_copy(first, last_exclusive)   for every run of original chain entries that is kept as is.
// Returns the number of blocks, or -1 when the read has no good syncmer at all (it is then left untouched).
template <class FB, class FC>
__device__ int ec_blocks(const uint8_t *scm_del, const uint64_t *km, const uint32_t *mp, int32_t n, uint32_t hoco_l, int K, FB on_block, FC on_copy)
{
    int32_t beg = -1, end, nb = 0;
    bool updated = true;
    for (;;) {
        uint32_t beg_pos = beg < 1? 0u : (mp[beg - 1] >> 1) + (uint32_t) K;
        beg_pos += EC_MIN_ERR_SEQ_LEN;
        for (end = beg + 1; end < n; ++end)
            if (!scm_del[km[end] >> 1] && !(km[end] & 1ULL) && (mp[end] >> 1) >= beg_pos) break;
        if (beg >= 0 || end < n) {
            EcBlock b;
            if (beg < 0) {
                beg = end;
                b.beg_utg = (km[beg] & ~1ULL) | (uint64_t) !(mp[beg] & 1u);
                b.beg_pos = 0, b.end_utg = EC_NONE, b.l = (int32_t) (mp[beg] >> 1), b.r = 1;
            } else {
                --beg;
                b.beg_utg = (km[beg] & ~1ULL) | (mp[beg] & 1u);
                b.beg_pos = (mp[beg] >> 1) + (uint32_t) K;
                if (end >= n) b.end_utg = EC_NONE, b.l = (int32_t) hoco_l - (int32_t) b.beg_pos;
                else b.end_utg = (km[end] & ~1ULL) | (mp[end] & 1u), b.l = (int32_t) (mp[end] >> 1) - (int32_t) b.beg_pos;
                b.r = 0;
            }
            b.beg = beg, b.end = end;
            on_block(nb, b);
            ++nb;
        } else {
            updated = false;
        }
        for (beg = end + 1; beg < n; ++beg)
            if (scm_del[km[beg] >> 1] || (km[end] & 1ULL)) break;     // [end], as written in the reference (syncerr.c:579)
        if (beg > n) break;
        on_copy(end, beg);
    }
    return updated? nb : -1;
}

struct EcBlockOut {
    uint32_t status;              // EC_*; EC_FAILURE also for blocks shorter than EC_MIN_ERR_SEQ_LEN
    uint32_t np;                  // entries of the optimum path
    uint64_t path_off;            // into the path pool
    uint32_t flags;               // 1 = did not fit the scratch slab (must be re-run with a large one)
    uint32_t short_block;         // 1 = l < EC_MIN_ERR_SEQ_LEN (stats[10])
    uint32_t tried, n_path;       // the search's effort: arcs followed (DFS steps), dead ends counted (syncerr.c:147) -- OATK_BUF_EC_BLOCK_OUT
    uint32_t wf_steps, wf_diag;   // ... wavefront steps taken, and the diagonals they covered in all (>> 6: units of 64)
    uint32_t ticks, tier;         // ... the time the wave that finished the block spent on it (s_memrealtime, 100 MHz), and the tier it ran in
};

// The arcs the search may follow: the graph's arc array with the deleted arcs squeezed out (same order), each carrying
// what the search needs to know about its target, so that one 32-byte load per arc is the only graph access.  At high
// coverage a good syncmer has thousands of deleted arcs to one-off error syncmers; the search never sees them.
struct __attribute__((aligned(32))) EcLiveArc {
    uint32_t w, ls;               // target oriented vertex, overlap
    uint32_t hs16, mpos;          // the target's k-mer: hoco byte offset / 16 of its read, pos << 1 | rev on it
    uint32_t lp, ln;              // the target's own live arcs
    uint32_t pad[2];
};
struct EcLive {
    const uint32_t *idx_p, *idx_n;  // [2 n_vtx] first live arc / live arc count of an oriented vertex
    const EcLiveArc *arc;
};

struct __attribute__((aligned(16))) EcWork {   // one block, self-contained for the solver
    uint64_t beg_utg, end_utg;
    uint32_t read, beg_pos;
    int32_t l, r;
    uint32_t hs16;                // hoco byte offset / 16 of the read
    uint32_t lp, ln;              // live arcs of beg_utg
    uint32_t pad;                 // chain entries the read keeps if this block is NOT corrected (syncerr.c:533-542); nothing on the device reads it any more
};

// What the assembly needs of a block besides its outcome, left by the walk that stages the blocks (one per EcWork, same index): the chain indices that
// delimit it (EcBlock::beg, EcBlock::end cut at the chain's length) and two flags (EcBlock::r, an open end).  With them the corrected chain is a table of segments -- per block the originals kept in front of it, then its body (the optimum path's
// interior, or the originals it keeps) -- and nobody walks the chain again (ec_new_n_seg_kernel, ec_assemble_seg_kernel).
#define EC_SEG_R 1u               // leading block (EcBlock::r)
#define EC_SEG_OPEN 2u            // end_utg == EC_NONE
struct EcSeg {
    uint32_t beg;                 // EcBlock::beg
    uint32_t end_fl;              // min(EcBlock::end, n) << 2 | EC_SEG_*
};
__device__ __forceinline__ EcSeg ec_seg_of(const EcBlock &b, int32_t n)
{
    EcSeg d;
    d.beg = (uint32_t) b.beg;
    d.end_fl = (uint32_t) (b.end < n? b.end : n) << 2 | (b.end_utg == EC_NONE? EC_SEG_OPEN : 0u) | (b.r? EC_SEG_R : 0u);
    return d;
}
// original entries kept in front of a block: from the end of the block before it (0 for the first) up to and including its left anchor -- what on_copy sees
// between two blocks (ec_blocks: [end, beg) with beg one past the next block's anchor); a leading block starts the chain and has nothing in front
__device__ __forceinline__ uint32_t ec_seg_front(const EcSeg &d, uint32_t prev_end)
{
    return (d.end_fl & EC_SEG_R) || d.beg + 1u <= prev_end? 0u : d.beg + 1u - prev_end;
}
// entries a block contributes itself: the optimum path's interior (syncerr.c:513-532), or the originals it keeps when it is not corrected (:533-542)
__device__ __forceinline__ uint32_t ec_seg_body(const EcSeg &d, uint32_t status, uint32_t np_)
{
    const int32_t np = (int32_t) np_, beg = (int32_t) d.beg, end = (int32_t) (d.end_fl >> 2);
    if (status == EC_SUCCESS) return d.end_fl & EC_SEG_R? (uint32_t) (np >= 1? np - 1 : 0) : (uint32_t) ((np >= 2? np - 2 : 0) + ((d.end_fl & EC_SEG_OPEN) && np > 1? 1 : 0));
    if (d.end_fl & EC_SEG_R) return (uint32_t) beg;                     // copy(0, beg)
    return end > beg + 1? (uint32_t) (end - beg - 1) : 0u;             // copy(beg + 1, min(end, n)), which is empty when beg + 1 >= n
}

__global__ void ec_live_flag_kernel(uint64_t n_arc, const uint8_t *arc_del, uint32_t *live)
{
    uint64_t a = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (a < n_arc) live[a] = !arc_del[a];
}
// ... and whether the live graph BRANCHES anywhere: *branches becomes nonzero when some oriented vertex has more than one live arc out (api_ec.inc: a graph that
// does not is searched by walking, and the solver without budgets and second stage is the faster one for it)
__global__ void ec_live_idx_kernel(uint64_t n_ovtx, const uint64_t *idx_p, const uint32_t *idx_n, const uint64_t *live_off, uint32_t *lidx_p, uint32_t *lidx_n, uint32_t *branches)
{
    uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_ovtx) return;
    const uint32_t n = idx_n[v];
    const uint64_t p = n? live_off[idx_p[v]] : 0;
    const uint32_t ln = n? (uint32_t) (live_off[idx_p[v] + n] - p) : 0u;
    lidx_p[v] = (uint32_t) p, lidx_n[v] = ln;
    if (ln > 1u && *(volatile uint32_t *) branches == 0u) atomicOr(branches, 1u);       // (read first: a graph may have millions of them, and they would all queue on one address)
}
__global__ void ec_live_arc_kernel(uint64_t n_arc, const uint8_t *arc_del, const uint64_t *live_off, const uint64_t *arc_w, const uint32_t *arc_ls,
                                   const uint64_t *vtx_hs_off, const uint32_t *vtx_mpos, const uint32_t *lidx_p, const uint32_t *lidx_n, EcLiveArc *larc,
                                   uint32_t *no_src)
{
    uint64_t a = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_arc || arc_del[a]) return;
    const uint64_t w = arc_w[a];
    if (vtx_hs_off[w >> 1] == EC_NO_SRC) *no_src = 1u;          // sharded reads: the k-mer of a live vertex was never imported
    EcLiveArc x;
    x.w = (uint32_t) w, x.ls = arc_ls[a], x.hs16 = (uint32_t) (vtx_hs_off[w >> 1] >> 4), x.mpos = vtx_mpos[w >> 1];
    x.lp = lidx_p[w], x.ln = lidx_n[w], x.pad[0] = x.pad[1] = 0;
    larc[live_off[a]] = x;
}

// ---- assemble the corrected chains (syncerr.c:513-542, :585-612) ----
struct EcAssembleArgs {
    EcReads rd;
    const uint8_t *scm_del;
    const uint64_t *scm_s;
    const uint64_t *blk_off;
    const EcBlockOut *out;
    const uint64_t *path_pool;
    uint32_t *new_n;              // [n_reads]
    const uint64_t *new_off;      // [n_reads + 1]
    uint64_t *new_k_mer, *new_s_mer;
    uint32_t *new_m_pos;
    uint32_t *key_id;             // the (syncmer, occurrence) pairs update_syncmer_db sorts, written along with the chains
    uint64_t *val_occ;
    uint64_t sid0;
    const uint64_t *old_s_mer;
    unsigned long long *stats;    // [11]
    int pass;
    const EcSeg *seg;             // [n_work] (ec_assemble_seg_kernel)
    const uint8_t *keep_all;      // [n_reads] 1 = the read has no good syncmer and keeps its chain (ec_assemble_seg_kernel)
};

// ---------------------------------------------------------------------------------------------------------------------------------
// The same walk with ONE WAVE PER READ.  A HiFi read carries a few dozen syncmers, so its whole chain sits in the lanes of a wave: lane j
// holds entry j, the two searches of the loop at syncerr.c:394-598 ("first good syncmer at or beyond a position", "first deleted syncmer
// after it") are one ballot and a count-trailing-zeros each, and everything the callbacks write goes out with the lanes side by side
// instead of one lane striding through its own read.  ec_stage_blocks_wave_kernel uses it, and the lane-per-read version above remains for
// reads with more than 64 syncmers (lane 0 runs it).
// ---------------------------------------------------------------------------------------------------------------------------------
// entry `lane` of v, in a scalar register: `lane` is the same in every active lane of the wave wherever these are called, so it goes to an SGPR and v_readlane
// takes the value (a __shfl is a ds_bpermute, a wait on LDS and a v_readfirstlane -- inside the walk's serial loop)
__device__ __forceinline__ int32_t ecr_s(int32_t v) { return wave_uniform(v); }
__device__ __forceinline__ uint32_t ecr_u32(uint32_t v, int lane) { return wave_read(v, lane); }
__device__ __forceinline__ uint64_t ecr_u64(uint64_t v, int lane) { return (uint64_t) ecr_u32((uint32_t) (v >> 32), lane) << 32 | ecr_u32((uint32_t) v, lane); }
__device__ __forceinline__ uint64_t ecr_above(int32_t j) { return j < 0? ~0ULL : (j >= 63? 0ULL : ~0ULL << (j + 1)); }      // lanes > j

// km, mp, del: this lane's chain entry (lane < n <= 64); every argument of the callbacks is wave-uniform.  The whole wave walks (lanes at or beyond n
// stay active) and n is the read's, so beg, end, nb and everything the loop branches on -- ballots, their trailing-zero counts, broadcast entries -- are the
// same in every lane: ecr_s says so where such a value enters the loop, and the loop's state then lives in scalar registers
template <class FB, class FC>
__device__ int ec_blocks_wave(int lane, int32_t n_, uint64_t km, uint32_t mp, bool del, uint32_t hoco_l, int K, FB on_block, FC on_copy)
{
    const int32_t n = ecr_s(n_);
    const bool in = lane < n;
    const uint64_t goodm = __ballot(in && !del && !(km & 1ULL)), delm = __ballot(in && del);
    const uint32_t pos = mp >> 1;
    int32_t beg = -1, end, nb = 0;
    bool updated = true;
    for (;;) {
        uint32_t beg_pos = beg < 1? 0u : ecr_u32(pos, beg - 1) + (uint32_t) K;
        beg_pos += EC_MIN_ERR_SEQ_LEN;
        const uint64_t m = __ballot(pos >= beg_pos) & goodm & ecr_above(beg);
        end = ecr_s(m? (int32_t) __builtin_ctzll(m) : (beg + 1 < n? n : beg + 1));
        if (beg >= 0 || end < n) {
            EcBlock b;
            if (beg < 0) {
                beg = end;
                const uint64_t kb = ecr_u64(km, beg);
                const uint32_t mb = ecr_u32(mp, beg);
                b.beg_utg = (kb & ~1ULL) | (uint64_t) !(mb & 1u);
                b.beg_pos = 0, b.end_utg = EC_NONE, b.l = (int32_t) (mb >> 1), b.r = 1;
            } else {
                --beg;
                const uint64_t kb = ecr_u64(km, beg);
                const uint32_t mb = ecr_u32(mp, beg);
                b.beg_utg = (kb & ~1ULL) | (mb & 1u);
                b.beg_pos = (mb >> 1) + (uint32_t) K;
                if (end >= n) b.end_utg = EC_NONE, b.l = (int32_t) hoco_l - (int32_t) b.beg_pos;
                else {
                    const uint64_t ke = ecr_u64(km, end);
                    const uint32_t me = ecr_u32(mp, end);
                    b.end_utg = (ke & ~1ULL) | (me & 1u), b.l = (int32_t) (me >> 1) - (int32_t) b.beg_pos;
                }
                b.r = 0;
            }
            b.beg = beg, b.end = end;
            on_block(nb, b);
            ++nb;
        } else {
            updated = false;
        }
        if (end + 1 < n) {
            if (ecr_u64(km, end) & 1ULL) beg = end + 1;                   // [end], as written in the reference (syncerr.c:579)
            else { const uint64_t m2 = delm & ecr_above(end); beg = m2? (int32_t) __builtin_ctzll(m2) : n; }
        } else {
            beg = end + 1;
        }
        beg = ecr_s(beg);
        if (beg > n) break;
        on_copy(end, beg);
    }
    return updated? nb : -1;
}

// A wave takes ECR_RPW consecutive reads: everything the walks need of them is requested first (the loads of all of them are in flight
// together), then the reads are walked one after the other.  Measured at config 3 (2 M reads, on the walks of that time: DESIGN.md 7): two
// reads per wave were no faster than one -- the walks are not bound by the rate at which waves launch but by what each does once its
// data is there -- so a wave takes ONE read.
#ifndef ECR_RPW
#define ECR_RPW 1
#endif
#define ECR_READS_PER_BLOCK (4 * ECR_RPW)

struct EcrRead {                  // one read of the wave's, as the lanes hold it
    uint64_t r, o;
    int32_t n;                    // -1: no such read
    uint64_t km;
    uint32_t mp, hoco_l;
    bool del;
};
__device__ __forceinline__ void ecr_load(const EcReads &rd, const uint8_t *scm_del, uint64_t r0, int lane, EcrRead (&q)[ECR_RPW])
{
#pragma unroll
    for (int k = 0; k < ECR_RPW; ++k) {
        q[k].r = r0 + k;
        const bool live = q[k].r < rd.n_reads;
        q[k].o = live? rd.scm_off[q[k].r] : 0;
        q[k].n = live? (int32_t) (rd.scm_off[q[k].r + 1] - q[k].o) : -1;
        q[k].hoco_l = live? rd.hoco_l[q[k].r] : 0;
    }
#pragma unroll
    for (int k = 0; k < ECR_RPW; ++k) {
        const bool in = q[k].n >= 0 && q[k].n <= 64 && lane < q[k].n;
        q[k].km = in? rd.k_mer[q[k].o + lane] : 0;
        q[k].mp = in? rd.m_pos[q[k].o + lane] : 0;
    }
#pragma unroll
    for (int k = 0; k < ECR_RPW; ++k) q[k].del = q[k].n >= 0 && q[k].n <= 64 && lane < q[k].n && scm_del[q[k].km >> 1];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The blocks listed in ONE walk (r16).  The walk that counts a read's blocks cannot write a block where it belongs -- blk_off[r] is a scan away -- but it finds
// out everything there is to know: copy_n and keep_all need nothing from the scan, and a block is the 8 bytes of its EcSeg (EcBlock::beg and EcBlock::end, the
// chain indices of its anchors, and the flags for EcBlock::r and an open end; every other field of its EcWork is a function of the chain entries at those two
// indices).  So the walk leaves the descriptors in a staging array at a place known beforehand, and a kernel without a walk in it builds the work items
// behind the scan (ec_fill_work_kernel).
//
// Staging: read r owns the n + 1 entries from scm_off[r] + r on, n = its chain's length.  That is enough: a round of the walk yields at most one block and
// moves `beg` on (-1, then end + 1 >= 1, then at least two further each round) until it exceeds n -- at most n + 1 rounds.  A block beyond that, or beyond
// the array, is not written and raises *overflow, and the call fails.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ec_stage_blocks_wave_kernel(EcReads rd, const uint8_t *scm_del, uint32_t *n_blocks, uint32_t *copy_n, uint8_t *keep_all, EcSeg *stage,
                                                                   uint64_t stage_cap, uint32_t *overflow)
{
    const uint64_t r0 = ((uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * ECR_RPW;
    const int lane = threadIdx.x & 63;
    if (r0 >= rd.n_reads) return;
    EcrRead q[ECR_RPW];
    ecr_load(rd, scm_del, r0, lane, q);
#pragma unroll
    for (int k = 0; k < ECR_RPW; ++k) {
        const EcrRead &x = q[k];
        if (x.n < 0) continue;
        const int32_t n = x.n;
        const uint64_t s0 = x.o + x.r;                   // the read's first staging entry
        auto put = [&](int i, const EcBlock &b) {
            if (i <= n && s0 + (uint64_t) i < stage_cap) stage[s0 + (uint64_t) i] = ec_seg_of(b, n); else *overflow = 1u;
        };
        // what the assembly copies between the blocks whatever becomes of them; a read without a good syncmer keeps its chain (syncerr.c:562-572)
        uint32_t cp = 0;
        auto on_copy = [&](int32_t first, int32_t last) { if (last > first) cp += (uint32_t) (last - first); };
        if (n > 64) {
            if (lane == 0) {
                const int nbs = ec_blocks(scm_del, rd.k_mer + x.o, rd.m_pos + x.o, n, x.hoco_l, rd.K, put, on_copy);
                n_blocks[x.r] = nbs < 0? 0u : (uint32_t) nbs;
                copy_n[x.r] = nbs < 0? (uint32_t) n : cp;
                keep_all[x.r] = nbs < 0;
            }
            continue;
        }
        // lane i keeps block i and writes it after the walk (n <= 64: at most 65 blocks, and lane 0 writes the 65th on the spot)
        EcBlock mine;
        mine.beg_utg = 0, mine.end_utg = 0, mine.beg_pos = 0, mine.l = 0, mine.beg = 0, mine.end = 0, mine.r = 0;
        int nb = 0;
        const int res = ec_blocks_wave(lane, n, x.km, x.mp, x.del, x.hoco_l, rd.K,
                                       [&](int i, const EcBlock &b) { ++nb; if (i < 64) { if (lane == i) mine = b; } else if (lane == 0) put(i, b); }, on_copy);
        if (lane < nb) put(lane, mine);
        if (lane == 0) n_blocks[x.r] = (uint32_t) nb, copy_n[x.r] = res < 0? (uint32_t) n : cp, keep_all[x.r] = res < 0;
    }
}

// The work item of a block from its staged descriptor: beg_utg, end_utg, beg_pos, l and r as the walk's EcBlock has them, read back from the chain entries at
// the descriptor's two indices (ec_blocks: the three cases -- leading, open, closed); `pad` from EcBlock::beg and EcBlock::end alone.
// o, n: the read's chain; d: the block's staged descriptor.
__device__ __forceinline__ EcWork ec_work_of(const EcReads &rd, const EcLive &lv, uint64_t r, uint64_t o, int32_t n, const EcSeg &d)
{
    const int32_t beg = (int32_t) d.beg, end = (int32_t) (d.end_fl >> 2);       // end: min(EcBlock::end, n)
    const uint64_t kb = rd.k_mer[o + d.beg];
    const uint32_t mb = rd.m_pos[o + d.beg];
    EcWork y;
    y.read = (uint32_t) r, y.hs16 = (uint32_t) (rd.off[r] >> 6);
    if (d.end_fl & EC_SEG_R) {
        y.beg_utg = (kb & ~1ULL) | (uint64_t) !(mb & 1u);
        y.beg_pos = 0, y.end_utg = EC_NONE, y.l = (int32_t) (mb >> 1), y.r = 1;
        y.pad = d.beg;
    } else {
        y.beg_utg = (kb & ~1ULL) | (mb & 1u);
        y.beg_pos = (mb >> 1) + (uint32_t) rd.K;
        if (d.end_fl & EC_SEG_OPEN) y.end_utg = EC_NONE, y.l = (int32_t) rd.hoco_l[r] - (int32_t) y.beg_pos;
        else {
            const uint64_t ke = rd.k_mer[o + (uint32_t) end];
            const uint32_t me = rd.m_pos[o + (uint32_t) end];
            y.end_utg = (ke & ~1ULL) | (me & 1u), y.l = (int32_t) (me >> 1) - (int32_t) y.beg_pos;
        }
        y.r = 0;
        y.pad = beg + 1 < n && end > beg + 1? (uint32_t) (end - beg - 1) : 0u;
    }
    y.lp = lv.idx_p[y.beg_utg], y.ln = lv.idx_n[y.beg_utg];
    return y;
}

// The work items and the descriptors at their places: a workgroup per 256 reads, its lanes side by side over their blocks -- the 257 offsets sit in LDS and a lane
// finds its block's read by bisection -- so the 48-byte items leave in order and every lane has a block.  (A lane per read looping over its blocks, 3.9 on
// average, was built and measured beside it: the `ec_mark` timer 2.26 ms against 1.80 at config 3, profiles/r16a_fill_layout.txt)
__global__ __launch_bounds__(256) void ec_fill_work_kernel(EcReads rd, EcLive lv, const uint64_t *blk_off, const EcSeg *stage, EcWork *work, EcSeg *seg)
{
    __shared__ uint64_t offs[257];
    const uint64_t r0 = (uint64_t) blockIdx.x * 256;
    for (uint32_t t = threadIdx.x; t < 257; t += 256) offs[t] = blk_off[r0 + t < rd.n_reads? r0 + t : rd.n_reads];
    __syncthreads();
    for (uint64_t j = offs[0] + threadIdx.x; j < offs[256]; j += 256) {
        uint32_t lo = 0, hi = 256;                       // the last read with offs[.] <= j
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (offs[mid] <= j) lo = mid; else hi = mid; }
        const uint64_t r = r0 + lo, o = rd.scm_off[r];
        const EcSeg d = stage[o + r + (j - offs[lo])];
        work[j] = ec_work_of(rd, lv, r, o, (int32_t) (rd.scm_off[r + 1] - o), d);
        seg[j] = d;
    }
}

// stats[11] of read_error_correction (syncerr.c:502-504, :513-542) from the solved blocks; a small fixed grid strides over them and every
// workgroup adds its eleven sums once (eleven addresses take atomics one at a time: 90 k of them cost 0.4 ms, 3 k nothing)
__global__ __launch_bounds__(256) void ec_block_stats_kernel(const EcWork *work, const EcBlockOut *out, uint64_t n_work, unsigned long long *stats)
{
    __shared__ uint32_t part[4][11];
    uint32_t loc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_work; i += (uint64_t) gridDim.x * blockDim.x) {
        const EcBlockOut x = out[i];
        if (x.short_block) ++loc[10];
        else if (work[i].end_utg == EC_NONE) ++loc[0], ++loc[1 + x.status];
        else ++loc[5], ++loc[6 + x.status];
    }
    for (int i = 0; i < 11; ++i) {
        uint32_t v = loc[i];
        for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 11) {
        const uint32_t v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v) atomicAdd(&stats[threadIdx.x], (unsigned long long) v);
    }
}

// one read, lane-serial, by a walk of its own over the chain: reads with more than 64 syncmers or blocks (ec_assemble_seg_read hands them over)
__device__ inline void ec_assemble_read_serial(const EcAssembleArgs &a, uint64_t r)
{
    const uint64_t o = a.rd.scm_off[r];
    const int32_t n = (int32_t) (a.rd.scm_off[r + 1] - o);
    const uint64_t *km = a.rd.k_mer + o;
    const uint32_t *mp = a.rd.m_pos + o;
    const EcBlockOut *bo = a.out + a.blk_off[r];
    uint64_t wpos = a.pass? a.new_off[r] : 0;
    const uint64_t w0 = wpos;
    uint32_t cnt = 0;
    auto put = [&](uint64_t k, uint32_t m) {
        if (a.pass) {
            a.new_k_mer[wpos] = k, a.new_m_pos[wpos] = m, a.new_s_mer[wpos] = a.scm_s[k >> 1];
            a.key_id[wpos] = (uint32_t) (k >> 1), a.val_occ[wpos] = (a.sid0 + r) << 32 | (wpos - w0) << 1 | (m & 1u);
            ++wpos;
        }
        ++cnt;
    };
    int nb = ec_blocks(a.scm_del, km, mp, n, a.rd.hoco_l[r], a.rd.K,
        [&](int k, const EcBlock &b) {
            const EcBlockOut &x = bo[k];
            if (x.status == EC_SUCCESS) {
                const uint64_t *path = a.path_pool + x.path_off;
                const int32_t np = (int32_t) x.np;
                if (b.r) {
                    for (int32_t j = np - 1; j > 0; --j) put((path[j] & ~1ULL) | 1ULL, 0xFFFFFFFFu ^ (uint32_t) (path[j] & 1ULL));
                } else {
                    int32_t j;
                    for (j = 1; j < np - 1; ++j) put((path[j] & ~1ULL) | 1ULL, 0xFFFFFFFEu | (uint32_t) (path[j] & 1ULL));
                    if (b.end_utg == EC_NONE && np > 1) put((path[j] & ~1ULL) | 1ULL, 0xFFFFFFFEu | (uint32_t) (path[j] & 1ULL));
                }
            } else if (b.r) {
                for (int32_t j = 0; j < b.beg; ++j) put(km[j], mp[j]);
            } else if (b.beg + 1 < n) {
                for (int32_t j = b.beg + 1; j < b.end; ++j) put(km[j], mp[j]);
            }
        },
        [&](int32_t first, int32_t last) { for (int32_t j = first; j < last; ++j) put(km[j], mp[j]); });
    if (nb < 0) {
        if (a.pass) {
            uint64_t q = a.new_off[r];
            for (int32_t j = 0; j < n; ++j) {
                a.new_k_mer[q + j] = km[j], a.new_m_pos[q + j] = mp[j], a.new_s_mer[q + j] = a.old_s_mer[o + j];
                a.key_id[q + j] = (uint32_t) (km[j] >> 1), a.val_occ[q + j] = (a.sid0 + r) << 32 | (uint64_t) j << 1 | (mp[j] & 1u);
            }
        }
        cnt = (uint32_t) n;
    }
    if (!a.pass) a.new_n[r] = cnt;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The corrected chains WITHOUT a walk: from the descriptors the block walk left (EcSeg) and the blocks' outcomes.  A read with blocks 0 .. nb - 1 becomes
//   front(0) body(0) front(1) body(1) ... front(nb - 1) body(nb - 1)
// front(i) = the originals [end(i - 1), beg(i)] (ec_seg_front), body(i) = ec_seg_body entries; the last block of a read always ends at or beyond n (the walk
// leaves its loop nowhere else), so nothing follows it.  A read without a block is one without a good syncmer (the first round of the walk either finds the
// leading block or gives the read up) and keeps its chain; the block walk says so in keep_all[] all the same.
// ---------------------------------------------------------------------------------------------------------------------------------
// the chains' lengths: a lane per read over its blocks' 8-byte descriptors and outcomes
__global__ __launch_bounds__(256) void ec_new_n_seg_kernel(uint64_t n_reads, const uint32_t *copy_n, const uint64_t *blk_off, const EcSeg *seg, const EcBlockOut *out, uint32_t *new_n)
{
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t b0 = blk_off[r], b1 = blk_off[r + 1];
    if (b0 == b1) { new_n[r] = copy_n[r]; return; }         // no block: what the walk kept (the whole chain)
    uint32_t s = 0, prev_end = 0;
    for (uint64_t i = b0; i < b1; ++i) {
        const EcSeg d = seg[i];
        s += ec_seg_front(d, prev_end) + ec_seg_body(d, out[i].status, out[i].np);
        prev_end = d.end_fl >> 2;
    }
    new_n[r] = s;
}

// inclusive wave sum by DPP (rows of sixteen, then row_bcast 15 and 31); every lane of the wave must be active
__device__ __forceinline__ uint32_t ecr_incl_sum(uint32_t v)
{
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x111, 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x112, 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x114, 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x118, 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x142, 0xa, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x143, 0xc, 0xf, false);
    return v;
}

// One wave per read, lane i holds chain entry i AND block i.  Two prefix sums over the blocks give every segment's place (all entries) and every path
// interior's place among the path entries; a lane then finds the block its chain entry belongs to by comparing its index with the blocks' boundaries and
// writes the entry if it stays, and the path interiors of all solved blocks of the read are copied together, 64 entries at a time.  Reads with more than 64
// syncmers or blocks, and reads with neither a block nor keep_all, take ec_assemble_read_serial.
// one read by the whole wave (r and everything read through it are wave-uniform)
__device__ __forceinline__ void ec_assemble_seg_read(const EcAssembleArgs &a, uint64_t r, int lane)
{
    const uint64_t o = a.rd.scm_off[r], b0 = a.blk_off[r], w0 = a.new_off[r];
    const int32_t n = ecr_s((int32_t) (a.rd.scm_off[r + 1] - o));
    const uint64_t nb64 = a.blk_off[r + 1] - b0;
    const int32_t nb = ecr_s(nb64 > 64? 65 : (int32_t) nb64);
    const uint32_t room = (uint32_t) ecr_s((int32_t) (uint32_t) (a.new_off[r + 1] - w0));      // new_n[r]: nothing is written beyond it
    const bool keep_all = ecr_s((int32_t) a.keep_all[r]) != 0;
    if (n > 64 || nb > 64 || (nb == 0 && !keep_all)) {
        if (lane == 0) ec_assemble_read_serial(a, r);
        return;
    }
    const bool in = lane < n;
    const uint64_t km = in? a.rd.k_mer[o + lane] : 0;
    const uint32_t mp = in? a.rd.m_pos[o + lane] : 0;
    const uint64_t my_s = in? a.old_s_mer[o + lane] : 0;    // a syncmer's s-mer is the same at every occurrence (count.hpp: check_smer_kernel)
    const uint64_t sid = (a.sid0 + r) << 32;
    auto write = [&](uint32_t idx, uint64_t kk, uint32_t m, uint64_t sv) {          // entry idx of the corrected chain
        if (idx >= room) return;
        const uint64_t w = w0 + idx;
        a.new_k_mer[w] = kk, a.new_m_pos[w] = m, a.new_s_mer[w] = sv;
        a.key_id[w] = (uint32_t) (kk >> 1), a.val_occ[w] = sid | (uint64_t) idx << 1 | (m & 1u);                  // syncerr.c:796-805
    };
    if (nb == 0) {                                   // no good syncmer: the read keeps its arrays (syncerr.c:562-572)
        if (in) write((uint32_t) lane, km, mp, my_s);
        return;
    }
    const bool isb = lane < nb;
    EcSeg d;
    d.beg = 0, d.end_fl = 0;
    uint32_t status = EC_FAILURE, np = 0;
    uint64_t path_off = 0;
    if (isb) d = a.seg[b0 + lane], status = a.out[b0 + lane].status, np = a.out[b0 + lane].np, path_off = a.out[b0 + lane].path_off;
    const uint32_t end = d.end_fl >> 2, prev = wave_prev(end), prev_end = lane == 0? 0u : prev;
    const bool solved = isb && status == EC_SUCCESS;
    const uint32_t front = isb? ec_seg_front(d, prev_end) : 0u, body = isb? ec_seg_body(d, status, np) : 0u, pc = solved? body : 0u;
    const uint32_t at_incl = ecr_incl_sum(front + body), pt_incl = ecr_incl_sum(pc);
    const uint32_t at = at_incl - (front + body), pt = pt_incl - pc;          // where block `lane`'s front starts; its path interior's place among the path entries
    const uint32_t n_path = ecr_u32(pt_incl, 63);
    // originals: entry `lane` lies in the stretch [prev_end(i), end(i)) of exactly one block i.  It stays if it is in front of the block (up to the anchor), or
    // if the block is not corrected; its place is its distance from the stretch's start (front and body are adjacent in the chain, too)
    {
        const uint32_t meta = d.beg | (d.end_fl & EC_SEG_R) << 8 | (uint32_t) solved << 9;
        const uint32_t base = at - prev_end;
        uint32_t my_meta = 0, my_base = 0;
        for (int32_t i = 0; i < nb; ++i) {
            const uint32_t pe = ecr_u32(prev_end, i), mi = ecr_u32(meta, i), bi = ecr_u32(base, i);
            if ((uint32_t) lane >= pe) my_meta = mi, my_base = bi;
        }
        const bool stays = !(my_meta >> 9 & 1u) || (!(my_meta >> 8 & 1u) && (uint32_t) lane <= (my_meta & 0xFFu));
        if (in && stays) write(my_base + (uint32_t) lane, km, mp, my_s);
    }
    // path interiors: entry t of all of them belongs to the last block whose interiors start at or before t
    for (uint32_t t0 = 0; t0 < n_path; t0 += 64) {
        const uint32_t t = t0 + (uint32_t) lane;
        int32_t bi = 0;
        for (int32_t i = 0; i < nb; ++i) if (t >= ecr_u32(pt, i)) bi = i;
        const uint32_t q = t - (uint32_t) __shfl((int32_t) pt, bi), dst = (uint32_t) __shfl((int32_t) (at + front), bi);
        const int32_t bnp = __shfl((int32_t) np, bi);
        const bool br = __shfl((int32_t) (d.end_fl & EC_SEG_R), bi) != 0;
        const uint64_t poff = (uint64_t) (uint32_t) __shfl((int32_t) (uint32_t) (path_off >> 32), bi) << 32 | (uint32_t) __shfl((int32_t) (uint32_t) path_off, bi);
        if (t < n_path) {
            const uint64_t p = br? a.path_pool[poff + (uint32_t) (bnp - 1) - q] : a.path_pool[poff + 1 + q];
            const uint64_t kk = (p & ~1ULL) | 1ULL;
            write(dst + q, kk, br? 0xFFFFFFFFu ^ (uint32_t) (p & 1ULL) : 0xFFFFFFFEu | (uint32_t) (p & 1ULL), a.scm_s[kk >> 1]);
        }
    }
}
__global__ __launch_bounds__(256) void ec_assemble_seg_kernel(EcAssembleArgs a)
{
    const uint64_t r0 = ((uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * ECR_RPW;
    const int lane = threadIdx.x & 63;
    if (r0 >= a.rd.n_reads) return;
#pragma unroll
    for (int k = 0; k < ECR_RPW; ++k) {
        const uint64_t r = r0 + k;
        if (r >= a.rd.n_reads) break;
        ec_assemble_seg_read(a, r, lane);
    }
}

// inclusive sums over the two halves of a wave, each on its own (rows of sixteen, then row_bcast 15 into rows 1 and 3); every lane must be active
__device__ __forceinline__ uint32_t ecr_incl_sum32(uint32_t v)
{
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x111, 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x112, 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x114, 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x118, 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int32_t) v, 0x142, 0xa, 0xf, false);
    return v;
}

// Two reads to a wave (r20).  A read of config 3 has 21 chain entries (99.9 % have at most 32), so a wave per read ran a third full and the kernel's time was its
// waves times a chain of dependent loads.  Wave w takes reads 2 w and 2 w + 1: when both have at most 32 chain entries and at most 32 blocks (and are not the
// block-less kind that the serial routine takes), lanes 0 - 31 hold the first and lanes 32 - 63 the second, entry l and block l in lane l of the half -- the prefix
// sums are 32-lane sums, the per-block broadcasts read lane i and lane 32 + i and a lane takes its half's, and the loops run as long as the longer half needs.
// Any other pair is two passes of ec_assemble_seg_read by the same wave.  Which reads share a wave is a function of their counts alone, and a read's entries go
// to the same places either way.  OATK_DEBUG_EC_ASSEMBLE_PAIRS=0 launches ec_assemble_seg_kernel, a wave per read.
__global__ __launch_bounds__(256) void ec_assemble_pair_kernel(EcAssembleArgs a)
{
    const uint64_t rp = ((uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
    const int lane = threadIdx.x & 63, h = lane >> 5, l = lane & 31;
    if (rp >= a.rd.n_reads) return;
    bool ok = rp + 1 < a.rd.n_reads;
    if (ok) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint64_t n64 = a.rd.scm_off[rp + k + 1] - a.rd.scm_off[rp + k], nb64 = a.blk_off[rp + k + 1] - a.blk_off[rp + k];
            ok = ok && n64 <= 32 && nb64 <= 32 && (nb64 > 0 || a.keep_all[rp + k] != 0);
        }
    }
    if (!ecr_s((int32_t) ok)) {
        ec_assemble_seg_read(a, rp, lane);
        if (rp + 1 < a.rd.n_reads) ec_assemble_seg_read(a, rp + 1, lane);
        return;
    }
    const uint64_t r = rp + (uint64_t) h;              // this half's read; what follows is uniform within a half
    const uint64_t o = a.rd.scm_off[r], b0 = a.blk_off[r], w0 = a.new_off[r];
    const int32_t n = (int32_t) (a.rd.scm_off[r + 1] - o), nb = (int32_t) (a.blk_off[r + 1] - b0);
    const uint32_t room = (uint32_t) (a.new_off[r + 1] - w0);
    const int32_t nb_max = ecr_s(__builtin_amdgcn_readlane(nb, 0) > __builtin_amdgcn_readlane(nb, 32)? __builtin_amdgcn_readlane(nb, 0) : __builtin_amdgcn_readlane(nb, 32));
    const bool in = l < n;
    const uint64_t km = in? a.rd.k_mer[o + l] : 0;
    const uint32_t mp = in? a.rd.m_pos[o + l] : 0;
    const uint64_t my_s = in? a.old_s_mer[o + l] : 0;
    const uint64_t sid = (a.sid0 + r) << 32;
    auto write = [&](uint32_t idx, uint64_t kk, uint32_t m, uint64_t sv) {
        if (idx >= room) return;
        const uint64_t w = w0 + idx;
        a.new_k_mer[w] = kk, a.new_m_pos[w] = m, a.new_s_mer[w] = sv;
        a.key_id[w] = (uint32_t) (kk >> 1), a.val_occ[w] = sid | (uint64_t) idx << 1 | (m & 1u);
    };
    const bool isb = l < nb;
    EcSeg d;
    d.beg = 0, d.end_fl = 0;
    uint32_t status = EC_FAILURE, np = 0;
    uint64_t path_off = 0;
    if (isb) d = a.seg[b0 + l], status = a.out[b0 + l].status, np = a.out[b0 + l].np, path_off = a.out[b0 + l].path_off;
    const uint32_t end = d.end_fl >> 2, prev = wave_prev(end), prev_end = l == 0? 0u : prev;
    const bool solved = isb && status == EC_SUCCESS;
    const uint32_t front = isb? ec_seg_front(d, prev_end) : 0u, body = isb? ec_seg_body(d, status, np) : 0u, pc = solved? body : 0u;
    const uint32_t at_incl = ecr_incl_sum32(front + body), pt_incl = ecr_incl_sum32(pc);
    const uint32_t at = at_incl - (front + body), pt = pt_incl - pc;
    const uint32_t np0 = ecr_u32(pt_incl, 31), np1 = ecr_u32(pt_incl, 63);
    const uint32_t n_path = h? np1 : np0, n_path_max = np0 > np1? np0 : np1;
    // originals (a half without a block keeps its chain: my_meta and my_base stay 0, every entry stays where it is)
    {
        const uint32_t meta = d.beg | (d.end_fl & EC_SEG_R) << 8 | (uint32_t) solved << 9;
        const uint32_t base = at - prev_end;
        uint32_t my_meta = 0, my_base = 0;
        for (int32_t i = 0; i < nb_max; ++i) {
            const uint32_t pe = h? ecr_u32(prev_end, 32 + i) : ecr_u32(prev_end, i), mi = h? ecr_u32(meta, 32 + i) : ecr_u32(meta, i),
                           bi = h? ecr_u32(base, 32 + i) : ecr_u32(base, i);
            if (i < nb && (uint32_t) l >= pe) my_meta = mi, my_base = bi;
        }
        const bool stays = !(my_meta >> 9 & 1u) || (!(my_meta >> 8 & 1u) && (uint32_t) l <= (my_meta & 0xFFu));
        if (in && stays) write(my_base + (uint32_t) l, km, mp, my_s);
    }
    // path interiors, 32 entries of each half at a time
    for (uint32_t t0 = 0; t0 < n_path_max; t0 += 32) {
        const uint32_t t = t0 + (uint32_t) l;
        int32_t bi = 0;
        for (int32_t i = 0; i < nb_max; ++i) {
            const uint32_t pti = h? ecr_u32(pt, 32 + i) : ecr_u32(pt, i);
            if (i < nb && t >= pti) bi = i;
        }
        const int src = (h << 5) + bi;
        const uint32_t q = t - (uint32_t) __shfl((int32_t) pt, src), dst = (uint32_t) __shfl((int32_t) (at + front), src);
        const int32_t bnp = __shfl((int32_t) np, src);
        const bool br = __shfl((int32_t) (d.end_fl & EC_SEG_R), src) != 0;
        const uint64_t poff = (uint64_t) (uint32_t) __shfl((int32_t) (uint32_t) (path_off >> 32), src) << 32 | (uint32_t) __shfl((int32_t) (uint32_t) path_off, src);
        if (t < n_path) {
            const uint64_t p = br? a.path_pool[poff + (uint32_t) (bnp - 1) - q] : a.path_pool[poff + 1 + q];
            const uint64_t kk = (p & ~1ULL) | 1ULL;
            write(dst + q, kk, br? 0xFFFFFFFFu ^ (uint32_t) (p & 1ULL) : 0xFFFFFFFEu | (uint32_t) (p & 1ULL), a.scm_s[kk >> 1]);
        }
    }
}

// ---- update_syncmer_db (syncerr.c:769-814): coverage, forward-strand presence; occurrence lists come from a stable sort ----
// Coverage and forward counts in one pass over the sorted pairs (r20): a lane per entry, and a wave finds the runs of equal keys in its 64 entries with two ballots.  The lane at a run's head counts the run's entries
// and its forward strands in the ballots; a run that begins behind the wave's first lane and ends in front of its last valid one belongs to nobody else and is stored, the
// (at most two) runs that may go on in a neighbouring wave are added atomically -- cov and fwd are zero before the pass, and sums of integers do not depend on their order
__global__ __launch_bounds__(256) void ec_cov_runs_kernel(uint64_t tot, const uint32_t *key_sorted, const uint64_t *occ, uint32_t *cov, uint32_t *fwd)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = i < tot;
    const uint32_t k = valid? key_sorted[i] : 0u;
    const bool f = valid && !(occ[valid? i : 0] & 1ULL);
    const uint32_t prev = (uint32_t) __shfl_up((int) k, 1);
    const bool head = valid && (lane == 0 || prev != k);
    const uint64_t heads = __ballot(head), fw = __ballot(f), vm = __ballot(valid);
    if (!head) return;
    const uint64_t above = lane == 63? 0ULL : heads & ~((2ULL << lane) - 1ULL);         // heads behind this one
    const int end = above? __builtin_ctzll(above) : __builtin_popcountll(vm);           // one past the run's last lane here (the valid lanes are the low ones)
    const uint64_t m = (end == 64? ~0ULL : (1ULL << end) - 1ULL) & ~((1ULL << lane) - 1ULL);
    const uint32_t c = (uint32_t) (end - lane), fc = (uint32_t) __builtin_popcountll(fw & m);
    if (lane > 0 && above) cov[k] = c, fwd[k] = fc;
    else atomicAdd(cov + k, c), atomicAdd(fwd + k, fc);
}

__global__ void ec_del_kernel(uint64_t n, const uint32_t *fwd, uint8_t *del)
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) del[i] = !fwd[i];
}

}  // namespace oatk
