// oatk_amd/csrc/api_multi.inc -- reads sharded over several GPUs, from C (include/oatk_hip_multi.h); part of api.hip.
//
// Two collective steps of the hot path -- the count-table merge and the sharded error-correction round -- over a thin communicator that is
// either RCCL (one process per GPU or one thread per GPU; librccl is dlopen'ed when the first RCCL communicator is made) or a group of ranks
// inside one process that meet at a host barrier and copy device-to-device (what the single-GPU test box can run).  Four primitives carry
// everything: all-gather of a few numbers, all-gather of byte ranges of different sizes (as grouped broadcasts straight into place: no padding,
// no compaction), all-reduce of an integer vector, and a personalised exchange (every rank sends every other its own range: grouped
// ncclSend / ncclRecv).
//
// The merged table is PARTITIONED BY HASH RANGE (SURVEY.md 8e option 1): rank r owns the hashes h with floor(h * N / 2^64) = r.  A shard's
// table is sorted by hash, so what it owes each owner is a contiguous range of it -- no bucketing pass -- and the owners' ranges in rank
// order are the global table in hash order: a global id is the owner's first id plus the rank inside its range.  Per rank the exchange and
// the sort are the size of ONE shard's table, whatever the number of shards.
#include "../../include/oatk_hip_multi.h"
#include <dlfcn.h>
#include <pthread.h>
#include <time.h>
#include <unistd.h>
#include <rccl/rccl.h>
#include <rocprim/device/device_select.hpp>
#include <initializer_list>

namespace {

struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t *) = nullptr;     // optional
};
RcclApi g_rccl;
pthread_mutex_t g_rccl_mu = PTHREAD_MUTEX_INITIALIZER;

bool rccl_load()
{
    pthread_mutex_lock(&g_rccl_mu);
    if (!g_rccl.lib) {
        const char *ov = getenv("OATK_RCCL_LIB");          // test hook: another library with RCCL's entry points (tests/c/mock_rccl.cpp runs several ranks on one GPU)
        void *h = ov && ov[0]? dlopen(ov, RTLD_NOW | RTLD_LOCAL) : nullptr;
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            RcclApi a;
            a.lib = h;
#define OATK_SYM(f, name) *(void **) (&a.f) = dlsym(h, name)
            OATK_SYM(GetUniqueId, "ncclGetUniqueId"); OATK_SYM(CommInitRank, "ncclCommInitRank"); OATK_SYM(CommDestroy, "ncclCommDestroy"); OATK_SYM(CommAbort, "ncclCommAbort");
            OATK_SYM(AllGather, "ncclAllGather"); OATK_SYM(AllReduce, "ncclAllReduce"); OATK_SYM(Broadcast, "ncclBroadcast");
            OATK_SYM(GroupStart, "ncclGroupStart"); OATK_SYM(GroupEnd, "ncclGroupEnd"); OATK_SYM(GetErrorString, "ncclGetErrorString");
            OATK_SYM(Send, "ncclSend"); OATK_SYM(Recv, "ncclRecv"); OATK_SYM(CommGetAsyncError, "ncclCommGetAsyncError");
#undef OATK_SYM
            if (a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllGather && a.AllReduce && a.Broadcast && a.GroupStart && a.GroupEnd && a.Send && a.Recv) g_rccl = a;
            else dlclose(h);
        }
    }
    const bool ok = g_rccl.lib != nullptr;
    pthread_mutex_unlock(&g_rccl_mu);
    return ok;
}

}  // namespace

struct oatk_comm_group {
    int n = 0;
    // a barrier that can be POISONED: a rank that fails between two collectives must not leave the others waiting for it for ever
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int waiting = 0, poisoned = 0;
    uint64_t gen = 0;
    const void *ptr[64];
    uint64_t val[64][64];
    uint64_t off[64][65];
};

struct oatk_comm {
    uint64_t entered = 0;               // collectives entered (test hook: OATK_DEBUG_FAIL_RANK)
    uint64_t traffic[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // calls and bytes this rank put in, per kind (oatk_comm_traffic)
    int rank = 0, n = 1;
    int device = -1;                    // RCCL: the device the communicator was made on (the handle's must be the same)
    bool agreed = false;                // the error being returned is a verdict every rank reached together (a refusal): nobody is left waiting
    bool dead = false;                  // aborted after a rank-local failure
    ncclComm_t nccl = nullptr;          // RCCL
    oatk_comm_group *grp = nullptr;     // or ranks of one process
};

// 0: everybody arrived; 1: somebody failed instead of arriving
static int grp_wait(oatk_comm_group *g)
{
    pthread_mutex_lock(&g->mu);
    if (g->poisoned) { pthread_mutex_unlock(&g->mu); return 1; }
    const uint64_t my = g->gen;
    if (++g->waiting == g->n) { g->waiting = 0, ++g->gen; pthread_cond_broadcast(&g->cv); }
    else while (g->gen == my && !g->poisoned) pthread_cond_wait(&g->cv, &g->mu);
    const int bad = g->gen == my;       // woken by the poison, not by the last arrival
    pthread_mutex_unlock(&g->mu);
    return bad;
}
static void grp_poison(oatk_comm_group *g)
{
    pthread_mutex_lock(&g->mu);
    g->poisoned = 1;
    pthread_cond_broadcast(&g->cv);
    pthread_mutex_unlock(&g->mu);
}
#define GWAIT(c)                                                                                   \
    do {                                                                                           \
        if (grp_wait((c)->grp)) { ctx->err = "a peer rank failed between two collectives: the communicator group is poisoned"; return OATK_E_STATE; } \
    } while (0)

struct MultiState {
    // the exchange plan of the table merge: what this shard owes each owner (ranges of its hash-sorted table) and what it receives
    uint64_t send_off[65] = {0}, recv_off[65] = {0}, first_id[65] = {0};
    DevBuf recv_h, recv_s, recv_cov, srt_h, srt_i, iota, flag, grp, grp_of, own_h, own_s, own_cov, reply, back, l2g, lcov, plan_d, num, bad;
    DevBuf need_j, need8, pos_of_j, rep, clhead, req_j, req_k, asked, lid, seq_out, seq_in;          // k-mers of entries that share a hash
    DevBuf gcov, S;                      // dense over the global ids, filled where this rank needs them: its own syncmers and the candidates
    DevBuf cand, cand_cov, cand_s, cand_mine, ccov_mine, cs_mine, opack, sel_tmp;
    DevBuf keys_all, dist_all, need, need_all, need_srt, uni, owner, mine, kout, krev, ids_all, rev_all, km_all, lack, ids_i, rev_i, km_i;
    DevBuf ec_cov, ec_fwd, ec_del, st64, loc_c, loc_f, rcv_c, rcv_f, pc;
    DevBuf x[64];                        // the graph hand-off (api_multi_tail.inc: MX_*)
    uint64_t n_global = 0, n_owned = 0, table_occ = 0, gkid_n = 0;
    int rank = 0, table_root = -1;
    bool merged = false, ec_done = false;
};

static void multi_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->multi;          // (its buffers free themselves: ~DevBuf)
    ctx->multi = nullptr;
}

static int multi_buffer(oatk_hip_ctx *ctx, int which, const void **d_ptr, uint64_t *bytes)
{
    MultiState *m = ctx->multi;
    if (!m || !m->merged) { ctx->err = "merged table requested before oatk_hip_merge_counts"; return OATK_E_STATE; }
    const uint64_t no = m->n_owned, nl = ctx->n_scm_total;
    switch (which) {
        case OATK_BUF_MG_H: *d_ptr = m->own_h.p, *bytes = no * 8; break;
        case OATK_BUF_MG_S: *d_ptr = m->own_s.p, *bytes = no * 8; break;
        case OATK_BUF_MG_COV: *d_ptr = m->own_cov.p, *bytes = no * 4; break;
        case OATK_BUF_MG_L2G: *d_ptr = m->l2g.p, *bytes = nl * 4; break;
        case OATK_BUF_MG_LCOV: *d_ptr = m->lcov.p, *bytes = nl * 4; break;
        default:
            if (!m->ec_done) { ctx->err = "sharded correction results requested before oatk_hip_ec_sharded"; return OATK_E_STATE; }
            if (which == OATK_BUF_MG_EC_COV) *d_ptr = m->ec_cov.p, *bytes = no * 4;
            else *d_ptr = m->ec_del.p, *bytes = no;
    }
    return OATK_OK;
}

// ---------------------------------------------------------------- the primitives ----------------------------------------------------------------

#define MENSURE(buf, bytes) ENSURE_IN(m, "multi.", buf, bytes)
// MultiState::num, in 64-bit numbers: the all-gather of comm_allgather_vec (up to 64 ranks' 64 numbers, then this rank's own), behind it the counters rocPRIM writes
// (mg_select_u32, the distinct ids of ec_step2_kmers, the byte-wide select of ec_import_kmers)
enum { NUM_GATHER_END = 64 * 65, NUM_SELECT = NUM_GATHER_END + 8, NUM_UNIQUE, NUM_SELECT8, NUM_COUNT_ = NUM_GATHER_END + 64 };
static_assert(NUM_SELECT8 < NUM_COUNT_, "the counters of MultiState::num lie inside the buffer");
#define NUM_ENSURE() MENSURE(num, NUM_COUNT_ * 8)
#define NCK(call)                                                                                  \
    do {                                                                                           \
        ncclResult_t r_ = (call);                                                                  \
        if (r_ != ncclSuccess) { ctx->err = std::string(#call) + ": " + (g_rccl.GetErrorString? g_rccl.GetErrorString(r_) : "RCCL error"); return OATK_E_NODEV; } \
    } while (0)

// Waiting for an RCCL collective (round 4).  A rank that fails between two collectives aborts its OWN communicator (comm_finish); its peers are then
// inside a collective that will never complete, and a plain hipStreamSynchronize would wait for ever.  So the wait polls: the stream, the communicator's
// asynchronous error state (ncclCommGetAsyncError reports a peer that went away, where the library offers it), and a clock -- OATK_COMM_TIMEOUT_S seconds
// (default 600) without completion abort the local communicator and return an error; the drop-in then runs the original routine.
// a collective that will not complete: the communicator is aborted HERE and the stream drained before the caller's host buffers go out of scope -- a copy queued behind the
// collective (the counts of comm_allgather_vec land in the caller's array) must not complete into memory that is gone (ADVICE r04)
static void comm_give_up(oatk_hip_ctx *ctx, oatk_comm *c)
{
    if (c->nccl) { if (g_rccl.CommAbort) (void) g_rccl.CommAbort(c->nccl); else (void) g_rccl.CommDestroy(c->nccl); c->nccl = nullptr; }
    c->dead = true;
    (void) hipStreamSynchronize(ctx->stream);
}
static int comm_wait(oatk_hip_ctx *ctx, oatk_comm *c)
{
    static double limit = -1;
    if (limit < 0) { const char *e = getenv("OATK_COMM_TIMEOUT_S"); limit = e && atof(e) > 0? atof(e) : 600.0; }
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned spin = 0;; ++spin) {
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q == hipSuccess) return OATK_OK;
        if (q != hipErrorNotReady) { ctx->err = std::string("collective: ") + hipGetErrorString(q); return OATK_E_NODEV; }
        if (spin < 2000) continue;                                   // (the first microseconds without a system call: most collectives are short)
        if (c->nccl && g_rccl.CommGetAsyncError) {
            ncclResult_t ar = ncclSuccess;
            if (g_rccl.CommGetAsyncError(c->nccl, &ar) == ncclSuccess && ar != ncclSuccess && (int) ar != 7 /* ncclInProgress */) {
                ctx->err = std::string("collective: the communicator reports ") + (g_rccl.GetErrorString? g_rccl.GetErrorString(ar) : "an asynchronous error") + " (a peer rank failed?)";
                comm_give_up(ctx, c);
                return OATK_E_NODEV;
            }
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if ((double) (t1.tv_sec - t0.tv_sec) + 1e-9 * (double) (t1.tv_nsec - t0.tv_nsec) > limit) {
            ctx->err = "collective: no completion within OATK_COMM_TIMEOUT_S (a peer rank failed or hangs): communicator aborted";
            comm_give_up(ctx, c);
            return OATK_E_STATE;
        }
        usleep(spin < 20000? 20 : 500);
    }
}
// every collective starts here.  OATK_DEBUG_FAIL_RANK=<rank>,<k>: that rank fails instead of entering its k-th collective (tests: what its peers do then)
static int comm_enter(oatk_hip_ctx *ctx, oatk_comm *c)
{
    ++c->entered;
    static int f_rank = -2; static uint64_t f_at = 0;
    if (f_rank == -2) { const char *e = getenv("OATK_DEBUG_FAIL_RANK"); f_rank = -1; if (e && e[0]) { f_rank = atoi(e); const char *k = strchr(e, ','); f_at = k? (uint64_t) atoll(k + 1) : 1; } }
    if (c->rank == f_rank && c->entered == f_at) { ctx->err = "collective: failure injected (OATK_DEBUG_FAIL_RANK)"; return OATK_E_NOMEM; }
    return OATK_OK;
}

__global__ void multi_reduce_kernel(const void *const *src, int n, void *dst, uint64_t count, int is64, int is_min)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (is64) {
        uint64_t v = ((const uint64_t *) src[0])[i];
        for (int r = 1; r < n; ++r) { const uint64_t u = ((const uint64_t *) src[r])[i]; v = is_min? (u < v? u : v) : v + u; }
        ((uint64_t *) dst)[i] = v;
    } else {
        uint32_t v = ((const uint32_t *) src[0])[i];
        for (int r = 1; r < n; ++r) { const uint32_t u = ((const uint32_t *) src[r])[i]; v = is_min? (u < v? u : v) : v + u; }
        ((uint32_t *) dst)[i] = v;
    }
}

// every rank's k numbers (k <= 64), on the host of every rank: all[r * k + i]
static int comm_allgather_vec(oatk_hip_ctx *ctx, oatk_comm *c, const uint64_t *mine, int k, uint64_t *all)
{
    MultiState *m = ctx->multi;
    { int rc = comm_enter(ctx, c); if (rc) return rc; }
    c->traffic[0] += 1, c->traffic[1] += (uint64_t) k * 8;
    if (c->grp) {
        for (int i = 0; i < k; ++i) c->grp->val[c->rank][i] = mine[i];
        GWAIT(c);
        for (int r = 0; r < c->n; ++r) for (int i = 0; i < k; ++i) all[r * k + i] = c->grp->val[r][i];
        GWAIT(c);
        return OATK_OK;
    }
    NUM_ENSURE();
    uint64_t *d_all = m->num.as<uint64_t>(), *d_mine = d_all + (size_t) c->n * k;        // (at most 64 * 64 + 64 = NUM_GATHER_END numbers)
    CK(hipMemcpyAsync(d_mine, mine, (size_t) k * 8, hipMemcpyHostToDevice, ctx->stream));
    NCK(g_rccl.AllGather(d_mine, d_all, (size_t) k, ncclUint64, c->nccl, ctx->stream));
    CK(hipMemcpyAsync(all, d_all, (size_t) c->n * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    return comm_wait(ctx, c);
}
static int comm_allgather_u64(oatk_hip_ctx *ctx, oatk_comm *c, uint64_t mine, uint64_t *all) { return comm_allgather_vec(ctx, c, &mine, 1, all); }

// rank r contributes bytes[r] bytes; d_dst receives all contributions back to back in rank order
static int comm_allgatherv(oatk_hip_ctx *ctx, oatk_comm *c, const void *d_src, const uint64_t *bytes, void *d_dst)
{
    uint64_t off = 0;
    { int rc = comm_enter(ctx, c); if (rc) return rc; }
    c->traffic[2] += 1, c->traffic[3] += bytes[c->rank];
    if (c->grp) {
        c->grp->ptr[c->rank] = d_src;
        CK(hipStreamSynchronize(ctx->stream));                       // what the others are about to read is complete
        GWAIT(c);
        for (int r = 0; r < c->n; off += bytes[r], ++r)
            if (bytes[r]) CK(hipMemcpyAsync((uint8_t *) d_dst + off, c->grp->ptr[r], bytes[r], hipMemcpyDeviceToDevice, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        GWAIT(c);                          // nobody's source goes away before everybody has read it
        return OATK_OK;
    }
    NCK(g_rccl.GroupStart());
    for (int r = 0; r < c->n; off += bytes[r], ++r)
        if (bytes[r]) NCK(g_rccl.Broadcast(r == c->rank? d_src : (const void *) ((uint8_t *) d_dst + off), (uint8_t *) d_dst + off, bytes[r], ncclUint8, r, c->nccl, ctx->stream));
    NCK(g_rccl.GroupEnd());
    return comm_wait(ctx, c);
}

// in place; 32- or 64-bit unsigned, sum or minimum
static int comm_allreduce(oatk_hip_ctx *ctx, oatk_comm *c, void *d_buf, uint64_t count, bool is64, bool is_min)
{
    MultiState *m = ctx->multi;
    if (count == 0) return OATK_OK;              // (the counts are global quantities: every rank returns here or none does)
    { int rc = comm_enter(ctx, c); if (rc) return rc; }
    c->traffic[4] += 1, c->traffic[5] += count * (is64? 8 : 4);
    if (c->grp) {
        const size_t bytes = count * (is64? 8 : 4);
        MENSURE(sel_tmp, bytes + (size_t) c->n * sizeof(void *) + 64);
        c->grp->ptr[c->rank] = d_buf;
        CK(hipStreamSynchronize(ctx->stream));
        GWAIT(c);
        void **d_list = (void **) (m->sel_tmp.as<uint8_t>() + ((bytes + 15) & ~(size_t) 15));
        CK(hipMemcpyAsync(d_list, c->grp->ptr, (size_t) c->n * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(multi_reduce_kernel, dim3((unsigned) ((count + 255) / 256)), dim3(256), 0, ctx->stream, (const void *const *) d_list, c->n, m->sel_tmp.p,
                           count, is64? 1 : 0, is_min? 1 : 0);
        CK(hipStreamSynchronize(ctx->stream));
        GWAIT(c);                          // everybody has read everybody's input
        CK(hipMemcpyAsync(d_buf, m->sel_tmp.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        GWAIT(c);
        return OATK_OK;
    }
    NCK(g_rccl.AllReduce(d_buf, d_buf, count, is64? ncclUint64 : ncclUint32, is_min? ncclMin : ncclSum, c->nccl, ctx->stream));
    return comm_wait(ctx, c);
}

// Every rank's variable-length arrays of items, concatenated in rank order (the buffers are grown as needed); *n_all = items.  Several arrays with the same number of
// items per rank (a struct of arrays) take ONE exchange of counts and ONE collective for all of them -- what the per-step latency budget
// of eight GPUs is spent on is the number of collectives, not their bytes (DESIGN.md 9.2).  A column is one of the arrays: {this rank's items, where everybody's land,
// bytes per item}.  cnt_extra: one more number per rank travels with the counts (a verdict, see ec_step2_kmers), extra_all[r] receives it.
struct GatherCol { const void *src; DevBuf *dst; uint32_t width; };
static int comm_gather_cols(oatk_hip_ctx *ctx, oatk_comm *c, std::initializer_list<GatherCol> cols, uint64_t n_mine, uint64_t *n_all, uint64_t cnt_extra = 0,
                            uint64_t *extra_all = nullptr)
{
    uint64_t mine2[2] = {n_mine, cnt_extra}, all2[128], cnt[64], tot = 0;
    { int rc = comm_allgather_vec(ctx, c, mine2, extra_all? 2 : 1, all2); if (rc) return rc; }
    for (int r = 0; r < c->n; ++r) { cnt[r] = all2[extra_all? 2 * r : r]; if (extra_all) extra_all[r] = all2[2 * r + 1]; tot += cnt[r]; }
    for (const GatherCol &col : cols)
        if (!col.dst->ensure(tot * col.width + 64, ctx->stream)) { ctx->err = "hipMalloc failed (gather)"; return OATK_E_NOMEM; }
    *n_all = tot;
    if (extra_all) for (int r = 0; r < c->n; ++r) if (extra_all[r]) return OATK_OK;      // (somebody refuses: nobody enters the data's collective)
    if (c->grp) {
        uint64_t bytes[64];
        for (const GatherCol &col : cols) {
            for (int r = 0; r < c->n; ++r) bytes[r] = cnt[r] * col.width;
            int rc = comm_allgatherv(ctx, c, col.src, bytes, col.dst->p);
            if (rc) return rc;
            if (&col != cols.begin()) c->traffic[2] -= 1, c->entered -= 1;       // (counted as the one collective it is on the wire)
        }
        return OATK_OK;
    }
    { int rc = comm_enter(ctx, c); if (rc) return rc; }
    c->traffic[2] += 1;
    NCK(g_rccl.GroupStart());
    for (const GatherCol &col : cols) {
        uint64_t off = 0;
        uint8_t *to = (uint8_t *) col.dst->p;
        c->traffic[3] += cnt[c->rank] * col.width;
        for (int r = 0; r < c->n; off += cnt[r] * col.width, ++r)
            if (cnt[r]) NCK(g_rccl.Broadcast(r == c->rank? col.src : (const void *) (to + off), to + off, cnt[r] * col.width, ncclUint8, r, c->nccl, ctx->stream));
    }
    NCK(g_rccl.GroupEnd());
    return comm_wait(ctx, c);
}

// The personalised exchange: items [out_off[r], out_off[r + 1]) of a column's `out` go to rank r, and what rank r sends here lands at
// [in_off[r], in_off[r + 1]) of its `in` (the two offset arrays agree across the ranks: comm_plan).  The same plan serves both directions and every column.
struct XchgCol { const void *out; void *in; uint32_t width; };
static int comm_exchange_cols(oatk_hip_ctx *ctx, oatk_comm *c, std::initializer_list<XchgCol> cols, const uint64_t *out_off, const uint64_t *in_off)
{
    const int me = c->rank;
    { int rc = comm_enter(ctx, c); if (rc) return rc; }
    c->traffic[6] += 1;
    for (const XchgCol &col : cols) c->traffic[7] += (out_off[c->n] - out_off[0]) * col.width;
    if (c->grp) {
        for (const XchgCol &col : cols) {
            c->grp->ptr[me] = col.out;
            for (int r = 0; r <= c->n; ++r) c->grp->off[me][r] = out_off[r];
            CK(hipStreamSynchronize(ctx->stream));
            GWAIT(c);
            for (int r = 0; r < c->n; ++r) {
                const uint64_t cnt = in_off[r + 1] - in_off[r];
                if (cnt) CK(hipMemcpyAsync((uint8_t *) col.in + in_off[r] * col.width, (const uint8_t *) c->grp->ptr[r] + c->grp->off[r][me] * col.width, cnt * col.width, hipMemcpyDeviceToDevice, ctx->stream));
            }
            CK(hipStreamSynchronize(ctx->stream));
            GWAIT(c);
        }
        return OATK_OK;
    }
    for (const XchgCol &col : cols) {   // a rank's own range does not go through the network
        const uint64_t cnt = in_off[me + 1] - in_off[me];
        if (cnt) CK(hipMemcpyAsync((uint8_t *) col.in + in_off[me] * col.width, (const uint8_t *) col.out + out_off[me] * col.width, cnt * col.width, hipMemcpyDeviceToDevice, ctx->stream));
    }
    NCK(g_rccl.GroupStart());
    for (const XchgCol &col : cols)
        for (int r = 0; r < c->n; ++r) {
            if (r == me) continue;
            const uint64_t so = out_off[r + 1] - out_off[r], si = in_off[r + 1] - in_off[r];
            if (so) NCK(g_rccl.Send((const uint8_t *) col.out + out_off[r] * col.width, so * col.width, ncclUint8, r, c->nccl, ctx->stream));
            if (si) NCK(g_rccl.Recv((uint8_t *) col.in + in_off[r] * col.width, si * col.width, ncclUint8, r, c->nccl, ctx->stream));
        }
    NCK(g_rccl.GroupEnd());
    return comm_wait(ctx, c);
}
// from what this rank sends each peer (send_off, n + 1 entries) to where each peer's part lands (recv_off)
static int comm_plan(oatk_hip_ctx *ctx, oatk_comm *c, const uint64_t *send_off, uint64_t *recv_off, uint64_t *largest_recv = nullptr)
{
    uint64_t cnt[64], mat[64 * 64];
    for (int r = 0; r < c->n; ++r) cnt[r] = send_off[r + 1] - send_off[r];
    { int rc = comm_allgather_vec(ctx, c, cnt, c->n, mat); if (rc) return rc; }
    recv_off[0] = 0;
    for (int r = 0; r < c->n; ++r) recv_off[r + 1] = recv_off[r] + mat[r * c->n + c->rank];
    if (largest_recv) {                          // (the matrix is everybody's: what ANY rank is about to receive, without another round)
        *largest_recv = 0;
        for (int q = 0; q < c->n; ++q) { uint64_t t = 0; for (int r = 0; r < c->n; ++r) t += mat[r * c->n + q]; if (t > *largest_recv) *largest_recv = t; }
    }
    return OATK_OK;
}


// ---- who waits for whom ----
// Every rank makes the same calls, so a rank that leaves early -- hipMalloc failed, a kernel faulted, a bad argument -- would leave the others in a
// barrier or inside RCCL for ever.  Two rules: a data-dependent refusal (OATK_E_SPLIT / OATK_E_SMER, an id space that does not fit) is AGREED on by an
// exchange of verdicts before anybody returns (comm_agree); any other failure POISONS the communicator on the way out (comm_finish: the local group's
// barrier releases everybody with an error, an RCCL communicator is aborted), and it stays unusable afterwards.  Misuse that every rank commits alike
// BEFORE the call's first collective (a step called out of order, a root that does not exist) is marked agreed too: it is no reason to kill the communicator.
static int comm_check(oatk_hip_ctx *ctx, oatk_comm *c, const char *who)
{
    c->agreed = false;
    if (c->dead || (c->grp && c->grp->poisoned) || (!c->grp && !c->nccl)) { ctx->err = std::string(who) + ": the communicator was aborted after a failed rank"; return OATK_E_STATE; }
    if (c->nccl && c->device != ctx->device) { ctx->err = std::string(who) + ": the communicator was made for another device than the handle's"; return OATK_E_ARG; }
    return OATK_OK;
}
// (A call-order error found before the first collective -- "needs a resident scan + count" -- poisons too: a handle's state is its own, the peers may well be
//  inside the collective already, and only a verdict reached through comm_agree is known to be everybody's.  tests/test_gpu_multi_tail.py:
//  test_a_failing_rank_releases_the_others is exactly that case.)
static int comm_finish(oatk_comm *c, int rc)
{
    if (rc != OATK_OK && !c->agreed) {
        if (c->grp) grp_poison(c->grp);
        else if (c->nccl) { if (g_rccl.CommAbort) (void) g_rccl.CommAbort(c->nccl); else (void) g_rccl.CommDestroy(c->nccl); c->nccl = nullptr; }
        c->dead = true;
    }
    return rc;
}
// every rank's verdict on a step all of them just took: 0 when all are 0, otherwise the same non-zero code on every rank (a rank's own, if it has one)
static int comm_agree(oatk_hip_ctx *ctx, oatk_comm *c, int rc_mine, const char *what)
{
    uint64_t v[64];
    int rc2 = comm_allgather_u64(ctx, c, (uint64_t) rc_mine, v);
    if (rc2) return rc2;
    for (int r = 0; r < c->n; ++r)
        if (v[r]) {
            c->agreed = true;
            if (!rc_mine) ctx->err = std::string(what) + ": refused on rank " + std::to_string(r);
            return rc_mine? rc_mine : (int) v[r];
        }
    return OATK_OK;
}

// ---------------------------------------------------------------- communicators ----------------------------------------------------------------

extern "C" int oatk_comm_unique_id(uint8_t id[128])
{
    if (!rccl_load()) return OATK_E_NODEV;
    ncclUniqueId u;
    if (g_rccl.GetUniqueId(&u) != ncclSuccess) return OATK_E_NODEV;
    static_assert(sizeof(u) == 128, "RCCL's unique id is 128 bytes");
    memcpy(id, &u, 128);
    return OATK_OK;
}

extern "C" oatk_comm *oatk_comm_create(const uint8_t id[128], int rank, int n_ranks, int device)
{
    if (n_ranks < 1 || n_ranks > 64 || rank < 0 || rank >= n_ranks || !rccl_load()) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    ncclUniqueId u;
    memcpy(&u, id, 128);
    oatk_comm *c = new oatk_comm();
    c->rank = rank, c->n = n_ranks, c->device = device;
    if (g_rccl.CommInitRank(&c->nccl, n_ranks, u, rank) != ncclSuccess) { delete c; return nullptr; }
    return c;
}

extern "C" oatk_comm_group *oatk_comm_group_create(int n_ranks)
{
    if (n_ranks < 1 || n_ranks > 64) return nullptr;
    oatk_comm_group *g = new oatk_comm_group();
    g->n = n_ranks;
    if (pthread_mutex_init(&g->mu, nullptr) != 0) { delete g; return nullptr; }
    if (pthread_cond_init(&g->cv, nullptr) != 0) { pthread_mutex_destroy(&g->mu); delete g; return nullptr; }
    return g;
}

extern "C" oatk_comm *oatk_comm_group_rank(oatk_comm_group *g, int rank)
{
    if (!g || rank < 0 || rank >= g->n) return nullptr;
    oatk_comm *c = new oatk_comm();
    c->rank = rank, c->n = g->n, c->grp = g;
    return c;
}

extern "C" void oatk_comm_group_destroy(oatk_comm_group *g)
{
    if (!g) return;
    pthread_cond_destroy(&g->cv);
    pthread_mutex_destroy(&g->mu);
    delete g;
}

extern "C" void oatk_comm_destroy(oatk_comm *c)
{
    if (!c) return;
    if (c->nccl) (void) g_rccl.CommDestroy(c->nccl);
    delete c;
}

extern "C" int oatk_comm_rank(const oatk_comm *c) { return c? c->rank : -1; }
extern "C" void oatk_comm_traffic(oatk_comm *c, uint64_t out[8], int reset)
{
    if (!c) return;
    if (out) memcpy(out, c->traffic, sizeof(c->traffic));
    if (reset) memset(c->traffic, 0, sizeof(c->traffic));
}
extern "C" int oatk_comm_size(const oatk_comm *c) { return c? c->n : 0; }
extern "C" const char *oatk_comm_backend(const oatk_comm *c) { return !c? "" : (c->grp? "local" : "rccl"); }

// ---------------------------------------------------------------- count-table merge ----------------------------------------------------------------

// where the part of a hash-sorted table that rank r owns begins: the first hash h with floor(h * n / 2^64) >= r, i.e. h >= key[r] = ceil(r 2^64 / n)
// (off: n + 1 results; key: n + 1 inputs right behind them)
__global__ void mg_bounds_kernel(const uint64_t *h, uint64_t nl, int n, uint64_t *off)
{
    const int r = threadIdx.x;
    if (r > n) return;
    if (r == n) { off[r] = nl; return; }
    const uint64_t key = off[65 + r];
    uint64_t lo = 0, hi = nl;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (h[mid] < key) lo = mid + 1; else hi = mid; }
    off[r] = lo;
}
__global__ void mg_iota_kernel(uint32_t *a, uint64_t n)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (uint32_t) i;
}
// the received entries sorted by hash (srt_i = where each sits in the receive buffer; the sort is stable, so inside one hash the entries stand
// in (shard, local first-seen) order -- the order in which the reference meets the k-mers of a hash group, syncmer.c:1410).  head[i] = 1 where a
// new hash begins; need_j[j] = 1 for an entry that shares its hash with another one: its k-mer has to be looked at.
__global__ void mg_heads_kernel(const uint64_t *srt_h, const uint32_t *srt_i, uint64_t n, uint32_t *head, uint32_t *need_j)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool nw = i == 0 || srt_h[i] != srt_h[i - 1], nx = i + 1 == n || srt_h[i + 1] != srt_h[i];
    head[i] = nw;
    need_j[srt_i[i]] = !(nw && nx);
}
// requests: k-th needed entry (ascending receive index j) -> which shard it came from and where in what that shard sent here
__global__ void mg_req_kernel(const uint32_t *req_j, uint64_t n, const uint64_t *recv_off, int nranks, uint32_t *req_k)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t j = req_j[t];
    int r = 0;
    while (r + 1 < nranks && recv_off[r + 1] <= j) ++r;
    req_k[t] = (uint32_t) (j - recv_off[r]);
}
__global__ void mg_req_bounds_kernel(const uint32_t *req_j, uint64_t n, const uint64_t *recv_off, int nranks, uint64_t *req_off)
{
    const int r = threadIdx.x;
    if (r > nranks) return;
    const uint64_t key = recv_off[r];
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (req_j[mid] < key) lo = mid + 1; else hi = mid; }
    req_off[r] = lo;
}
// what the owners ask of this shard -> its own syncmer ids (plan: send_off[65]; asked_off[65] right behind first_id)
__global__ void mg_asked_ids_kernel(const uint32_t *asked, uint64_t n, const uint64_t *send_off, const uint64_t *asked_off, int nranks, uint32_t *lid)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int r = 0;
    while (r + 1 < nranks && asked_off[r + 1] <= t) ++r;
    lid[t] = (uint32_t) (send_off[r] + asked[t]);
}
// the oriented k-mer of a local syncmer (its first occurrence), 32 bases per 64-bit word, one wave per syncmer
__global__ __launch_bounds__(64) void mg_export_kmers_kernel(const uint32_t *lid, uint64_t n, const uint64_t *occ_off, const uint64_t *occ, uint64_t sid0, const uint64_t *off,
                                                             const uint64_t *scm_off, const uint32_t *m_pos, const uint8_t *hoco_s, int K, int nw, uint64_t *out)
{
    const uint64_t t = blockIdx.x;
    if (t >= n) return;
    const uint64_t o = occ[occ_off[lid[t]]], rd = (o >> 32) - sid0;
    const uint32_t idx = (uint32_t) o >> 1, mp = m_pos[scm_off[rd] + idx];
    const uint32_t *hs = (const uint32_t *) (hoco_s + (off[rd] >> 2));
    for (int wd = (int) threadIdx.x; wd < nw; wd += 64) out[t * (uint64_t) nw + wd] = oatk::kmer_word_global(hs, mp >> 1, mp & 1u, K, wd);
}
// first-seen clustering of every hash group by k-mer (process_kmer_cluster, syncmer.c:1293-1335): rep[i] = sorted index of the first entry of
// the group with the same k-mer (i itself for a new k-mer).  One lane per group; groups are as large as the number of shards, give or take
// a true 64-bit collision.  Equal k-mers with different s-mers are the reference's fatal condition (syncmer.c:1370).
__global__ void mg_cluster_kernel(const uint32_t *head, const uint32_t *srt_i, uint64_t n, const uint32_t *need_j, const uint32_t *pos_of_j, const uint64_t *seq, int nw,
                                  const uint64_t *recv_s, uint32_t *rep, uint32_t *clhead, uint32_t *bad)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    uint64_t e = i + 1;
    while (e < n && !head[e]) ++e;
    for (uint64_t t = i; t < e; ++t) {
        uint32_t r = (uint32_t) t;
        if (t > i) {
            const uint64_t *a = seq + (uint64_t) pos_of_j[srt_i[t]] * (uint64_t) nw;
            for (uint64_t f = i; f < t; ++f) {
                if (rep[f] != (uint32_t) f) continue;
                const uint64_t *b = seq + (uint64_t) pos_of_j[srt_i[f]] * (uint64_t) nw;
                int w = 0;
                while (w < nw && a[w] == b[w]) ++w;
                if (w == nw) { r = (uint32_t) f; break; }
            }
            if (r != (uint32_t) t && recv_s[srt_i[t]] != recv_s[srt_i[r]]) *bad = 1u;
        }
        rep[t] = r, clhead[t] = r == (uint32_t) t;
    }
    (void) need_j;
}
// cid[i] = inclusive prefix sum of clhead: entry i belongs to the (cid[rep[i]] - 1)-th syncmer of this owner's range
__global__ void mg_groups_kernel(const uint64_t *srt_h, const uint32_t *srt_i, const uint32_t *cid, const uint32_t *rep, const uint64_t *recv_s, const uint32_t *recv_cov, uint64_t n,
                                 uint64_t *own_h, uint64_t *own_s, uint32_t *own_cov, uint32_t *grp_of)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = cid[rep[i]] - 1u, j = srt_i[i];
    if (rep[i] == (uint32_t) i) own_h[g] = srt_h[i], own_s[g] = recv_s[j];
    atomicAdd(&own_cov[g], recv_cov[j]);
    grp_of[j] = g;
}
__global__ void mg_narrow8_kernel(const uint32_t *in, uint64_t n, uint8_t *out)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] != 0;
}
__global__ void mg_reply_kernel(const uint32_t *grp_of, const uint32_t *own_cov, uint64_t n, uint64_t *reply)
{
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) reply[j] = (uint64_t) own_cov[grp_of[j]] << 32 | grp_of[j];
}
// plan_d: send_off[65] then first_id[65]
__global__ void mg_l2g_kernel(const uint64_t *back, uint64_t nl, const uint64_t *plan_d, int n, uint32_t *l2g, uint32_t *lcov)
{
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nl) return;
    int r = 0;
    while (r + 1 < n && plan_d[r + 1] <= j) ++r;
    l2g[j] = (uint32_t) (plan_d[65 + r] + (uint32_t) back[j]);
    lcov[j] = (uint32_t) (back[j] >> 32);
}

static int mg_select_u32(oatk_hip_ctx *ctx, MultiState *m, const uint32_t *in, const uint8_t *flag, uint64_t n, DevBuf &out, uint64_t *n_out);

// The host ends of the table merge's asynchronous copies: they live in merge_counts_impl's frame, for the whole call.
struct MergeHost { uint64_t key[65] = {0}, req_off[65] = {0}, asked_off[65] = {0}; };

// 1. what this shard owes each owner: ranges of its own (hash-sorted) table
static int mg_send_ranges(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, uint64_t *key)
{
    const uint64_t nl = ctx->n_scm_total;
    const int n = c->n;
    int rc;
    MENSURE(bad, 64); MENSURE(plan_d, 130 * 8);
    CK(hipMemsetAsync(m->bad.p, 0, 64, ctx->stream));
    for (int r = 0; r < n; ++r) key[r] = (uint64_t) ((((unsigned __int128) (uint64_t) r << 64) + (uint64_t) (n - 1)) / (uint64_t) n);      // ceil(r 2^64 / n) < 2^64
    CK(hipMemcpyAsync(m->plan_d.as<uint64_t>() + 65, key, 65 * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(mg_bounds_kernel, dim3(1), dim3(128), 0, ctx->stream, ctx->scm_h.as<uint64_t>(), nl, n, m->plan_d.as<uint64_t>());
    CK(hipMemcpyAsync(m->send_off, m->plan_d.p, (size_t) (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    uint64_t largest = 0;
    if ((rc = comm_plan(ctx, c, m->send_off, m->recv_off, &largest)) != OATK_OK) return rc;
    const uint64_t nr = m->recv_off[n];
    if (largest >= 0x7FFFFFFFULL) {              // what ONE owner sees, known to everybody from the counts that just went round: the verdict is everybody's
        c->agreed = true;
        ctx->err = "an owner's part of the merged table is too large for 32-bit indices";
        return OATK_E_ARG;
    }
    MENSURE(recv_h, (nr + 1) * 8); MENSURE(recv_s, (nr + 1) * 8); MENSURE(recv_cov, (nr + 1) * 4);
    // hashes, s-mers and coverage along the same routes: one exchange
    return comm_exchange_cols(ctx, c, {{ctx->scm_h.p, m->recv_h.p, 8}, {ctx->scm_s.p, m->recv_s.p, 8}, {ctx->scm_cov.p, m->recv_cov.p, 4}}, m->send_off, m->recv_off);
}

// 2. the owner's range: sorted by hash; entries that share a hash are compared k-mer by k-mer (their shards send the k-mers: a true syncmer is
//    on every shard, a sequencing error on one, so this is thousands of k-mers) and clustered in first-seen order -- the reference's ids for
//    the union of the shards, hash collisions included; coverage summed per k-mer
static int mg_owner_range(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, uint64_t *req_off, uint64_t *asked_off)
{
    const int n = c->n;
    const uint64_t nr = m->recv_off[n];
    uint64_t n_own = 0, n_req = 0;
    int rc;
    MENSURE(srt_h, (nr + 1) * 8); MENSURE(srt_i, (nr + 1) * 4); MENSURE(iota, (nr + 1) * 4); MENSURE(flag, (nr + 1) * 4); MENSURE(grp, (nr + 1) * 4); MENSURE(grp_of, (nr + 1) * 4);
    MENSURE(own_h, (nr + 1) * 8); MENSURE(own_s, (nr + 1) * 8); MENSURE(own_cov, (nr + 1) * 4); MENSURE(reply, (nr + 1) * 8);
    MENSURE(need_j, (nr + 1) * 4); MENSURE(pos_of_j, (nr + 2) * 4); MENSURE(rep, (nr + 1) * 4); MENSURE(clhead, (nr + 1) * 4); MENSURE(req_j, (nr + 1) * 4); MENSURE(req_k, (nr + 1) * 4);
    MENSURE(need8, nr + 8);
    const int nw = (ctx->K + 31) / 32;
    CK(hipMemsetAsync(m->need_j.p, 0, (nr + 1) * 4, ctx->stream));
    if (nr) {
        hipLaunchKernelGGL(mg_iota_kernel, grid256(nr), dim3(256), 0, ctx->stream, m->iota.as<uint32_t>(), nr);
        // stable: within a hash the entries stay in (shard, local) order -- the global first-seen order of its k-mers
        PRIM(rocprim::radix_sort_pairs, m->recv_h.as<uint64_t>(), m->srt_h.as<uint64_t>(), m->iota.as<uint32_t>(), m->srt_i.as<uint32_t>(), nr, 0, 64, ctx->stream);
        hipLaunchKernelGGL(mg_heads_kernel, grid256(nr), dim3(256), 0, ctx->stream, m->srt_h.as<uint64_t>(), m->srt_i.as<uint32_t>(), nr, m->flag.as<uint32_t>(), m->need_j.as<uint32_t>());
        PRIM(rocprim::exclusive_scan, m->need_j.as<uint32_t>(), m->pos_of_j.as<uint32_t>(), 0u, nr + 1, rocprim::plus<uint32_t>(), ctx->stream);
        uint32_t nq = 0;
        CK(hipMemcpyAsync(&nq, m->pos_of_j.as<uint32_t>() + nr, 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        n_req = nq;
        if (n_req) {
            hipLaunchKernelGGL(mg_narrow8_kernel, grid256(nr), dim3(256), 0, ctx->stream, m->need_j.as<uint32_t>(), nr, m->need8.as<uint8_t>());
            uint64_t chk = 0;
            if ((rc = mg_select_u32(ctx, m, m->iota.as<uint32_t>(), m->need8.as<uint8_t>(), nr, m->req_j, &chk)) != OATK_OK) return rc;
        }
    }
    // the requests travel against the routes of the exchange above, the k-mers along them
    CK(hipMemcpyAsync(m->plan_d.as<uint64_t>(), m->recv_off, 65 * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_req) {
        hipLaunchKernelGGL(mg_req_bounds_kernel, dim3(1), dim3(128), 0, ctx->stream, m->req_j.as<uint32_t>(), n_req, m->plan_d.as<uint64_t>(), n, m->plan_d.as<uint64_t>() + 65);
        hipLaunchKernelGGL(mg_req_kernel, grid256(n_req), dim3(256), 0, ctx->stream, m->req_j.as<uint32_t>(), n_req, m->plan_d.as<uint64_t>(), n, m->req_k.as<uint32_t>());
        CK(hipMemcpyAsync(req_off, m->plan_d.as<uint64_t>() + 65, (size_t) (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    if ((rc = comm_plan(ctx, c, req_off, asked_off)) != OATK_OK) return rc;
    const uint64_t n_asked = asked_off[n];
    MENSURE(asked, (n_asked + 1) * 4); MENSURE(lid, (n_asked + 1) * 4); MENSURE(seq_out, (n_asked + 1) * (size_t) nw * 8); MENSURE(seq_in, (n_req + 1) * (size_t) nw * 8);
    if ((rc = comm_exchange_cols(ctx, c, {{m->req_k.p, m->asked.p, 4}}, req_off, asked_off)) != OATK_OK) return rc;
    if (n_asked) {
        CK(hipMemcpyAsync(m->plan_d.as<uint64_t>(), m->send_off, 65 * 8, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(m->plan_d.as<uint64_t>() + 65, asked_off, 65 * 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(mg_asked_ids_kernel, grid256(n_asked), dim3(256), 0, ctx->stream, m->asked.as<uint32_t>(), n_asked, m->plan_d.as<uint64_t>(), m->plan_d.as<uint64_t>() + 65, n,
                           m->lid.as<uint32_t>());
        hipLaunchKernelGGL(mg_export_kmers_kernel, dim3((unsigned) n_asked), dim3(64), 0, ctx->stream, m->lid.as<uint32_t>(), n_asked, ctx->scm_occ_off.as<uint64_t>(),
                           ctx->scm_occ.as<uint64_t>(), ctx->sid0, ctx->d_off, ctx->scm_off.as<uint64_t>(), ctx->pos_mpos.as<uint32_t>(), ctx->hoco_s.as<uint8_t>(), ctx->K, nw,
                           m->seq_out.as<uint64_t>());
    }
    if ((rc = comm_exchange_cols(ctx, c, {{m->seq_out.p, m->seq_in.p, (uint32_t) nw * 8u}}, asked_off, req_off)) != OATK_OK) return rc;
    if (nr) {
        hipLaunchKernelGGL(mg_cluster_kernel, grid256(nr), dim3(256), 0, ctx->stream, m->flag.as<uint32_t>(), m->srt_i.as<uint32_t>(), nr, m->need_j.as<uint32_t>(), m->pos_of_j.as<uint32_t>(),
                           m->seq_in.as<uint64_t>(), nw, m->recv_s.as<uint64_t>(), m->rep.as<uint32_t>(), m->clhead.as<uint32_t>(), m->bad.as<uint32_t>() + 1);
        PRIM(rocprim::inclusive_scan, m->clhead.as<uint32_t>(), m->grp.as<uint32_t>(), nr, rocprim::plus<uint32_t>(), ctx->stream);
        CK(hipMemsetAsync(m->own_cov.p, 0, (nr + 1) * 4, ctx->stream));
        hipLaunchKernelGGL(mg_groups_kernel, grid256(nr), dim3(256), 0, ctx->stream, m->srt_h.as<uint64_t>(), m->srt_i.as<uint32_t>(), m->grp.as<uint32_t>(), m->rep.as<uint32_t>(),
                           m->recv_s.as<uint64_t>(), m->recv_cov.as<uint32_t>(), nr, m->own_h.as<uint64_t>(), m->own_s.as<uint64_t>(), m->own_cov.as<uint32_t>(), m->grp_of.as<uint32_t>());
        hipLaunchKernelGGL(mg_reply_kernel, grid256(nr), dim3(256), 0, ctx->stream, m->grp_of.as<uint32_t>(), m->own_cov.as<uint32_t>(), nr, m->reply.as<uint64_t>());
        uint32_t last = 0;
        CK(hipMemcpyAsync(&last, m->grp.as<uint32_t>() + (nr - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        n_own = last;
    }
    m->n_owned = n_own;
    return OATK_OK;
}

// every rank must come to the same verdict, or the ones that go on wait for the ones that left; the same call tells everybody every range's size
static int mg_verdict_ranges(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m)
{
    const int n = c->n;
    int rc;
    uint32_t bad[2] = {0, 0};
    CK(hipMemcpyAsync(bad, m->bad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    uint64_t mine2[2] = {(uint64_t) (bad[1]? 1 : 0), m->n_owned}, all2[128], worst = 0, ng = 0;
    if ((rc = comm_allgather_vec(ctx, c, mine2, 2, all2)) != OATK_OK) return rc;
    for (int r = 0; r < n; ++r) { worst = all2[2 * r] > worst? all2[2 * r] : worst; m->first_id[r] = ng; ng += all2[2 * r + 1]; }
    m->first_id[n] = m->n_global = ng;
    if (worst == 1) { c->agreed = true; ctx->err = "identical k-mers with different s-mers across shards (syncmer.c:1370: fatal in the reference)"; return OATK_E_SMER; }
    if (ng >= 0x7FFFFFFFULL) { c->agreed = true; ctx->err = "merged syncmer table too large for 32-bit ids"; return OATK_E_ARG; }      // (the same sum on every rank)
    return OATK_OK;
}

// 3. every entry goes back to where it came from with its rank inside the owner's range and the coverage over all shards
static int mg_reply_l2g(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m)
{
    const uint64_t nl = ctx->n_scm_total;
    int rc;
    MENSURE(back, (nl + 1) * 8); MENSURE(l2g, (nl + 1) * 4); MENSURE(lcov, (nl + 1) * 4);
    if ((rc = comm_exchange_cols(ctx, c, {{m->reply.p, m->back.p, 8}}, m->recv_off, m->send_off)) != OATK_OK) return rc;
    CK(hipMemcpyAsync(m->plan_d.p, m->send_off, 65 * 8, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(m->plan_d.as<uint64_t>() + 65, m->first_id, 65 * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nl) hipLaunchKernelGGL(mg_l2g_kernel, grid256(nl), dim3(256), 0, ctx->stream, m->back.as<uint64_t>(), nl, m->plan_d.as<uint64_t>(), c->n, m->l2g.as<uint32_t>(), m->lcov.as<uint32_t>());
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    return OATK_OK;
}

static int merge_counts_impl(oatk_hip_ctx *ctx, oatk_comm *c, uint64_t *n_global)
{
    int rc;
    if ((rc = comm_check(ctx, c, "oatk_hip_merge_counts")) != OATK_OK) return rc;
    if (!ctx->counted) { ctx->err = "oatk_hip_merge_counts needs a resident scan + count"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->multi) ctx->multi = new MultiState();
    MultiState *m = ctx->multi;
    m->merged = m->ec_done = false, m->rank = c->rank, m->table_root = -1;
    MergeHost H;
    if ((rc = mg_send_ranges(ctx, c, m, H.key)) != OATK_OK) return rc;
    if ((rc = mg_owner_range(ctx, c, m, H.req_off, H.asked_off)) != OATK_OK) return rc;
    if ((rc = mg_verdict_ranges(ctx, c, m)) != OATK_OK) return rc;
    if ((rc = mg_reply_l2g(ctx, c, m)) != OATK_OK) return rc;
    m->merged = true;
    if (n_global) *n_global = m->n_global;
    return OATK_OK;
}

extern "C" int oatk_hip_merge_counts(oatk_hip_ctx *ctx, oatk_comm *c, uint64_t *n_global)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_merge_counts: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, merge_counts_impl(ctx, c, n_global));
}

extern "C" int oatk_hip_multi_range(oatk_hip_ctx *ctx, uint64_t *first_id, uint64_t *n_owned, uint64_t *n_global)
{
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->multi || !ctx->multi->merged) { ctx->err = "oatk_hip_multi_range before oatk_hip_merge_counts"; return OATK_E_STATE; }
    if (first_id) *first_id = ctx->multi->first_id[ctx->multi->rank];
    if (n_owned) *n_owned = ctx->multi->n_owned;
    if (n_global) *n_global = ctx->multi->n_global;
    return OATK_OK;
}

// ---------------------------------------------------------------- sharded error correction ----------------------------------------------------------------

__global__ void mg_need_flag_kernel(const uint8_t *err_del, const uint64_t *src, uint64_t n, uint8_t *flag, int nothing)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = !nothing && err_del[i] == 0 && src[i] == EC_NO_SRC;
}
__global__ void mg_owner_kernel(const uint32_t *ids, uint64_t n, const uint64_t *src, uint32_t rank, uint32_t nobody, uint32_t *owner)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) owner[i] = src[ids[i]] != EC_NO_SRC? rank : nobody;
}
__global__ void mg_eq_flag_kernel(const uint32_t *v, uint64_t n, uint32_t what, uint8_t *flag, uint32_t *any_left, uint32_t nobody)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = v[i] == what;
    if (v[i] == nobody) *any_left = 1u;
}
__global__ void mg_need_cand_kernel(const uint32_t *cand, uint64_t n, const uint8_t *err_del, const uint64_t *src, uint8_t *flag, int nothing)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = !nothing && err_del[cand[i]] == 0 && src[cand[i]] == EC_NO_SRC;
}
__global__ void mg_lack_kernel(const uint32_t *ids, uint64_t n, const uint64_t *src, uint8_t *flag, int nothing)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = !nothing && src[ids[i]] == EC_NO_SRC;
}
// rows of `stride` bytes picked by a list of row indices
__global__ void mg_rows_kernel(const uint8_t *in, const uint32_t *rows, uint64_t n, uint32_t stride, uint8_t *out)
{
    const uint64_t i = blockIdx.x;
    if (i >= n) return;
    const uint4 *a = (const uint4 *) (in + (uint64_t) rows[i] * stride);
    uint4 *b = (uint4 *) (out + i * stride);
    for (uint32_t t = threadIdx.x; t < stride / 16; t += blockDim.x) b[t] = a[t];
}
// dense[ids[i]] = val[i]
template <class T>
__global__ void mg_scatter_kernel(const uint32_t *ids, const T *val, uint64_t n, T *dense)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dense[ids[i]] = val[i];
}
// an owner's candidates: the syncmers of its range seen at least c times over all shards
__global__ void mg_cand_flag_kernel(const uint32_t *cov, uint64_t n, uint32_t c, uint8_t *flag)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = cov[i] >= c;
}
__global__ void mg_cand_emit_kernel(const uint32_t *idx, uint64_t n, uint32_t first, const uint32_t *own_cov, const uint64_t *own_s, uint32_t *ids, uint32_t *cov, uint64_t *s)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = first + idx[i], cov[i] = own_cov[idx[i]], s[i] = own_s[idx[i]];
}
// light graph over shards: the "has arcs that were never materialised" flags of the candidate vertices, packed for an all-reduce and back
__global__ void mg_other_pack_kernel(const uint32_t *cand, uint64_t n2, const uint8_t *other, uint8_t *packed)
{
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n2) packed[j] = other[(uint64_t) cand[j >> 1] << 1 | (j & 1ULL)];
}
__global__ void mg_other_unpack_kernel(const uint32_t *cand, uint64_t n2, const uint8_t *packed, uint8_t *other)
{
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n2) other[(uint64_t) cand[j >> 1] << 1 | (j & 1ULL)] = packed[j] != 0;
}
// update_syncmer_db over shards: candidates are summed by an all-reduce over their short list, everything else goes to its owner
__global__ void mg_pack_cand_kernel(const uint32_t *cand, uint64_t nc, const uint32_t *cov, const uint32_t *fwd, uint32_t *pc)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nc) pc[i] = cov[cand[i]], pc[nc + i] = fwd[cand[i]];
}
__global__ void mg_local_contrib_kernel(const uint32_t *l2g, uint64_t nl, const uint32_t *gcov, uint32_t c, const uint32_t *cov, const uint32_t *fwd, uint32_t *lc, uint32_t *lf)
{
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nl) return;
    const uint32_t g = l2g[j];
    const bool cand = gcov[g] >= c;                    // (their sums come from the all-reduce)
    lc[j] = cand? 0u : cov[g], lf[j] = cand? 0u : fwd[g];
}
__global__ void mg_owner_add_kernel(const uint32_t *grp_of, uint64_t n, const uint32_t *rc, const uint32_t *rf, uint32_t *ec_cov, uint32_t *ec_fwd)
{
    const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (rc[j]) atomicAdd(&ec_cov[grp_of[j]], rc[j]);
    if (rf[j]) atomicAdd(&ec_fwd[grp_of[j]], rf[j]);
}
__global__ void mg_owner_cand_kernel(const uint32_t *cand, uint64_t nc, const uint32_t *pc, uint32_t first, uint32_t n_owned, uint32_t *ec_cov, uint32_t *ec_fwd)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const uint32_t g = cand[i];
    if (g >= first && g - first < n_owned) ec_cov[g - first] = pc[i], ec_fwd[g - first] = pc[nc + i];
}
__global__ void mg_del_kernel(const uint32_t *fwd, uint64_t n, uint8_t *del)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) del[i] = fwd[i] == 0;
}

// out = the items of `in` (32-bit) whose flag is set; *n_out on the host (prim_select with this area's room for the output and counter slot)
static int mg_select_u32(oatk_hip_ctx *ctx, MultiState *m, const uint32_t *in, const uint8_t *flag, uint64_t n, DevBuf &out, uint64_t *n_out)
{
    *n_out = 0;
    if (!out.ensure((n + 1) * 4, ctx->stream)) { ctx->err = "hipMalloc failed (select)"; return OATK_E_NOMEM; }
    if (n == 0) return OATK_OK;
    NUM_ENSURE();
    return prim_select(ctx, in, flag, n, out.as<uint32_t>(), m->num.as<uint64_t>() + NUM_SELECT, n_out);
}

// What the steps of one sharded round hand each other: the sizes of the whole table, this shard's table, this owner's range and the candidates' list, this owner's first
// id, the coverage threshold, whether this rank has no syncmer at all (it corrects nothing and needs no k-mers), and which graph travels.
struct EcRound { uint64_t ng, nl, no, nc; uint32_t first_me, err_mer_c; int nothing; bool light; };
// room for n flags and n indices (DevBuf::ensure never shrinks: a smaller request after a larger one keeps the larger buffer)
#define FLAG_ROOM(n) do { MENSURE(flag, (n) + 8); MENSURE(iota, ((n) + 1) * 4); } while (0)

// step 0, light: the candidates (seen >= err_mer_c times over all shards) that every owner announces -- a few thousand at HiFi error rates
static int ec_cov_candidates(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, EcRound &R)
{
    const uint64_t no = R.no;
    uint64_t nc_me = 0, nc = 0;
    int rc;
    hipLaunchKernelGGL(mg_iota_kernel, grid256(no), dim3(256), 0, ctx->stream, m->iota.as<uint32_t>(), no);
    hipLaunchKernelGGL(mg_cand_flag_kernel, grid256(no), dim3(256), 0, ctx->stream, m->own_cov.as<uint32_t>(), no, R.err_mer_c, m->flag.as<uint8_t>());
    if ((rc = mg_select_u32(ctx, m, m->iota.as<uint32_t>(), m->flag.as<uint8_t>(), no, m->opack, &nc_me)) != OATK_OK) return rc;
    MENSURE(cand_mine, (nc_me + 1) * 4); MENSURE(ccov_mine, (nc_me + 1) * 4); MENSURE(cs_mine, (nc_me + 1) * 8);
    if (nc_me) hipLaunchKernelGGL(mg_cand_emit_kernel, grid256(nc_me), dim3(256), 0, ctx->stream, m->opack.as<uint32_t>(), nc_me, R.first_me, m->own_cov.as<uint32_t>(),
                                  m->own_s.as<uint64_t>(), m->cand_mine.as<uint32_t>(), m->ccov_mine.as<uint32_t>(), m->cs_mine.as<uint64_t>());
    // ids, coverage and s-mers of the candidates: rank order = id order, the list is ascending
    if ((rc = comm_gather_cols(ctx, c, {{m->cand_mine.p, &m->cand, 4}, {m->ccov_mine.p, &m->cand_cov, 4}, {m->cs_mine.p, &m->cand_s, 8}}, nc_me, &nc)) != OATK_OK) return rc;
    if (nc) {
        hipLaunchKernelGGL(mg_scatter_kernel<uint32_t>, grid256(nc), dim3(256), 0, ctx->stream, m->cand.as<uint32_t>(), m->cand_cov.as<uint32_t>(), nc, m->gcov.as<uint32_t>());
        hipLaunchKernelGGL(mg_scatter_kernel<uint64_t>, grid256(nc), dim3(256), 0, ctx->stream, m->cand.as<uint32_t>(), m->cand_s.as<uint64_t>(), nc, m->S.as<uint64_t>());
    }
    R.nc = nc;
    return OATK_OK;
}
// step 0, full (thresholds the light graph cannot serve): every owner's range
static int ec_cov_everything(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const EcRound &R)
{
    int rc;
    uint64_t cnt[64], bytes[64];
    if ((rc = comm_allgather_u64(ctx, c, R.no, cnt)) != OATK_OK) return rc;
    for (int r = 0; r < c->n; ++r) bytes[r] = cnt[r] * 4;
    if ((rc = comm_allgatherv(ctx, c, m->own_cov.p, bytes, m->gcov.p)) != OATK_OK) return rc;
    for (int r = 0; r < c->n; ++r) bytes[r] = cnt[r] * 8;
    return comm_allgatherv(ctx, c, m->own_s.p, bytes, m->S.p);
}
// 0. coverage and s-mers over the global ids, as far as this rank will look: its own syncmers, and the candidates or everything
static int ec_step0_cov_smers(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, EcRound &R)
{
    const uint64_t ng = R.ng, nl = R.nl;
    int rc;
    MENSURE(gcov, (ng + 1) * 4); MENSURE(S, (ng + 1) * 8); FLAG_ROOM(ng);      // (what the round flags -- an owner's range, candidates, distinct ids -- is never more than the table)
    CK(hipMemsetAsync(m->gcov.p, 0, (ng + 1) * 4, ctx->stream));
    CK(hipMemsetAsync(m->S.p, 0, (ng + 1) * 8, ctx->stream));
    if ((rc = R.light? ec_cov_candidates(ctx, c, m, R) : ec_cov_everything(ctx, c, m, R)) != OATK_OK) return rc;
    if (nl) {
        hipLaunchKernelGGL(mg_scatter_kernel<uint32_t>, grid256(nl), dim3(256), 0, ctx->stream, m->l2g.as<uint32_t>(), m->lcov.as<uint32_t>(), nl, m->gcov.as<uint32_t>());
        hipLaunchKernelGGL(mg_scatter_kernel<uint64_t>, grid256(nl), dim3(256), 0, ctx->stream, m->l2g.as<uint32_t>(), ctx->scm_s.as<uint64_t>(), nl, m->S.as<uint64_t>());
    }
    return OATK_OK;
}

// step 1, light (include/oatk_hip_ec.h): what travels is each shard's pairs between two candidates, sorted by key and run-length compressed into (key, distance, calls)
// segments -- a few per true arc instead of one per read -- and one flag per oriented candidate for arcs to rarer syncmers.  The per-rank cost does not grow with the
// number of shards.  *verdict: the graph's (a refusal -- duplicate arcs -- is the same on every rank, a failure need not be); the return value is this rank's way there.
static int ec_graph_light(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const EcRound &R, int *verdict)
{
    using namespace oatk;
    EcState *e = ctx->ec;
    const uint64_t nc = R.nc;
    int rc;
    const uint64_t *lk = nullptr;
    const uint32_t *ld = nullptr;
    uint64_t nk = 0, n_seg = 0, np_all = 0;
    if ((rc = ec_light_pairs(ctx, R.err_mer_c, &lk, &ld, &nk)) != OATK_OK) return rc;
    EENSURE(g_keys2, (nk + 1) * 8); EENSURE(g_dist2, (nk + 1) * 4); EENSURE(g_head, nk + 8); EENSURE(g_hpos, (nk + 1) * 4); EENSURE(g_iota, (nk + 1) * 4);
    if (nk) {
        // stable: a key's distances stay in (read, slot) order, so a segment is a run of consecutive calls
        PRIM(rocprim::radix_sort_pairs, const_cast<uint64_t *>(lk), e->g_keys2.as<uint64_t>(), const_cast<uint32_t *>(ld), e->g_dist2.as<uint32_t>(), nk, 0, 64, ctx->stream);
        hipLaunchKernelGGL(egr_seg_head_kernel, grid256(nk), dim3(256), 0, ctx->stream, nk, e->g_keys2.as<uint64_t>(), e->g_dist2.as<uint32_t>(), e->g_head.as<uint8_t>());
        hipLaunchKernelGGL(mg_iota_kernel, grid256(nk), dim3(256), 0, ctx->stream, e->g_iota.as<uint32_t>(), nk);
        EENSURE(g_nruns, 64);
        if ((rc = prim_select(ctx, e->g_iota.as<uint32_t>(), e->g_head.as<uint8_t>(), nk, e->g_hpos.as<uint32_t>(), e->g_nruns.as<uint64_t>() + 2, &n_seg)) != OATK_OK) return rc;
    }
    EENSURE(g_segk, (n_seg + 1) * 8); EENSURE(g_segv, (n_seg + 1) * 8);
    if (n_seg) hipLaunchKernelGGL(egr_seg_emit_kernel, grid256(n_seg), dim3(256), 0, ctx->stream, n_seg, nk, e->g_hpos.as<uint32_t>(), e->g_keys2.as<uint64_t>(),
                                  e->g_dist2.as<uint32_t>(), e->g_segk.as<uint64_t>(), e->g_segv.as<uint64_t>());
    if ((rc = comm_gather_cols(ctx, c, {{e->g_segk.p, &m->keys_all, 8}, {e->g_segv.p, &m->dist_all, 8}}, n_seg, &np_all)) != OATK_OK) return rc;
    const int rc_graph = *verdict = ec_graph_build(ctx, m->keys_all.as<uint64_t>(), nullptr, m->dist_all.as<uint64_t>(), np_all, true);
    // a candidate has arcs to rarer syncmers if it has them on any shard (a rank whose graph was refused goes through the motions of the collective)
    if (nc) {
        const uint64_t words = (2 * nc + 3) / 4;
        MENSURE(opack, words * 4 + 16);
        CK(hipMemsetAsync(m->opack.p, 0, words * 4, ctx->stream));
        if (!rc_graph) hipLaunchKernelGGL(mg_other_pack_kernel, grid256(2 * nc), dim3(256), 0, ctx->stream, m->cand.as<uint32_t>(), 2 * nc, e->g_other.as<uint8_t>(), m->opack.as<uint8_t>());
        if ((rc = comm_allreduce(ctx, c, m->opack.p, words, false, false)) != OATK_OK) return rc;     // at most 64 ranks: the byte sums do not carry
        if (!rc_graph) hipLaunchKernelGGL(mg_other_unpack_kernel, grid256(2 * nc), dim3(256), 0, ctx->stream, m->cand.as<uint32_t>(), 2 * nc, m->opack.as<uint8_t>(), e->g_other.as<uint8_t>());
    }
    if (!rc_graph) e->light_c = R.err_mer_c;
    return OATK_OK;
}
// step 1, full: every pair of every shard travels
static int ec_graph_full(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, int *verdict)
{
    int rc;
    const void *d_keys = nullptr, *d_dist = nullptr;
    uint64_t np = 0, np_all = 0;
    if ((rc = oatk_hip_ec_pairs(ctx, &d_keys, &d_dist, &np)) != OATK_OK) return rc;
    if ((rc = comm_gather_cols(ctx, c, {{d_keys, &m->keys_all, 8}, {d_dist, &m->dist_all, 4}}, np, &np_all)) != OATK_OK) return rc;
    *verdict = oatk_hip_ec_graph_from_pairs(ctx, m->keys_all.as<uint64_t>(), m->dist_all.as<uint32_t>(), np_all);
    return OATK_OK;
}
// 1. chains in global ids; the graph of all reads; the marks.  *verdict is the graph's and the marks': step 2 takes it round with its counts
static int ec_step1_graph(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const EcRound &R, uint32_t max_err_c, uint32_t err_arc_c, double max_arc_f, int *verdict)
{
    int rc;
    if ((rc = oatk_hip_ec_set_global(ctx, R.ng, m->l2g.as<uint32_t>(), m->gcov.as<uint32_t>(), m->S.as<uint64_t>())) != OATK_OK) return rc;
    if ((rc = R.light? ec_graph_light(ctx, c, m, R, verdict) : ec_graph_full(ctx, c, m, verdict)) != OATK_OK) return rc;
    if (!*verdict) *verdict = oatk_hip_ec_mark(ctx, R.err_mer_c, max_err_c, err_arc_c, max_arc_f);
    return OATK_OK;
}

// step 2, light: flags over the candidate list instead of the whole table
static int ec_need_light(oatk_hip_ctx *ctx, MultiState *m, const EcRound &R, uint64_t *n_need)
{
    EcState *e = ctx->ec;
    const uint64_t nc = R.nc;
    FLAG_ROOM(nc);
    if (nc) hipLaunchKernelGGL(mg_need_cand_kernel, grid256(nc), dim3(256), 0, ctx->stream, m->cand.as<uint32_t>(), nc, (const uint8_t *) e->err_del.p,
                               e->vtx_hs_off.as<uint64_t>(), m->flag.as<uint8_t>(), R.nothing);
    return mg_select_u32(ctx, m, m->cand.as<uint32_t>(), m->flag.as<uint8_t>(), nc, m->need, n_need);
}
// step 2, full: flags over the whole table
static int ec_need_full(oatk_hip_ctx *ctx, MultiState *m, const EcRound &R, uint64_t *n_need)
{
    EcState *e = ctx->ec;
    const uint64_t ng = R.ng;
    FLAG_ROOM(ng);
    hipLaunchKernelGGL(mg_iota_kernel, grid256(ng), dim3(256), 0, ctx->stream, m->iota.as<uint32_t>(), ng);
    hipLaunchKernelGGL(mg_need_flag_kernel, grid256(ng), dim3(256), 0, ctx->stream, (const uint8_t *) e->err_del.p, e->vtx_hs_off.as<uint64_t>(), ng, m->flag.as<uint8_t>(), R.nothing);
    return mg_select_u32(ctx, m, m->iota.as<uint32_t>(), m->flag.as<uint8_t>(), ng, m->need, n_need);
}
// the k-mers of the nu distinct ids somebody needs (m->uni): the owner of each (the lowest rank that has it) exports it, all of them travel to everybody, and every
// rank imports what it lacks
static int ec_import_kmers(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const EcRound &R, uint64_t nu, uint64_t *n_imported)
{
    EcState *e = ctx->ec;
    int rc;
    const uint32_t nobody = (uint32_t) c->n;
    MENSURE(owner, (nu + 1) * 4); MENSURE(bad, 64);
    hipLaunchKernelGGL(mg_owner_kernel, grid256(nu), dim3(256), 0, ctx->stream, m->uni.as<uint32_t>(), nu, e->vtx_hs_off.as<uint64_t>(), (uint32_t) c->rank, nobody, m->owner.as<uint32_t>());
    if ((rc = comm_allreduce(ctx, c, m->owner.p, nu, false, true)) != OATK_OK) return rc;
    CK(hipMemsetAsync(m->bad.p, 0, 64, ctx->stream));
    FLAG_ROOM(nu);
    hipLaunchKernelGGL(mg_eq_flag_kernel, grid256(nu), dim3(256), 0, ctx->stream, m->owner.as<uint32_t>(), nu, (uint32_t) c->rank, m->flag.as<uint8_t>(), m->bad.as<uint32_t>(), nobody);
    uint32_t orphan = 0;
    CK(hipMemcpyAsync(&orphan, m->bad.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    uint64_t n_mine = 0;
    if ((rc = mg_select_u32(ctx, m, m->uni.as<uint32_t>(), m->flag.as<uint8_t>(), nu, m->mine, &n_mine)) != OATK_OK) return rc;
    if (orphan) { c->agreed = true; ctx->err = "sharded error correction: a live syncmer occurs on no shard"; return OATK_E_STATE; }      // (the same on every rank)
    const uint32_t stride = (uint32_t) (((ctx->K + 3) / 4 + 8 + 15) / 16 * 16);
    MENSURE(kout, (n_mine + 1) * (size_t) stride); MENSURE(krev, n_mine + 8);
    if ((rc = oatk_hip_ec_export_kmers(ctx, m->mine.as<uint32_t>(), n_mine, m->kout.as<uint8_t>(), stride, m->krev.as<uint8_t>())) != OATK_OK) return rc;
    uint64_t n_all = 0, n_imp = 0, chk = 0;
    if ((rc = comm_gather_cols(ctx, c, {{m->mine.p, &m->ids_all, 4}, {m->krev.p, &m->rev_all, 1}, {m->kout.p, &m->km_all, stride}}, n_mine, &n_all)) != OATK_OK) return rc;
    // of everything that travelled, what THIS rank lacks
    FLAG_ROOM(n_all);
    hipLaunchKernelGGL(mg_iota_kernel, grid256(n_all), dim3(256), 0, ctx->stream, m->iota.as<uint32_t>(), n_all);
    hipLaunchKernelGGL(mg_lack_kernel, grid256(n_all), dim3(256), 0, ctx->stream, m->ids_all.as<uint32_t>(), n_all, e->vtx_hs_off.as<uint64_t>(), m->flag.as<uint8_t>(), R.nothing);
    if ((rc = mg_select_u32(ctx, m, m->iota.as<uint32_t>(), m->flag.as<uint8_t>(), n_all, m->lack, &n_imp)) != OATK_OK) return rc;
    if (n_imp) {
        MENSURE(ids_i, (n_imp + 1) * 4); MENSURE(rev_i, n_imp + 16); MENSURE(km_i, (n_imp + 1) * (size_t) stride);
        hipLaunchKernelGGL(mg_rows_kernel, dim3((unsigned) n_imp), dim3(64), 0, ctx->stream, m->km_all.as<uint8_t>(), m->lack.as<uint32_t>(), n_imp, stride, m->km_i.as<uint8_t>());
        // ids and strands are rows too (4 and 1 byte): gather them with the generic selects
        if ((rc = mg_select_u32(ctx, m, m->ids_all.as<uint32_t>(), m->flag.as<uint8_t>(), n_all, m->ids_i, &chk)) != OATK_OK) return rc;
        PRIM(rocprim::select, m->rev_all.as<uint8_t>(), m->flag.as<uint8_t>(), m->rev_i.as<uint8_t>(), m->num.as<uint64_t>() + NUM_SELECT8, n_all, ctx->stream);
        if ((rc = oatk_hip_ec_import_kmers(ctx, m->ids_i.as<uint32_t>(), m->rev_i.as<uint8_t>(), m->km_i.as<uint8_t>(), n_imp, stride)) != OATK_OK) return rc;
    }
    if (n_imported) *n_imported = n_imp;
    return OATK_OK;
}
// 2. good syncmers this rank has no k-mer for: somebody who has one sends it (the lowest such rank).  Only candidates can be good.
static int ec_step2_kmers(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const EcRound &R, int rc_graph, uint64_t *n_imported)
{
    int rc;
    uint64_t n_need = 0, n_need_all = 0, nu = 0, verdict[64];
    if (rc_graph) MENSURE(need, 64);
    else if ((rc = R.light? ec_need_light(ctx, m, R, &n_need) : ec_need_full(ctx, m, R, &n_need)) != OATK_OK) return rc;
    // The counts, and with them everybody's verdict on the graph and the marks.  A refusal (duplicate arcs) is the same on every rank, a failure need not be, so a rank
    // with a bad verdict of its own has gone through the motions of every collective up to here (an empty list of needs included) and leaves together with the others.
    if ((rc = comm_gather_cols(ctx, c, {{m->need.p, &m->need_all, 4}}, n_need, &n_need_all, (uint64_t) (uint32_t) rc_graph, verdict)) != OATK_OK) return rc;
    for (int r = 0; r < c->n; ++r)
        if (verdict[r]) {
            c->agreed = true;
            if (!rc_graph) ctx->err = "EC graph: refused on rank " + std::to_string(r);
            return rc_graph? rc_graph : (int) (int32_t) (uint32_t) verdict[r];
        }
    if (n_need_all) {
        MENSURE(need_srt, (n_need_all + 1) * 4); MENSURE(uni, (n_need_all + 1) * 4); NUM_ENSURE();
        PRIM(rocprim::radix_sort_keys, m->need_all.as<uint32_t>(), m->need_srt.as<uint32_t>(), n_need_all, 0, 32, ctx->stream);
        uint64_t *d_cnt = m->num.as<uint64_t>() + NUM_UNIQUE;
        PRIM(rocprim::unique, m->need_srt.as<uint32_t>(), m->uni.as<uint32_t>(), d_cnt, n_need_all, rocprim::equal_to<uint32_t>(), ctx->stream);
        CK(hipMemcpyAsync(&nu, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    return nu? ec_import_kmers(ctx, c, m, R, nu, n_imported) : OATK_OK;
}

// step 3, light: a corrected chain holds the rank's own syncmers and candidates (what a path can be made of).  Candidates: one all-reduce over their list.
// The rest: every shard tells each owner what it still holds of the owner's syncmers, along the routes of the table merge.
static int ec_refresh_light(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const EcRound &R)
{
    EcState *e = ctx->ec;
    const uint64_t nc = R.nc, nl = R.nl, no = R.no, nr = m->recv_off[c->n];
    int rc;
    CK(hipMemsetAsync(m->ec_cov.p, 0, (no + 1) * 4, ctx->stream));
    CK(hipMemsetAsync(m->ec_fwd.p, 0, (no + 1) * 4, ctx->stream));
    MENSURE(pc, (2 * nc + 2) * 4); MENSURE(loc_c, (nl + 1) * 4); MENSURE(loc_f, (nl + 1) * 4);
    MENSURE(rcv_c, (nr + 1) * 4); MENSURE(rcv_f, (nr + 1) * 4);
    if (nc) hipLaunchKernelGGL(mg_pack_cand_kernel, grid256(nc), dim3(256), 0, ctx->stream, m->cand.as<uint32_t>(), nc, e->cov.as<uint32_t>(), e->fwd.as<uint32_t>(), m->pc.as<uint32_t>());
    if ((rc = comm_allreduce(ctx, c, m->pc.p, 2 * nc, false, false)) != OATK_OK) return rc;
    if (nl) hipLaunchKernelGGL(mg_local_contrib_kernel, grid256(nl), dim3(256), 0, ctx->stream, m->l2g.as<uint32_t>(), nl, m->gcov.as<uint32_t>(), R.err_mer_c, e->cov.as<uint32_t>(),
                               e->fwd.as<uint32_t>(), m->loc_c.as<uint32_t>(), m->loc_f.as<uint32_t>());
    if ((rc = comm_exchange_cols(ctx, c, {{m->loc_c.p, m->rcv_c.p, 4}, {m->loc_f.p, m->rcv_f.p, 4}}, m->send_off, m->recv_off)) != OATK_OK) return rc;
    if (nr) hipLaunchKernelGGL(mg_owner_add_kernel, grid256(nr), dim3(256), 0, ctx->stream, m->grp_of.as<uint32_t>(), nr, m->rcv_c.as<uint32_t>(), m->rcv_f.as<uint32_t>(),
                               m->ec_cov.as<uint32_t>(), m->ec_fwd.as<uint32_t>());
    if (nc) hipLaunchKernelGGL(mg_owner_cand_kernel, grid256(nc), dim3(256), 0, ctx->stream, m->cand.as<uint32_t>(), nc, m->pc.as<uint32_t>(), R.first_me, (uint32_t) no,
                               m->ec_cov.as<uint32_t>(), m->ec_fwd.as<uint32_t>());
    return OATK_OK;
}
// step 3, full: every id may matter: two all-reduces over the whole table, of which the rank keeps its own range
static int ec_refresh_full(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const EcRound &R)
{
    EcState *e = ctx->ec;
    const uint64_t ng = R.ng, no = R.no;
    int rc;
    MENSURE(loc_c, (ng + 1) * 4); MENSURE(loc_f, (ng + 1) * 4);
    CK(hipMemcpyAsync(m->loc_c.p, e->cov.p, ng * 4, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipMemcpyAsync(m->loc_f.p, e->fwd.p, ng * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = comm_allreduce(ctx, c, m->loc_c.p, ng, false, false)) != OATK_OK) return rc;
    if ((rc = comm_allreduce(ctx, c, m->loc_f.p, ng, false, false)) != OATK_OK) return rc;
    CK(hipMemcpyAsync(m->ec_cov.p, m->loc_c.as<uint32_t>() + R.first_me, no * 4, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipMemcpyAsync(m->ec_fwd.p, m->loc_f.as<uint32_t>() + R.first_me, no * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return OATK_OK;
}
// 3. every rank corrects its own reads; the refreshed table (update_syncmer_db, syncerr.c:769-814) is partitioned like the merged one
static int ec_step3_correct(oatk_hip_ctx *ctx, oatk_comm *c, MultiState *m, const EcRound &R, double max_edist, uint64_t *stats12)
{
    EcState *e = ctx->ec;
    const uint64_t no = R.no;
    int rc = oatk_hip_ec_correct(ctx, max_edist);
    if ((rc = comm_agree(ctx, c, rc, "correction")) != OATK_OK) return rc;
    MENSURE(ec_cov, (no + 1) * 4); MENSURE(ec_fwd, (no + 1) * 4); MENSURE(ec_del, no + 8); MENSURE(st64, 16 * 8);
    CK(hipMemcpyAsync(m->st64.p, e->stats_h, 12 * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = R.light? ec_refresh_light(ctx, c, m, R) : ec_refresh_full(ctx, c, m, R)) != OATK_OK) return rc;
    if ((rc = comm_allreduce(ctx, c, m->st64.p, 12, true, false)) != OATK_OK) return rc;
    hipLaunchKernelGGL(mg_del_kernel, grid256(no), dim3(256), 0, ctx->stream, m->ec_fwd.as<uint32_t>(), no, m->ec_del.as<uint8_t>());
    uint64_t st[12];
    CK(hipMemcpyAsync(st, m->st64.p, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    if (stats12) memcpy(stats12, st, sizeof(st));
    return OATK_OK;
}

static int ec_sharded_impl(oatk_hip_ctx *ctx, oatk_comm *c, double max_edist, uint32_t err_mer_c, uint32_t max_err_c, uint32_t err_arc_c,
                           double max_arc_f, uint64_t *stats12, uint64_t *n_imported)
{
    int rc, rc_graph = OATK_OK;
    if ((rc = comm_check(ctx, c, "oatk_hip_ec_sharded")) != OATK_OK) return rc;
    if (!ctx->counted) { ctx->err = "oatk_hip_ec_sharded needs a resident scan + count"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    if (!ctx->multi || !ctx->multi->merged) { if ((rc = merge_counts_impl(ctx, c, nullptr)) != OATK_OK) return rc; }
    MultiState *m = ctx->multi;
    m->ec_done = false, m->table_root = -1;
    if (n_imported) *n_imported = 0;
    const bool light = err_mer_c > 0 && err_arc_c >= err_mer_c && max_err_c >= err_mer_c && !getenv("OATK_DEBUG_FULL_GRAPH");
    EcRound R = {m->n_global, ctx->n_scm_total, m->n_owned, 0, (uint32_t) m->first_id[c->rank], err_mer_c, ctx->n_occ == 0, light};
    if ((rc = ec_step0_cov_smers(ctx, c, m, R)) != OATK_OK) return rc;
    if ((rc = ec_step1_graph(ctx, c, m, R, max_err_c, err_arc_c, max_arc_f, &rc_graph)) != OATK_OK) return rc;
    if ((rc = ec_step2_kmers(ctx, c, m, R, rc_graph, n_imported)) != OATK_OK) return rc;      // (a bad rc_graph comes back from here, agreed on by every rank)
    if ((rc = ec_step3_correct(ctx, c, m, R, max_edist, stats12)) != OATK_OK) return rc;
    m->ec_done = true;
    return OATK_OK;
}

extern "C" int oatk_hip_ec_sharded(oatk_hip_ctx *ctx, oatk_comm *c, double max_edist, uint32_t err_mer_c, uint32_t max_err_c, uint32_t err_arc_c,
                                   double max_arc_f, uint64_t *stats12, uint64_t *n_imported)
{
    if (!ctx) return OATK_E_NODEV;
    if (!c) { ctx->err = "oatk_hip_ec_sharded: no communicator"; return OATK_E_ARG; }
    return comm_finish(c, ec_sharded_impl(ctx, c, max_edist, err_mer_c, max_err_c, err_arc_c, max_arc_f, stats12, n_imported));
}
