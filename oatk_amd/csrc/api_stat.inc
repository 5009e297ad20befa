// oatk_amd/csrc/api_stat.inc -- C ABI of the scan statistics (include/oatk_hip_stat.h); part of api.hip.
#include "../../include/oatk_hip_stat.h"

namespace oatk {

// sum and number of (p1 - p0 - K) over entries adjacent on a read that both carry a position (syncmer.c:892-903)
__global__ void stat_dist_kernel(uint64_t n_reads, const uint64_t *chain_off, const uint32_t *m_pos, int K, long long *sum, unsigned long long *cnt)
{
    uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    long long s = 0;
    unsigned long long c = 0;
    if (r < n_reads) {
        const uint64_t o = chain_off[r], n = chain_off[r + 1] - o;
        uint32_t p0 = 0x7FFFFFFFu;
        for (uint64_t j = 0; j < n; ++j) {
            const uint32_t p1 = m_pos[o + j] >> 1;
            if (p0 != 0x7FFFFFFFu && p1 != 0x7FFFFFFFu) s += (long long) (int) p1 - (long long) (int) p0 - K, ++c;
            p0 = p1;
        }
    }
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d), c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0 && c) { atomicAdd((unsigned long long *) sum, (unsigned long long) s); atomicAdd(cnt, c); }
}
__global__ void stat_key_kernel(uint64_t n, const uint64_t *k_mer, uint64_t *key)
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = k_mer[i] >> 1;
}
// histogram of run lengths, clamped at MAX_DEPTH (kh_ctab_cnt, syncmer.c:648-667)
__global__ void stat_hist_kernel(uint32_t n_runs, const uint32_t *counts, unsigned long long *hist)
{
    __shared__ unsigned int h[OATK_STAT_MAX_DEPTH + 1];
    for (uint32_t i = threadIdx.x; i <= OATK_STAT_MAX_DEPTH; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_runs; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t c = counts[i];
        atomicAdd(&h[c < OATK_STAT_MAX_DEPTH? c : OATK_STAT_MAX_DEPTH], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= OATK_STAT_MAX_DEPTH; i += blockDim.x) if (h[i]) atomicAdd(&hist[i], (unsigned long long) h[i]);
}

}  // namespace oatk

// khashl<khint_t, int> as instantiated at syncmer.c:558 (kh_hash_uint32, Fibonacci bucket mapping, linear probing, growth at 75 % checked
// by every put, kick-out rehash; khashl.h:150-218): enough of it to replay a sequence of kh_ctab_put1 calls and name the last bucket
struct StatKhl {
    uint32_t bits = 0, count = 0;
    bool alloc = false;
    std::vector<uint8_t> used;
    std::vector<uint32_t> keys;
    std::vector<int> vals;
    static uint32_t hash(uint32_t key)
    {
        key += ~(key << 15); key ^= (key >> 10); key += (key << 3); key ^= (key >> 6); key += ~(key << 11); key ^= (key >> 16);
        return key;
    }
    static uint32_t h2b(uint32_t h, uint32_t b) { return (h * 2654435769U) >> (32 - b); }
    uint32_t nb() const { return alloc? 1U << bits : 0U; }
    void resize(uint32_t want)
    {
        uint32_t j = 0, x = want;
        while ((x >>= 1) != 0) ++j;
        if (want & (want - 1)) ++j;
        const uint32_t nbits = j > 2? j : 2, n_old = nb(), n_new = 1U << nbits;
        std::vector<uint8_t> nused(n_new, 0);
        keys.resize(n_new > n_old? n_new : n_old), vals.resize(n_new > n_old? n_new : n_old);
        for (j = 0; j != n_old; ++j) {
            if (!used[j]) continue;
            uint32_t key = keys[j];
            int val = vals[j];
            used[j] = 0;
            for (;;) {
                uint32_t i = h2b(hash(key), nbits);
                while (nused[i]) i = (i + 1) & (n_new - 1);
                nused[i] = 1;
                if (i < n_old && used[i]) {
                    std::swap(keys[i], key), std::swap(vals[i], val);
                    used[i] = 0;
                } else {
                    keys[i] = key, vals[i] = val;
                    break;
                }
            }
        }
        used.swap(nused), bits = nbits, alloc = true;
    }
    void put1(uint32_t key)
    {
        uint32_t n = nb();
        if (count >= (n >> 1) + (n >> 2)) { resize(n + 1U); n = nb(); }
        uint32_t i = h2b(hash(key), bits);
        const uint32_t last = i;
        while (used[i] && keys[i] != key) { i = (i + 1U) & (n - 1); if (i == last) break; }
        if (!used[i]) keys[i] = key, vals[i] = 1, used[i] = 1, ++count;
        else ++vals[i];
    }
    int last_val() const
    {
        for (uint32_t k = nb(); k-- > 0; ) if (used[k]) return vals[k];
        return 0;
    }
};

struct StatState {
    DevBuf key, sorted, uniq, counts, nruns, hist, acc;
};

static void stat_state_free(oatk_hip_ctx *ctx)
{
    delete ctx->stat;          // (its buffers free themselves: ~DevBuf)
    ctx->stat = nullptr;
}

#define TENSURE(buf, bytes) ENSURE_IN(t, "stat.", buf, bytes)

// multiplicities of the values of keys[0..n): histogram and number of distinct values
static int stat_tabulate(oatk_hip_ctx *ctx, StatState *t, const uint64_t *keys, uint64_t n, int64_t *hist_out, uint64_t *uniq_out, int64_t *no_singleton)
{
    using namespace oatk;
    { int rc = prim_sort_runs(ctx, const_cast<uint64_t *>(keys), t->sorted.as<uint64_t>(), (void *) nullptr, (void *) nullptr, n, 0, 64, t->uniq.as<uint64_t>(), t->counts.as<uint32_t>(),
                              t->nruns.as<uint32_t>()); if (rc) return rc; }
    uint32_t n_runs = 0;
    CK(hipMemcpyAsync(&n_runs, t->nruns.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemsetAsync(t->hist.p, 0, (OATK_STAT_MAX_DEPTH + 1) * 8, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    unsigned nb = (n_runs + 255) / 256;
    if (nb > 1024) nb = 1024;
    if (nb) hipLaunchKernelGGL(stat_hist_kernel, dim3(nb), dim3(256), 0, ctx->stream, n_runs, t->counts.as<uint32_t>(), (unsigned long long *) t->hist.p);
    CK(hipMemcpyAsync(hist_out, t->hist.p, (OATK_STAT_MAX_DEPTH + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    *uniq_out = n_runs;
    *no_singleton = 0;
    if (n_runs && hist_out[1] == 0) {                  // the reference's report then depends on the layout of its count table: replay it
        std::vector<uint32_t> c(n_runs);
        CK(hipMemcpyAsync(c.data(), t->counts.p, (size_t) n_runs * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        StatKhl h;
        for (uint32_t i = 0; i < n_runs; ++i) h.put1(c[i]);     // runs come in sorted key order, the order of the qsort'ed walk (:916-927)
        *no_singleton = h.last_val();
    }
    return OATK_OK;
}

// this batch's part of sr_db_stat: the s-mer code and the k-mer key (hash, id or global id) of every chain entry, and the four additive figures
extern "C" int oatk_hip_stat_keys(oatk_hip_ctx *ctx, const void **d_smer, const void **d_kkey, uint64_t *n_keys, int64_t *add4)
{
    using namespace oatk;
    if (!ctx) return OATK_E_NODEV;
    if (!ctx->scanned) { ctx->err = "oatk_hip_stat needs a resident scan"; return OATK_E_STATE; }
    CK(hipSetDevice(ctx->device));
    const bool after_ec = ctx->ec && ctx->ec->done;
    EcState *e = ctx->ec;
    if (e && e->global && !after_ec) { ctx->err = "oatk_hip_stat_keys: sharded reads are tabulated after oatk_hip_ec_correct"; return OATK_E_STATE; }
    const uint64_t nr = ctx->n_reads, n = after_ec? e->new_tot : ctx->n_occ;
    add4[0] = (int64_t) nr, add4[1] = (int64_t) n, add4[2] = add4[3] = 0;
    *d_smer = *d_kkey = nullptr, *n_keys = 0;
    if (n == 0 || nr == 0) return OATK_OK;
    if (n >= 0xFFFFFFFFULL) { ctx->err = "oatk_hip_stat: more than 2^32 syncmers"; return OATK_E_ARG; }
    if (!ctx->stat) ctx->stat = new StatState();
    StatState *t = ctx->stat;
    const uint64_t *chain_off = after_ec? e->new_off.as<uint64_t>() : ctx->scm_off.as<uint64_t>();
    const uint32_t *m_pos = after_ec? e->new_m.as<uint32_t>() : ctx->pos_mpos.as<uint32_t>();
    const uint64_t *s_mer = after_ec? e->new_s.as<uint64_t>() : ctx->pos_smer.as<uint64_t>();
    const uint64_t *k_mer = after_ec? e->new_k.as<uint64_t>() : (ctx->counted? ctx->pos_kid.as<uint64_t>() : ctx->pos_hash.as<uint64_t>());
    TENSURE(key, (n + 1) * 8); TENSURE(acc, 64);
    CK(hipMemsetAsync(t->acc.p, 0, 64, ctx->stream));
    hipLaunchKernelGGL(stat_dist_kernel, dim3((unsigned) ((nr + 255) / 256)), dim3(256), 0, ctx->stream, nr, chain_off, m_pos, ctx->K, (long long *) t->acc.p,
                       (unsigned long long *) t->acc.p + 1);
    hipLaunchKernelGGL(stat_key_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, n, k_mer, t->key.as<uint64_t>());
    long long acc[2] = {0, 0};
    CK(hipMemcpyAsync(acc, t->acc.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    add4[2] = acc[0], add4[3] = acc[1];
    *d_smer = s_mer, *d_kkey = t->key.p, *n_keys = n;
    return OATK_OK;
}

// the tabulation over the keys of ALL reads (one batch, or the shards' lists in any order) and the summed additive figures
extern "C" int oatk_hip_stat_from_keys(oatk_hip_ctx *ctx, const uint64_t *d_smer, const uint64_t *d_kkey, uint64_t n, const int64_t *add4, oatk_stat_raw_t *out)
{
    if (!ctx) return OATK_E_NODEV;
    CK(hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    out->n_reads = (uint64_t) add4[0], out->n_syncmers = (uint64_t) add4[1], out->sum_dist = add4[2], out->n_dist = (uint64_t) add4[3];
    if (n == 0) return OATK_OK;
    if (n >= 0xFFFFFFFFULL) { ctx->err = "oatk_hip_stat: more than 2^32 syncmers"; return OATK_E_ARG; }
    if (!ctx->stat) ctx->stat = new StatState();
    StatState *t = ctx->stat;
    TENSURE(sorted, (n + 1) * 8); TENSURE(uniq, (n + 1) * 8); TENSURE(counts, (n + 1) * 4); TENSURE(nruns, 64); TENSURE(hist, (OATK_STAT_MAX_DEPTH + 1) * 8);
    { int rc = stat_tabulate(ctx, t, d_smer, n, out->smer_cnt, &out->smer_unique, &out->smer_no_singleton); if (rc) return rc; }
    { int rc = stat_tabulate(ctx, t, d_kkey, n, out->kmer_cnt, &out->kmer_unique, &out->kmer_no_singleton); if (rc) return rc; }
    CK(hipGetLastError());
    return OATK_OK;
}

extern "C" int oatk_hip_stat(oatk_hip_ctx *ctx, oatk_stat_raw_t *out)
{
    if (!ctx) return OATK_E_NODEV;
    memset(out, 0, sizeof(*out));
    if (ctx->ec && ctx->ec->global) { ctx->err = "oatk_hip_stat: reads are sharded; gather the keys and call oatk_hip_stat_from_keys"; return OATK_E_STATE; }
    const void *s = nullptr, *k = nullptr;
    uint64_t n = 0;
    int64_t add4[4];
    int rc = oatk_hip_stat_keys(ctx, &s, &k, &n, add4);
    if (rc) return rc;
    return oatk_hip_stat_from_keys(ctx, (const uint64_t *) s, (const uint64_t *) k, n, add4, out);
}
