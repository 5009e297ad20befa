// oatk_amd/csrc/api_prim.inc -- the host-side idioms every area of the C ABI shares: growing a buffer or failing, rocPRIM's two-step calls, the launch grid of
// a 256-thread kernel, scans whose total the host needs, selection by flag, and the arc counter (sort + run-length encode).  Included by api.hip.
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_select.hpp>
#include <type_traits>

// owner->buf has room for `bytes`, or the entry point returns OATK_E_NOMEM; `area` is the prefix of the buffer's name in the error text.
// The areas' own names for it (ENSURE, EENSURE, ...) are one-line aliases next to their state structs.
#define ENSURE_IN(owner, area, buf, bytes, ...)                                                    \
    do {                                                                                           \
        if (!(owner)->buf.ensure((bytes), ctx->stream, ##__VA_ARGS__)) {                           \
            ctx->err = "hipMalloc failed for " area #buf;                                          \
            return OATK_E_NOMEM;                                                                   \
        }                                                                                          \
    } while (0)
#define ENSURE(buf, bytes, ...) ENSURE_IN(ctx, "", buf, bytes, ##__VA_ARGS__)

// A rocPRIM call: once without storage for the size of its temporary, then with the temporary grown to it.  The arguments are everything behind
// (storage, size), the stream included; they are evaluated twice and must have no side effects.  PRIM works in ctx->tmp on ctx->stream.  PRIM_IN
// is for a call on another stream, which must not share ctx->tmp with the main one, and for the areas that keep a temporary of their own.
#define PRIM_IN(buf, st, what, fn, ...)                                                            \
    do {                                                                                           \
        size_t tb_ = 0;                                                                            \
        CK(fn(nullptr, tb_, __VA_ARGS__));                                                         \
        if (!(buf).ensure(tb_, (st))) { ctx->err = what; return OATK_E_NOMEM; }                    \
        CK(fn((buf).p, tb_, __VA_ARGS__));                                                         \
    } while (0)
#define PRIM(fn, ...)                                                                              \
    do {                                                                                           \
        size_t tb_ = 0;                                                                            \
        CK(fn(nullptr, tb_, __VA_ARGS__));                                                         \
        ENSURE(tmp, tb_);                                                                          \
        CK(fn(ctx->tmp.p, tb_, __VA_ARGS__));                                                      \
    } while (0)

// blocks of 256 threads for n items, one block when there are none
static inline dim3 grid256(uint64_t n) { return dim3((unsigned) ((n + 255) / 256 > 0? (n + 255) / 256 : 1)); }

__global__ void widen_kernel(const uint32_t *in, uint64_t *out, uint64_t n)      // out has n + 1 entries
{
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i];
    if (i == n) out[i] = 0;
}

// exclusive scan of in[0..n] (in[n] = 0) into out[0..n]; *total = out[n], on the host when this returns
static int prim_scan_total(oatk_hip_ctx *ctx, DevBuf &tmp, uint64_t *in, uint64_t *out, uint64_t n, uint64_t *total)
{
    PRIM_IN(tmp, ctx->stream, "hipMalloc failed (scan tmp)", rocprim::exclusive_scan, in, out, (uint64_t) 0, n + 1, rocprim::plus<uint64_t>(), ctx->stream);
    CK(hipMemcpyAsync(total, out + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OATK_OK;
}
// the same of n 32-bit counts: widened into tmp64 (n + 1 entries, grown here like out64), scanned in ctx->tmp
static int prim_scan_total_u32(oatk_hip_ctx *ctx, DevBuf &in32, DevBuf &tmp64, DevBuf &out64, uint64_t n, uint64_t *total)
{
    if (!tmp64.ensure((n + 1) * 8, ctx->stream) || !out64.ensure((n + 1) * 8, ctx->stream)) { ctx->err = "hipMalloc failed (scan)"; return OATK_E_NOMEM; }
    hipLaunchKernelGGL(widen_kernel, dim3((unsigned) ((n + 1 + 255) / 256)), dim3(256), 0, ctx->stream, in32.as<uint32_t>(), tmp64.as<uint64_t>(), n);
    return prim_scan_total(ctx, ctx->tmp, tmp64.as<uint64_t>(), out64.as<uint64_t>(), n, total);
}

// out = the entries of `in` whose flag is set; their number through the caller's device counter d_cnt to the host
template <class T>
static int prim_select(oatk_hip_ctx *ctx, const T *in, const uint8_t *flag, uint64_t n, T *out, uint64_t *d_cnt, uint64_t *n_out)
{
    PRIM(rocprim::select, in, flag, out, d_cnt, n, ctx->stream);
    CK(hipMemcpyAsync(n_out, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OATK_OK;
}

// The arc counter: the keys sorted on bits [bit_lo, bit_hi) -- stable, each with its value when V is not void --, then one entry per run of equal
// keys in ukeys / counts and the number of runs in *d_nruns.  That number stays on the device: the callers fetch it with whatever else they wait for.
template <class K, class V>
static int prim_sort_runs(oatk_hip_ctx *ctx, K *keys, K *sorted, V *vals, V *vals_sorted, uint64_t n, unsigned bit_lo, unsigned bit_hi, K *ukeys, uint32_t *counts,
                          uint32_t *d_nruns)
{
    if constexpr (std::is_void<V>::value) PRIM(rocprim::radix_sort_keys, keys, sorted, n, bit_lo, bit_hi, ctx->stream);
    else PRIM(rocprim::radix_sort_pairs, keys, sorted, vals, vals_sorted, n, bit_lo, bit_hi, ctx->stream);
    PRIM(rocprim::run_length_encode, sorted, (unsigned int) n, ukeys, counts, d_nruns, ctx->stream);
    return OATK_OK;
}
