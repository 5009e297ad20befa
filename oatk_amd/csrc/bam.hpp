// oatk_amd/csrc/bam.hpp -- unaligned BAM records on the device (include/oatk_hip_ingest.h: oatk_hip_ingest_bam).
//
// A record's start is known only from the record before it, and a walk by one lane pays a dependent HBM miss per record.  Here the chain is built by maps and scans:
//   bam_count_cand / bam_fill_cand   one lane per byte offset: ok(o) of bam_core.hpp; 4 KiB per workgroup, ballot + popcount, a scan between the passes, no atomics
//                                    -> the sorted candidate offsets c[0, m): every true record is one, and some offsets that merely look like a record
//   bam_succ_kernel                  jump[i] = the index of next(c[i]) in c (bisection), or m, the sentinel; mark[0] = (c[0] == s0)
//   bam_double_kernel                mark[jump[i]] for every marked i, jump = jump o jump: after ceil(log2(m + 1)) rounds the marked candidates are exactly those the
//                                    serial walk from s0 visits (reachability along jump is exact, whatever the false candidates link to)
//   (exclusive scan) bam_compact     the marked candidates in order: the records
//   bam_stop_kernel                  where the chain stops, and as what (clean end, cut record, no record)
//   bam_record_kernel                per record: length, padded length, header offset, the refused flags
//   (exclusive scan) bam_unpack      one wave per record: 8 source bytes -> 16 letters -> one aligned 16-byte store per lane and trip
#pragma once
#include "common.hpp"
#include "bam_core.hpp"

namespace oatk {

#define BAM_BLOCK 4096

__global__ __launch_bounds__(256) void bam_count_cand_kernel(const uint8_t *text, uint64_t n, uint64_t s0, uint32_t *cnt)
{
    __shared__ uint32_t w[4];
    const uint64_t base = (uint64_t) blockIdx.x * BAM_BLOCK;
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < BAM_BLOCK; i += 256) { const uint64_t p = base + i; c += p >= s0 && p < n && oatk_bam::ok(text, n, p); }
    for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}

__global__ __launch_bounds__(256) void bam_fill_cand_kernel(const uint8_t *text, uint64_t n, uint64_t s0, const uint64_t *blk_off, uint64_t *cand)
{
    __shared__ uint32_t w[4];
    const uint64_t base = (uint64_t) blockIdx.x * BAM_BLOCK;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t out = blk_off[blockIdx.x];
    for (uint32_t i0 = 0; i0 < BAM_BLOCK; i0 += 256) {
        const uint64_t p = base + i0 + threadIdx.x;
        const bool is = p >= s0 && p < n && oatk_bam::ok(text, n, p);
        const uint64_t m = __ballot(is);
        if (lane == 0) w[wid] = (uint32_t) __builtin_popcountll(m);
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t j = 0; j < wid; ++j) before += w[j];
        const uint32_t tot = w[0] + w[1] + w[2] + w[3];
        if (is) cand[out + before + (uint32_t) __builtin_popcountll(m & ((1ULL << lane) - 1ULL))] = p;
        out += tot;
        __syncthreads();
    }
}

// jump[i]: the candidate that starts where candidate i ends, or m; jump[m] = m.  mark[]: u64 for the scan that follows the rounds
__global__ __launch_bounds__(256) void bam_succ_kernel(const uint8_t *text, const uint64_t *cand, uint64_t m, uint64_t s0, uint32_t *jump, uint64_t *mark)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i > m) return;
    if (i == m) { jump[i] = (uint32_t) m, mark[i] = 0; return; }
    const uint64_t t = oatk_bam::next(text, cand[i]);
    uint64_t lo = i + 1, hi = m;                                          // the first candidate at or behind t
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (cand[mid] < t) lo = mid + 1; else hi = mid; }
    jump[i] = (uint32_t) (lo < m && cand[lo] == t? lo : m);
    mark[i] = i == 0 && cand[0] == s0;
}

// One round.  A mark that another lane sets in this round may or may not be seen: either way only candidates reachable from the start are ever marked, and all
// within 2^round steps are marked after it.
__global__ __launch_bounds__(256) void bam_double_kernel(uint64_t m, const uint32_t *jump, uint32_t *jump_out, uint64_t *mark)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i > m) return;
    const uint32_t j = jump[i];
    if (i < m && j < m && mark[i]) mark[j] = 1;
    jump_out[i] = jump[j];                                                // (jump[m] = m: the sentinel maps to itself)
}

__global__ __launch_bounds__(256) void bam_compact_kernel(const uint64_t *cand, uint64_t m, const uint64_t *mark, const uint64_t *rank, uint64_t *rec)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i < m && mark[i]) rec[rank[i]] = cand[i];
}

// out[0] = t, where the chain stops; out[1] = what it stops at (oatk_bam::STOP_*)
__global__ void bam_stop_kernel(const uint8_t *text, uint64_t n, uint64_t s0, const uint64_t *rec, uint64_t n_rec, uint64_t *out)
{
    const uint64_t t = n_rec? oatk_bam::next(text, rec[n_rec - 1]) : s0;
    out[0] = t, out[1] = (uint64_t) oatk_bam::classify(text, n, t);
}

// per record: length (u32 + widened, padded to 64), header offset; flags[1]: a record samtools fasta would reverse or drop, bad_rec: the first such record
__global__ void bam_record_kernel(const uint8_t *text, const uint64_t *rec, uint64_t n_rec, uint32_t *len, uint64_t *padded, uint64_t *hdr_off, uint32_t *flags,
                                  unsigned long long *bad_rec)
{
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { padded[r] = 0; return; }
    const uint64_t o = rec[r];
    const oatk_bam::Rec x = oatk_bam::record(text, o);
    if (x.flag & oatk_bam::REFUSED_FLAGS) { flags[1] = 1u; atomicMin(bad_rec, (unsigned long long) r); }
    len[r] = x.l_seq;
    padded[r] = ((uint64_t) x.l_seq + 63) & ~63ULL;
    hdr_off[r] = o;
}

// One wave per record.  A lane's trip: the 8 source bytes at seq + 8 idx (an unaligned 8-byte load of exactly these bytes: they lie inside the record's packed
// bases) become letters [16 idx, 16 idx + 16), stored with one 16-byte store (off[r] is a multiple of 64).  What is left of a read -- fewer than 16 letters, the
// last of them in a high nibble when l_seq is odd -- goes byte by byte, and reads no byte behind the last one that holds a base.
__global__ __launch_bounds__(256) void bam_unpack_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ rec, uint64_t n_rec, const uint64_t *__restrict__ off,
                                                         uint8_t *__restrict__ seq)
{
    const uint64_t r = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= n_rec) return;
    const oatk_bam::Rec x = oatk_bam::record(text, rec[r]);
    const uint8_t *src = text + x.seq_at;
    uint8_t *dst = seq + off[r];
    const uint32_t L = x.l_seq, n_full = L >> 4;                          // lane trips that make 16 letters
    for (uint32_t idx = lane; idx < n_full; idx += 64) {
        uint2 w;
        __builtin_memcpy(&w, src + 8 * (uint64_t) idx, 8);
        uint32_t a[2], b[2];
        oatk_bam::unpack8(w.x, a);
        oatk_bam::unpack8(w.y, b);
        *(uint4 *) (dst + 16 * (uint64_t) idx) = make_uint4(a[0], a[1], b[0], b[1]);
    }
    if (lane == (n_full & 63u))
        for (uint32_t j = n_full << 4; j < L; ++j) {
            const uint32_t by = src[j >> 1];
            dst[j] = oatk_bam::letter((j & 1u)? by & 15u : by >> 4);
        }
}

// ---- names of BAM records (oatk_hip_ingest_names after a BAM ingest): the bytes at hdr + 36 up to the first NUL ----
__global__ __launch_bounds__(256) void ing_bam_name_len_kernel(const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ hdr, uint64_t n, uint64_t *__restrict__ len)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    uint64_t l = 0;
    if (i < n) {
        const uint64_t p = hdr[i] + oatk_bam::FIXED;
        const uint64_t lim = hdr[i] + 12 < n_bytes? text[hdr[i] + 12] : 0;                // l_read_name: the NUL is among these bytes
        while (l < lim && p + l < n_bytes && text[p + l]) ++l;
    }
    len[i] = l;
}

__global__ __launch_bounds__(256) void ing_bam_name_copy_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ hdr, uint64_t n, const uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    uint64_t *out_off = (uint64_t *) out;
    uint8_t *packed = out + (n + 1) * 8;
    const uint64_t o = off[i];
    out_off[i] = o;
    if (i == n) return;
    const uint64_t l = off[i + 1] - o, p = hdr[i] + oatk_bam::FIXED;
    for (uint64_t k = 0; k < l; ++k) packed[o + k] = text[p + k];
}

}  // namespace oatk
