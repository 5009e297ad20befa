// oatk_amd/csrc/ec_seq.hpp -- the corrected reads' SEQUENCES (hoco space), what read_error_correction writes to its FILE *fo (syncerr.c:544-558, :590-597,
// :614-624), from what a correction with oatk_hip_ec_keep_seq leaves resident: the blocks' descriptors and outcomes, q_end and the optimum consensus of every
// replaced block (ec_wave.hpp: ec_keep_seq), and the reads' own hoco strings.
//
// The blocks of a read and the stretches kept between them tile [0, hoco_l): block i covers [beg_pos, beg_pos + l) -- a leading block [0, l), the last block ends
// at hoco_l (the walk of syncerr.c:406-598 leaves its loop nowhere else) -- and the stretch kept in front of block i is what lies between the block before it and
// beg_pos, the chain entries [end, beg - 1] of :590-597 being the bases from m_pos[end] to m_pos[beg - 1] + k.  A corrected read is therefore
//   front(0) body(0) front(1) body(1) ... front(nb - 1) body(nb - 1) tail
// with body(i) the first q_end bases of the optimum consensus where the block ended EC_SUCCESS or EC_AMBISNQ (reverse-complemented for a leading block, which is
// solved on the other strand) and the block's own l bases otherwise; the tail is empty unless the read has no block, i.e. no good syncmer, and is then the whole
// read (:615-620).  Nothing here assumes the tiling beyond "blocks come in read order": fronts and the tail are computed as differences, so a read none of whose
// blocks is replaced comes out as its own hoco string -- which tests/test_gpu_ec_seq.py asserts.
//
// Output: packed like hoco_s -- two bits per base, four bases to a byte, first base in the top bits (syncmer.c:290) -- every read on a 16-byte boundary, pad bits
// and pad bytes zero.
#pragma once
#include "ec.hpp"

namespace oatk {

// one per block of a read, and one more per read behind its blocks (the tail): where in the corrected read the stretch in front of the block and its body start
struct __attribute__((aligned(16))) EcSeqBlk {
    uint32_t o_front;             // first base (corrected read) of the stretch kept in front of the block
    uint32_t o_body;              // first base of its body
    uint32_t r_front;             // where the stretch starts on the read; the body's own bases follow it there
    uint32_t len_fl;              // bases of the body << 2 | EC_SEQ_* (the tail's record: 0)
};
#define EC_SEQ_REV 1u             // replaced by a leading block's optimum: reverse-complemented
#define EC_SEQ_OPT 2u             // replaced by the optimum consensus in the block's slot

__global__ void ec_slot_words_kernel(const EcWork *work, uint64_t n_work, double max_edist, uint32_t *words)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_work) words[i] = ec_slot_words(work[i].l, max_edist);
}

// lengths: a lane per read over its blocks.  sb has n_work + n_reads records: those of read r start at blk_off[r] + r.
__global__ __launch_bounds__(256) void ec_cseq_len_kernel(EcReads rd, const uint64_t *blk_off, const EcWork *work, const EcBlockOut *out, const uint32_t *qend, EcSeqBlk *sb,
                                                          uint32_t *clen, uint32_t *cbytes)
{
    const uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rd.n_reads) return;
    const uint64_t b0 = blk_off[r], b1 = blk_off[r + 1];
    EcSeqBlk *q = sb + b0 + r;
    uint32_t o = 0, pos = 0;
    for (uint64_t i = b0; i < b1; ++i) {
        const uint32_t beg_pos = work[i].beg_pos, l = (uint32_t) work[i].l, st = out[i].status;
        const bool opt = (st == EC_SUCCESS || st == EC_AMBISNQ) && !out[i].short_block;
        EcSeqBlk x;
        x.o_front = o, x.r_front = pos;
        x.o_body = o + (beg_pos > pos? beg_pos - pos : 0u);
        const uint32_t bl = opt? qend[i] : l;
        x.len_fl = bl << 2 | (opt? EC_SEQ_OPT | (work[i].r? EC_SEQ_REV : 0u) : 0u);
        q[i - b0] = x;
        o = x.o_body + bl, pos = beg_pos + l;
    }
    const uint32_t hl = rd.hoco_l[r], n = o + (hl > pos? hl - pos : 0u);
    EcSeqBlk t;
    t.o_front = o, t.o_body = n, t.r_front = pos, t.len_fl = 0;
    q[b1 - b0] = t;
    clen[r] = n, cbytes[r] = ((n + 3u) / 4u + 15u) & ~15u;
}

// sixteen bases of a hoco string from base p on, the first in the top two bits; bases at or beyond word n_words are zeros
__device__ __forceinline__ uint32_t ecs_read16(const uint32_t *hs, uint32_t p, uint32_t n_words)
{
    const uint32_t i = p >> 4, sh = (p & 15u) << 1;
    const uint32_t w0 = i < n_words? __builtin_bswap32(hs[i]) : 0u, w1 = sh && i + 1 < n_words? __builtin_bswap32(hs[i + 1]) : 0u;
    return (uint32_t) (((uint64_t) w0 << 32 | w1) >> (32u - sh));
}
// fields q .. q + 15 of a solver string (field s of word i = base 16 i + s at bits 2 s), field q in the low bits; q >= -15, and fields outside the string are zeros
__device__ __forceinline__ uint32_t ecs_slot16(const uint32_t *sl, int32_t q, uint32_t n_words)
{
    if (q < 0) return (n_words? sl[0] : 0u) << ((uint32_t) (-q) << 1);
    const uint32_t i = (uint32_t) q >> 4, sh = ((uint32_t) q & 15u) << 1;
    const uint32_t x0 = i < n_words? sl[i] : 0u, x1 = sh && i + 1 < n_words? sl[i + 1] : 0u;
    return (uint32_t) (((uint64_t) x1 << 32 | x0) >> sh);
}
// the sixteen two-bit groups of x in reverse order
__device__ __forceinline__ uint32_t ecs_rev16(uint32_t x)
{
    x = __builtin_bitreverse32(x);
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}

struct EcSeqArgs {
    EcReads rd;
    const uint64_t *blk_off;      // [n_reads + 1]
    const EcSeqBlk *sb;           // [n_work + n_reads]
    const uint32_t *slots;        // the optimum consensus of every replaced block (ec_keep_seq)
    const uint64_t *slot_off;     // [n_work + 1]
    const uint64_t *coff;         // [n_reads + 1] bytes
    uint8_t *cseq;
};

// A wave per read; a lane writes four consecutive words, 64 bases, with one 16-byte store.  The read's records sit in LDS (up to 64 of them; a read with more
// blocks than that reads them where they are): a lane finds the block its first base falls in or behind by bisection and walks on from there -- a block of a
// dozen bases means one word can span three segments.  A piece of a segment is sixteen bases fetched at its own offset (two words of the source, funnel-shifted),
// cut to the bases that belong to the word and shifted into place.
__global__ __launch_bounds__(256) void ec_cseq_write_kernel(EcSeqArgs a)
{
    __shared__ uint4 recs[4][64];
    const int wave = (int) (threadIdx.x >> 6), lane = (int) (threadIdx.x & 63);
    const uint64_t r = (uint64_t) blockIdx.x * 4 + (uint64_t) wave;
    const bool live = r < a.rd.n_reads;
    const uint64_t b0 = live? a.blk_off[r] : 0;
    const uint32_t nb = live? (uint32_t) (a.blk_off[r + 1] - b0) : 0u, nrec = nb + 1u;
    const uint4 *grec = (const uint4 *) (a.sb + b0 + r);
    const bool staged = nrec <= 64u;
    if (live && staged && (uint32_t) lane < nrec) recs[wave][lane] = grec[lane];
    __syncthreads();
    if (!live) return;
    auto rec = [&](uint32_t i) -> uint4 { return staged? recs[wave][i] : grec[i]; };
    const uint32_t hl = a.rd.hoco_l[r];
    const uint32_t *hs = (const uint32_t *) (a.rd.hoco_s + ((a.rd.off[r] >> 6) << 4));
    const uint32_t hs_words = (hl + 15u) >> 4;
    uint4 *dst = (uint4 *) (a.cseq + a.coff[r]);
    const uint32_t n_groups = (uint32_t) ((a.coff[r + 1] - a.coff[r]) >> 4);
    for (uint32_t g = (uint32_t) lane; g < n_groups; g += 64u) {
        const uint32_t g0 = g << 6, g1 = g0 + 64u;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        // bases [s, e) of the corrected read come from `kind` (0: the read from base `src` on; else the slot at `sl`, o_len bases, forward or reversed)
        auto emit = [&](uint32_t s, uint32_t e, uint32_t kind, uint32_t src, const uint32_t *sl, uint32_t sl_words, uint32_t o_len) {
            if (e <= g0 || s >= g1 || e <= s) return;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t d0 = g0 + 16u * (uint32_t) u;
                const uint32_t os = s > d0? s : d0, oe = e < d0 + 16u? e : d0 + 16u;
                if (oe <= os) continue;
                const uint32_t j = os - s, cnt = oe - os;
                uint32_t m;
                if (kind == 0u) m = ecs_read16(hs, src + j, hs_words);
                else if (kind & EC_SEQ_REV) m = ~ecs_slot16(sl, (int32_t) o_len - 16 - (int32_t) j, sl_words);     // base t = comp(opt[o_len - 1 - j - t]): field 15 - t of the window, where it belongs
                else m = ecs_rev16(ecs_slot16(sl, (int32_t) j, sl_words));
                if (cnt < 16u) m &= ~(0xFFFFFFFFu >> (cnt << 1));
                w[u] |= m >> ((os - d0) << 1);
            }
        };
        // the last record whose stretch starts at or before g0 (record 0 starts at 0)
        uint32_t lo = 0, hi = nb;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (rec(mid).x <= g0) lo = mid; else hi = mid - 1u;
        }
        for (uint32_t b = lo; ; ++b) {
            const uint4 x = rec(b);                    // o_front, o_body, r_front, len_fl
            const uint32_t bl = x.w >> 2, kind = x.w & 3u, be = x.y + bl;
            emit(x.x, x.y, 0u, x.z, nullptr, 0u, 0u);
            if (kind & EC_SEQ_OPT) {
                const uint64_t s0 = a.slot_off[b0 + b];
                emit(x.y, be, kind, 0u, a.slots + s0, (uint32_t) (a.slot_off[b0 + b + 1] - s0), bl);
            } else {
                emit(x.y, be, 0u, x.z + (x.y - x.x), nullptr, 0u, 0u);
            }
            if (b == nb || be >= g1) break;
        }
        dst[g] = make_uint4(__builtin_bswap32(w[0]), __builtin_bswap32(w[1]), __builtin_bswap32(w[2]), __builtin_bswap32(w[3]));
    }
}

}  // namespace oatk
