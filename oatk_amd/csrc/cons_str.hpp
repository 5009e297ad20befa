// oatk_amd/csrc/cons_str.hpp -- the strings of scg_consensus (syncasm.c:716-823) on the device: every unitig's text, and the lengths the arcs need, from the
// tables oatk_hip_consensus left resident (consensus.hpp).  A sequence is a list of pieces (cons_str_core.hpp decides what a piece reads as); the host sends the
// graph-sized plan, the text comes back, CONS_RL never leaves the device.
//
//   cstr_len_kernel    one wave per piece: lanes stride over the positions and add up 1 + rl, a wave reduction gives the piece's length; unprepared pieces flagged
//   cstr_seq_kernel    one wave per sequence: its length and status, and its pieces' lengths masked (0 where the sequence takes no bytes) for the scan
//   (one exclusive scan over the pieces: where each starts in CONS_STR)
//   cstr_kmer_kernel   sharded reads only, once per consensus: one wave per selected slot writes the syncmer's own k-mer where this rank holds it, zeros elsewhere
//   cstr_fill_kernel   one wave per piece, 64 positions at a time: a lane loads its position's base and count, a wave prefix sum puts the 64 start offsets in LDS,
//                      and the stores are output-stationary -- lane l writes bytes l, l + 64, ... of the tile's text and finds each one's source position in the
//                      starts by bisection -- so a run of 700 bases goes out as eleven coalesced 64-byte stores, not as one lane's loop
//
// Waves work on their own (no workgroup barrier: pieces differ in length); what a lane wrote to LDS is read by other lanes of the same wave only.
#pragma once
#include "common.hpp"
#include "cons_str_core.hpp"

namespace oatk {

#define CSTR_WAVES 4              // pieces per workgroup

struct CstrArgs {
    oatk_cstr::Tables T;
    uint64_t n_seq, n_piece;
    const uint64_t *seq_off;      // [n_seq + 1]
    const uint64_t *piece_v;      // [n_piece]
    const int32_t *piece_beg;     // [n_piece]
    const uint8_t *want;          // [n_seq], nullptr = all
    int hoco_seq;
    uint64_t *piece_len;          // [n_piece]
    uint8_t *piece_bad;           // [n_piece]
    uint64_t *piece_put;          // [n_piece + 1] bytes the piece takes in CONS_STR (the scan's input)
    const uint64_t *piece_at;     // [n_piece + 1] where they start (the scan's output)
    uint64_t *str_off, *str_len;  // [n_seq + 1], [n_seq]
    uint8_t *status;              // [n_seq]
    uint8_t *str;                 // [total]
    uint64_t total;
};

__device__ __forceinline__ void cstr_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ uint64_t cstr_wave_sum(uint64_t x)
{
    for (int d = 32; d; d >>= 1) x += (uint64_t) __shfl_xor((long long) x, d);
    return x;
}

__global__ __launch_bounds__(64 * CSTR_WAVES) void cstr_len_kernel(CstrArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t) blockIdx.x * CSTR_WAVES + (threadIdx.x >> 6);
    if (i >= a.n_piece) return;
    const oatk_cstr::Piece P = oatk_cstr::open(a.T, a.piece_v[i], a.piece_beg[i], a.hoco_seq);
    uint64_t len = 0;
    if (P.slot != (uint32_t) oatk_cstr::NO_SLOT) {
        uint64_t mine = 0;
        if (P.has_first && P.expand)
            for (uint32_t t = P.beg0 + lane; t < (uint32_t) a.T.k; t += 64) mine += oatk_cstr::count_at(a.T, P, t) - 1;
        len = P.pad + ((uint64_t) a.T.k - P.beg0) + cstr_wave_sum(mine);
    }
    if (lane == 0) a.piece_len[i] = len, a.piece_bad[i] = P.slot == (uint32_t) oatk_cstr::NO_SLOT;
}

__global__ __launch_bounds__(64 * CSTR_WAVES) void cstr_seq_kernel(CstrArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t) blockIdx.x * CSTR_WAVES + (threadIdx.x >> 6);
    if (s > a.n_seq) return;
    if (s == a.n_seq) { if (lane == 0) a.piece_put[a.n_piece] = 0; return; }       // (the scan reads one entry more)
    const uint64_t lo = a.seq_off[s], hi = a.seq_off[s + 1];
    uint64_t len = 0, bad = 0;
    for (uint64_t i = lo + lane; i < hi; i += 64) len += a.piece_len[i], bad += a.piece_bad[i];
    len = cstr_wave_sum(len), bad = cstr_wave_sum(bad);
    const bool put = !bad && (!a.want || a.want[s]);
    for (uint64_t i = lo + lane; i < hi; i += 64) a.piece_put[i] = put? a.piece_len[i] : 0;
    if (lane == 0) a.str_len[s] = bad? ~0ULL : len, a.status[s] = bad != 0;
}

__global__ void cstr_off_kernel(CstrArgs a)
{
    const uint64_t s = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (s <= a.n_seq) a.str_off[s] = a.piece_at[s < a.n_seq? a.seq_off[s] : a.n_piece];
}

// Reads sharded over several handles: CONS_FIRST may name a read of another rank, whose bases this rank does not hold.  Every rank writes the k-mer table of ALL
// selected slots -- the row of a slot whose first uncorrected occurrence lies in one of its own reads holds that occurrence's k-mer in the syncmer's forward
// orientation (cons_str_core.hpp: kmer_word), every other row zeros -- so that the sum of the ranks' tables is the table and no rank has to know who owns what.
// One wave per slot; lane l writes words l, l + 64, ... of the row (k above 1024: more than one): the stores of a wave are consecutive.  Every word of every row is
// written at every run.
struct CstrKmerArgs {
    oatk_cstr::Tables T;          // the reads' side; T.kmer is not read
    uint64_t n_sel, n_reads;
    uint32_t row_words;           // 32-bit words per row: 2 * ceil(k / 32)
    uint32_t *kmer;               // [n_sel * row_words]
};

__global__ __launch_bounds__(64 * CSTR_WAVES) void cstr_kmer_kernel(CstrKmerArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t slot = (uint64_t) blockIdx.x * CSTR_WAVES + (threadIdx.x >> 6);
    if (slot >= a.n_sel) return;
    uint32_t *row = a.kmer + slot * a.row_words;
    const uint64_t o = a.T.first[slot];
    const bool mine = o != ~0ULL && (o >> 32) >= a.T.sid0 && (o >> 32) - a.T.sid0 < a.n_reads;
    if (!mine) {
        for (uint32_t j = lane; j < a.row_words; j += 64) row[j] = 0;
        return;
    }
    const uint8_t *hs;
    const uint32_t mp = oatk_cstr::first_entry(a.T, o, hs);
    for (uint32_t j = lane; j < a.row_words; j += 64) row[j] = oatk_cstr::kmer_word(hs, mp >> 1, mp & 1u, a.T.k, j);
}

__global__ __launch_bounds__(64 * CSTR_WAVES) void cstr_fill_kernel(CstrArgs a)
{
    __shared__ uint64_t s_start[CSTR_WAVES][oatk_cstr::TILE];
    __shared__ uint8_t s_char[CSTR_WAVES][oatk_cstr::TILE];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t i = (uint64_t) blockIdx.x * CSTR_WAVES + w;
    if (i >= a.n_piece) return;
    const uint64_t L = a.piece_put[i];
    if (L == 0) return;                                                    // length only, refused, or empty
    const uint64_t at = a.piece_at[i];
    if (at > a.total || L > a.total - at) return;                          // (cannot happen: the scan made `at`; nothing is written outside CONS_STR)
    uint8_t *dst = a.str + at;
    const oatk_cstr::Piece P = oatk_cstr::open(a.T, a.piece_v[i], a.piece_beg[i], a.hoco_seq);
    if (!P.has_first) {
        for (uint64_t o = lane; o < L; o += 64) dst[o] = 'N';
        return;
    }
    for (uint64_t o = lane; o < P.pad && o < L; o += 64) dst[o] = 'N';
    uint64_t done = P.pad;                                                 // bytes of the piece in front of the tile at hand
    const uint32_t K = (uint32_t) a.T.k;
    for (uint32_t t0 = P.beg0; t0 < K; t0 += oatk_cstr::TILE) {
        const uint32_t t = t0 + lane;
        uint64_t cnt = 0;
        uint8_t ch = 0;
        if (t < K) cnt = oatk_cstr::count_at(a.T, P, t), ch = (uint8_t) oatk_cstr::letter(oatk_cstr::code_at(a.T, P, t));
        uint64_t inc = cnt;                                                // inclusive prefix sum over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t up = (uint64_t) __shfl_up((long long) inc, d);
            if ((int) lane >= d) inc += up;
        }
        const uint64_t tile_total = (uint64_t) __shfl((long long) inc, 63);
        s_start[w][lane] = inc - cnt, s_char[w][lane] = ch;
        cstr_wave_sync();
        for (uint64_t o = lane; o < tile_total; o += 64) {
            const uint32_t j = P.expand? oatk_cstr::find_source(s_start[w], o) : (uint32_t) o;
            if (done + o < L) dst[done + o] = s_char[w][j];
        }
        cstr_wave_sync();                                                  // the next tile overwrites the starts
        done += tile_total;
    }
}

}  // namespace oatk
