// oatk_amd/csrc/inflate.hpp -- BGZF members inflated on the device, one wave per member (include/oatk_hip_ingest.h: oatk_hip_inflate_bgzf).
//
// A BGZF member is a DEFLATE stream of at most 64 KiB that references nothing outside itself, so a file is as many independent streams as it has members.  Inside a
// member the Huffman decoding is serial; copying is not.  The wave stages the member's compressed bytes in LDS (the decoding lane never waits for global memory),
// lane 0 runs the token decoder of inflate_core.hpp over them and fills a batch of up to 64 tokens with their output offsets (a running sum), and the wave executes
// the batch: every literal at once, then the matches and stored runs in order, each wave-wide.  The member's text is built in LDS -- a match sees what earlier tokens
// wrote because LDS operations of one wave complete in order and a barrier separates the phases -- its CRC-32 is taken there in 64 pieces that are combined with the
// "append n zero bytes" operators, and it is written out once, 16 bytes per lane.  64 KiB of text + 64 KiB of input + tables is one member per CU at a time: the
// obviously correct form, the baseline every other form has to beat on a measurement.
//
// Memory safety: every offset that depends on the stream is checked in inflate_core.hpp before the token is handed out; what this file adds are the staging and
// write-out loops, bounded by in_len and out_len, which the host has checked against the buffers' sizes (and which are checked against the LDS arrays here again).
#pragma once
#include "common.hpp"
#include "inflate_core.hpp"
#include "../../include/oatk_hip_ingest.h"

namespace oatk {

constexpr uint32_t INF_PIECE = 1024;        // bytes of text per lane for the CRC: 64 lanes cover the largest member

struct InfShared {
    uint8_t out[oatk_inf::MAX_MEMBER + 16];     // the text, at the 16-byte phase of its place in global memory
    uint8_t in[oatk_inf::MAX_MEMBER + 16];      // the compressed bytes, at the 16-byte phase of theirs
    oatk_inf::Tables tab;
    uint32_t crc_tab[256], x2n[32];
    uint32_t tok[64], arg[64], off[64];         // a batch: kind | length << 2; literal byte / distance / input position; output offset
    uint32_t ctl[4];                            // tokens in the batch; the member has ended; its status
};

// res[0]: members with a status other than 0; res[1]: the last byte of member `last` (the member that ends the text)
__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t *__restrict__ comp, const oatk_bgzf_member_t *__restrict__ mem, uint8_t *__restrict__ text,
                                                          const uint32_t *__restrict__ x2n, uint8_t *__restrict__ status, uint32_t *__restrict__ res, uint64_t last)
{
    using namespace oatk_inf;
    __shared__ __attribute__((aligned(16))) InfShared S;
    const uint64_t m = blockIdx.x;
    const int lane = threadIdx.x;
    const oatk_bgzf_member_t M = mem[m];
    if (M.in_len > MAX_MEMBER || M.out_len > MAX_MEMBER) {      // (the host refuses such a table: never taken)
        if (lane == 0) { status[m] = ST_STREAM; atomicAdd(&res[0], 1u); }
        return;
    }
    // ---- stage: whole 16-byte granules of global memory; each holds at least one byte of the member, so none lies outside the pages the buffer occupies ----
    const uint8_t *src = comp + M.in_off;
    const uint32_t ph_in = (uint32_t) ((uintptr_t) src & 15);
    if (M.in_len) {
        const uint4 *g = (const uint4 *) (src - ph_in);
        const uint32_t n16 = (ph_in + M.in_len + 15) >> 4;      // <= (15 + 65536 + 15) / 16 = 4097 granules = sizeof(S.in)
        for (uint32_t c = lane; c < n16; c += 64) ((uint4 *) S.in)[c] = g[c];
    }
    for (uint32_t i = lane; i < 256; i += 64) S.crc_tab[i] = crc_table_entry(i);
    if (lane < 32) S.x2n[lane] = x2n[lane];
    uint8_t *dst = text + M.out_off;
    const uint32_t ph_out = (uint32_t) ((uintptr_t) dst & 15);
    uint8_t *out = S.out + ph_out;
    const uint8_t *in = S.in + ph_in;
    __syncthreads();

    // ---- decode: lane 0 fills a batch, the wave executes it ----
    Inflater inf;
    inf_init(inf, &S.tab, in, M.in_len, ph_in, M.out_len);
    uint32_t calls_left = 8 * M.in_len + 16;                    // inf_next takes at least a bit per call
    for (;;) {
        if (lane == 0) {
            uint32_t nt = 0, ended = 0;
            while (nt < 64) {
                if (calls_left == 0) { if (!inf.err) inf.err = ST_STREAM; ended = 1; break; }
                --calls_left;
                const uint32_t o = inf.produced;
                uint32_t a, b;
                const uint32_t k = inf_next(inf, a, b);
                if (k == TOK_NONE) continue;
                if (k >= TOK_END) { ended = 1; break; }
                S.tok[nt] = k == TOK_LIT? (uint32_t) TOK_LIT : (k | a << 2), S.arg[nt] = k == TOK_LIT? a : b, S.off[nt] = o;
                ++nt;
            }
            S.ctl[0] = nt, S.ctl[1] = ended, S.ctl[2] = inf.err;
        }
        __syncthreads();
        const uint32_t nt = S.ctl[0], ended = S.ctl[1];
        const uint32_t tk = (uint32_t) lane < nt? S.tok[lane] : (uint32_t) TOK_LIT;
        if ((uint32_t) lane < nt && (tk & 3) == TOK_LIT) out[S.off[lane]] = (uint8_t) S.arg[lane];
        uint64_t copies = __ballot((uint32_t) lane < nt && (tk & 3) != TOK_LIT);
        __syncthreads();
        while (copies) {                                        // (the same in every lane)
            const int i = __builtin_ctzll(copies);
            copies &= copies - 1;
            const uint32_t t = S.tok[i], len = t >> 2, a = S.arg[i], o = S.off[i];
            if ((t & 3) == TOK_MATCH) {                         // a = distance <= o; o + len <= out_len
                const uint8_t *from = out + (o - a);
                if (a >= len) for (uint32_t j = lane; j < len; j += 64) out[o + j] = from[j];
                else for (uint32_t j = lane; j < len; j += 64) out[o + j] = from[j % a];      // the source period, all of it written before this token
            } else {                                            // a = position in the input; a + len <= in_len
                for (uint32_t j = lane; j < len; j += 64) out[o + j] = in[a + j];
            }
            __syncthreads();
        }
        if (ended) break;
    }
    uint32_t st = S.ctl[2];
    const uint32_t n = M.out_len;

    // ---- CRC-32 of the text against the member's trailer ----
    if (st == ST_OK) {
        const uint32_t beg = (uint32_t) lane * INF_PIECE, end = beg + INF_PIECE < n? beg + INF_PIECE : n;
        uint32_t c = lane == 0? 0xFFFFFFFFu : 0u;
        if (beg < end) c = crc_bytes(S.crc_tab, c, out + beg, end - beg);
        uint32_t term = beg < end || lane == 0? crc_mul(c, crc_shift_op(S.x2n, n - end)) : 0u;
        for (int d = 1; d < OATK_WAVE; d <<= 1) term ^= (uint32_t) __shfl_xor((int) term, d);
        if ((term ^ 0xFFFFFFFFu) != M.crc) st = ST_CRC;
    }
    // ---- the text to its place: bytes up to the first 16-byte boundary, whole granules, the rest ----
    if (st == ST_OK || st == ST_CRC) {
        const uint32_t head = ((16 - ph_out) & 15) < n? ((16 - ph_out) & 15) : n, n16 = (n - head) >> 4, tail = head + (n16 << 4);
        if ((uint32_t) lane < head) dst[lane] = out[lane];
        for (uint32_t c = lane; c < n16; c += 64) ((uint4 *) (dst + head))[c] = ((const uint4 *) (out + head))[c];
        if (tail + lane < n) dst[tail + lane] = out[tail + lane];
    }
    if (lane == 0) {
        status[m] = (uint8_t) st;
        if (st) atomicAdd(&res[0], 1u);
        if (m == last && n) res[1] = st == ST_OK || st == ST_CRC? out[n - 1] : 0u;
    }
}

}  // namespace oatk
