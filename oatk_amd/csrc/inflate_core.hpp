// oatk_amd/csrc/inflate_core.hpp -- a DEFLATE decoder (RFC 1951) for ONE BGZF member, in the form the device kernel of inflate.hpp needs: everything that turns
// stream content into an address or a length lives here, compiles for host and device alike (no HIP builtins), and is fuzzed on the CPU under ASan + UBSan against
// zlib (tests/c/inflate_core_fuzz.cpp) before a damaged byte reaches a GPU.
//
// The decoder does not copy: it yields TOKENS -- a literal, a (length, distance) pair, a stored run (input position, length) -- and the caller executes them (the
// kernel wave-wide, the fuzzer with a scalar loop).  What a token says has been checked before it is handed out:
//   * no read passes in + in_len (the bit reader stops there and hands out zeros; taking more bits than were read is an error);
//   * no token writes outside [0, out_len); a distance never reaches before the member's first byte (BGZF members share no window);
//   * over-subscribed code-length sets, block type 3, LEN != ~NLEN, a length other than out_len at the end, a stream that ends early and bytes behind the
//     final block are errors.  Errors are values (ST_*), nothing traps, and every loop is bounded by a constant or by in_len.
// It may refuse what zlib takes (incomplete code sets other than a single 1-bit code); it never accepts a member with other bytes than zlib's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OATK_HD __host__ __device__ inline
#else
#define OATK_HD inline
#endif

namespace oatk_inf {

enum { ST_OK = 0, ST_STREAM = 1, ST_LEN = 2, ST_CRC = 3 };                        // status of a member (include/oatk_hip_ingest.h)
enum { TOK_LIT = 0, TOK_MATCH = 1, TOK_STORED = 2, TOK_NONE = 3, TOK_END = 4, TOK_ERR = 5 };
enum { FAST_BITS = 10, MAX_MEMBER = 65536 };

// Code tables of the block at hand.  fast[]: the next FAST_BITS bits of the stream -> symbol << 4 | code length (0: a longer code, or none); codes longer than
// that are found the canonical way from cnt[] and sym[] (symbols in code order).
struct Tables {
    uint16_t ll_fast[1 << FAST_BITS], d_fast[1 << FAST_BITS];
    uint16_t ll_sym[288], d_sym[32];
    uint16_t ll_cnt[16], d_cnt[16];
    uint8_t lens[320];                      // the code lengths as read: literal/length ones, then the distance ones
};

// ---- bit reader: LSB first, at most 64 bits ahead; bits above cnt are zero ----
struct Bits {
    const uint8_t *in;
    uint32_t len, pos, cnt, a0;             // a0: the address of in[0] modulo 4 (whole aligned words are loaded where there are any)
    uint64_t buf;
};

OATK_HD void bits_refill(Bits &b)
{
    while (b.cnt <= 32) {                   // every turn adds 8 or 32 bits: at most five turns
        if (((b.a0 + b.pos) & 3) == 0 && b.pos + 4 <= b.len) {
            uint32_t w;
            __builtin_memcpy(&w, __builtin_assume_aligned(b.in + b.pos, 4), 4);
            b.buf |= (uint64_t) w << b.cnt, b.cnt += 32, b.pos += 4;
        } else if (b.pos < b.len) {
            b.buf |= (uint64_t) b.in[b.pos] << b.cnt, b.cnt += 8, b.pos += 1;
        } else break;
    }
}

struct Inflater {
    Bits b;
    Tables *t;
    uint32_t out_len, produced;
    uint32_t in_block, final_seen, done;
    uint32_t err;                           // ST_*
    uint32_t n_cross;                       // (statistics, tests) code-length repeats that ran from the literal/length lengths into the distance lengths
};

OATK_HD uint32_t inf_take(Inflater &s, uint32_t n)      // n <= 16
{
    if (n > s.b.cnt) { if (!s.err) s.err = ST_STREAM; return 0; }      // the stream ends early
    const uint32_t v = (uint32_t) s.b.buf & ((1u << n) - 1);
    s.b.buf >>= n, s.b.cnt -= n;
    return v;
}

OATK_HD uint32_t bit_reverse(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < 15; ++i) if (i < n) r = r << 1 | ((v >> i) & 1);
    return r;
}

// canonical code tables from n code lengths (each <= 15).  false: over-subscribed, or incomplete in a way zlib refuses too (zlib takes a single code of one bit;
// no code at all only where allow_empty says so: the distance code of a block of literals)
OATK_HD bool build_tables(const uint8_t *lens, uint32_t n, uint16_t *fast, uint16_t *sym, uint16_t *cnt, bool allow_empty)
{
    uint16_t offs[16];
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    for (uint32_t i = 0; i < n; ++i) cnt[lens[i] & 15]++;
    for (uint32_t i = 0; i < (1u << FAST_BITS); ++i) fast[i] = 0;
    if (cnt[0] == n) return allow_empty;
    int32_t left = 1;
    for (uint32_t l = 1; l < 16; ++l) {
        left = (left << 1) - (int32_t) cnt[l];
        if (left < 0) return false;
    }
    if (left > 0 && !(n - cnt[0] == 1 && cnt[1] == 1)) return false;
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t) (offs[l] + cnt[l]);
    for (uint32_t i = 0; i < n; ++i) if (lens[i] & 15) sym[offs[lens[i] & 15]++] = (uint16_t) i;
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= FAST_BITS; ++l) {
        for (uint32_t k = 0; k < cnt[l]; ++k, ++code) {
            const uint32_t e = (uint32_t) sym[idx++] << 4 | l;
            for (uint32_t j = bit_reverse(code, l); j < (1u << FAST_BITS); j += 1u << l) fast[j] = (uint16_t) e;
        }
        code <<= 1;
    }
    return true;
}

// the next symbol of a code; -1: bits that are no code (or the stream ended)
OATK_HD int32_t inf_symbol(Inflater &s, const uint16_t *fast, const uint16_t *sym, const uint16_t *cnt)
{
    const uint32_t e = fast[(uint32_t) s.b.buf & ((1u << FAST_BITS) - 1)];
    uint32_t n = e & 15;
    int32_t v = (int32_t) (e >> 4);
    if (!n) {                               // a code longer than FAST_BITS, bit by bit from its first (15 turns at most)
        uint32_t code = 0, first = 0, index = 0, bits = (uint32_t) s.b.buf;
        v = -1;
        for (uint32_t l = 1; l <= 15; ++l) {
            code |= bits & 1, bits >>= 1;
            const uint32_t c = cnt[l];
            if (code < first + c) { v = (int32_t) sym[index + (code - first)], n = l; break; }
            index += c, first = (first + c) << 1, code <<= 1;
        }
        if (v < 0) { if (!s.err) s.err = ST_STREAM; return -1; }
    }
    if (n > s.b.cnt) { if (!s.err) s.err = ST_STREAM; return -1; }
    s.b.buf >>= n, s.b.cnt -= n;
    return v;
}

OATK_HD void inf_init(Inflater &s, Tables *t, const uint8_t *in, uint32_t in_len, uint32_t in_align, uint32_t out_len)
{
    s.b.in = in, s.b.len = in_len, s.b.pos = 0, s.b.cnt = 0, s.b.a0 = in_align & 3, s.b.buf = 0;
    s.t = t, s.out_len = out_len, s.produced = 0, s.in_block = 0, s.final_seen = 0, s.done = 0, s.n_cross = 0;
    s.err = in_len > MAX_MEMBER || out_len > MAX_MEMBER? ST_STREAM : ST_OK;
}

// the header of a dynamic block (RFC 1951 3.2.7)
OATK_HD void inf_dynamic(Inflater &s)
{
    Tables &T = *s.t;
    bits_refill(s.b);
    const uint32_t nl = inf_take(s, 5) + 257, nd = inf_take(s, 5) + 1, nc = inf_take(s, 4) + 4;
    if (s.err) return;
    if (nl > 286 || nd > 30) { s.err = ST_STREAM; return; }
    uint8_t cl[19];
    for (uint32_t i = 0; i < 19; ++i) cl[i] = 0;
    for (uint32_t i = 0; i < nc; ++i) {
        const uint32_t order = i < 3? 16 + i : (i == 3? 0 : (i & 1? 8 - ((i - 3) >> 1) : 7 + ((i - 2) >> 1)));      // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        bits_refill(s.b);
        cl[order] = (uint8_t) inf_take(s, 3);
    }
    if (s.err) return;
    if (!build_tables(cl, 19, T.ll_fast, T.d_sym, T.d_cnt, false)) { s.err = ST_STREAM; return; }
    const uint32_t total = nl + nd;
    uint32_t i = 0;
    while (i < total) {                     // every turn writes at least one length or ends with an error
        bits_refill(s.b);
        const int32_t c = inf_symbol(s, T.ll_fast, T.d_sym, T.d_cnt);
        if (c < 0) return;
        if (c < 16) { T.lens[i++] = (uint8_t) c; continue; }
        uint32_t rep, v = 0;
        if (c == 16) { if (i == 0) { s.err = ST_STREAM; return; } v = T.lens[i - 1], rep = 3 + inf_take(s, 2); }
        else if (c == 17) rep = 3 + inf_take(s, 3);
        else rep = 11 + inf_take(s, 7);
        if (s.err) return;
        if (i + rep > total) { s.err = ST_STREAM; return; }
        if (i < nl && i + rep > nl) ++s.n_cross;
        for (uint32_t k = 0; k < rep; ++k) T.lens[i++] = (uint8_t) v;
    }
    if (T.lens[256] == 0) { s.err = ST_STREAM; return; }      // no end-of-block code
    if (!build_tables(T.lens, nl, T.ll_fast, T.ll_sym, T.ll_cnt, false) || !build_tables(T.lens + nl, nd, T.d_fast, T.d_sym, T.d_cnt, true)) s.err = ST_STREAM;
}

OATK_HD void inf_fixed(Inflater &s)
{
    Tables &T = *s.t;
    for (uint32_t i = 0; i < 288; ++i) T.lens[i] = (uint8_t) (i < 144? 8 : (i < 256? 9 : (i < 280? 7 : 8)));
    for (uint32_t i = 0; i < 32; ++i) T.lens[288 + i] = 5;       // (32 codes make the set complete; 30 and 31 are refused where they are used)
    if (!build_tables(T.lens, 288, T.ll_fast, T.ll_sym, T.ll_cnt, false) || !build_tables(T.lens + 288, 32, T.d_fast, T.d_sym, T.d_cnt, false)) s.err = ST_STREAM;
}

// One step.  TOK_LIT: a = the byte.  TOK_MATCH: a = length (3..258), b = distance (1..produced so far).  TOK_STORED: a = length (> 0), b = position of the run in
// the input.  The token's output begins where the tokens before it ended and lies inside [0, out_len).  TOK_NONE: a header or an end of block was read, call again.
// TOK_END: the member is complete, out_len bytes long and nothing follows it.  TOK_ERR: s.err says what.  Every call takes at least one bit of the input or ends the
// member, so 8 * in_len + 8 calls are the most a caller ever needs.
OATK_HD uint32_t inf_next(Inflater &s, uint32_t &a, uint32_t &b)
{
    a = b = 0;
    if (s.err || s.done) return s.err? TOK_ERR : TOK_END;
    bits_refill(s.b);
    if (!s.in_block) {
        if (s.final_seen) {
            if ((s.b.cnt >> 3) + (s.b.len - s.b.pos) != 0) s.err = ST_STREAM;       // bytes behind the final block
            else if (s.produced != s.out_len) s.err = ST_LEN;
            s.done = 1;
            return s.err? TOK_ERR : TOK_END;
        }
        const uint32_t hdr = inf_take(s, 3);
        if (s.err) return TOK_ERR;
        s.final_seen = hdr & 1;
        const uint32_t type = hdr >> 1;
        if (type == 0) {
            (void) inf_take(s, s.b.cnt & 7);                                        // to the byte boundary
            bits_refill(s.b);
            const uint32_t len = inf_take(s, 16), nlen = inf_take(s, 16);
            if (s.err) return TOK_ERR;
            if ((len ^ nlen) != 0xFFFFu) { s.err = ST_STREAM; return TOK_ERR; }
            const uint32_t at = s.b.pos - (s.b.cnt >> 3);                           // (cnt is a multiple of 8 here)
            if (len > s.b.len - at) { s.err = ST_STREAM; return TOK_ERR; }          // the stream ends inside the run
            if (len > s.out_len - s.produced) { s.err = ST_LEN; return TOK_ERR; }
            s.b.pos = at + len, s.b.cnt = 0, s.b.buf = 0;
            s.produced += len;
            a = len, b = at;
            return len? TOK_STORED : TOK_NONE;
        }
        if (type == 1) inf_fixed(s);
        else if (type == 2) inf_dynamic(s);
        else s.err = ST_STREAM;
        if (s.err) return TOK_ERR;
        s.in_block = 1;
        return TOK_NONE;
    }
    const Tables &T = *s.t;
    const int32_t c = inf_symbol(s, T.ll_fast, T.ll_sym, T.ll_cnt);
    if (c < 0) return TOK_ERR;
    if (c < 256) {
        if (s.produced >= s.out_len) { s.err = ST_LEN; return TOK_ERR; }
        s.produced += 1;
        a = (uint32_t) c;
        return TOK_LIT;
    }
    if (c == 256) { s.in_block = 0; return TOK_NONE; }
    if (c > 285) { s.err = ST_STREAM; return TOK_ERR; }
    uint32_t len;
    if (c < 265) len = (uint32_t) c - 254;
    else if (c == 285) len = 258;
    else { const uint32_t e = ((uint32_t) c - 261) >> 2; len = 3 + ((4 + (((uint32_t) c - 261) & 3)) << e) + inf_take(s, e); }
    bits_refill(s.b);
    const int32_t d = inf_symbol(s, T.d_fast, T.d_sym, T.d_cnt);
    if (d < 0) return TOK_ERR;
    if (d > 29) { s.err = ST_STREAM; return TOK_ERR; }
    uint32_t dist;
    if (d < 4) dist = (uint32_t) d + 1;
    else {
        const uint32_t e = ((uint32_t) d >> 1) - 1;      // up to 13 extra bits
        dist = 1 + ((2 + ((uint32_t) d & 1)) << e) + inf_take(s, e);
    }
    if (s.err) return TOK_ERR;
    if (dist > s.produced) { s.err = ST_STREAM; return TOK_ERR; }                   // reaches before the member's first byte
    if (len > s.out_len - s.produced) { s.err = ST_LEN; return TOK_ERR; }
    s.produced += len;
    a = len, b = dist;
    return TOK_MATCH;
}

// ---- CRC-32 (the zlib polynomial, reflected), in pieces ----
// A piece's CRC register is taken on its own (the first piece starts from 0xFFFFFFFF, the others from 0); feeding n zero bytes to a register is multiplying it by
// x^(8n) modulo the polynomial, which is how the pieces combine (zlib: crc32_combine).  x2n[k] = x^(2^k) is the precomputed operator table.
#define OATK_CRC_POLY 0xEDB88320u

OATK_HD uint32_t crc_table_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = c & 1? (c >> 1) ^ OATK_CRC_POLY : c >> 1;
    return c;
}

OATK_HD uint32_t crc_bytes(const uint32_t *tab, uint32_t c, const uint8_t *p, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c;
}

OATK_HD uint32_t crc_mul(uint32_t a, uint32_t b)       // a * b modulo the polynomial, reflected bit order (bit 31 is x^0)
{
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = b & 1? (b >> 1) ^ OATK_CRC_POLY : b >> 1;
    }
    return p;
}

OATK_HD void crc_x2n_table(uint32_t *x2n)              // 32 entries
{
    uint32_t p = 0x40000000u;                          // x^1
    x2n[0] = p;
    for (uint32_t k = 1; k < 32; ++k) x2n[k] = p = crc_mul(p, p);
}

OATK_HD uint32_t crc_shift_op(const uint32_t *x2n, uint32_t n_bytes)      // x^(8 n_bytes), n_bytes < 2^28
{
    uint32_t p = 0x80000000u;                          // x^0
    const uint32_t m = n_bytes << 3;
    for (uint32_t k = 0; k < 31; ++k) if ((m >> k) & 1) p = crc_mul(x2n[k], p);
    return p;
}

}  // namespace oatk_inf
