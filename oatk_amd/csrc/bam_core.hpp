// oatk_amd/csrc/bam_core.hpp -- what decides, from the bytes of an inflated unaligned BAM stream, where a record starts, whether it is one, and which letters it
// holds: the header walk, the two predicates whole(o) / ok(o), the classification of the place the record chain stops at, and the nibble -> letter tables.  Like
// inflate_core.hpp it compiles for host and device alike and is run on the CPU under ASan + UBSan (tests/c/bam_core_check.cpp) over every stream the GPU tests use,
// damaged ones included, before such bytes reach a GPU.
//
// Layout (SAM/BAM specification, all integers little-endian): magic "BAM\1", l_text i32, text, n_ref i32, n_ref x { l_name i32, name, l_ref i32 }, then records:
//   +0 block_size i32 (the bytes behind it)  +12 l_read_name u8 (with the NUL)  +16 n_cigar_op u16  +18 flag u16  +20 l_seq u32  +36 read_name, cigar[4 n_cigar_op],
//   seq[(l_seq + 1) / 2] (two bases a byte, the first in the high nibble), qual[l_seq], tags.
// Every function reads only bytes of [b, b + n): a field is looked at after the fields that bound it have been checked.
#pragma once
#include <stdint.h>

#ifndef OATK_HD
#if defined(__HIPCC__)
#define OATK_HD __host__ __device__ inline
#else
#define OATK_HD inline
#endif
#endif

namespace oatk_bam {

enum { MIN_BLOCK = 32, MAX_BLOCK = 1 << 28, FIXED = 36 };                 // FIXED: block_size and the fixed fields in front of the read name
enum { REFUSED_FLAGS = 0x910 };                                           // reverse-complemented, secondary, supplementary: samtools fasta would reverse or drop it
enum { STOP_CLEAN = 0, STOP_CUT = 1, STOP_BAD = 2, STOP_NONE = 3 };       // what the chain stops at (STOP_NONE: it does not stop here, the record is fine)
enum { HDR_OK = 0, HDR_MORE = 1, HDR_BAD = 2 };

OATK_HD uint32_t ld16(const uint8_t *p) { return (uint32_t) p[0] | (uint32_t) p[1] << 8; }
OATK_HD uint32_t ld32(const uint8_t *p) { return (uint32_t) p[0] | (uint32_t) p[1] << 8 | (uint32_t) p[2] << 16 | (uint32_t) p[3] << 24; }

// block_size as an unsigned number: a negative one is larger than MAX_BLOCK
OATK_HD bool size_in_range(uint32_t bs) { return bs >= (uint32_t) MIN_BLOCK && bs <= (uint32_t) MAX_BLOCK; }

// whole(o): a block_size field lies at o, is in range, and the block it announces ends inside the chunk
OATK_HD bool whole(const uint8_t *b, uint64_t n, uint64_t o, uint32_t *block_size)
{
    if (o > n || n - o < 4) return false;
    const uint32_t bs = ld32(b + o);
    *block_size = bs;
    return size_in_range(bs) && (uint64_t) bs <= n - o - 4;
}

// ok(o): whole(o), a name of at least its NUL, the variable parts fit the block, and the name ends in NUL
OATK_HD bool ok(const uint8_t *b, uint64_t n, uint64_t o)
{
    uint32_t bs;
    if (!whole(b, n, o, &bs)) return false;
    const uint64_t lrn = b[o + 12], ncig = ld16(b + o + 16), lseq = ld32(b + o + 20);
    if (lrn < 1) return false;
    if (32 + lrn + 4 * ncig + (lseq + 1) / 2 + lseq > (uint64_t) bs) return false;
    return b[o + FIXED + lrn - 1] == 0;
}

// next(o) of an offset for which whole(o) holds
OATK_HD uint64_t next(const uint8_t *b, uint64_t o) { return o + 4 + (uint64_t) ld32(b + o); }

// What the chain's walk meets at t (t <= n): the clean end, a record cut by the end of the chunk, something that is no record -- or a record (STOP_NONE).
OATK_HD int classify(const uint8_t *b, uint64_t n, uint64_t t)
{
    if (t == n) return STOP_CLEAN;
    if (n - t < 4) return STOP_CUT;
    const uint32_t bs = ld32(b + t);
    if (!size_in_range(bs)) return STOP_BAD;
    if ((uint64_t) bs > n - t - 4) return STOP_CUT;
    return ok(b, n, t)? STOP_NONE : STOP_BAD;
}

// The fields the record kernel and the unpack kernel take from a record for which ok(o) holds
struct Rec { uint32_t l_seq, flag; uint64_t seq_at; };                     // seq_at: offset of the packed bases in the chunk
OATK_HD Rec record(const uint8_t *b, uint64_t o)
{
    Rec r;
    r.l_seq = ld32(b + o + 20), r.flag = ld16(b + o + 18);
    r.seq_at = o + FIXED + (uint64_t) b[o + 12] + 4 * (uint64_t) ld16(b + o + 16);
    return r;
}

// The header in the first `have` bytes of the stream.  HDR_OK: *len is where the first record starts.  HDR_MORE: it is not whole in these bytes -- *need is the least
// number of bytes that lets the walk go one step further.  HDR_BAD: a wrong magic or a negative length.
inline int header_walk(const uint8_t *b, uint64_t have, uint64_t *len, uint64_t *need)
{
    static const uint8_t magic[4] = {'B', 'A', 'M', 1};
    *len = 0, *need = 0;
    for (uint64_t i = 0; i < 4 && i < have; ++i) if (b[i] != magic[i]) return HDR_BAD;
    if (have < 8) { *need = 8; return HDR_MORE; }
    const uint32_t l_text = ld32(b + 4);
    if (l_text & 0x80000000u) return HDR_BAD;
    uint64_t p = 8 + (uint64_t) l_text;
    if (have < p + 4) { *need = p + 4; return HDR_MORE; }
    const uint32_t n_ref = ld32(b + p);
    if (n_ref & 0x80000000u) return HDR_BAD;
    p += 4;
    for (uint32_t r = 0; r < n_ref; ++r) {                                // (every turn needs four more bytes than the one before: bounded by have)
        if (have < p + 4) { *need = p + 4; return HDR_MORE; }
        const uint32_t l_name = ld32(b + p);
        if (l_name & 0x80000000u) return HDR_BAD;
        p += 4 + (uint64_t) l_name + 4;
    }
    if (have < p) { *need = p; return HDR_MORE; }
    *len = p;
    return HDR_OK;
}

// ---- nibble -> letter: "=ACMGRSVTWYHKDBN", sixteen bytes held in registers ----
#define OATK_BAM_T0 0x4D43413Du           /* = A C M */
#define OATK_BAM_T1 0x56535247u           /* G R S V */
#define OATK_BAM_T2 0x48595754u           /* T W Y H */
#define OATK_BAM_T3 0x4E42444Bu           /* K D B N */

// one code: two 64-bit constants and a shift (the tail of a read, the CPU's check)
OATK_HD uint8_t letter(uint32_t code)
{
    const uint64_t lo = (uint64_t) OATK_BAM_T1 << 32 | OATK_BAM_T0, hi = (uint64_t) OATK_BAM_T3 << 32 | OATK_BAM_T2;
    return (uint8_t) (((code & 8u)? hi : lo) >> ((code & 7u) * 8u));
}

// v_perm_b32: byte i of the result is byte sel[i] of the eight bytes { hi : lo } for selectors 0 .. 7 (the only ones used here)
OATK_HD uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = (uint64_t) hi << 32 | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint32_t) ((v >> (((sel >> (8 * i)) & 7u) * 8u)) & 0xFFu) << (8 * i);
    return r;
#endif
}

// four codes, one a byte -> their four letters
OATK_HD uint32_t letters4(uint32_t codes)
{
    const uint32_t sel = codes & 0x07070707u;
    const uint32_t a = perm(OATK_BAM_T1, OATK_BAM_T0, sel), c = perm(OATK_BAM_T3, OATK_BAM_T2, sel);
    const uint32_t m = ((codes >> 3) & 0x01010101u) * 0xFFu;              // 0xFF in the bytes whose code is 8 .. 15
    return (a & ~m) | (c & m);
}

// four source bytes (w, little-endian) -> their eight letters in stream order: out[0] the first four
OATK_HD void unpack8(uint32_t w, uint32_t out[2])
{
    const uint32_t h = letters4((w >> 4) & 0x0F0F0F0Fu), l = letters4(w & 0x0F0F0F0Fu);      // first and second base of each byte
    out[0] = perm(l, h, 0x05010400u);
    out[1] = perm(l, h, 0x07030602u);
}

}  // namespace oatk_bam
