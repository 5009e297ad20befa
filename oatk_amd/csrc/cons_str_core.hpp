// oatk_amd/csrc/cons_str_core.hpp -- what decides the text of one piece of a consensus sequence: a piece is (v = syncmer id << 1 | rev, beg), the part of
// scg_syncmer_consensus(scm, rev, beg) (syncasm.c:888-1001) that a unitig's string is made of.  Whether the piece is prepared, how long it is, and which
// character stands at any offset inside it are decided here and nowhere else: the device kernels (cons_str.hpp) and the CPU check
// (tests/c/cons_str_core_check.cpp, under ASan + UBSan) run these functions.  Like bam_core.hpp it compiles for host and device alike.
//
// The piece, in the reference's words: max(-beg, 0) letters 'N'; then positions t = max(beg, 0) .. k - 1 of the k-mer of the syncmer's first uncorrected
// occurrence, oriented by `rev` (the 2-bit code complemented when the occurrence's strand XOR rev is 1), every base 1 + rl[t] times in base space (rl: the rounded
// mean run length of the FORWARD k-mer, so a reverse request reads index k - 1 - t) and once in hoco space.  A syncmer without such an occurrence (:924-930) gives
// k - max(beg, 0) letters 'N' behind the padding.
//
// With reads sharded over several handles the occurrence may lie in another rank's reads: kmer_word is the one definition of a syncmer's own k-mer as a row of a
// table (cons_str.hpp: cstr_kmer_kernel writes it, the ranks add their tables up), and open() reads the letters from that row when Tables::kmer is set
// (tests/c/cons_kmer_core_check.cpp).
#pragma once
#include <stdint.h>

#ifndef OATK_HD
#if defined(__HIPCC__)
#define OATK_HD __host__ __device__ inline
#else
#define OATK_HD inline
#endif
#endif

namespace oatk_cstr {

enum { NO_SLOT = 0xFFFFFFFFu, TILE = 64 };                                 // TILE: positions a wave takes at a time (cons_str.hpp)

// the arrays a piece is read from: the consensus tables (include/oatk_hip_cons.h) and the reads they point into
struct Tables {
    uint64_t n_scm;
    int k;
    const uint32_t *slot;         // [n_scm] CONS_SLOT
    const uint32_t *rl;           // [n_sel * k] CONS_RL
    const uint32_t *m_seq;        // [n_sel] CONS_MSEQ
    const uint64_t *first;        // [n_sel] CONS_FIRST: sid << 32 | idx << 1 | rev, ~0 if none
    uint64_t sid0;
    const uint64_t *chain_off;    // [n_reads] first chain entry of a read
    const uint32_t *m_pos;        // chain entries: hoco position << 1 | strand
    const uint64_t *off;          // [n_reads] offset of a read in the packed stream; its hoco string starts at byte off / 4 of hoco_s
    const uint8_t *hoco_s;        // 2-bit bases, four to a byte, the first in the top bits
    // the second source of the letters, for reads sharded over several handles (CONS_FIRST may name a read of another rank): row `slot` holds the syncmer's own
    // k-mer in its forward orientation, laid out like hoco_s (kmer_word below).  nullptr: the letters come from the reads
    const uint8_t *kmer = nullptr;        // [n_sel * kmer_stride] CONS_KMER
    uint64_t kmer_stride = 0;     // bytes per row
};

struct Piece {
    uint32_t slot;                // NO_SLOT: not prepared
    uint32_t rev;
    uint32_t beg0;                // max(beg, 0): the first k-mer position that is written
    uint64_t pad;                 // max(-beg, 0) letters 'N' in front
    bool has_first;               // false: N's only
    bool expand;                  // base space and run lengths to apply
    uint32_t flip;                // the occurrence's strand XOR rev
    uint64_t p;                   // hoco position of the k-mer on its read
    const uint8_t *hs;            // the read's hoco string
};

OATK_HD bool prepared(const Tables &T, uint64_t v) { return (v >> 1) < T.n_scm && T.slot[v >> 1] != (uint32_t) NO_SLOT; }

// the chain entry a CONS_FIRST word o != ~0 names (hoco position << 1 | strand) and its read's hoco string; the read must be one of T's own
OATK_HD uint32_t first_entry(const Tables &T, uint64_t o, const uint8_t *&hs)
{
    const uint64_t rd = (o >> 32) - T.sid0;
    hs = T.hoco_s + (T.off[rd] >> 2);
    return T.m_pos[T.chain_off[rd] + ((o >> 1) & 0x7FFFFFFFULL)];
}

// beg < k is the caller's to check (the reference asserts it)
OATK_HD Piece open(const Tables &T, uint64_t v, int32_t beg, int hoco_seq)
{
    Piece P;
    P.slot = prepared(T, v)? T.slot[v >> 1] : (uint32_t) NO_SLOT;
    P.rev = (uint32_t) (v & 1);
    P.beg0 = beg > 0? (uint32_t) beg : 0u;
    P.pad = beg < 0? (uint64_t) (-(int64_t) beg) : 0;
    P.has_first = false, P.expand = false, P.flip = 0, P.p = 0, P.hs = nullptr;
    if (P.slot == (uint32_t) NO_SLOT) return P;
    const uint64_t o = T.first[P.slot];
    if (o == ~0ULL) return P;
    P.has_first = true;
    P.expand = !hoco_seq && T.m_seq[P.slot] != 0;
    if (T.kmer) {                                                          // the stored row is the forward k-mer: position 0, strand 0
        P.flip = P.rev, P.p = 0, P.hs = T.kmer + (uint64_t) P.slot * T.kmer_stride;
        return P;
    }
    const uint32_t mp = first_entry(T, o, P.hs);
    P.flip = (mp & 1u) ^ P.rev;
    P.p = mp >> 1;
    return P;
}

// position t of the oriented k-mer (0 <= t < k): its 2-bit code, and how often it stands in the output
OATK_HD uint32_t code_at(const Tables &T, const Piece &P, uint32_t t)
{
    const uint64_t q = P.flip? P.p + (uint64_t) ((uint32_t) T.k - 1u - t) : P.p + (uint64_t) t;      // get_kmer_seq, syncmer.c:1218-1235
    const uint32_t c = (P.hs[q >> 2] >> (((q & 3) ^ 3) << 1)) & 3u;
    return P.flip? c ^ 3u : c;
}
// codes q .. q + n - 1 (1 <= n <= 16) of a packed string, the first in the top two bits of the result, zeros behind the last: a funnel shift over the bytes
// q >> 2 .. (q + n - 1) >> 2, at most five, and no other byte is loaded
OATK_HD uint32_t codes_from(const uint8_t *hs, uint64_t q, uint32_t n)
{
    const uint64_t b0 = q >> 2, b1 = (q + n - 1) >> 2;
    uint64_t acc = 0;
    for (uint64_t b = b0; b <= b1; ++b) acc |= (uint64_t) hs[b] << (56 - 8 * (uint32_t) (b - b0));
    const uint32_t w = (uint32_t) ((acc << ((q & 3) << 1)) >> 32);
    return n < 16? w & ~(0xFFFFFFFFu >> (n << 1)) : w;
}
// Word j of the k-mer of a chain entry (hs, p: hoco position, flip: its strand) in the syncmer's forward orientation: the codes code_at gives for rev = 0 at
// positions 16 j .. 16 j + 15, zeros past k - 1, as the four bytes a 32-bit store puts into memory -- so a table of such rows is laid out like hoco_s (four codes to
// a byte, the first in the top bits) and code_at reads a row with p = 0.  flip: the window is read backwards (p + k - 1 - t) and complemented.
OATK_HD uint32_t kmer_word(const uint8_t *hs, uint64_t p, uint32_t flip, int k, uint32_t j)
{
    const uint32_t t0 = j << 4;
    if (t0 >= (uint32_t) k) return 0;
    const uint32_t n = (uint32_t) k - t0 < 16u? (uint32_t) k - t0 : 16u;
    uint32_t w;
    if (!flip) w = codes_from(hs, p + t0, n);
    else {
        w = codes_from(hs, p + ((uint32_t) k - t0 - n), n);                // positions p + k - 1 - t for t = t0 + n - 1 .. t0
        w = ((w >> 2) & 0x33333333u) | ((w & 0x33333333u) << 2);           // the sixteen codes in reverse order: the n that count end up at the bottom
        w = ((w >> 4) & 0x0F0F0F0Fu) | ((w & 0x0F0F0F0Fu) << 4);
        w = __builtin_bswap32(w);
        w = ~w << ((16 - n) << 1);                                         // complemented, moved to the top; the shift fills the tail with zeros
    }
    return __builtin_bswap32(w);                                           // the first four codes in the byte at the lowest address
}
OATK_HD uint64_t count_at(const Tables &T, const Piece &P, uint32_t t)
{
    if (!P.expand) return 1;
    return 1ULL + T.rl[(uint64_t) P.slot * (uint64_t) T.k + (P.rev? (uint32_t) T.k - 1u - t : t)];
}
OATK_HD char letter(uint32_t code) { return (char) (0x54474341u >> (code << 3)); }      // "ACGT"

// length of the piece (0 for an unprepared one): what scg_syncmer_consensus returns
OATK_HD uint64_t length(const Tables &T, const Piece &P)
{
    if (P.slot == (uint32_t) NO_SLOT) return 0;
    uint64_t l = P.pad + ((uint64_t) T.k - P.beg0);
    if (P.has_first && P.expand)
        for (uint32_t t = P.beg0; t < (uint32_t) T.k; ++t) l += count_at(T, P, t) - 1;
    return l;
}

// the character at offset o of the piece, 0 <= o < length (a walk over the positions: the kernels use find_source on a tile's starts instead)
OATK_HD char char_at(const Tables &T, const Piece &P, uint64_t o)
{
    if (o < P.pad || !P.has_first) return 'N';
    o -= P.pad;
    if (!P.expand) return letter(code_at(T, P, P.beg0 + (uint32_t) o));
    uint32_t t = P.beg0;
    for (;; ++t) {
        const uint64_t c = count_at(T, P, t);
        if (o < c) break;
        o -= c;
    }
    return letter(code_at(T, P, t));
}

// starts[0 .. TILE) ascending, starts[0] <= o: the last j with starts[j] <= o, in six steps.  With starts the exclusive prefix sums of a tile's counts (positions
// past the k-mer's end counting 0, so that they start at the tile's total) this is the position whose run covers output offset o < total.
OATK_HD uint32_t find_source(const uint64_t *starts, uint64_t o)
{
    uint32_t j = 0;
    for (uint32_t step = TILE / 2; step; step >>= 1)
        if (starts[j + step] <= o) j += step;
    return j;
}

}  // namespace oatk_cstr
