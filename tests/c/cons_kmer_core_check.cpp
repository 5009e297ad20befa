// tests/c/cons_kmer_core_check.cpp -- the k-mer rows of oatk_amd/csrc/cons_str_core.hpp on the CPU, under ASan + UBSan (tests/test_host_cons_kmer_core.py builds and
// runs it).  kmer_word is what cstr_kmer_kernel (csrc/cons_str.hpp) stores for reads sharded over several handles, and open() with Tables::kmer set is what the string
// kernels read then.  Checked here, for one k and every source phase p & 3 and both strands:
//   1. every word of a row against a restatement that takes one code at a time (p + t, or p + k - 1 - t complemented), the codes behind k - 1 zero, the row as wide as
//      the table's stride (8 * ceil(k / 32) bytes);
//   2. code_at on the stored row with p = 0, for rev 0 and 1, against code_at on the read itself;
//   3. over a small table of reads and syncmers, the text of every piece (syncmer x rev x beg x space) from a Tables whose kmer is set against the read-backed one.
// A source string sits in a heap block that ends with the k-mer's last byte, and for p < 4 begins with its first: a load outside [p >> 2, (p + k - 1) >> 2] is a
// sanitizer report.
//
// usage: cons_kmer_core_check <k> <seed>
// output: one line  OK words=<row words compared> codes=<codes compared> tail=<zero codes behind k - 1> phases=<bit mask of p & 3 seen: strand 0 bits 0-3, strand 1
//         bits 4-7> pieces=<pieces compared> chars=<their characters> nofirst=<pieces without a first occurrence>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "cons_str_core.hpp"

using namespace oatk_cstr;

static uint64_t rng_state;
static uint32_t rnd(uint32_t n)                                           // xorshift64*
{
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return (uint32_t) ((rng_state * 2685821657736338717ULL) >> 33) % n;
}

template <class T> static T *exact(const std::vector<T> &v)               // a heap block of exactly the vector's size
{
    T *p = (T *) malloc(v.size() * sizeof(T) + (v.empty()? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static uint32_t code_of(const uint8_t *s, uint64_t q) { return (s[q >> 2] >> (((q & 3) ^ 3) << 1)) & 3u; }

static uint64_t n_words, n_codes, n_tail, phases;

// one k-mer at hoco position p of a string made for it; false on a mismatch
static bool one_kmer(int k, uint64_t p, uint32_t strand)
{
    const uint64_t nb = ((p + (uint64_t) k - 1) >> 2) + 1;                 // the block ends with the k-mer's last byte
    uint8_t *hs = (uint8_t *) malloc(nb);
    for (uint64_t b = 0; b < nb; ++b) hs[b] = (uint8_t) rnd(256);
    const uint32_t row_words = 2 * (((uint32_t) k + 31) / 32);
    uint32_t *row = (uint32_t *) malloc(row_words * sizeof(uint32_t));
    for (uint32_t j = 0; j < row_words; ++j) row[j] = kmer_word(hs, p, strand, k, j);
    const uint8_t *rb = (const uint8_t *) row;                            // the row as it lies in memory
    bool ok = true;
    for (uint32_t t = 0; t < 16 * row_words && ok; ++t) {
        const uint32_t got = code_of(rb, t);
        if (t < (uint32_t) k) {
            const uint32_t want = strand? 3u ^ code_of(hs, p + (uint64_t) (k - 1) - t) : code_of(hs, p + t);
            if (got != want) { printf("FAIL k=%d p=%lu strand=%u: code %u is %u, restated %u\n", k, (unsigned long) p, strand, t, got, want); ok = false; }
            ++n_codes;
        } else {
            if (got) { printf("FAIL k=%d p=%lu strand=%u: code %u behind the k-mer is %u\n", k, (unsigned long) p, strand, t, got); ok = false; }
            ++n_tail;
        }
    }
    // the stored row read back by code_at: position 0, strand 0
    Tables T;
    T.k = k;
    for (uint32_t rev = 0; rev < 2 && ok; ++rev) {
        Piece Pr, Pk;
        Pr.hs = hs, Pr.p = p, Pr.flip = strand ^ rev;
        Pk.hs = rb, Pk.p = 0, Pk.flip = rev;
        for (uint32_t t = 0; t < (uint32_t) k && ok; ++t)
            if (code_at(T, Pr, t) != code_at(T, Pk, t)) { printf("FAIL k=%d p=%lu strand=%u rev=%u: code_at %u differs on the row\n", k, (unsigned long) p, strand, rev, t); ok = false; }
    }
    n_words += row_words, phases |= 1ULL << ((p & 3) + 4 * strand);
    free(row); free(hs);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <k> <seed>\n", argv[0]); return 2; }
    const int k = atoi(argv[1]);
    rng_state = 0x9E3779B97F4A7C15ULL ^ (uint64_t) atoll(argv[2]) * 1000003ULL;
    if (k < 5) return 2;

    // ---- 1, 2: rows ----
    for (uint32_t ph = 0; ph < 4; ++ph)
        for (uint32_t strand = 0; strand < 2; ++strand) {
            if (!one_kmer(k, ph, strand)) return 1;                        // the k-mer's first byte is the block's first
            for (int rep = 0; rep < 3; ++rep) if (!one_kmer(k, ph + 4 * (1 + rnd(9)), strand)) return 1;
        }

    // ---- 3: pieces through open() ----
    // four reads; read r holds k-mers at every 2-bit phase, its string ends with its last k-mer's last base (as tests/c/cons_str_core_check.cpp lays them out)
    std::vector<uint32_t> v_slot, v_rl, v_mseq, v_mpos;
    std::vector<uint64_t> v_first, v_choff, v_off;
    std::vector<uint8_t> v_hs;
    const uint64_t sid0 = 1000;
    const uint32_t n_reads = 4, per_read = 3;
    uint64_t byte_at = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        v_choff.push_back(v_mpos.size());
        uint32_t last = 0;
        for (uint32_t j = 0; j < per_read; ++j) {
            const uint32_t p = 4 * (3 * j + rnd(3)) + ((r + j) & 3);
            v_mpos.push_back(p << 1 | ((r ^ j) & 1));
            last = p;
        }
        v_off.push_back(byte_at * 4);
        const uint64_t nb = (last + (uint32_t) k + 3) / 4;
        for (uint64_t b = 0; b < nb; ++b) v_hs.push_back((uint8_t) rnd(256));
        if (r + 1 < n_reads) while (v_hs.size() % 16) v_hs.push_back(0xA5);
        byte_at = v_hs.size();
    }
    // syncmers 0 .. 11: the chain entries in turn; 12: no first occurrence; 13: m_seq 0; 14: not prepared; 15: as 3
    const uint32_t n_scm = 16;
    uint32_t n_sel = 0;
    for (uint32_t id = 0; id < n_scm; ++id) {
        if (id == 14) { v_slot.push_back(0xFFFFFFFFu); continue; }
        v_slot.push_back(n_sel++);
        const uint32_t e = id % (n_reads * per_read), rd = e / per_read, idx = e % per_read;
        v_first.push_back(id == 12? UINT64_MAX : (sid0 + rd) << 32 | (uint64_t) idx << 1 | (id & 1));
        v_mseq.push_back(id == 13? 0 : 1 + rnd(40));
        for (int t = 0; t < k; ++t) v_rl.push_back(rnd(8) < 5? 0 : (rnd(30) == 0? 300 : rnd(4)));
    }
    Tables T;
    T.n_scm = n_scm, T.k = k, T.sid0 = sid0;
    uint32_t *slot = exact(v_slot), *rl = exact(v_rl), *m_seq = exact(v_mseq), *m_pos = exact(v_mpos);
    uint64_t *first = exact(v_first), *chain_off = exact(v_choff), *off = exact(v_off);
    uint8_t *hoco_s = exact(v_hs);
    T.slot = slot, T.rl = rl, T.m_seq = m_seq, T.m_pos = m_pos, T.first = first, T.chain_off = chain_off, T.off = off, T.hoco_s = hoco_s;
    // the table as cstr_kmer_kernel writes it on a rank that holds every read: a row per slot, zeros where there is no first occurrence
    const uint64_t stride = 8 * (((uint64_t) k + 31) / 32);
    uint32_t *table = (uint32_t *) malloc(n_sel * stride);
    for (uint32_t sl = 0; sl < n_sel; ++sl)
        for (uint32_t j = 0; j < stride / 4; ++j) {
            uint32_t w = 0;
            if (first[sl] != UINT64_MAX) {
                const uint8_t *hs;
                const uint32_t mp = first_entry(T, first[sl], hs);
                w = kmer_word(hs, mp >> 1, mp & 1u, k, j);
            }
            table[sl * (stride / 4) + j] = w;
        }
    Tables TK = T;
    TK.kmer = (const uint8_t *) table, TK.kmer_stride = stride;
    TK.hoco_s = nullptr, TK.off = nullptr, TK.chain_off = nullptr, TK.m_pos = nullptr;      // the reads are another rank's: touching them is a fault
    const int begs[4] = {0, 9 < k? 9 : 1, k - 1, -4};
    uint64_t pieces = 0, chars = 0, nofirst = 0;
    for (uint64_t id = 0; id <= n_scm; ++id)
        for (uint64_t rev = 0; rev < 2; ++rev)
            for (int bi = 0; bi < 4; ++bi)
                for (int hoco = 0; hoco < 2; ++hoco) {
                    const uint64_t v = id << 1 | rev;
                    const Piece P = open(T, v, begs[bi], hoco), Q = open(TK, v, begs[bi], hoco);
                    if (P.slot != Q.slot || P.has_first != Q.has_first || P.expand != Q.expand || P.pad != Q.pad || P.beg0 != Q.beg0) { printf("FAIL open id=%lu\n", (unsigned long) id); return 1; }
                    const uint64_t L = length(T, P);
                    if (length(TK, Q) != L) { printf("FAIL length id=%lu rev=%lu beg=%d hoco=%d\n", (unsigned long) id, (unsigned long) rev, begs[bi], hoco); return 1; }
                    if (P.slot == (uint32_t) NO_SLOT) continue;
                    for (uint64_t o = 0; o < L; ++o)
                        if (char_at(T, P, o) != char_at(TK, Q, o)) { printf("FAIL text id=%lu rev=%lu beg=%d hoco=%d offset %lu\n", (unsigned long) id, (unsigned long) rev, begs[bi], hoco, (unsigned long) o); return 1; }
                    ++pieces, chars += L, nofirst += !P.has_first;
                }
    printf("OK words=%lu codes=%lu tail=%lu phases=%lu pieces=%lu chars=%lu nofirst=%lu\n", (unsigned long) n_words, (unsigned long) n_codes, (unsigned long) n_tail,
           (unsigned long) phases, (unsigned long) pieces, (unsigned long) chars, (unsigned long) nofirst);
    free(table); free(slot); free(rl); free(m_seq); free(m_pos); free(first); free(chain_off); free(off); free(hoco_s);
    return 0;
}
