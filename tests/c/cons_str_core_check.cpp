// tests/c/cons_str_core_check.cpp -- oatk_amd/csrc/cons_str_core.hpp on the CPU, under ASan + UBSan (tests/test_host_cons_str_core.py builds and runs it): for small
// hand-made tables, every piece (syncmer x rev x beg x space) as the core reads it -- prepared or not, its length, the character at every offset, and the text put
// together tile by tile from the starts and find_source as the fill kernel does (csrc/cons_str.hpp) -- against a restatement that appends one character at a time
// the way scg_syncmer_consensus does (syncasm.c:888-1001).  Every array sits in a heap block of exactly its size, so a read outside it is a sanitizer report.
//
// usage: cons_str_core_check <k> <seed>
// output: one line  OK pieces=<n> chars=<n> n_first=<pieces without a first occurrence> m0=<pieces with m_seq 0> unprepared=<n> phases=<bit mask of p & 3 seen, forward
//         strand bits 0-3, reverse 4-7> rl0=<n> rl254=<n> rl700=<n> (positions with that run length inside a compared piece)
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

struct Made {
    Tables T;
    std::vector<uint32_t> slot, rl, m_seq, m_pos;
    std::vector<uint64_t> first, chain_off, off;
    std::vector<uint8_t> hoco_s;
};

// the piece one character at a time; false: not prepared
static bool naive(const Made &M, uint64_t v, int64_t beg, int hoco, std::string &out)
{
    const int k = M.T.k;
    const uint64_t id = v >> 1, rev = v & 1;
    out.clear();
    if (id >= M.slot.size() || M.slot[id] == 0xFFFFFFFFu) return false;
    const uint32_t sl = M.slot[id];
    while (beg < 0) out.push_back('N'), ++beg;
    const int64_t l = k - beg;
    if (M.first[sl] == UINT64_MAX) { out.append((size_t) l, 'N'); return true; }
    const uint64_t o = M.first[sl], rd = (o >> 32) - M.T.sid0;
    uint64_t p = M.m_pos[M.chain_off[rd] + ((o >> 1) & 0x7FFFFFFFULL)];
    const uint64_t r = (p & 1) ^ rev;
    p >>= 1;
    const uint8_t *hs = M.hoco_s.data() + (M.off[rd] >> 2);
    for (int64_t i = 0; i < l; ++i) {
        const uint64_t q = r? p + (uint64_t) (l - 1 - i) : p + (uint64_t) (beg + i);
        uint32_t c = (hs[q >> 2] >> (((q & 3) ^ 3) << 1)) & 3;
        if (r) c ^= 3;
        out.push_back("ACGT"[c]);
        if (!hoco && M.m_seq[sl]) {
            const uint32_t b = M.rl[(size_t) sl * k + (rev? k - 1 - (beg + i) : beg + i)];
            out.append(b, "ACGT"[c]);
        }
    }
    return true;
}

// the text as the fill kernel assembles it: per tile of 64 positions the exclusive prefix sums of the counts, then every output byte finds its position
static std::string by_tiles(const Tables &T, const Piece &P, uint64_t L)
{
    std::string s((size_t) L, '?');
    if (!P.has_first) { for (auto &c : s) c = 'N'; return s; }
    for (uint64_t o = 0; o < P.pad && o < L; ++o) s[o] = 'N';
    uint64_t done = P.pad;
    for (uint32_t t0 = P.beg0; t0 < (uint32_t) T.k; t0 += TILE) {
        uint64_t *starts = (uint64_t *) malloc(TILE * sizeof(uint64_t));
        char ch[TILE];
        uint64_t run = 0;
        for (uint32_t l = 0; l < TILE; ++l) {
            const uint32_t t = t0 + l;
            starts[l] = run, ch[l] = 0;
            if (t < (uint32_t) T.k) run += count_at(T, P, t), ch[l] = letter(code_at(T, P, t));
        }
        for (uint64_t o = 0; o < run; ++o) {
            const uint32_t j = P.expand? find_source(starts, o) : (uint32_t) o;
            if (done + o < L) s[done + o] = ch[j];
        }
        free(starts);
        done += run;
    }
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <k> <seed>\n", argv[0]); return 2; }
    const int k = atoi(argv[1]);
    rng_state = 0x9E3779B97F4A7C15ULL ^ (uint64_t) atoll(argv[2]) * 1000003ULL;
    if (k < 5) return 2;
    Made M;
    // four reads; read r holds k-mers at hoco positions 4 j + r .. (every 2-bit phase), its string ends with its last k-mer's last base
    const uint64_t sid0 = 1000;
    const uint32_t n_reads = 4, per_read = 3;
    uint64_t byte_at = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        M.chain_off.push_back(M.m_pos.size());
        uint32_t last = 0;
        for (uint32_t j = 0; j < per_read; ++j) {
            const uint32_t p = 4 * (3 * j + rnd(3)) + ((r + j) & 3);      // phases r, r + 1, r + 2 (mod 4)
            M.m_pos.push_back(p << 1 | ((r ^ j) & 1));
            last = p;
        }
        const uint32_t hoco_l = last + (uint32_t) k;
        M.off.push_back(byte_at * 4);                                      // (read offsets are multiples of 64 in the packed stream, so of 16 here)
        const uint64_t nb = (hoco_l + 3) / 4;
        for (uint64_t b = 0; b < nb; ++b) M.hoco_s.push_back((uint8_t) rnd(256));
        if (r + 1 < n_reads) while (M.hoco_s.size() % 16) M.hoco_s.push_back(0xA5);
        byte_at = M.hoco_s.size();
    }
    // syncmers: 0 .. 11 take the chain entries in turn as first occurrence; 12: no first occurrence; 13: m_seq 0; 14: not prepared (in the middle of the ids); 15: as 0
    const uint32_t n_scm = 16;
    uint32_t n_sel = 0;
    for (uint32_t id = 0; id < n_scm; ++id) {
        if (id == 14) { M.slot.push_back(0xFFFFFFFFu); continue; }
        M.slot.push_back(n_sel++);
        const uint32_t e = id % (n_reads * per_read), rd = e / per_read, idx = e % per_read;
        M.first.push_back(id == 12? UINT64_MAX : (sid0 + rd) << 32 | (uint64_t) idx << 1 | (id & 1));
        M.m_seq.push_back(id == 13? 0 : 1 + rnd(40));
        for (int t = 0; t < k; ++t) {
            uint32_t b = rnd(8) < 5? 0 : rnd(4);
            if (rnd(40) == 0) b = 254;
            if (rnd(90) == 0) b = 700;
            M.rl.push_back(b);
        }
        uint32_t *row = M.rl.data() + (size_t) (n_sel - 1) * k;
        row[0] = 700, row[k - 1] = 254, row[k / 2] = 0, row[1] = 0;         // the ends and the middle hold the three named run lengths whatever the seed
    }
    Tables &T = M.T;
    T.n_scm = n_scm, T.k = k, T.sid0 = sid0;
    uint32_t *slot = exact(M.slot), *rl = exact(M.rl), *m_seq = exact(M.m_seq), *m_pos = exact(M.m_pos);
    uint64_t *first = exact(M.first), *chain_off = exact(M.chain_off), *off = exact(M.off);
    uint8_t *hoco_s = exact(M.hoco_s);
    T.slot = slot, T.rl = rl, T.m_seq = m_seq, T.m_pos = m_pos, T.first = first, T.chain_off = chain_off, T.off = off, T.hoco_s = hoco_s;

    const int begs[4] = {0, 1, k - 1, -4};
    uint64_t pieces = 0, chars = 0, n_first = 0, m0 = 0, unprepared = 0, phases = 0, c0 = 0, c254 = 0, c700 = 0;
    std::string want;
    for (uint64_t id = 0; id <= n_scm; ++id)                               // (id n_scm: past the table)
        for (uint64_t rev = 0; rev < 2; ++rev)
            for (int bi = 0; bi < 4; ++bi)
                for (int hoco = 0; hoco < 2; ++hoco) {
                    const uint64_t v = id << 1 | rev;
                    const int beg = begs[bi];
                    const bool ok = naive(M, v, beg, hoco, want);
                    if (prepared(T, v) != ok) { printf("FAIL prepared id=%lu\n", (unsigned long) id); return 1; }
                    const Piece P = open(T, v, beg, hoco);
                    if ((P.slot != (uint32_t) NO_SLOT) != ok) { printf("FAIL open id=%lu\n", (unsigned long) id); return 1; }
                    const uint64_t L = length(T, P);
                    if (!ok) { ++unprepared; if (L != 0) { printf("FAIL length of an unprepared piece\n"); return 1; } continue; }
                    if (L != want.size()) { printf("FAIL length id=%lu rev=%lu beg=%d hoco=%d: %lu, naive %lu\n", (unsigned long) id, (unsigned long) rev, beg, hoco, (unsigned long) L, (unsigned long) want.size()); return 1; }
                    for (uint64_t o = 0; o < L; ++o)
                        if (char_at(T, P, o) != want[o]) { printf("FAIL char_at id=%lu rev=%lu beg=%d hoco=%d offset %lu\n", (unsigned long) id, (unsigned long) rev, beg, hoco, (unsigned long) o); return 1; }
                    if (by_tiles(T, P, L) != want) { printf("FAIL tiles id=%lu rev=%lu beg=%d hoco=%d\n", (unsigned long) id, (unsigned long) rev, beg, hoco); return 1; }
                    ++pieces, chars += L;
                    if (!P.has_first) ++n_first;
                    else {
                        phases |= 1ULL << ((P.p & 3) + 4 * P.flip);
                        if (M.m_seq[P.slot] == 0) { ++m0; if (P.expand || L != P.pad + (uint64_t) (k - (int) P.beg0)) { printf("FAIL m_seq 0 expands\n"); return 1; } }
                        if (P.expand)
                            for (uint32_t t = P.beg0; t < (uint32_t) k; ++t) { const uint64_t c = count_at(T, P, t); c0 += c == 1, c254 += c == 255, c700 += c == 701; }
                    }
                }
    printf("OK pieces=%lu chars=%lu n_first=%lu m0=%lu unprepared=%lu phases=%lu rl0=%lu rl254=%lu rl700=%lu\n", (unsigned long) pieces, (unsigned long) chars,
           (unsigned long) n_first, (unsigned long) m0, (unsigned long) unprepared, (unsigned long) phases, (unsigned long) c0, (unsigned long) c254, (unsigned long) c700);
    free(slot); free(rl); free(m_seq); free(m_pos); free(first); free(chain_off); free(off); free(hoco_s);
    return 0;
}
