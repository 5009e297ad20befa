// tests/c/bam_core_check.cpp -- oatk_amd/csrc/bam_core.hpp on the CPU, under ASan + UBSan (tests/test_host_bam_core.py builds and runs it): the header walk, the
// predicates at every byte offset, the serial chain walk, the chain by successors + pointer doubling as the device builds it (csrc/bam.hpp), and the letters as the
// unpack kernel makes them (unpack8 for whole groups of 16, letter() for the rest) -- over case files the test writes.  Every stream sits in a heap block of exactly
// its size, so a read one byte outside it is a sanitizer report.
//
// usage: bam_core_check <cases>      cases: per case  u64 n, u8 header, u8 letters, n bytes
// output per case:  H <verdict> <len> <need>   C <m> <offsets>   R <n_rec> <t> <stop> <offsets>   D <1: doubling gave the serial chain>   [S <name hex> <letters>]*
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "bam_core.hpp"

using namespace oatk_bam;

static std::vector<uint64_t> by_doubling(const uint8_t *b, const std::vector<uint64_t> &c, uint64_t s0)
{
    const uint64_t m = c.size();
    std::vector<uint64_t> jump(m + 1, m), mark(m + 1, 0), out;
    if (!m) return out;
    for (uint64_t i = 0; i < m; ++i) {
        const uint64_t t = next(b, c[i]);
        uint64_t lo = i + 1, hi = m;
        while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (c[mid] < t) lo = mid + 1; else hi = mid; }
        jump[i] = lo < m && c[lo] == t? lo : m;
    }
    mark[0] = c[0] == s0;
    for (uint64_t reach = 1; reach < m + 1; reach <<= 1) {
        std::vector<uint64_t> j2(m + 1);
        for (uint64_t i = 0; i <= m; ++i) {
            if (i < m && jump[i] < m && mark[i]) mark[jump[i]] = 1;
            j2[i] = jump[jump[i]];
        }
        jump.swap(j2);
    }
    for (uint64_t i = 0; i < m; ++i) if (mark[i]) out.push_back(c[i]);
    return out;
}

static std::string letters_of(const uint8_t *b, uint64_t o)
{
    const Rec x = record(b, o);
    const uint8_t *src = b + x.seq_at;
    std::string s(x.l_seq, '?');
    const uint32_t n_full = x.l_seq >> 4;
    for (uint32_t idx = 0; idx < n_full; ++idx) {
        uint32_t w[2], a[2], c[2], out[4];
        memcpy(w, src + 8 * (uint64_t) idx, 8);
        unpack8(w[0], a), unpack8(w[1], c);
        out[0] = a[0], out[1] = a[1], out[2] = c[0], out[3] = c[1];
        memcpy(&s[16 * (size_t) idx], out, 16);
    }
    for (uint32_t j = n_full << 4; j < x.l_seq; ++j) { const uint32_t by = src[j >> 1]; s[j] = (char) letter((j & 1u)? by & 15u : by >> 4); }
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: bam_core_check <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    for (;;) {
        uint64_t n;
        uint8_t hdr, want_letters;
        if (fread(&n, 8, 1, f) != 1) break;
        if (fread(&hdr, 1, 1, f) != 1 || fread(&want_letters, 1, 1, f) != 1) return 3;
        uint8_t *b = (uint8_t *) malloc(n? n : 1);          // exactly n bytes (one where n = 0: never read)
        if (n && fread(b, 1, n, f) != n) return 3;
        uint64_t s0 = 0, need = 0;
        int hv = HDR_OK;
        if (hdr) hv = header_walk(b, n, &s0, &need);
        printf("H %d %llu %llu\n", hv, (unsigned long long) s0, (unsigned long long) need);
        if (hv == HDR_OK) {
            std::vector<uint64_t> c, rec;
            for (uint64_t o = s0; o < n; ++o) if (ok(b, n, o)) c.push_back(o);
            printf("C %zu", c.size());
            for (uint64_t o : c) printf(" %llu", (unsigned long long) o);
            uint64_t t = s0;
            int why;
            while ((why = classify(b, n, t)) == STOP_NONE) rec.push_back(t), t = next(b, t);
            printf("\nR %zu %llu %d", rec.size(), (unsigned long long) t, why);
            for (uint64_t o : rec) printf(" %llu", (unsigned long long) o);
            printf("\nD %d\n", by_doubling(b, c, s0) == rec);
            if (want_letters)
                for (uint64_t o : rec) {
                    printf("S ");
                    for (const uint8_t *p = b + o + FIXED; *p; ++p) printf("%02x", *p);
                    printf("- %s\n", letters_of(b, o).c_str());
                }
        }
        free(b);
    }
    fclose(f);
    return 0;
}
