// tests/c/inflate_core_fuzz.cpp -- oatk_amd/csrc/inflate_core.hpp (the decoder the device kernel runs) on the CPU, under ASan + UBSan, against zlib.
//
//   inflate_core_fuzz <rounds> <seed>    raw deflate members made here with zlib -- every level and strategy, every memLevel, stored members, flushes inside a
//                                        member, texts of runs, short periods and random ACGT -- must come out as zlib's text with status 0; damaged copies of
//                                        them (bits flipped, bytes dropped, tails cut, stretches overwritten, a wrong length) must come out as an error or as
//                                        the bytes zlib makes of them -- a member is never accepted with other bytes.  Input and output live in heap blocks of
//                                        exactly their sizes, so a read or write one byte outside them is a sanitizer report; every run is bounded.
//   inflate_core_fuzz members <file>     one member per line, "<hex of the deflate stream> <out_len>": prints "<status> <n_cross> <crc32 of the text, hex>", so that
//                                        a test can ask the core about streams it made itself (tests/test_host_inflate_core_fuzz.py)
// Tokens are executed by a scalar loop; the CRC is taken the way the kernel takes it: 64 pieces of 1024 bytes, combined with the shift operators.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <zlib.h>

#include "inflate_core.hpp"

using namespace oatk_inf;

static uint64_t rng_s;
static uint32_t rnd(void) { rng_s = rng_s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t) (rng_s >> 33); }

struct Result { uint32_t status, n_cross, crc; std::vector<uint8_t> text; };

static uint32_t crc_in_pieces(const uint8_t *p, uint32_t n)
{
    static uint32_t tab[256], x2n[32];
    static int ready = 0;
    if (!ready) { for (uint32_t i = 0; i < 256; ++i) tab[i] = crc_table_entry(i); crc_x2n_table(x2n); ready = 1; }
    uint32_t total = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t beg = lane * 1024, end = beg + 1024 < n? beg + 1024 : n;
        uint32_t c = lane == 0? 0xFFFFFFFFu : 0u;
        if (beg < end) c = crc_bytes(tab, c, p + beg, end - beg);
        if (beg < end || lane == 0) total ^= crc_mul(c, crc_shift_op(x2n, n - end));
    }
    return total ^ 0xFFFFFFFFu;
}

// the member executed into a heap block of exactly out_len bytes, read from the END of a heap block of in_len + shift bytes: a read past the member or a write past the
// text is a sanitizer report, and the shift gives the reader every alignment (whole aligned words where there are any, single bytes elsewhere)
static Result run_member_at(const uint8_t *in_bytes, uint32_t in_len, uint32_t out_len, uint32_t shift)
{
    Result R;
    uint8_t *blk = (uint8_t *) malloc(in_len + shift), *inp = blk + shift, *out = (uint8_t *) malloc(out_len? out_len : 1);
    if (in_len) memcpy(inp, in_bytes, in_len);
    Tables T;
    Inflater s;
    inf_init(s, &T, inp, in_len, (uint32_t) ((uintptr_t) inp & 3), out_len);
    uint64_t calls_left = 8ull * in_len + 16;
    for (;;) {
        if (calls_left-- == 0) { fprintf(stderr, "FAIL: the decoder did not end within its bound\n"); exit(2); }
        const uint32_t o = s.produced;
        uint32_t a, b;
        const uint32_t k = inf_next(s, a, b);
        if (k == TOK_NONE) continue;
        if (k >= TOK_END) break;
        if (k == TOK_LIT) out[o] = (uint8_t) a;
        else if (k == TOK_MATCH) for (uint32_t j = 0; j < a; ++j) out[o + j] = out[o - b + (j % b)];
        else for (uint32_t j = 0; j < a; ++j) out[o + j] = inp[b + j];
    }
    R.status = s.err, R.n_cross = s.n_cross, R.crc = 0;
    if (s.err == ST_OK) { R.text.assign(out, out + out_len); R.crc = crc_in_pieces(out, out_len); }
    free(blk), free(out);
    return R;
}

// what zlib makes of a raw stream: 1 with the text when it is a complete stream with nothing behind it
static int zlib_inflate(const std::vector<uint8_t> &in, std::vector<uint8_t> &text)
{
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) { fprintf(stderr, "inflateInit2\n"); exit(2); }
    text.assign(70000, 0);
    uint8_t none = 0;
    z.next_in = in.empty()? &none : (Bytef *) in.data(), z.avail_in = (uInt) in.size();
    z.next_out = text.data(), z.avail_out = (uInt) text.size();
    const int r = inflate(&z, Z_FINISH);
    const int ok = r == Z_STREAM_END && z.avail_in == 0;
    text.resize(z.total_out);
    inflateEnd(&z);
    return ok;
}

static std::vector<uint8_t> make_text(uint32_t kind, uint32_t n)
{
    std::vector<uint8_t> t(n);
    static const char nt[] = "ACGT";
    switch (kind) {
        case 0: for (uint32_t i = 0; i < n; ++i) t[i] = nt[rnd() & 3]; break;                                   // random ACGT
        case 1: for (uint32_t i = 0; i < n; ++i) t[i] = 'A'; break;                                             // one run
        case 2: { const uint32_t p = 1 + rnd() % 7; for (uint32_t i = 0; i < n; ++i) t[i] = nt[(i % p) & 3]; } break;      // a short period
        case 3: { uint32_t i = 0; while (i < n) { const uint32_t r = 1 + rnd() % 400; const uint8_t c = nt[rnd() & 3]; for (uint32_t k = 0; k < r && i < n; ++k) t[i++] = c; } } break;      // runs
        case 4: for (uint32_t i = 0; i < n; ++i) t[i] = (uint8_t) rnd(); break;                                // every byte value (codes longer than the fast table)
        case 5: {                                                                                               // FASTA-like: headers, lines, repeats at long distances
            std::vector<uint8_t> g(20000);
            for (auto &c : g) c = nt[rnd() & 3];
            uint32_t i = 0;
            while (i < n) {
                char h[64];
                const int hl = snprintf(h, sizeof(h), ">read_%u some comment\n", rnd() % 100000);
                for (int k = 0; k < hl && i < n; ++k) t[i++] = (uint8_t) h[k];
                uint32_t p = rnd() % 15000, L = 500 + rnd() % 4000;
                for (uint32_t k = 0; k < L && i < n; ++k) { t[i++] = g[(p + k) % g.size()]; if (k % 80 == 79 && i < n) t[i++] = '\n'; }
                if (i < n) t[i++] = '\n';
            }
        } break;
        default: { const uint32_t half = n / 2; for (uint32_t i = 0; i < half; ++i) t[i] = nt[rnd() & 3]; for (uint32_t i = half; i < n; ++i) t[i] = t[i - half]; } break;      // the second half repeats the first
    }
    return t;
}

static std::vector<uint8_t> deflate_raw(const std::vector<uint8_t> &text, int level, int strategy, int mem_level, int flushes)
{
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (deflateInit2(&z, level, Z_DEFLATED, -15, mem_level, strategy) != Z_OK) { fprintf(stderr, "deflateInit2\n"); exit(2); }
    std::vector<uint8_t> out(deflateBound(&z, (uLong) text.size()) + 64 * (flushes + 1) + 64);
    z.next_out = out.data(), z.avail_out = (uInt) out.size();
    size_t at = 0;
    uint8_t none = 0;
    for (int f = 0; f < flushes; ++f) {
        const size_t take = text.size() > at? rnd() % (text.size() - at + 1) : 0;
        static const int kinds[] = {Z_SYNC_FLUSH, Z_FULL_FLUSH, Z_PARTIAL_FLUSH, Z_BLOCK};
        z.next_in = text.empty()? &none : (Bytef *) text.data() + at, z.avail_in = (uInt) take;
        { const int r = deflate(&z, kinds[rnd() & 3]); if (r != Z_OK && r != Z_BUF_ERROR) { fprintf(stderr, "deflate flush\n"); exit(2); } }      // (Z_BUF_ERROR: nothing to flush)
        at += take;
    }
    z.next_in = text.empty()? &none : (Bytef *) text.data() + at, z.avail_in = (uInt) (text.size() - at);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "deflate finish\n"); exit(2); }
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

static uint64_t n_good, n_damaged, n_dam_ok, n_dam_err, n_cross_seen;

static void check_good(const std::vector<uint8_t> &comp, const std::vector<uint8_t> &text, const char *what)
{
    if (comp.size() > MAX_MEMBER) return;                  // (not a BGZF member's size)
    for (uint32_t shift = 0; shift < 4; ++shift) {
        const Result R = run_member_at(comp.data(), (uint32_t) comp.size(), (uint32_t) text.size(), shift);
        if (R.status != ST_OK || R.text != text) { fprintf(stderr, "FAIL: %s: a member of zlib's (%zu -> %zu bytes) came out with status %u%s\n", what, comp.size(), text.size(), R.status, R.status? "" : " and other bytes"); exit(1); }
        if (R.crc != (uint32_t) crc32(crc32(0L, Z_NULL, 0), text.data(), (uInt) text.size())) { fprintf(stderr, "FAIL: %s: the CRC in pieces differs from zlib's\n", what); exit(1); }
        n_cross_seen += R.n_cross;
    }
    ++n_good;
    // a wrong length is a length error, never another text
    if (!text.empty()) { const Result R = run_member_at(comp.data(), (uint32_t) comp.size(), (uint32_t) text.size() - 1, 0); if (R.status != ST_LEN) { fprintf(stderr, "FAIL: %s: out_len one short gave status %u\n", what, R.status); exit(1); } }
    if (text.size() < MAX_MEMBER) { const Result R = run_member_at(comp.data(), (uint32_t) comp.size(), (uint32_t) text.size() + 1, 0); if (R.status != ST_LEN) { fprintf(stderr, "FAIL: %s: out_len one long gave status %u\n", what, R.status); exit(1); } }
}

static void check_damaged(const std::vector<uint8_t> &comp, uint32_t out_len, const char *what)
{
    if (comp.size() > MAX_MEMBER) return;
    const Result R = run_member_at(comp.data(), (uint32_t) comp.size(), out_len, rnd() & 3);
    ++n_damaged;
    if (R.status != ST_OK) { ++n_dam_err; return; }
    std::vector<uint8_t> zt;
    const int zok = zlib_inflate(comp, zt);
    if (!zok || zt != R.text) { fprintf(stderr, "FAIL: %s: a damaged member (%zu bytes) was ACCEPTED with %s\n", what, comp.size(), zok? "other bytes than zlib's" : "a text zlib refuses"); exit(1); }
    ++n_dam_ok;
}

static void damage_all(const std::vector<uint8_t> &comp, uint32_t out_len)
{
    if (comp.empty()) return;
    for (int rep = 0; rep < 12; ++rep) {
        std::vector<uint8_t> d = comp;
        switch (rep % 6) {
            case 0: d[rnd() % d.size()] ^= (uint8_t) (1u << (rnd() & 7)); break;                               // one bit
            case 1: { const int k = 1 + rnd() % 8; for (int i = 0; i < k; ++i) d[rnd() % d.size()] ^= (uint8_t) (1u << (rnd() & 7)); } break;
            case 2: d.erase(d.begin() + rnd() % d.size()); break;                                               // a byte dropped
            case 3: d.resize(rnd() % d.size()); break;                                                          // the tail cut
            case 4: { const size_t a = rnd() % d.size(), n = 1 + rnd() % 16; for (size_t i = a; i < a + n && i < d.size(); ++i) d[i] = (uint8_t) rnd(); } break;
            default: d[rnd() % (d.size() < 12? d.size() : 12)] ^= (uint8_t) (1u << (rnd() & 7)); break;        // the block header and the code lengths
        }
        check_damaged(d, out_len, "damage");
    }
    { std::vector<uint8_t> d = comp; d.resize(d.size() - 1); check_damaged(d, out_len, "cut by one"); }
    { std::vector<uint8_t> d = comp; d.resize(d.size() / 2); check_damaged(d, out_len, "cut by half"); }
    { std::vector<uint8_t> d = comp; d.push_back((uint8_t) rnd());                                              // a byte behind the final block: an error whatever it is
      const Result R = run_member_at(d.data(), (uint32_t) d.size(), out_len, 0);
      if (d.size() <= MAX_MEMBER && R.status == ST_OK) { fprintf(stderr, "FAIL: a byte behind the final block was accepted\n"); exit(1); } }
}

static int hexval(int c) { return c >= '0' && c <= '9'? c - '0' : (c >= 'a' && c <= 'f'? c - 'a' + 10 : (c >= 'A' && c <= 'F'? c - 'A' + 10 : -1)); }

static int members_mode(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) { perror(path); return 2; }
    std::string hex;
    int c;
    for (;;) {
        hex.clear();
        while ((c = fgetc(f)) != EOF && c != ' ' && c != '\n') hex.push_back((char) c);
        if (c == EOF && hex.empty()) break;
        unsigned long out_len = 0;
        if (c == ' ' && fscanf(f, "%lu", &out_len) != 1) { fprintf(stderr, "bad line\n"); return 2; }
        while (c != '\n' && c != EOF) c = fgetc(f);
        std::vector<uint8_t> m;
        if (hex != "-") for (size_t i = 0; i + 1 < hex.size(); i += 2) m.push_back((uint8_t) (hexval(hex[i]) << 4 | hexval(hex[i + 1])));
        if (m.size() > MAX_MEMBER || out_len > MAX_MEMBER) { printf("1 0 0\n"); continue; }
        const Result R = run_member_at(m.data(), (uint32_t) m.size(), (uint32_t) out_len, 0);
        printf("%u %u %08x\n", R.status, R.n_cross, R.crc);
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "members")) return members_mode(argv[2]);
    const int rounds = argc > 1? atoi(argv[1]) : 10;
    rng_s = argc > 2? (uint64_t) atoll(argv[2]) * 0x9E3779B97F4A7C15ULL + 1 : 1;
    static const int strategies[] = {Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED};
    static const uint32_t sizes[] = {0, 1, 2, 3, 257, 258, 259, 700, 4095, 32768, 32769, 65280, 65535, 65536};
    for (int r = 0; r < rounds; ++r) {
        for (uint32_t kind = 0; kind < 7; ++kind) {
            const uint32_t n = r < (int) (sizeof(sizes) / sizeof(sizes[0]))? sizes[r] : rnd() % 65537;
            const std::vector<uint8_t> text = make_text(kind, n);
            for (int si = 0; si < 5; ++si) {
                const int level = (r + si + (int) kind) % 10, mem_level = 1 + rnd() % 9, flushes = (rnd() & 3) == 0? 1 + rnd() % 3 : 0;
                const std::vector<uint8_t> comp = deflate_raw(text, level, strategies[si], mem_level, flushes);
                check_good(comp, text, "made");
                damage_all(comp, (uint32_t) text.size());
            }
        }
        // every level once per round on one text, default strategy
        { const std::vector<uint8_t> text = make_text(5, 20000 + rnd() % 45000);
          for (int level = 0; level <= 9; ++level) { const std::vector<uint8_t> comp = deflate_raw(text, level, Z_DEFAULT_STRATEGY, 8, 0); check_good(comp, text, "levels"); if (level % 3 == 0) damage_all(comp, (uint32_t) text.size()); } }
    }
    printf("%llu members equal to zlib's text; %llu damaged members: %llu refused, %llu accepted with zlib's bytes; no member accepted with other bytes\n",
           (unsigned long long) n_good, (unsigned long long) n_damaged, (unsigned long long) n_dam_err, (unsigned long long) n_dam_ok);
    return 0;
}
