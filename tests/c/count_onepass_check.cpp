// tests/c/count_onepass_check.cpp -- stand-alone check of oatk_amd/csrc/count_onepass_core.hpp (built with -fsanitize=address,undefined by
// tests/test_host_count_onepass_core.py): the tile / strip walk of gather_verify_kernel (count.hpp) restated on the host over heap arrays of
// exactly n records, against the plain statement "a hash group is bad when it holds two different k-mers, and is reported at its head".
//   * every record that is no head is compared with its predecessor, once, and nothing else is compared;
//   * a strip loads at most STRIP + 1 k-mers, all of them records of the batch (the one in front of a tile only when the tile asks for it),
//     and a strip of heads loads nothing; words of k-mers that were not loaded are poisoned and must not matter;
//   * the reported heads equal the brute-force ones, also with the difference at a tile's first record, inside a group and at the last record.
// usage: count_onepass_check SEED -> "OK batches=.. records=.. compared=.. loads=.. bad=.. pred=.."
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "count_onepass_core.hpp"

using namespace oatk;

static const int STRIP = 8, TILE = 256;
static uint64_t rng_s;
static uint64_t rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return rng_s; }

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

struct Tot { uint64_t batches = 0, records = 0, compared = 0, loads = 0, bad = 0, pred = 0; };

// newclus[i]: 1 at a group head; kmer[i]: the record's k-mer (one word stands for all of them)
static void one_batch(const std::vector<uint32_t> &newclus_v, const std::vector<uint64_t> &kmer_v, Tot &tot)
{
    const uint32_t n = (uint32_t) newclus_v.size();
    // heap copies of exactly n elements: an index one past either end is the sanitizer's to report
    uint32_t *newclus = new uint32_t[n];
    uint64_t *kmer = new uint64_t[n];
    for (uint32_t i = 0; i < n; ++i) newclus[i] = newclus_v[i], kmer[i] = kmer_v[i];
    std::vector<uint32_t> bad(n, 0), want(n, 0), times(n, 0);
    for (uint32_t t0 = 0; t0 < n; t0 += TILE) {
        const bool pred = onepass_tile_needs_pred(newclus, n, t0);
        REQUIRE(pred == (t0 > 0 && !newclus[t0]));
        tot.pred += pred;
        for (uint32_t s0 = 0; s0 < (uint32_t) TILE; s0 += STRIP) {
            uint32_t live = 0;
            for (int r = 0; r < STRIP; ++r) {
                const uint64_t i = (uint64_t) t0 + s0 + r;
                if (i < n && i > 0 && !newclus[i]) live |= 1u << r;
            }
            const uint32_t need = onepass_need_mask(live);
            if (live == 0) { REQUIRE(need == 0); continue; }
            REQUIRE((need >> (STRIP + 1)) == 0);
            uint64_t w[STRIP + 1];
            for (int j = 0; j <= STRIP; ++j) {
                if ((need >> j) & 1u) {
                    const int64_t i = (int64_t) t0 + s0 + j - 1;
                    REQUIRE(i >= 0 && i < (int64_t) n);
                    if (s0 == 0 && j == 0) REQUIRE(pred);            // the slot in front of the tile is only filled then
                    w[j] = kmer[i];
                    ++tot.loads;
                } else
                    w[j] = rnd();                                    // (never loaded on the device: anything)
            }
            const uint32_t diff = onepass_diff_mask<STRIP>(w, live);
            REQUIRE((diff & ~live) == 0);
            for (int r = 0; r < STRIP; ++r) {
                if (!((live >> r) & 1u)) continue;
                const uint32_t i = t0 + s0 + r;
                ++times[i], ++tot.compared;
                REQUIRE(((diff >> r) & 1u) == (uint32_t) (kmer[i] != kmer[i - 1]));
                if ((diff >> r) & 1u) {
                    const uint32_t h = onepass_head_of(newclus, i);
                    REQUIRE(h < i && newclus[h]);
                    for (uint32_t x = h + 1; x <= i; ++x) REQUIRE(!newclus[x]);
                    bad[h] = 1;
                }
            }
        }
    }
    // brute force: every group against its head
    for (uint32_t i = 0, h = 0; i < n; ++i) {
        if (newclus[i]) h = i;
        else if (kmer[i] != kmer[h]) want[h] = 1;
        REQUIRE(times[i] == (newclus[i] ? 0u : 1u));
    }
    for (uint32_t i = 0; i < n; ++i) {
        REQUIRE(bad[i] == want[i]);
        tot.bad += bad[i];
    }
    REQUIRE(onepass_head_of(newclus, 0) == 0);
    ++tot.batches, tot.records += n;
    delete[] newclus;
    delete[] kmer;
}

// groups of random lengths; with probability 1 / bad_one_in a group holds up to three k-mers (A A B B, A B A, a lone record at either end)
static void random_batch(uint32_t n, uint32_t mean_len, uint32_t bad_one_in, Tot &tot)
{
    std::vector<uint32_t> nc(n);
    std::vector<uint64_t> km(n);
    uint32_t i = 0;
    while (i < n) {
        const uint32_t len = 1 + (uint32_t) (rnd() % (2 * mean_len));
        const bool mixed = bad_one_in && rnd() % bad_one_in == 0;
        const uint64_t base = rnd() << 2;
        for (uint32_t r = 0; r < len && i < n; ++r, ++i) {
            nc[i] = r == 0;
            km[i] = base + (mixed ? (uint64_t) (rnd() % 3) * (rnd() % 4 == 0) : 0);
        }
    }
    one_batch(nc, km, tot);
}

int main(int argc, char **argv)
{
    rng_s = 0x9E3779B97F4A7C15ULL ^ (uint64_t) (argc > 1 ? std::atoll(argv[1]) : 1) * 0xD6E8FEB86659FD93ULL;
    Tot tot;
    // the sizes round every tile and strip edge, with singletons only, one group only and mixed groups
    static const uint32_t sizes[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 263, 264, 265, 511, 512, 513, 1023, 1025};
    for (uint32_t n : sizes) {
        one_batch(std::vector<uint32_t>(n, 1), std::vector<uint64_t>(n, 5), tot);                       // heads only: nothing compared
        std::vector<uint32_t> nc(n, 0);
        nc[0] = 1;
        one_batch(nc, std::vector<uint64_t>(n, 5), tot);                                                // one clean group over every edge
        for (uint32_t at : {1u, n / 2, 255u, 256u, 257u, n - 1}) {                                      // one group, the difference planted at `at`
            if (at == 0 || at >= n) continue;
            std::vector<uint64_t> km(n, 5);
            for (uint32_t i = at; i < n; ++i) km[i] = 6;                                                // A .. A B .. B
            one_batch(nc, km, tot);
            km.assign(n, 5);
            km[at] = 6;                                                                                 // A .. A B A .. A
            one_batch(nc, km, tot);
        }
        for (uint32_t mean : {1u, 3u, 20u, 300u}) {
            random_batch(n, mean, 0, tot);
            random_batch(n, mean, 3, tot);
        }
    }
    for (int it = 0; it < 300; ++it) random_batch(1 + (uint32_t) (rnd() % 3000), 1 + (uint32_t) (rnd() % 40), (uint32_t) (rnd() % 6), tot);
    std::printf("OK batches=%llu records=%llu compared=%llu loads=%llu bad=%llu pred=%llu\n", (unsigned long long) tot.batches, (unsigned long long) tot.records,
                (unsigned long long) tot.compared, (unsigned long long) tot.loads, (unsigned long long) tot.bad, (unsigned long long) tot.pred);
    return 0;
}
