// tests/c/minicircle_core_check.cpp -- oatk_amd/csrc/minicircle_core.hpp (the per-record rule and the canonical path element the device kernels run) and
// oatk_mc_path_stats of oatk_amd/csrc/host/minicircle_host.c, as a stand-alone program under ASan + UBSan (tests/test_host_minicircle_core.py).
//
// Every record goes through three forms of the rule -- unit_of (a lane's walk), the chunked form a wave runs (hits_add_chunk over 64-fragment masks, then
// period_ok per fragment) and a restatement below that follows the reference's loop a fragment at a time, its counter k and all -- and through two forms of the
// path: path_uid / path_elem per element, and push, reverse, flip.  Records live in heap blocks of their exact size, so a read past either end is ASan's.
//
//   minicircle_core_check SEED  ->  "OK records=.. valid=.. long=.. chunk_first=.. distinct=.."
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "minicircle_core.hpp"
#include "oatk_hip_racov.h"
#include "oatk_syncasm.h"

// what minicircle_host.c calls on a device: never reached from here
extern "C" {
int oatk_hip_ra_minicircle_units(oatk_hip_ctx *, const oatk_racov_aln_t *, uint64_t, uint64_t *, uint64_t *, uint64_t *) { abort(); }
int oatk_hip_buffer(oatk_hip_ctx *, int, const void **, uint64_t *) { abort(); }
int oatk_hip_d2h(oatk_hip_ctx *, void *, const void *, uint64_t) { abort(); }
const oatk_racov_aln_t *oatk_host_racov_aln(const oatk_scg_ra_v *, uint64_t, void **) { abort(); }
void oatk_host_racov_aln_free(void *) { abort(); }
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static const uint32_t NO = 0xFFFFFFFFu;

// minicircle_analysis_thread, a fragment at a time in its own order
static uint64_t restated_unit(const std::vector<uint64_t> &f, uint64_t sid)
{
    const uint32_t n = (uint32_t) f.size();
    if (n < 2) return UINT64_MAX;
    uint32_t beg = NO, end = NO, rev = NO;
    for (uint32_t j = 0; j < n; ++j) {
        if (f[j] >> 1 != sid) continue;
        if (beg == NO) beg = j;
        else if (end == NO) end = j - 1;
        if (rev == NO) rev = (uint32_t) (f[j] & 1);
        else if (rev != (f[j] & 1)) { rev = NO; break; }
    }
    if (beg == NO || end == NO || rev == NO) return UINT64_MAX;
    bool valid = true;
    if (beg > 0 || end < n - 2) {
        const uint32_t r = end - beg;
        if (beg > r) valid = false;
        else {
            uint32_t k = r - beg;
            if (++k > r) k = 0;
            for (uint32_t j = 0; j < n; ++j) {
                if (f[j] != f[beg + k]) { valid = false; break; }
                if (++k > r) k = 0;
            }
        }
    }
    return valid? (uint64_t) beg << 33 | (uint64_t) end << 1 | rev : UINT64_MAX;
}
static std::vector<uint32_t> restated_path(const std::vector<uint64_t> &f, uint64_t mc)
{
    std::vector<uint32_t> vt;
    for (uint64_t j = mc >> 33; j <= (uint32_t) (mc >> 1); ++j) vt.push_back((uint32_t) f[j]);
    if (mc & 1) {
        std::reverse(vt.begin() + 1, vt.end());
        for (uint32_t &x : vt) x ^= 1;
    }
    return vt;
}

// the wave's form: 64 fragments at a time through two masks, then the period fragment by fragment
static uint64_t chunked_unit(const uint64_t *p, uint32_t n, uint64_t anchor)
{
    oatk_mc::Hits h;
    oatk_mc::hits_init(h);
    for (uint32_t base = 0; base < n; base += oatk_mc::CHUNK) {
        uint64_t hm = 0, rm = 0;
        for (uint32_t l = 0; l < oatk_mc::CHUNK && base + l < n; ++l)
            if (oatk_mc::hit(p[base + l], anchor)) hm |= 1ULL << l, rm |= (p[base + l] & 1) << l;
        oatk_mc::hits_add_chunk(h, base, hm, rm);
    }
    bool period;
    uint64_t v = oatk_mc::verdict(h, n, &period);
    if (v != oatk_mc::NONE && period) {
        const uint32_t beg = oatk_mc::unit_beg(v), r = oatk_mc::unit_end(v) - beg;
        for (uint32_t j = 0; j < n; ++j) if (!oatk_mc::period_ok(p, j, beg, r)) return oatk_mc::NONE;
    }
    return v;
}

struct Tally { uint64_t records = 0, valid = 0, longer = 0, chunk_first = 0; std::vector<std::vector<uint32_t>> paths; };

static void one_record(const std::vector<uint64_t> &f, uint64_t anchor, Tally &T, uint64_t want = 1, const std::vector<uint32_t> *want_path = nullptr)
{
    const uint32_t n = (uint32_t) f.size();
    uint64_t *p = (uint64_t *) malloc(n? 8 * (size_t) n : 1);              // exactly the record
    if (n) memcpy(p, f.data(), 8 * (size_t) n);
    const uint64_t u = oatk_mc::unit_of(p, n, anchor);
    CHECK(u == restated_unit(f, anchor));
    CHECK(u == chunked_unit(p, n, anchor));
    if (want != 1) CHECK(u == want);
    ++T.records, T.longer += n > oatk_mc::SHORT;
    if (u != oatk_mc::NONE) {
        ++T.valid, T.chunk_first += oatk_mc::unit_beg(u) >= oatk_mc::CHUNK;
        const std::vector<uint32_t> vt = restated_path(f, u);
        CHECK(vt.size() == oatk_mc::unit_nv(u) && vt[0] == (uint32_t) (anchor << 1));
        uint64_t h = oatk_mc::hash_seed(vt.size()), hr = h;
        for (uint32_t t = 0; t < vt.size(); ++t) {
            CHECK(oatk_mc::path_elem(oatk_mc::path_uid(p, u, t), u) == vt[t]);
            h += oatk_mc::hash_term(t, vt[t]);
        }
        for (uint32_t t = (uint32_t) vt.size(); t-- > 0;) hr += oatk_mc::hash_term(t, vt[t]);       // any order of the terms
        CHECK(h == hr);
        if (want_path) CHECK(vt == *want_path);
        T.paths.push_back(vt);
    } else CHECK(!want_path);
    free(p);
}

static uint64_t rng_state;
static uint64_t rnd() { rng_state += 0x9E3779B97F4A7C15ULL; return oatk_mc::mix64(rng_state); }

static void table(Tally &T)
{
    struct Case { std::vector<uint64_t> f; int beg, end, rev; std::vector<uint32_t> path; };
    const std::vector<Case> cases = {
        {{}, -1, 0, 0, {}}, {{10}, -1, 0, 0, {}}, {{10, 14}, -1, 0, 0, {}},
        {{10, 10}, 0, 0, 0, {10}},
        {{10, 14, 10}, 0, 1, 0, {10, 14}},
        {{10, 14, 11}, -1, 0, 0, {}}, {{10, 14, 10, 14, 11}, -1, 0, 0, {}},
        {{14, 10, 14, 10}, 1, 2, 0, {10, 14}},
        {{18, 10, 14, 10}, -1, 0, 0, {}},
        {{14, 18, 10, 14, 10}, -1, 0, 0, {}},
        {{18, 14, 10, 18, 14, 10, 18}, 2, 4, 0, {10, 18, 14}},
        {{11, 15, 11}, 0, 1, 1, {10, 14}},
        {{11, 19, 15, 11}, 0, 2, 1, {10, 14, 18}},
        {{10, 14, 18, 10}, 0, 2, 0, {10, 14, 18}},
        {{10, 14, 10, 18, 10}, -1, 0, 0, {}},
    };
    for (const Case &c : cases) {
        if (c.beg < 0) one_record(c.f, 5, T, UINT64_MAX);
        else one_record(c.f, 5, T, oatk_mc::pack((uint32_t) c.beg, (uint32_t) c.end, (uint32_t) c.rev), &c.path);
    }
    // the distinct paths of the table, in path_cmpfunc order with their multiplicities
    std::vector<std::vector<uint32_t>> ps = T.paths;
    std::sort(ps.begin(), ps.end(), [](const std::vector<uint32_t> &x, const std::vector<uint32_t> &y) { return oatk_mc::path_cmp(x.data(), x.size(), y.data(), y.size()) < 0; });
    const std::vector<std::pair<std::vector<uint32_t>, int>> want = {{{10}, 1}, {{10, 14}, 3}, {{10, 14, 18}, 2}, {{10, 18, 14}, 1}};
    size_t i = 0;
    for (const auto &w : want) {
        int c = 0;
        for (; i < ps.size() && ps[i] == w.first; ++i) ++c;
        CHECK(c == w.second);
    }
    CHECK(i == ps.size());
}

// seeded records over 6 unitigs: a third built periodic (a unit round the anchor, started at any phase, any number of turns), some of those with one fragment
// changed or one hit flipped; lengths from 0 to a few chunks
static void random_records(Tally &T, int count)
{
    for (int c = 0; c < count; ++c) {
        const uint64_t anchor = rnd() % 6;
        const uint32_t cls = (uint32_t) (rnd() % 8);
        const uint32_t n = cls == 0? (uint32_t) (rnd() % 1200) : cls < 3? (uint32_t) (rnd() % 200) : (uint32_t) (rnd() % 12);
        std::vector<uint64_t> f(n);
        if (rnd() % 3 == 0 && n) {
            const uint32_t period = 1 + (uint32_t) (rnd() % (n < 70? n : 70)), phase = (uint32_t) (rnd() % period);
            std::vector<uint64_t> unit(period);
            const uint64_t strand = rnd() & 1;
            unit[0] = anchor << 1 | strand;
            for (uint32_t t = 1; t < period; ++t) { do unit[t] = rnd() % 12; while (unit[t] >> 1 == anchor); }
            for (uint32_t j = 0; j < n; ++j) f[j] = unit[(j + phase) % period];
            const uint32_t spoil = (uint32_t) (rnd() % 4);
            if (spoil == 1) f[rnd() % n] ^= 2 + (rnd() % 3 << 2);                                   // another unitig somewhere
            if (spoil == 2) { const uint32_t j = (uint32_t) (rnd() % n); if (f[j] >> 1 == anchor) f[j] ^= 1; }      // one hit turned round
        } else
            for (uint32_t j = 0; j < n; ++j) f[j] = rnd() % 12;
        one_record(f, anchor, T);
    }
}

static void statistics()
{
    // A = unitig 5 (len 1000, cov 30), B = 7 (400, 10), C = 9 (250, 7); A+ -> C+ is there but deleted
    struct Arc { uint64_t v, w, ls; uint32_t del; };
    std::vector<Arc> arcs = {{10, 14, 100, 0}, {14, 10, 50, 0}, {10, 10, 20, 0}, {14, 18, 30, 0}, {18, 10, 40, 0}, {10, 18, 60, 1}};
    std::sort(arcs.begin(), arcs.end(), [](const Arc &x, const Arc &y) { return x.v != y.v? x.v < y.v : x.w < y.w; });
    oatk_asmg_t g;
    memset(&g, 0, sizeof(g));
    g.n_vtx = g.m_vtx = 10, g.n_arc = g.m_arc = arcs.size();
    g.vtx = (oatk_asmg_vtx_t *) calloc(g.n_vtx, sizeof(oatk_asmg_vtx_t));
    g.arc = (oatk_asmg_arc_t *) calloc(g.n_arc, sizeof(oatk_asmg_arc_t));
    g.idx_p = (uint64_t *) calloc(2 * g.n_vtx, 8), g.idx_n = (uint64_t *) calloc(2 * g.n_vtx, 8);
    g.vtx[5].len = 1000, g.vtx[5].cov = 30, g.vtx[7].len = 400, g.vtx[7].cov = 10, g.vtx[9].len = 250, g.vtx[9].cov = 7;
    for (size_t i = 0; i < arcs.size(); ++i) {
        g.arc[i].v = arcs[i].v, g.arc[i].w = arcs[i].w, g.arc[i].ls = arcs[i].ls, g.arc[i].del = arcs[i].del;
        if (g.idx_n[arcs[i].v]++ == 0) g.idx_p[arcs[i].v] = i;
    }
    auto make = [](const std::vector<std::vector<uint32_t>> &ps) {
        oatk_mc_paths P;
        P.n = P.m = ps.size();
        P.a = (oatk_mc_path *) calloc(ps.size(), sizeof(oatk_mc_path));
        for (size_t i = 0; i < ps.size(); ++i) {
            P.a[i].nv = (uint32_t) ps[i].size(), P.a[i].v = (uint32_t *) malloc(4 * ps[i].size()), P.a[i].len = 77, P.a[i].wlen = -7., P.a[i].cnt = i + 1;
            memcpy(P.a[i].v, ps[i].data(), 4 * ps[i].size());
        }
        return P;
    };
    oatk_mc_paths P = make({{10}, {10, 14}, {10, 14, 18}});
    CHECK(oatk_mc_path_stats(&g, &P) == OATK_OK);
    CHECK(P.a[0].len == 980 && P.a[0].wlen == 29400.);                     // 1000 - 20; 30 * 1000 - 30 * 20
    CHECK(P.a[1].len == 1250 && P.a[1].wlen == 31500.);                    // 1000 - 50 + 400 - 100; 30000 - 1500 + 4000 - 1000
    CHECK(P.a[2].len == 1480 && P.a[2].wlen == 33340.);                    // ... + 250 - 30, closing arc C -> A (40); 30000 - 1200 + 4000 - 1000 + 1750 - 210
    CHECK(P.a[2].cnt == 3);
    oatk_mc_paths_free(&P);
    CHECK(P.n == 0 && P.a == nullptr);
    // a path over the deleted arc: refused, and the sound path beside it is not written either
    P = make({{10, 14}, {10, 18}});
    CHECK(oatk_mc_path_stats(&g, &P) == OATK_E_ARG);
    CHECK(P.a[0].len == 77 && P.a[0].wlen == -7. && P.a[1].len == 77);
    oatk_mc_paths_free(&P);
    P = make({{10, 40}});                                                  // a vertex outside the graph
    CHECK(oatk_mc_path_stats(&g, &P) == OATK_E_ARG);
    oatk_mc_paths_free(&P);
    // len is 32 bits wide like the reference's: a unitig of 2^32 + 1000 bases counts as 1000
    g.vtx[5].len = (1ULL << 32) + 1000;
    P = make({{10}});
    CHECK(oatk_mc_path_stats(&g, &P) == OATK_OK && P.a[0].len == 980 && P.a[0].wlen == 29400.);
    oatk_mc_paths_free(&P);
    free(g.vtx); free(g.arc); free(g.idx_p); free(g.idx_n);
}

int main(int argc, char **argv)
{
    rng_state = argc > 1? strtoull(argv[1], 0, 10) : 1;
    Tally T;
    table(T);
    CHECK(T.records == 15 && T.valid == 7);
    // the hits of a record in its last chunk only, and a record whose second hit lies in another chunk than the first
    {
        std::vector<uint64_t> f(1100, 14);
        f[1090] = f[1095] = 10;
        one_record(f, 5, T, UINT64_MAX);                                   // beg = 1090 > r
        for (uint32_t j = 0; j < 1100; ++j) f[j] = j % 70 == 65? 11 : 15 + 2 * (j % 70);
        one_record(f, 5, T, oatk_mc::pack(65, 134, 1));
        f[1099] ^= 4;
        one_record(f, 5, T, UINT64_MAX);
    }
    random_records(T, 20000);
    statistics();
    std::sort(T.paths.begin(), T.paths.end());
    const size_t distinct = std::unique(T.paths.begin(), T.paths.end()) - T.paths.begin();
    printf("OK records=%llu valid=%llu long=%llu chunk_first=%llu distinct=%zu\n", (unsigned long long) T.records, (unsigned long long) T.valid,
           (unsigned long long) T.longer, (unsigned long long) T.chunk_first, distinct);
    return 0;
}
