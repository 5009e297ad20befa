"""GPU: every route of the error-block solver (oatk_amd/csrc/api_ec.inc) against the COMPILED REFERENCE's read_error_correction (syncerr.c:819),
bit for bit, away from the one operating point test_gpu_ec.py holds (max_edist 0.02, max_arc_f 0.35, max_err_c 10 c, err_arc_c c).

Long blocks on the shipping caps, no cap hooks: a diploid genome (SNP bubbles: the live graph branches, so by default the classes run) with no
homopolymer, tiled at 2 c per haplotype, plus one read per planned length of the form genome[a:b] + X + genome[c:d].  X is homopolymer-free and
unique to its read, b is the end of a genome syncmer and c the start of one, so the read has ONE block of exactly |X| bases (its syncmers that
touch X are seen once).  The lengths sit on both sides of every cap at the max_edist under test -- the first tier, classes 1 - 3, the second
stage's five classes, round 4's tiers and ec_band_cap's 60 000 -- derived below from the formulas of api_ec.inc / ec_heavy.hpp / ec_fused.hpp /
ec_wave.hpp.  Every planned block is found in the solver's work list with its length, the kernel that finished it (EcBlockOut.tier) must be one
its length allows, and OATK_DEBUG_EC_STAGES must show each intended route running.

Thresholds: max_arc_f (with exact ties of arc_cov == min(cov_v, cov_w) * a), c of 1, 2 and above most coverages, err_arc_c < err_mer_c and
max_err_c <= err_mer_c, on the full graph and -- where it can serve them -- the light one."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import adversarial as A
import ec_util as E
import ref_lib as R
import test_gpu_ec as G
from test_gpu_dropin import device_dbs

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")]

# ---- the solver's caps (api_ec.inc, ec_heavy.hpp, ec_fused.hpp, ec_wave.hpp, ec.hpp) ----
EC_CAP_T0, EC_CAP_T1 = 3072, 16384        # api_ec.inc: the first tier; round 4's last LDS tier
EC_MIN_ERR_BASE = 6                       # ec.hpp
ECH_NW = 4                                # ec_heavy.hpp: waves of class 3
ECF_S = 4                                 # ec_fused.hpp: a wave owns 64 - 2 ECF_S slots of the wavefront
ECF_OWN = 64 - 2 * ECF_S
LDS = 64 * 1024
CLIP = 60000                              # ec_band_cap: no class takes longer blocks


def band_cap(bwmax, e):
    """ec_band_cap: the longest block whose band ceil(l * max_edist) fits bwmax diagonals, at most 60 000 bases"""
    ct = math.floor(bwmax / e) if e > 0 else 0x3FFFFFFF
    while ct > 0 and math.ceil(ct * e) > bwmax:
        ct -= 1
    return min(ct, CLIP)


def cap_c(t, K):                          # ec_cap_c: the consensus of a block of t bases
    return t + t // 8 + 2 * K + 64


def words(b):                             # ecw_words
    return (b + 15) // 16 + 2


def ech_lds(t, K, fl, R):                 # ech_lds_words * 4 (ech_misc_words uses ECH_NW whatever the kernel's waves)
    misc = (2 * ECH_NW * 2 + 2 * R * ECH_NW * 2 + 2 * ECH_NW + 8 + 1) & ~1
    return 4 * (((misc + words(t) + words(cap_c(t, K)) + 1) & ~1) + fl // 4)


def ecf_lds(t, K, fl, NW):                # ecf_lds_words * 4
    misc = (2 * NW + 2 * NW * 2 * ECF_S + 2 * NW * 2 + 2 * NW + 8 + 1) & ~1
    return 4 * (((misc + words(t) + words(cap_c(t, K)) + 1) & ~1) + fl // 4)


def lds_tier(t, path, fl, hybrid, e, K):
    """ec_lds_tier: (cap_t, usable)"""
    bw = int(t * e) + 1
    cw = 2 * max(bw, EC_MIN_ERR_BASE) + 12
    if hybrid:
        b = 4 * ((words(t) + words(cap_c(t, K)) + 2 * (cw + 2) + 1) & ~1)
    else:
        b = 4 * (((words(t) + words(cap_c(t, K)) + 2 * (cw + 2) + 1) & ~1) + 4 * path + fl // 4)
    return t, b <= LDS


# kernel variants (EcBlockOut.tier): ec_wave_kernel's MODE, 16 + R / 8 + R for ec_heavy_kernel with one / ECH_NW waves, 32 + NW for ec_fused_kernel
T_LDS, T_SLAB, T_HYBRID = 0, 1, 2
T_CLASS = {1: 16 + 4, 2: 16 + 8, 3: 8 + 6}
T_STAGE2 = [32 + 16, 32 + 8, 32 + 4, 32 + 2, 16 + 1]


def class_plan(e, K):
    """ec_solve_classes and ec_second_stage at max_edist e: caps and whether each carve-up fits LDS"""
    cls = {}
    for c, (R, fl) in {1: (4, 4096), 2: (8, 4096), 3: (6, 32768)}.items():
        t = band_cap(((64 if c < 3 else 256) * R - 3) // 2, e)
        cls[c] = (t, ech_lds(t, K, fl, R) <= LDS)
    routes = {1: cls[1][1], 2: cls[2][1] and cls[2][0] > cls[1][0]}
    t0, t0_ok = lds_tier(EC_CAP_T0, 32, 2048, False, e, K)
    t0_ok = t0_ok and cls[1][1] and t0 <= cls[1][0]
    st2 = []
    for NW, fl in ((16, 32768), (8, 24576), (4, 16384), (2, 12288), (1, 8192)):
        t = band_cap(((64 if NW == 1 else NW * ECF_OWN) - 3) // 2, e)
        st2.append((t, (ech_lds(t, K, fl, 1) if NW == 1 else ecf_lds(t, K, fl, NW)) <= LDS))
    narrowest = len(st2) - 1
    while narrowest > 0 and not st2[narrowest][1]:
        narrowest -= 1
    return {"t0": (t0, t0_ok), "cls": cls, "routes": routes, "st2": st2, "narrowest": narrowest}


def class_route(P, l):
    """where ec_route_kernel sends a block of l bases: 0 (first tier) .. 3"""
    caps = [P["t0"][0] if P["t0"][1] else -1, P["cls"][1][0] if P["routes"][1] else 0, P["cls"][2][0] if P["routes"][2] else 0]
    t = 0
    while t < 3 and l > caps[t]:
        t += 1
    return t


def stage2_class(P, l):
    """the second stage's class of a block of l bases (ec_route_longer_kernel over a list sorted longest first)"""
    st2, nar = P["st2"], P["narrowest"]
    for i in range(nar):
        if l > (st2[i + 1][0] if st2[i + 1][1] else -1):
            return i
    return nar


def class_tags(P, l):
    """(kernels that may finish a block of l bases on the classes path, whether it must reach the second stage, whether it must reach the slabs)"""
    r = class_route(P, l)
    tags, first_holds = {T_SLAB}, True
    if r == 0:
        tags |= {T_LDS, T_CLASS[1]}                     # (the first tier's left-overs go to class 1)
    elif P["cls"][r][1]:
        tags.add(T_CLASS[r])
        first_holds = l <= P["cls"][r][0]
    else:
        first_holds = False
    i = stage2_class(P, l)
    t, ok = P["st2"][i]
    second_holds = ok and l <= t
    if second_holds:
        tags.add(T_STAGE2[i])
    if not first_holds:
        tags.discard(T_CLASS.get(r))
    return tags, not first_holds, not first_holds and not second_holds


def tier_plan(e, K):
    """ec_solve_tiers at max_edist e: the three LDS tiers (the last one hybrid)"""
    return [lds_tier(EC_CAP_T0, 32, 2048, False, e, K), lds_tier(min(2 * EC_CAP_T0, EC_CAP_T1), 64, 4096, False, e, K),
            lds_tier(EC_CAP_T1, 0, 0, True, e, K)]


def tier_route(T, l):
    t = 0
    while t < 3 and l > (T[t][0] if T[t][1] else 0):
        t += 1
    return t


def tier_tags(T, l):
    r = tier_route(T, l)
    tags = {T_SLAB}
    for t in range(r, 3):
        if T[t][1] and l <= T[t][0]:
            tags.add(T_HYBRID if t == 2 else T_LDS)
    return tags, r == 3


def planned_lengths(e, K):
    """block lengths on both sides of every cap at max_edist e"""
    P, T = class_plan(e, K), tier_plan(e, K)
    caps = {P["t0"][0], CLIP} | {t for t, _ in P["cls"].values()} | {t for t, _ in P["st2"]} | {t for t, _ in T}
    return sorted({x for c in caps if 20 <= c <= CLIP for x in (c, c + 1)})


# ---- data ----
def nohp_base(rng, avoid):
    return int(rng.choice([b for b in b"ACGT" if b not in avoid]))


def diploid_nohp(rng, n, snp_every):
    """a homopolymer-free haplotype and a second one with a SNP every snp_every bases (still homopolymer-free); the SNP positions"""
    h1 = bytearray(A.rand_nohp(rng, n))
    h2 = bytearray(h1)
    snps = list(range(snp_every // 2, n - 1, snp_every))
    for p in snps:
        h2[p] = nohp_base(rng, {h1[p], h1[p - 1], h1[p + 1]})
    return bytes(h1), bytes(h2), snps


def tiled(h, n_reads, length, phase, rc_every):
    """n_reads reads of `length` bases evenly around the circular haplotype h (every base covered n_reads * length / len(h) times)"""
    hh = h + h
    out = []
    for i in range(n_reads):
        st = (phase + i * len(h) // n_reads) % len(h)
        r = hh[st:st + length]
        out.append(A.revcomp(r) if i % rc_every == 0 else r)
    return out


LONG_GENOME = {1001: (24000, 2600, 6000, 31), 2049: (36000, 5200, 9000, 31)}     # K: genome, SNP spacing, read length, S
LONG_C = 3


def long_block_reads(K, e):
    """tiled diploid reads at 2 c per haplotype, and one read with a block of exactly l bases for every planned l"""
    n, snp, rl, S = LONG_GENOME[K]
    rng = np.random.default_rng(K * 1000 + int(e * 1000))
    h1, h2, snps = diploid_nohp(rng, n, snp)
    per_hap = 2 * LONG_C * n // rl
    reads = tiled(h1, per_hap, rl, 0, 3) + tiled(h2, per_hap, rl, rl // 3, 4)
    # genome syncmers that no SNP touches, away from the ends: the anchors of the long blocks
    sr = R.SrDb.from_reads([h1], K, S)
    f = sr.flatten()
    sr.close()
    pos = (f["m_pos"][:int(f["n_scm"][0])] >> 1).astype(np.int64)
    snp_a = np.array(snps)
    ok = [int(p) for p in pos if 3000 <= p <= n - 3000 - K and not np.any((snp_a >= p) & (snp_a < p + K))]
    assert len(ok) >= 4, "too few clean anchor syncmers"
    plan = []
    for j, l in enumerate(planned_lengths(e, K)):
        p_left = ok[j % len(ok)]
        p_right = ok[(j + len(ok) // 2) % len(ok)]
        b, c = p_left + K, p_right
        x = bytearray(A.rand_nohp(rng, l))
        # no homopolymer across a junction, and no k-mer that overlaps X equal to the genome's at that place (X[0] != h1[b], X[-1] != h1[c - 1])
        if x[0] in (h1[b - 1], h1[b]):
            x[0] = nohp_base(rng, {h1[b - 1], h1[b], x[1]})
        if x[-1] in (h1[c], h1[c - 1]):
            x[-1] = nohp_base(rng, {h1[c], h1[c - 1], x[-2]})
        reads.append(h1[b - K - 1500:b] + bytes(x) + h1[c:c + K + 1500])
        plan.append(l)
    return reads, plan, S


class _H:
    def __init__(self, h):
        self.handle = h


def device_ec(hip, e, c, max_err_c, err_arc_c, a):
    L = hip.L
    L.oatk_hip_ec.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double]
    L.oatk_hip_ec_stats.argtypes = [C.c_void_p, C.c_void_p]
    rc = L.oatk_hip_ec(hip.h, None, e, c, max_err_c, err_arc_c, a)
    hip._check(rc, "oatk_hip_ec")
    st = np.zeros(12, np.uint64)
    hip._check(L.oatk_hip_ec_stats(hip.h, st.ctypes.data), "oatk_hip_ec_stats")
    got = {k: G.fetch_ec(hip, k) for k in G.EC_BUF}
    return st, got


def reference_run(db, scm, K, S, e, c, max_err_c, err_arc_c, a):
    """read_error_correction of the reference on the same structs: the corrected chains, the refreshed table, the summary and the error syncmers
    (find_error_syncmers(…, del_err = 1) deletes their vertices from the graph, and nothing after it touches a vertex: EC_ERR_DEL)"""
    L = R.lib()
    g = L.refx_make_graph(db, scm, 0, 0.0)
    L.refx_consensus(db, g, 1, 1)
    summary = E.reference_ec(_H(db), _H(scm), g, e, c, a, threads=3, max_err_c=max_err_c, err_arc_c=err_arc_c)
    marks = E.flatten_graph(g)["vtx_del"].copy()
    L.refx_scg_destroy(g)
    rdb, rscm = object.__new__(R.SrDb), object.__new__(R.ScmDb)
    rdb._h, rdb.K, rdb.S, rscm._h = db, K, S, scm
    out = (rdb.flatten(), rscm.flatten(), summary, marks)
    rscm.close(), rdb.close()
    return out


def assert_matches(st, got, ref):
    sr1, sc1, summary, marks = ref
    assert np.array_equal(got["EC_ERR_DEL"], marks)
    assert np.array_equal(got["EC_N_SCM"], sr1["n_scm"])
    assert np.array_equal(got["EC_KMER"], sr1["k_mer"])
    assert np.array_equal(got["EC_MPOS"], sr1["m_pos"])
    assert np.array_equal(got["EC_SMER"], sr1["s_mer"])
    assert np.array_equal(got["EC_SCM_COV"], sc1["cov"])
    assert np.array_equal(got["EC_SCM_DEL"], sc1["del"])
    assert np.array_equal(got["EC_SCM_OCC"], sc1["occ"])
    total = int(st[0] + st[5] + st[10])
    assert total == summary["total"]
    assert int(st[2] + st[7]) == summary["corrected"] and int(st[1] + st[6]) == summary["uncorrected"]
    assert int(st[3] + st[8]) == summary["ambiseq"] and int(st[4] + st[9]) == summary["ambipath"]


def stage_counts(err):
    """what OATK_DEBUG_EC_STAGES said about one call"""
    out = {}
    m = re.search(r"first stage done: (\d+) blocks go on \(classes got (\d+) \+ (\d+) \+ (\d+)(?:; (\d+) past)?", err)
    if m:
        out["on"], out["c1"], out["c2"], out["c3"], out["past"] = (int(x or 0) for x in m.groups())
    m = re.search(r"second stage [\d.]+ ms; (\d+) left for the slabs", err)
    out["left"] = int(m.group(1)) if m else None
    out["st2"] = {}
    for w, n in re.findall(r"\[ec stages\] (\d+) waves: (\d+) blocks", err):
        out["st2"][int(w)] = int(n)
    m = re.search(r"\[ec stages\] one wave: (\d+) blocks", err)
    if m:
        out["st2"][1] = int(m.group(1))
    out["tier"] = {}
    for t, n, how in re.findall(r"\[ec stages\] tier (\d): (\d+) blocks( routed by length| left over)?", err):
        out["tier"].setdefault(int(t), []).append((int(n), how.strip()))
    out["solver"] = "tiers" if "round 4's tiers" in err else ("classes" if "classes with budgets" in err else None)
    return out


SOLVERS = {"default": None, "tiers": "0", "classes": "1"}
MAX_EDIST = [0.0, 0.005, 0.01, 0.015, 0.02, 0.03, 0.05]


@pytest.mark.parametrize("e", MAX_EDIST)
@pytest.mark.parametrize("K", [1001, 2049])
def test_long_blocks_on_every_route(hip, capfd, monkeypatch, K, e):
    reads, plan, S = long_block_reads(K, e)
    P, T = class_plan(e, K), tier_plan(e, K)
    for k in ("OATK_DEBUG_EC_STEP_BUDGET", "OATK_DEBUG_EC_SERIAL_TIERS", "OATK_DEBUG_EC_FUSED_MIN_NW", "OATK_DEBUG_EC_HEAVY_CAP2", "OATK_DEBUG_EC_HEAVY_FL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("OATK_DEBUG_EC_STAGES", "1")
    hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, 0, 0), "oatk_hip_debug_ec_tiers")      # the shipping caps
    db, scm = device_dbs(hip, reads, K, S)
    G.device_graph(hip)
    c = LONG_C
    runs = {}
    for name, heavy in SOLVERS.items():
        if heavy is None:
            monkeypatch.delenv("OATK_DEBUG_EC_HEAVY", raising=False)
        else:
            monkeypatch.setenv("OATK_DEBUG_EC_HEAVY", heavy)
        capfd.readouterr()
        st, got = device_ec(hip, e, c, 10 * c, c, 0.35)
        err = capfd.readouterr().err
        w = hip.fetch("EC_BLOCK_WORK").reshape(-1, 12)
        o = hip.fetch("EC_BLOCK_OUT").reshape(-1, 12)
        closed = (w[:, 2] != 0xFFFFFFFF) | (w[:, 3] != 0xFFFFFFFF)           # an anchor on both sides (end_utg != EC_NONE)
        runs[name] = (st, got, err, w[:, 6].astype(np.int64), o[:, 11].astype(np.int64), np.where(closed, w[:, 4].astype(np.int64), -1))
    monkeypatch.delenv("OATK_DEBUG_EC_HEAVY", raising=False)
    ref = reference_run(db, scm, K, S, e, c, 10 * c, c, 0.35)
    n_plain = len(reads) - len(plan)
    for name, (st, got, err, lens, tags, rid) in runs.items():
        assert_matches(st, got, ref)
        sc = stage_counts(err)
        assert sc["solver"] == ("tiers" if name == "tiers" else "classes"), (name, err[:300])     # the live graph branches
        # every planned block: in the work list with exactly its length (the read's only block with two anchors; its ends are open blocks), finished
        # by a kernel its length allows
        for j, l in enumerate(plan):
            mine = rid == n_plain + j
            assert np.count_nonzero(mine) == 1 and int(lens[mine][0]) == l, (name, l, lens[mine])
            want = class_tags(P, l)[0] if sc["solver"] == "classes" else tier_tags(T, l)[0]
            assert int(tags[mine][0]) in want, (name, l, int(tags[mine][0]), want)
        if sc["solver"] == "classes":
            routes = [class_route(P, int(l)) for l in lens]
            for r in (2, 3):
                n_r = sum(1 for x in routes if x == r)
                if not P["cls"][r][1]:
                    assert sc["c%d" % r] == 0
                    continue
                assert sc["c%d" % r] == n_r, (name, r, sc, n_r)
            past = sum(1 for x in routes if x >= 1 and not P["cls"][x][1])
            assert sc["past"] == past, (name, sc, past)
            must2 = [int(l) for l in lens if class_tags(P, int(l))[1]]
            must_slab = [int(l) for l in lens if class_tags(P, int(l))[2]]
            assert sc["on"] >= len(must2)
            if must2:
                assert sc["left"] is not None                                            # the second stage ran
                for l in must2:                                                          # ... and every class it had to run
                    i = stage2_class(P, l)
                    if P["st2"][i][1]:
                        nw = [16, 8, 4, 2, 1][i]
                        assert sc["st2"].get(nw, 0) > 0, (name, l, nw, sc)
            if must_slab:
                assert sc["left"] >= len(must_slab) > 0, (name, sc, must_slab)         # left for the slabs
            # the cases reach every class whose carve-up fits, and the slabs
            assert any(class_route(P, l) == 3 for l in plan) and must_slab
        else:
            routed = [tier_route(T, int(l)) for l in lens]
            for t in (1, 2):
                if T[0][1] and T[t][1] and t in routed:                                 # (routed only beside a usable first tier)
                    assert (sum(1 for x in routed if x == t), "routed by length") in sc["tier"].get(t, []), (name, t, sc)
            n_slab = sum(1 for x in routed if x == 3)
            assert n_slab > 0 and sum(n for n, _ in sc["tier"].get(3, [])) >= n_slab, (name, sc)
    # the 60 000 clip and class 3 were reached by the planned lengths
    assert max(plan) > CLIP and any(l > P["cls"][2][0] for l in plan)


# ---- thresholds ----
def threshold_reads():
    return G.diploid_reads(101, 6000, 150, 500, 1200, 0.006)


THRESHOLDS = [
    # err_mer_c, max_err_c, err_arc_c, max_arc_f
    (3, 30, 3, 0.0), (3, 30, 3, 0.2), (3, 30, 3, 0.5), (3, 30, 3, 1.0), (3, 30, 3, 1.5),
    (1, 10, 1, 0.35), (2, 20, 2, 0.35),
    (40, 400, 40, 0.35),                      # above most coverages: nearly every syncmer goes
    (4, 40, 2, 0.35), (4, 40, 3, 0.5),        # err_arc_c < err_mer_c: the full graph only
    (4, 4, 4, 0.35), (4, 3, 6, 0.5),          # max_err_c <= err_mer_c: no syncmer is judged by its arcs; below it, the full graph only
]


@pytest.mark.parametrize("th", THRESHOLDS, ids=lambda t: "c%d-m%d-r%d-a%g" % t)
def test_thresholds_match_reference(hip, th):
    c, max_err_c, err_arc_c, a = th
    K, S, e = 101, 11, 0.02
    reads = threshold_reads()
    hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, 0, 0), "oatk_hip_debug_ec_tiers")
    db, scm = device_dbs(hip, reads, K, S)
    D = G.device_graph(hip)
    if a == 0.5:                               # ties: arc_cov == min(cov_v, cov_w) * a exactly, decided by the >= of ec_mark_kernel
        cov = hip.fetch("SCM_COV").astype(np.int64)
        mn = np.minimum(cov[(D["arc_v"] >> 1).astype(np.int64)], cov[(D["arc_w"] >> 1).astype(np.int64)])
        assert np.count_nonzero(2 * D["arc_cov"].astype(np.int64) == mn) > 0
    st, got = device_ec(hip, e, c, max_err_c, err_arc_c, a)
    light_ok = err_arc_c >= c and max_err_c >= c            # (below max_err_c a syncmer seen fewer than c times stays, with arcs the light graph never made)
    hip.ec_graph(light_c=c)
    L = hip.L
    if light_ok:
        st_l, got_l = device_ec(hip, e, c, max_err_c, err_arc_c, a)
        assert st_l.tolist() == st.tolist()
        for k in got:
            assert np.array_equal(got_l[k], got[k]), k
    else:
        assert L.oatk_hip_ec(hip.h, None, e, c, max_err_c, err_arc_c, a) == 2 and b"light" in L.oatk_hip_last_error(hip.h)
    ref = reference_run(db, scm, K, S, e, c, max_err_c, err_arc_c, a)
    assert_matches(st, got, ref)
    if c == 40:
        assert np.count_nonzero(got["EC_ERR_DEL"]) > 0.9 * len(got["EC_ERR_DEL"])
    else:
        assert int(st[0] + st[5] + st[10]) > 0
