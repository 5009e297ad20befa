"""GPU: the light EC graph on candidate ranks (ecgraph.hpp: packed pair keys, the pairs by a lane per chain entry) against the route it replaces.

Every comparison takes the graph arrays (OATK_BUF_EG_*, the flags of OATK_BUF_EG_OTHER among them), the results of hip.ec(...) on that graph and its
statistics, and holds them between OATK_DEBUG_EC_LIGHT_PACKED=0 (64-bit keys on vertex ids) and the route on candidate ranks, with the key width the
candidates give and with OATK_DEBUG_EC_LIGHT_KEYBITS=64.  Where the full graph is
built, the arcs are also held against the full graph's arcs between candidates, as test_gpu_light_graph does: test_gpu_ec.py holds the full graph to the
compiled reference."""
import ctypes as C
from collections import Counter, defaultdict

import numpy as np
import pytest

import adversarial as A
import test_gpu_ec as E
import test_gpu_light_graph as LG
from oatk_amd import OatkHipError, pack_reads

pytestmark = pytest.mark.gpu

EG_OTHER = 127
# name, OATK_DEBUG_EC_LIGHT_PACKED, _KEYBITS
ROUTES = [("old", "0", "0"), ("both", "1", "0"), ("both-64", "1", "64")]
ARCS = ("arc_v", "arc_w", "arc_ls", "arc_cov", "arc_comp")


def set_route(monkeypatch, route):
    _, packed, bits = route
    monkeypatch.setenv("OATK_DEBUG_EC_LIGHT_PACKED", packed)
    monkeypatch.setenv("OATK_DEBUG_EC_LIGHT_KEYBITS", bits)


def fetch_other(hip):
    p, b = C.c_void_p(), C.c_uint64()
    hip._check(hip.L.oatk_hip_buffer(hip.h, EG_OTHER, C.byref(p), C.byref(b)), "oatk_hip_buffer(EG_OTHER)")
    out = np.zeros(b.value, dtype=np.uint8)
    if b.value:
        hip._check(hip.L.oatk_hip_d2h(hip.h, out.ctypes.data, p, b.value), "d2h")
    return out


def scan_count(hip, reads, K, S):
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    hip.count()
    return hip.fetch_count()["cov"]


def light_run(hip, monkeypatch, route, c):
    """the light graph by one route, and the correction on it: graph arrays + other, results, statistics"""
    set_route(monkeypatch, route)
    hip.ec_graph(light_c=c)
    g = LG.graph_arrays(hip)
    g["other"] = fetch_other(hip)
    st = hip.ec(0.02, c, 0.35)
    return g, {k: E.fetch_ec(hip, k) for k in LG.RES}, st.tolist()


def full_run(hip, c):
    hip.ec_graph()
    assert len(fetch_other(hip)) == 0                       # no flags without a light graph
    g = LG.graph_arrays(hip)
    st = hip.ec(0.02, c, 0.35)
    return g, {k: E.fetch_ec(hip, k) for k in LG.RES}, st.tolist()


def compare_routes(hip, monkeypatch, c, cov=None, full=None, routes=ROUTES):
    """every route against the first; with `full`, also against the full graph's arcs between candidates and the correction on the full graph"""
    g0, r0, s0 = light_run(hip, monkeypatch, routes[0], c)
    assert len(g0["other"]) == len(g0["idx_n"])
    if full is not None:
        fg, fr, fs = full
        keep = (cov[(fg["arc_v"] >> 1).astype(np.int64)] >= c) & (cov[(fg["arc_w"] >> 1).astype(np.int64)] >= c)
        for k in ARCS:
            assert np.array_equal(g0[k], fg[k][keep]), (routes[0][0], k)
        for k in LG.RES:
            assert np.array_equal(r0[k], fr[k]), (routes[0][0], k)
        assert s0 == fs
        # the flags: an oriented candidate with an arc of the full graph to a syncmer below c
        cand_v, rare_w = cov[(fg["arc_v"] >> 1).astype(np.int64)] >= c, cov[(fg["arc_w"] >> 1).astype(np.int64)] < c
        want = np.zeros(len(g0["other"]), np.uint8)
        want[fg["arc_v"][cand_v & rare_w].astype(np.int64)] = 1
        assert np.array_equal(g0["other"], want), (routes[0][0], "other")
    for route in routes[1:]:
        g, r, s = light_run(hip, monkeypatch, route, c)
        for k in g0:
            assert np.array_equal(g[k], g0[k]), (route[0], k)
        for k in LG.RES:
            assert np.array_equal(r[k], r0[k]), (route[0], k)
        assert s == s0, route[0]
    return g0


def host_pairs(hip, cov, c):
    """the pairs the light graph keeps, from the resident chains: canonical key on oriented vertex ids and distance, in (read, slot) order"""
    n = hip.fetch("N_SCM").astype(np.int64)
    ids, mp = (hip.fetch("POS_KID") >> np.uint64(1)).astype(np.int64), hip.fetch("POS_MPOS").astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)])
    v, p = ids << 1 | (mp & 1), mp >> 1
    first = np.zeros(len(v), bool)
    first[off[:-1][n > 0]] = True
    i = np.nonzero(~first)[0]
    v0, v1, d = v[i - 1], v[i], p[i] - p[i - 1]
    keep = (cov[v0 >> 1] >= c) & (cov[v1 >> 1] >= c)
    v0, v1, d = v0[keep], v1[keep], d[keep]
    return np.where(v0 <= v1, v0 << 32 | v1, (v1 ^ 1) << 32 | (v0 ^ 1)), d, n


def key_bits(cov, c):
    """2 B of ecgraph.hpp: the width of a packed key"""
    n_cand = int((cov >= c).sum())
    return 2 * max(1, (2 * n_cand - 1).bit_length())


@pytest.mark.parametrize("case", range(len(LG.CASES)))
def test_existing_light_cases_by_every_route(hip, monkeypatch, case):
    K, S, c, mk = LG.CASES[case]
    cov = scan_count(hip, mk(), K or hip.L.oatk_hip_max_k(), S)
    full = full_run(hip, c)
    g = compare_routes(hip, monkeypatch, c, cov, full)
    assert 0 < len(g["arc_v"]) < len(full[0]["arc_v"]) and g["other"].any()


# ---- read shapes of the pair pass ----
SK, SS = 101, 11


def shape_reads():
    """every prefix of one sequence without homopolymers from below K to 4300 bases: a syncmer is a property of its k-mer, so the number of syncmers grows by at
    most one per base and every count from 0 on occurs, 64 and 65 among them (the test looks); syncmer i of the sequence lies on fewer prefixes than syncmer
    i - 1, so coverages are all different and a threshold picks exactly one, two, ... candidates.  Every third prefix is reverse-complemented.  Then one read with
    several hundred syncmers of its own.  4200 reads: seventeen workgroups of the pair pass, whose trips of 256 entries end inside reads and at reads' ends."""
    rng = np.random.default_rng(1812)
    base = A.rand_nohp(rng, 4300)
    reads = [base[:n] if n % 3 else A.revcomp(base[:n]) for n in range(SK - 6, 4300)]
    reads.append(A.rand_nohp(rng, 21000))
    return reads


@pytest.mark.parametrize("kind", ["mid", "none", "one", "two", "all"])
def test_read_shapes_and_thresholds(hip, monkeypatch, kind):
    cov = scan_count(hip, shape_reads(), SK, SS)
    n = hip.fetch("N_SCM")
    assert n[0] == 0 and all((n == x).any() for x in (0, 1, 2, 64, 65)) and n.max() > 300
    top = np.sort(cov)[::-1]
    assert top[0] > top[1] > top[2] > 2000
    c = {"mid": 2000, "none": int(top[0]) + 1, "one": int(top[0]), "two": int(top[1]), "all": 1}[kind]
    assert int((cov >= c).sum()) == {"none": 0, "one": 1, "two": 2, "all": len(cov)}.get(kind, int((cov >= c).sum()))
    full = full_run(hip, c)
    g = compare_routes(hip, monkeypatch, c, cov, full)
    if kind in ("none", "one"):
        assert len(g["arc_v"]) == 0                                             # (one candidate: it is never next to itself)
    elif kind == "all":
        assert len(g["arc_v"]) == len(full[0]["arc_v"]) and not g["other"].any()
    else:
        assert len(g["arc_v"]) > 0 and g["other"].any()


def test_more_candidates_than_a_32_bit_key_holds(hip, monkeypatch):
    """one-fold coverage of some 3.4 Mb, c = 1: more than 32 768 candidates, so two oriented ranks take more than 32 bits and the keys are 64-bit without the override"""
    rng = np.random.default_rng(64)
    reads = [A.rand_dna(rng, 2300) for _ in range(1500)]
    reads = [A.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    cov = scan_count(hip, reads, SK, SS)
    assert int((cov >= 1).sum()) > 32768 and key_bits(cov, 1) > 32
    full = full_run(hip, 1)
    g = compare_routes(hip, monkeypatch, 1, cov, full)
    assert len(g["arc_v"]) > 60000


# ---- ties of the overlap mode ----
def tie_reads():
    """600 loci `flank + unit * n + flank` with a unit of ten bases of the locus's own: the array yields no syncmer (its period divides K - S, so the first and the
    last s-mer of every window inside it are equal and the minimum is at both ends or at neither: test_gpu_config1s.many_distance_reads), so the last
    syncmer in front of it and the first one behind it are adjacent on every read of the locus, at a distance that follows n.  A locus is read two or three
    times, mostly with a different n each time: one arc, two or three distances seen once each, and its overlap is that of the distance khashl's bucket order
    puts first -- which depends on the order the distances arrive in.  Arrays of 11 to 16 units keep many of the distances below K, where overlaps differ."""
    rng = np.random.default_rng(2)
    reads = []
    for i in range(600):
        fa, fb, unit = A.rand_dna(rng, 260), A.rand_dna(rng, 260), A.rand_nohp(rng, 10)
        while unit[0] == unit[-1]:
            unit = A.rand_nohp(rng, 10)
        ns = [11 + int(x) for x in rng.permutation(6)[:2 + i % 2]]
        if i % 5 == 0:
            ns.append(ns[0])                                                    # one distance twice: no tie
        for j, n in enumerate(ns):
            r = fa + unit * n + fb
            reads.append(A.revcomp(r) if (i + j) % 3 == 0 else r)
    order = rng.permutation(len(reads))
    return [reads[i] for i in order] + [A.rand_dna(rng, 900) for _ in range(100)]


def count_ties(keys, dist, K):
    tab = defaultdict(Counter)
    for k, d in zip(keys.tolist(), dist.tolist()):
        tab[k][d] += 1
    tie = [m for m in (t.most_common(2) for t in tab.values()) if len(m) == 2 and m[0][1] == m[1][1]]
    return len(tie), sum(1 for m in tie if min(m[0][0], m[1][0]) < K)


def test_ties_of_the_overlap_mode_keep_read_order(hip, monkeypatch):
    cov = scan_count(hip, tie_reads(), SK, SS)
    keys, dist, _ = host_pairs(hip, cov, 2)
    n_tie, n_tie_short = count_ties(keys, dist, SK)
    print("arcs whose two most frequent distances tie: %d, %d of them with a distance below K" % (n_tie, n_tie_short))
    assert n_tie >= 300 and n_tie_short >= 100
    full = full_run(hip, 2)
    g = compare_routes(hip, monkeypatch, 2, cov, full)                          # arc_ls against the full graph's among them
    assert len(np.unique(g["arc_ls"])) > 20


# ---- sizes on both sides of rocPRIM's small-input paths ----
def test_a_batch_with_few_kept_pairs(hip, monkeypatch):
    cov = scan_count(hip, A.hifi_like(400, 30000, 3000, seed=77, err=0.003), SK, SS)
    keys, _, _ = host_pairs(hip, cov, 6)
    assert 1000 < len(keys) < 100_000
    compare_routes(hip, monkeypatch, 6, cov, full_run(hip, 6))


def test_a_batch_with_more_than_a_million_kept_pairs(hip, monkeypatch):
    """(41, 31): a syncmer every five or six bases, 1.5 M adjacent pairs from 14 Mb of reads; the routes against each other only"""
    cov = scan_count(hip, A.hifi_like(2800, 100_000, 5000, seed=78, err=0.0002), 41, 31)
    keys, _, n = host_pairs(hip, cov, 2)
    print("kept pairs: %d, candidates: %d, key bits: %d" % (len(keys), int((cov >= 2).sum()), key_bits(cov, 2)))
    assert len(keys) > 1_500_000 and key_bits(cov, 2) <= 32 and n.max() > 64
    g = compare_routes(hip, monkeypatch, 2)
    assert len(g["arc_v"]) > 10000 and g["other"].any()


# ---- a syncmer adjacent to itself on both strands ----
def test_duplicate_arcs_are_refused_by_every_route(hip, monkeypatch):
    """Reads never hold a syncmer next to itself on one strand (test_ref_self_adjacent.py), so the resident chains are patched: on one read an entry becomes a
    copy of its left neighbour on the forward strand, on another on the reverse strand -- keys (2v, 2v) and (2v + 1, 2v + 1), each of which brings the
    other as its complement (tests/adversarial.py, tandem_repeat_reads).  The full graph and every light route answer OATK_E_SPLIT with one text."""
    cov = scan_count(hip, A.hifi_like(60, 20000, 3000, seed=5, err=0.0), SK, SS)
    n = hip.fetch("N_SCM").astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)])
    kid, mp = hip.fetch("POS_KID"), hip.fetch("POS_MPOS")
    assert n[0] > 4 and n[1] > 4
    v = kid[off[0] + 1] >> np.uint64(1)
    for r, strand in ((0, 0), (1, 1)):
        for j in (1, 2):
            kid[off[r] + j] = v << np.uint64(1)
            mp[off[r] + j] = (mp[off[r] + j] & ~np.uint32(1)) | np.uint32(strand)
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for name, arr in (("POS_KID", kid), ("POS_MPOS", mp)):
        p, b = hip.buffer(name)
        assert b == arr.nbytes and rt.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
    assert cov[int(v)] >= 1
    texts = []
    with pytest.raises(OatkHipError, match="duplicate arcs") as ei:
        hip.ec_graph()
    texts.append(str(ei.value))
    for route in ROUTES:
        set_route(monkeypatch, route)
        with pytest.raises(OatkHipError, match="duplicate arcs") as ei:
            hip.ec_graph(light_c=1)
        texts.append(str(ei.value).replace("oatk_hip_ec_graph_light", "oatk_hip_ec_graph"))
    assert len(set(texts)) == 1 and "(code 5)" in texts[0], texts
