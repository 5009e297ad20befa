"""The second tier of the read alignment (align_big.hpp, ra_big_run) at every limit, against oracle/align.c: bit-exact, no tolerance.

Every read is random DNA of its own (K = 101, S = 11, scanned and counted, no error correction: every syncmer has coverage 1), so a read hits only the
unitigs that its own recipe (align_util: tandem, pieces, ladder, gapped, ugapped, singletons, compose) lays down, and its hit, fragment, predecessor and alignment
counts are known in closed form (tests/test_align_recipes.py proves the closed forms on the CPU).  Which reads take the second tier is measured: with
OATK_DEBUG_RA_NO_BIG set the first tier reports in RA_SKIPPED exactly the reads whose plan is over one of its limits."""
import contextlib
import functools
import re

import numpy as np
import pytest

import adversarial as A
import align_util as AU

pytestmark = pytest.mark.gpu
K, S = 101, 11
# read groups: ~13, ~18, ~52 and ~66 syncmers a read
GROUPS = {"a": (900, 160), "b": (1200, 260), "c": (3300, 140), "d": (4000, 8)}


@functools.lru_cache(maxsize=None)
def reads_of(seed, spec):
    rng = np.random.default_rng(seed)
    return tuple(A.rand_dna(rng, ln) for ln, cnt in spec for _ in range(cnt))


def resident(hip, seed=2024, spec=tuple(GROUPS.values())):
    """scan + count on the device; the chains as the aligner will read them"""
    from oatk_amd import pack_reads
    hip.scan_host(*pack_reads(list(reads_of(seed, spec))), K, S)
    hip.count()
    cov = hip.fetch("SCM_COV")
    assert cov.max() == 1, "the reads share a syncmer: a read would hit another read's unitigs"
    chains = hip.fetch("N_SCM"), hip.fetch("POS_KID"), hip.fetch("POS_MPOS")
    assert int(chains[0].sum()) == len(cov)
    return chains, len(cov)


@contextlib.contextmanager
def two_pass_mode(hip, mode):
    hip._check(hip.L.oatk_hip_debug_align_two_pass(hip.h, mode), "oatk_hip_debug_align_two_pass")
    try:
        yield
    finally:
        hip._check(hip.L.oatk_hip_debug_align_two_pass(hip.h, 0), "oatk_hip_debug_align_two_pass")


def without(want, reads):
    """the oracle's result less the alignments of `reads`"""
    keep = ~np.isin(want["sid"], np.asarray(sorted(reads), np.uint64))
    fk = np.repeat(keep, want["n"])
    return {k: (want[k][keep] if k in ("sid", "n", "s") else want[k][fk]) for k in AU.OUT_FIELDS}


def check(hip, monkeypatch, chains, G, exps, old=None, what=""):
    """first tier alone: RA_SKIPPED is exactly the reads planned over its limits (and the others equal the oracle); both tiers: only the reads planned
    over the second tier's limits are reported, everything else equals the oracle.  Returns (device result, oracle result, reads over the first tier)"""
    n_reads = len(chains[0])
    want = AU.oracle_align(*chains, G, old)
    live = [r for r in exps if old is None or old[r] & 1]                      # (bit 0 clear: the read is not looked at, alignment.c:225)
    big = sorted(r for r in live if AU.over_small(exps[r]))
    over = sorted(r for r in big if AU.over_big(exps[r]))
    assert np.array_equal(AU.graph_hits(chains, G)[sorted(exps)], [exps[r]["hits"] for r in sorted(exps)])
    monkeypatch.setenv("OATK_DEBUG_RA_NO_BIG", "1")
    got1 = AU.device_align(hip, G, old)
    sk1 = np.sort(hip.fetch("RA_SKIPPED")).tolist()
    monkeypatch.delenv("OATK_DEBUG_RA_NO_BIG")
    assert sk1 == big and got1["skipped"] == len(big), (what, "first tier alone", sk1, big)
    AU.assert_same(got1, without(want, big), (what, "first tier alone"))
    got = AU.device_align(hip, G, old)
    sk = np.sort(hip.fetch("RA_SKIPPED")).tolist()
    assert sk == over and got["skipped"] == len(over), (what, "both tiers", sk, over)
    AU.assert_same(got, without(want, over), what)
    if old is None:
        AU.assert_as_planned(got, exps, n_reads, skipped=set(over))
        assert (got["n_mapped"], got["n_unique"]) == (want["n_mapped"] - sum(1 for r in over if exps[r]["aln"]),
                                                      want["n_unique"] - sum(1 for r in over if sum(exps[r]["aln"].values()) == 1))
    return got, want, big


def batches(hip, monkeypatch, capfd, G):
    """how many batches the second tier cut its reads into, from its own stage report (one line per pass over the batches)"""
    monkeypatch.setenv("OATK_DEBUG_RA_STAGES", "1")
    capfd.readouterr()
    AU.device_align(hip, G)
    err = capfd.readouterr().err
    monkeypatch.delenv("OATK_DEBUG_RA_STAGES")
    seen = {int(x) for x in re.findall(r"\[ra\] (\d+) batches of reads with many hits", err)}
    assert len(seen) == 1, err
    return seen.pop()


def take(n_chain, lo, hi, used):
    """the next unused read with lo <= syncmers <= hi"""
    for r, n in enumerate(n_chain.tolist()):
        if r not in used and lo <= n <= hi:
            used.add(r)
            return r, n
    raise AssertionError("no read with %d..%d syncmers left" % (lo, hi))


def sweep_jobs(n_chain):
    """every first-tier limit one step either side, forward and flipped, on a few reads each"""
    jobs, used = [], set()
    for rep in range(3):
        for flip in (False, True):
            for hits in (159, 160, 161):
                for lo, hi in ((12, 30), (41, 70)):
                    r, n = take(n_chain, lo, hi, used)
                    jobs.append((r, AU.tandem(n, hits // n, hits % n, loop=bool(rep & 1) or hits != 160), flip))
            for f in (128, 129):
                r, n = take(n_chain, 8, 31, used)
                jobs.append((r, AU.tandem(n, 1, tail=f - 1), flip))
                r, n = take(n_chain, 8, 31, used)
                jobs.append((r, AU.compose(AU.tandem(n, 1), AU.singletons(n, f - 1)), flip))
                r, n = take(n_chain, 8, 16, used)
                jobs.append((r, AU.compose(AU.tandem(n, 2, tail=50), AU.singletons(n, f - 52)), flip))
            for w in (6, 7):
                r, n = take(n_chain, 8, 21, used)
                jobs.append((r, AU.ladder(n, [n // 2], w, rep & 1, dead=rep == 2), flip))
                r, n = take(n_chain, 12, 30, used)
                jobs.append((r, AU.ladder(n, [2, n - 2], [w, 1, 1], [0, rep & 1]), flip))
                r, n = take(n_chain, 9, 14, used)
                jobs.append((r, AU.ladder(n, [3, 6], [1, w, w], [1, 0]), flip))
            for depth in (47, 48, 49):
                r, n = take(n_chain, 52, 70, used)
                jobs.append((r, AU.pieces(n, range(1 + rep, depth + rep)), flip))
            r, n = take(n_chain, 41, 70, used)
            jobs.append((r, AU.pieces(n, range(2, 2 * 20, 2), [i & 1 for i in range(19)], dead=True), flip))
            r, n = take(n_chain, 12, 30, used)
            jobs.append((r, AU.gapped(n, n // 2, 1), flip))
    return jobs


def copies(n, more=0):
    """how often a chain of n syncmers is laid so that the tandem alone is over the first tier's 160 hits"""
    return 161 // n + 1 + more


def second_tier_jobs(n_chain):
    """reads over the hit limit whose fragments are multi-hit, gapped, chained over arcs of ln 0 and 1, self-loops and deleted arcs"""
    jobs, used = [], set()
    for rep in range(4):
        flip = bool(rep & 1)
        for lo, hi in ((12, 30), (41, 70)):
            r, n = take(n_chain, lo, hi, used)
            m = copies(n, rep)
            jobs.append((r, AU.compose(AU.tandem(n, m, rep), AU.ladder(n, [n // 3, n // 2], 3, [1, 0], dead=rep >= 2)), flip))
            r, n = take(n_chain, lo, hi, used)
            jobs.append((r, AU.compose(AU.ladder(n, [4, 6, n - 2], [2, 3, 1, 4], [rep & 1, 0, 1]), AU.tandem(n - 1, copies(n - 1, rep), n_read=n)), flip))
            # the gapped predecessor first, then the complete one that starts later: raise and reset; the shorter tandem only brings the hits
            r, n = take(n_chain, lo, hi, used)
            jobs.append((r, AU.compose(AU.gapped(n, n // 2, 1), AU.tandem(n - 2, copies(n - 2, rep), 1, n_read=n)), flip))
            r, n = take(n_chain, lo, hi, used)
            jobs.append((r, AU.compose(AU.gapped(n, 2 * (2 + rep), 2 + rep), AU.tandem(n - 2, copies(n - 2, 2), n_read=n)), flip))           # gapped score 0
            # the gap score in the open: GAP + B alone, n - 2g
            r, n = take(n_chain, lo, hi, used)
            g = 1 if n < 30 else 1 + rep
            jobs.append((r, AU.compose(AU.gapped(n, n // 2, g, late=False), AU.tandem(n - 2 * g - 1, copies(n - 2 * g - 1, 3), n_read=n)), flip))
            # under 90 % of the read: no alignment
            r, n = take(n_chain, lo, hi, used)
            k = (9 * n - 1) // 10
            assert k / n < 0.9 <= (k + 1) / n or k + 1 == n
            jobs.append((r, AU.compose(AU.pieces(k, [k // 2], rep & 1, n_read=n), AU.tandem(k - 1, copies(k - 1, 1), n_read=n)), flip))
            # the unitig's gap (u_gap > s_gap) against a tandem one syncmer shorter than the gapped chain's score
            r, n = take(n_chain, lo, hi, used)
            jobs.append((r, AU.compose(AU.ugapped(n, n // 2, 1 + rep), AU.tandem(n - 2 - rep, copies(n - 2 - rep, 1), n_read=n)), flip))
            r, n = take(n_chain, lo, hi, used)
            jobs.append((r, AU.tandem(n, m + 4, tail=3 * (rep & 1), loop=rep < 2), flip))      # singletons behind the chains of one unitig
            # 65 fragments: the predecessors of one fragment are recorded by turns j of two different rounds of 64, scores raised in one are read in the next
            r, n = take(n_chain, lo, hi, used)
            jobs.append((r, AU.ladder(n, [2, 4, 6, 8], [30, 2, 30, 1, 2], [0, 0, rep & 1, 0]), flip))
        for n in (20, 50):                                                     # exactly 90 % of the read: aligned (min_a_frac is a strict bound)
            r, n = take(n_chain, n, n, used)
            k = 9 * n // 10
            jobs.append((r, AU.compose(AU.pieces(k, [k // 3, k // 2], 0, n_read=n), AU.tandem(k - 1, copies(k - 1, rep), n_read=n)), flip))
    return jobs


@pytest.mark.parametrize("two_pass", [0, 1])
def test_limit_sweep_of_the_first_tier(hip, monkeypatch, two_pass):
    """hits 159 / 160 / 161, fragments 128 / 129, predecessors 6 / 7, depth 47 / 48 / 49: the reads one step over go to the second tier and come back
    equal to the oracle; the reads at the limit stay in the first"""
    chains, n_scm = resident(hip)
    jobs = sweep_jobs(chains[0])
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    with two_pass_mode(hip, two_pass):
        got, want, big = check(hip, monkeypatch, chains, G, exps)
    over = {k: sum(1 for r in big if exps[r][k] > v) for k, v in AU.SMALL_LIMITS.items()}
    at = {k: sum(1 for r in exps if r not in big and exps[r][k] == v) for k, v in AU.SMALL_LIMITS.items()}
    assert min(over.values()) >= 6 and min(at.values()) >= 6, (over, at)
    assert len(got["sid"]) > len(jobs)


@pytest.mark.parametrize("two_pass", [0, 1])
def test_second_tier_chains_gaps_arcs(hip, monkeypatch, two_pass):
    """every read is over the first tier's limits and its best chain needs what the one-syncmer graphs never ask for: followed links, gap scores of the
    read and of the unitig, the arc loop with deleted arcs first, a raised score that resets the predecessors, walks over several predecessors"""
    chains, n_scm = resident(hip)
    jobs = second_tier_jobs(chains[0])
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    assert G["arc_del"].sum() > 0 and set(G["arc_ln"].tolist()) == {0, 1}
    with two_pass_mode(hip, two_pass):
        got, want, big = check(hip, monkeypatch, chains, G, exps)
    assert big == sorted(exps)
    cnt = np.bincount(got["sid"].astype(np.int64), minlength=len(chains[0]))
    assert any(cnt[r] > 1 for r in big) and any(cnt[r] == 0 for r in big)
    assert any(got["n"][got["sid"] == r].max() >= 3 for r in big if cnt[r])


@pytest.mark.parametrize("two_pass", [0, 1])
def test_rab_prev_32_is_aligned_33_is_reported(hip, monkeypatch, two_pass):
    chains, n_scm = resident(hip)
    jobs, used = [], set()
    for w in (32, 33):
        for flip in (False, True):
            for ovl in (0, 1):
                r, n = take(chains[0], 8, 30, used)
                jobs.append((r, AU.ladder(n, [n // 2], w, ovl), flip))
            r, n = take(chains[0], 8, 30, used)
            jobs.append((r, AU.ladder(n, [n - 2], [w, 1]), flip))              # (only the predecessor count is over: 32 w + n - 2 hits)
    jobs += [(r, p, f) for r, p, f in sweep_jobs(chains[0])[:40] if r not in used]
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    with two_pass_mode(hip, two_pass):
        got, want, big = check(hip, monkeypatch, chains, G, exps)
    over = [r for r in big if AU.over_big(exps[r])]
    assert len(over) == 6 and all(exps[r]["prev"] == 33 for r in over)
    assert not np.isin(got["sid"], over).any()
    assert sum(1 for r in exps if exps[r]["aln"] == {2: 1024} and (got["sid"] == r).sum() == 1024) == 4


@pytest.mark.parametrize("two_pass", [0, 1])
def test_old_ra_threshold_on_big_reads(hip, monkeypatch, two_pass):
    """max_score one below, equal to and one above old_ra >> 1; bit 0 clear: not aligned and not reported"""
    chains, n_scm = resident(hip)
    jobs = second_tier_jobs(chains[0])
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    old = np.ones(len(chains[0]), np.int64)
    for i, (r, p, _) in enumerate(jobs):
        old[r] = ((p["exp"]["score"] + (1, 0, -1, 0)[i & 3]) << 1) | (0 if i & 3 == 3 else 1)
    with two_pass_mode(hip, two_pass):
        got, want, big = check(hip, monkeypatch, chains, G, exps, old)
    assert len(big) == len(jobs) - len(jobs[3::4])
    cnt = np.bincount(got["sid"].astype(np.int64), minlength=len(chains[0]))
    for i, (r, p, _) in enumerate(jobs):
        assert cnt[r] == (sum(p["exp"]["aln"].values()) if i & 3 in (1, 2) else 0), (i, r)
    assert cnt.sum() > 0


def test_batches_give_the_same_arrays(hip, monkeypatch, capfd):
    """every read a batch of its own, and a budget that cuts the reads into uneven batches: the same arrays as one batch"""
    chains, n_scm = resident(hip)
    jobs = second_tier_jobs(chains[0])
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    want = AU.oracle_align(*chains, G)
    hits = sorted(exps[r]["hits"] for r in exps)
    for two_pass in (0, 1):
        with two_pass_mode(hip, two_pass):
            base = AU.device_align(hip, G)
            assert base["skipped"] == 0 and batches(hip, monkeypatch, capfd, G) == 1
            AU.assert_same(base, want, "one batch")
            for budget in (1, hits[len(hits) // 2] + hits[0] + 1, 3 * hits[-1]):
                monkeypatch.setenv("OATK_DEBUG_RA_BUDGET", str(budget))
                got = AU.device_align(hip, G)
                nb = batches(hip, monkeypatch, capfd, G)
                monkeypatch.delenv("OATK_DEBUG_RA_BUDGET")
                assert nb == len(exps) if budget == 1 else 1 < nb < len(exps), (budget, nb)
                assert got["skipped"] == 0
                AU.assert_same(got, base, ("budget", budget, two_pass))


@pytest.mark.parametrize("two_pass", [0, 1])
def test_4100_big_reads_cross_the_batch_edge(hip, monkeypatch, capfd, two_pass):
    """4095 reads fill a batch (RAB_IDX_BITS = 12): the last reads of the first batch carry the top bit of the batch index in both sort keys, the rest
    start a second batch.  Every third read also chains across arcs."""
    spec = ((1200, 4100),)
    chains, n_scm = resident(hip, 77, spec)
    jobs = []
    for r, n in enumerate(chains[0].tolist()):
        m = copies(n, r % 3)
        p = AU.tandem(n, m, r % 5 if r % 5 < n else 0)
        if r % 3 == 0:
            p = AU.compose(p, AU.ladder(n, [n // 2], 2, r & 1))
        jobs.append((r, p, bool(r & 2)))
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    with two_pass_mode(hip, two_pass):
        got, want, big = check(hip, monkeypatch, chains, G, exps)
        assert batches(hip, monkeypatch, capfd, G) == 2                        # (4095 + 5: nowhere near the default budget of hits)
    assert len(big) == 4100


@pytest.mark.parametrize("two_pass", [0, 1])
def test_upper_edge_of_hits_per_read(hip, monkeypatch, two_pass):
    """64 syncmers laid 2^15 - 1 times: 2^21 - 64 hits, aligned, 32767 alignments; laid 2^15 times: 2^21 hits, reported, everybody else unchanged"""
    chains, n_scm = resident(hip)
    used = set()
    r, n = take(chains[0], 64, 71, used)
    others = [(r2, p, f) for r2, p, f in second_tier_jobs(chains[0])[:16] + sweep_jobs(chains[0])[:16] if r2 != r]
    others = list({j[0]: j for j in others}.values())
    with two_pass_mode(hip, two_pass):
        for m in ((1 << 15) - 1, 1 << 15):
            G, exps = AU.recipe_graph(n_scm, chains, [(r, AU.tandem(64, m, n_read=n), m & 1 == 0)] + others)
            assert exps[r]["hits"] == 64 * m
            got, want, big = check(hip, monkeypatch, chains, G, exps, what=m)
            assert int((got["sid"] == r).sum()) == (32767 if m < 1 << 15 else 0) and int((want["sid"] == r).sum()) == m
            assert (got["skipped"] == 1) == (m == 1 << 15)


@pytest.mark.parametrize("two_pass", [0, 1])
def test_pool_runs_short_in_both_tiers(hip, monkeypatch, two_pass):
    """ladders of width 2 and depth 8 (512 alignments a read), some under the first tier's limits, some made big by a tandem: more alignments than the
    pool holds (cap_a of oatk_hip_read_alignment), so with two-pass off the result comes from the in-place rerun of both tiers"""
    chains, n_scm = resident(hip)
    jobs, used = [], set()
    for i in range(150):
        r, n = take(chains[0], 12, 30, used)
        cuts = [1 + j * (n - 1) // 8 for j in range(8)]
        p = AU.ladder(n, cuts, 2)
        if i % 3 == 0:
            p = AU.compose(p, AU.tandem(n, copies(n)))
        jobs.append((r, p, bool(i & 1)))
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    with two_pass_mode(hip, two_pass):
        got, want, big = check(hip, monkeypatch, chains, G, exps)
    n_reads = len(chains[0])
    cap_a = 2 * n_reads + (1 << 16)
    assert len(big) == 50 and len(want["sid"]) > cap_a and sum(sum(exps[r]["aln"].values()) for r in big) > 50 * 512
