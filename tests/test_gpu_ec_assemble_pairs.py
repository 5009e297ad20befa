"""GPU: the corrected chains with two reads to a wave (oatk_amd/csrc/ec.hpp: ec_assemble_pair_kernel; r20) against a wave per read
(OATK_DEBUG_EC_ASSEMBLE_PAIRS=0: ec_assemble_seg_kernel) and against a round of the CPU oracle's on the same scan and count (tests/ec_util.py: oracle_round),
compared as tests/test_gpu_ec_assemble.py compares them: EC_N_SCM, EC_KMER, EC_MPOS, EC_SMER and, for the (syncmer id, occurrence) pairs, the sorted lists
and coverages made of them; where oracle/_ref is built, against the compiled reference too.

Wave w takes reads 2 w and 2 w + 1, in halves of 32 lanes when both have at most 32 chain entries and 32 blocks, one after the other otherwise.  The reads
are built the way that module builds its own (same haplotypes, K, S): 440 sampled reads of about 26 syncmers with errors and bubbles (solved and unsolved
blocks side by side, leading and open blocks of both kinds), then, from an even index on, every ordered pair of chain lengths 0, 1, 2, 31, 32, 33, 63, 64, 65
(clean prefixes; (32, 33) and (33, 32) must not share a wave), the pairs around 32 again with errors in them (one variant of the errors per pair), reads without a good syncmer (nb = 0, keep_all)
and without a syncmer on either side of a pair, reads of 27 .. 41 blocks (nb = 32 and 33 among them: a block costs a read three syncmers and more, so such a
read has more than 64 and takes the serial routine -- with n <= 32, nb cannot pass a dozen) beside short ones, and an odd last read."""
import os

import numpy as np
import pytest

import adversarial as A
import ref_lib as R
import test_gpu_ec_assemble as AS
from oatk_amd import pack_reads

pytestmark = pytest.mark.gpu

K, S, C_MIN = AS.K, AS.S, AS.C_MIN
PAIRS = "OATK_DEBUG_EC_ASSEMBLE_PAIRS"
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65)
_reads = {}


def case_reads(hip):
    if "r" in _reads:
        return _reads["r"]
    h1, h2 = AS.haplotypes()
    rng = np.random.default_rng(11)
    reads = AS.G.sample_reads(h1, 220, 1200, 0.006, 1) + AS.G.sample_reads(h2, 220, 1200, 0.006, 2)
    assert len(reads) % 2 == 0
    long_clean = (h1 + h1)[300:300 + 5200]
    cuts = (1, 2, 31, 32, 33, 63, 64, 65)
    clean = dict(zip(cuts, AS.cut_to_chain_length(hip, long_clean, cuts)))
    clean[0] = A.rand_dna(rng, 60)                                                      # shorter than k: no syncmer
    for a in LENGTHS:
        for b in LENGTHS:
            reads += [clean[a], clean[b]]
    # errors at places of their own per pair (a variant's two prefixes are all its copies: its errors stay below the coverage that would make them true)
    for (first, every), (a, b) in zip(((350, 700), (410, 650), (290, 750)), ((32, 33), (33, 32), (31, 32))):
        err = dict(zip((31, 32, 33), AS.cut_to_chain_length(hip, AS.with_errors(long_clean, every, first), (31, 32, 33))))
        reads += [err[a], A.revcomp(err[b])]
    unrelated = [A.rand_dna(rng, 900) for _ in range(4)]                                # syncmers, none of them good: the read keeps its chain
    reads += [unrelated[0], clean[31], clean[32], unrelated[1], unrelated[2], unrelated[3], clean[0], unrelated[0][:700], clean[0], clean[0]]
    for k in range(24, 39):                                                             # k + 1 errors at places of the read's own, so about k + 3 blocks
        first = 125 + 13 * (k - 24)
        p = AS.with_errors((h2 * 7)[100:100 + first + 410 * k + 205], 410, first)
        reads += [p, clean[31]] if k % 2 else [clean[32], p]
    if len(reads) % 2 == 0:
        reads.append(clean[32])
    _reads["r"] = reads
    return reads


def correct(hip, env):
    old = os.environ.get(PAIRS)
    os.environ.pop(PAIRS, None)
    os.environ.update(env)
    try:
        st = hip.ec(AS.EDIST, C_MIN, AS.ARC_F)
    finally:
        os.environ.pop(PAIRS, None)
        if old is not None:
            os.environ[PAIRS] = old
    got = {k: hip.fetch(k) for k in AS.OUT}
    got["stats"] = np.array(st[:11], np.uint64)
    return got


@pytest.fixture(scope="module")
def runs(hip):
    reads = case_reads(hip)
    ref = None
    seq, off, lens = pack_reads(reads)
    if R.available():
        from test_gpu_dropin import device_dbs
        db, scm = device_dbs(hip, reads, K, S)
    else:
        hip.scan_host(seq, off, lens, K, S)
        hip.count()
    n_scm = hip.fetch("N_SCM")
    hip.ec_graph()
    pairs = correct(hip, {})
    single = correct(hip, {PAIRS: "0"})
    orc = AS.oracle(hip, off)
    work = hip.fetch("EC_BLOCK_WORK").reshape(-1, 12)
    out = hip.fetch("EC_BLOCK_OUT").reshape(-1, 12)
    if R.available():
        from test_gpu_ec_routes import reference_run
        ref = reference_run(db, scm, K, S, AS.EDIST, C_MIN, 10 * C_MIN, C_MIN, AS.ARC_F)
    return {"reads": reads, "n_scm": n_scm, "pairs": pairs, "single": single, "oracle": orc, "work": work, "out": out, "ref": ref}


def test_two_reads_to_a_wave_give_what_one_gives(runs):
    AS.assert_same(runs["single"], runs["pairs"], "two reads to a wave against one")
    AS.assert_same(runs["oracle"], runs["pairs"], "two reads to a wave against the oracle's round")
    assert int(runs["pairs"]["EC_N_SCM"].sum()) == len(runs["pairs"]["EC_KMER"]) > 0


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
def test_two_reads_to_a_wave_give_what_the_reference_gives(runs):
    sr1, sc1, summary, marks = runs["ref"]
    got = runs["pairs"]
    assert np.array_equal(got["EC_N_SCM"], sr1["n_scm"]) and np.array_equal(got["EC_KMER"], sr1["k_mer"])
    assert np.array_equal(got["EC_MPOS"], sr1["m_pos"]) and np.array_equal(got["EC_SMER"], sr1["s_mer"])
    assert np.array_equal(got["EC_SCM_COV"], sc1["cov"]) and np.array_equal(got["EC_SCM_DEL"], sc1["del"]) and np.array_equal(got["EC_SCM_OCC"], sc1["occ"])
    st = got["stats"]
    assert int(st[0] + st[5] + st[10]) == summary["total"] and int(st[2] + st[7]) == summary["corrected"]


def test_cases_are_present(runs):
    n, n_reads = runs["n_scm"].astype(np.int64), len(runs["reads"])
    b = AS.block_table(runs)
    nb = np.bincount(b["read"], minlength=n_reads)
    assert n_reads % 2 == 1                                                             # an odd last read
    m = n_reads // 2
    n0, n1, nb0, nb1 = n[0:2 * m:2], n[1:2 * m:2], nb[0:2 * m:2], nb[1:2 * m:2]
    keeps = (nb == 0) & (n > 0)                                                         # no good syncmer: keep_all
    fits = (n <= 32) & (nb <= 32) & ((nb > 0) | keeps)
    shared = fits[0:2 * m:2] & fits[1:2 * m:2]
    print("%d reads, %d pairs, %d of them share a wave" % (n_reads, m, int(shared.sum())))
    assert int(shared.sum()) > 200 and int((~shared).sum()) > 60
    # every ordered pair of the chain lengths at a pair's two places
    for a in LENGTHS:
        for c in LENGTHS:
            assert np.any((n0 == a) & (n1 == c)), (a, c)
    # ... (32, 33) and (33, 32) with blocks beyond the two end blocks
    assert np.any((n0 == 32) & (n1 == 33) & (nb0 > 2)) and np.any((n0 == 33) & (n1 == 32) & (nb1 > 2)) and np.any(shared & (n0 == 31) & (n1 == 32) & (nb0 > 2) & (nb1 > 2))
    # nb = 0 with keep_all in either half, beside a read with blocks and beside another of its kind; no syncmer at all (the serial routine) in either half
    k0, k1 = keeps[0:2 * m:2], keeps[1:2 * m:2]
    assert np.any(shared & k0 & (nb1 > 0)) and np.any(shared & k1 & (nb0 > 0)) and np.any(shared & k0 & k1)
    assert np.any((n0 == 0) & (n1 > 0)) and np.any((n1 == 0) & (n0 > 0)) and np.any((n0 == 0) & (n1 == 0))
    # nb = 32 and 33, in either half, beside a read that would share
    for want in (32, 33):
        assert np.any(nb == want), (want, sorted(set(nb[nb > 20].tolist())))
    assert np.any((nb0 > 26) & fits[1:2 * m:2]) and np.any((nb1 > 26) & fits[0:2 * m:2])
    # in reads that share a wave: solved next to unsolved, both orders; leading and open blocks of both kinds; paths of 1, 2 and more entries
    sh_read = np.zeros(n_reads, bool)
    sh_read[0:2 * m:2], sh_read[1:2 * m:2] = shared, shared
    inr = sh_read[b["read"]]
    same = (b["read"][1:] == b["read"][:-1]) & inr[1:]
    assert np.any(same & b["solved"][1:] & ~b["solved"][:-1]) and np.any(same & ~b["solved"][1:] & b["solved"][:-1])
    for kind in ("r", "open"):
        assert np.any(inr & b[kind] & b["solved"]) and np.any(inr & b[kind] & ~b["solved"]), kind
    nps = b["np"][b["solved"] & inr]
    assert np.any(nps == 1) and np.any(nps == 2) and np.any(nps > 3)
    # both halves of a shared wave with path interiors of different lengths, and one half with none
    pc = np.bincount(b["read"], weights=np.where(b["solved"], np.maximum(b["np"] - 2, 0), 0), minlength=n_reads)
    p0, p1 = pc[0:2 * m:2], pc[1:2 * m:2]
    assert np.any(shared & (p0 > p1) & (p1 > 0)) and np.any(shared & (p1 > p0) & (p0 > 0)) and np.any(shared & (p0 == 0) & (p1 > 0))
    d = runs["pairs"]["EC_N_SCM"].astype(np.int64) - n
    assert np.any(d[sh_read] > 0) and np.any(d[sh_read] < 0)


@pytest.mark.parametrize("drop", [1, 2, 3])
def test_last_workgroup_partly_filled(hip, drop):
    """a workgroup holds four waves, eight reads: without its last one, two and three reads the set ends in an even pair, an odd read, and another workgroup fill"""
    reads = case_reads(hip)[:-drop]
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    hip.count()
    hip.ec_graph()
    AS.assert_same(correct(hip, {PAIRS: "0"}), correct(hip, {}), "drop %d" % drop)
