"""GPU: the corrected chains built from the blocks' descriptors (ec.hpp: EcSeg, ec_new_n_seg_kernel, ec_assemble_pair_kernel / ec_assemble_seg_kernel)
against a round of the CPU oracle's on the same scan and count (tests/ec_util.py: oracle_round -- oracle/ecgraph.c, oracle/ec.c) and, where oracle/_ref is
built, against the compiled reference's read_error_correction.

What is compared.  The assembly writes five arrays per chain entry: the three that stay (EC_KMER, EC_MPOS, EC_SMER) and the (syncmer id, occurrence)
pairs, which the stable sort behind it turns into EC_SCM_OCC / EC_SCM_COV / EC_SCM_OCC_OFF / EC_SCM_DEL before anything can fetch them: a run whose
sorted lists and coverages are the oracle's wrote the pairs the oracle's chains give.  EC_N_SCM is new_n.

The cases are the places a table of segments can go wrong, and test_cases_are_present holds the data to them, read from the solver's own work list
and outcomes (EC_BLOCK_WORK, EC_BLOCK_OUT), not from the assembly:
  * reads with no block at all.  The walk (ec_blocks) either finds the leading block in its first round or gives the read up, so these are exactly the
    reads without a good syncmer, which keep their chains: unrelated reads, and reads shorter than k (no syncmer);
  * a read always has its leading block (r) first and an open block (end_utg == EC_NONE) last, so a read "whose only block is an end block" has these two
    and nothing else: clean reads;
  * blocks with nothing but the anchor kept between them (the front of a block is never empty: it holds at least the anchor);
  * solved and unsolved blocks next to each other in one read, either order;
  * solved blocks with a path of 1 entry (an open end that reaches no further syncmer), 2 (source and sink adjacent: nothing goes in) and more; a
    solved block with np == 0 does not exist: a path holds at least its source;
  * reads of exactly 64 and 65 syncmers (the last that a wave holds, the first that takes ec_assemble_read_serial), with errors in them;
  * a read with more than 64 blocks (a substitution every 410 bases over 36 kb; with more than 64 syncmers it takes the serial walk like any long read);
  * a number of reads that is no multiple of the four reads of a workgroup, down to a single wave in the last one;
  * sid0 > 0; a batch assembled by oatk_hip_scan_append."""
import numpy as np
import pytest

import adversarial as A
import ec_util as EU
import ref_lib as R
import test_gpu_ec as G
from oatk_amd import HipSyncasm, pack_reads

pytestmark = pytest.mark.gpu

K, S, C_MIN, EDIST, ARC_F = 101, 11, 4, 0.02, 0.35
OUT = ["EC_N_SCM", "EC_SCM_OFF", "EC_KMER", "EC_MPOS", "EC_SMER", "EC_SCM_COV", "EC_SCM_DEL", "EC_SCM_OCC_OFF", "EC_SCM_OCC"]


def haplotypes():
    rng = np.random.default_rng(20250)
    h1 = bytearray(A.rand_dna(rng, 6000))
    h2 = bytearray(h1)
    for p in range(75, 6000, 150):
        h2[p] = b"ACGT"[(b"ACGT".index(bytes([h2[p]])) + 1 + int(rng.integers(0, 3))) & 3]
    return bytes(h1), bytes(h2)


def cut_to_chain_length(hip, read, wants):
    """the shortest prefixes of `read` that carry exactly the given numbers of syncmers (one scan of every candidate prefix)"""
    lens = list(range(K, len(read) + 1))
    seq, off, ln = pack_reads([read[:n] for n in lens])
    hip.scan_host(seq, off, ln, K, S)
    n_scm = hip.fetch("N_SCM")
    out = []
    for w in wants:
        at = np.flatnonzero(n_scm == w)
        assert len(at), "no prefix with %d syncmers" % w
        out.append(read[:lens[int(at[0])]])
    return out


def with_errors(read, every, first):
    r = bytearray(read)
    for p in range(first, len(r), every):
        r[p] = b"ACGT"[(b"ACGT".index(bytes([r[p]])) + 1) & 3]
    return bytes(r)


_reads = {}


def case_reads(hip):
    if "r" in _reads:
        return _reads["r"]
    h1, h2 = haplotypes()
    rng = np.random.default_rng(7)
    reads = G.sample_reads(h1, 220, 1200, 0.006, 1) + G.sample_reads(h2, 220, 1200, 0.006, 2)       # a few blocks each, bubbles: unsolved ones among them
    reads += [(h1 + h1)[s:s + 1500] for s in range(0, 6000, 700)]                                      # clean: the two end blocks and nothing else
    reads += [A.rand_dna(rng, 900) for _ in range(5)] + [A.rand_dna(rng, 60), A.rand_dna(rng, 100)]   # no good syncmer; no syncmer
    long_clean = (h1 + h1)[300:300 + 5200]
    reads += cut_to_chain_length(hip, long_clean, (64, 65))
    reads += cut_to_chain_length(hip, with_errors(long_clean, 900, 400), (64, 65))                    # (cut after the errors: they make and unmake syncmers)
    reads += [A.revcomp(r) for r in cut_to_chain_length(hip, with_errors(long_clean, 700, 350), (64, 65))]
    reads += [with_errors((h2 * 7)[100:36100], 410, 125)]                                               # more than 64 blocks (410: no error twice at one place of the genome)
    reads += G.sample_reads(h1, 30, 3000, 0.004, 3)                                                     # chains around 50 syncmers, ten or more blocks
    if len(reads) % 4 == 0:
        reads.append((h2 + h2)[1000:2300])
    _reads["r"] = reads
    return reads


def correct(h):
    """one correction on the resident scan + count + graph; what it left"""
    st = h.ec(EDIST, C_MIN, ARC_F)
    got = {k: h.fetch(k) for k in OUT}
    got["stats"] = np.array(st[:11], np.uint64)
    return got


def oracle(h, off, blocks=False):
    """the oracle's round on the scan + count resident in `h`, under the names of `correct`'s arrays; with `blocks`, also the list of the blocks it visited"""
    o = EU.oracle_round(h, off, K, C_MIN, EDIST, ARC_F, blocks=blocks)
    scm_off = np.concatenate([[0], np.cumsum(o["n_scm"].astype(np.uint64))]).astype(np.uint64)
    res = {"EC_N_SCM": o["n_scm"], "EC_SCM_OFF": scm_off, "EC_KMER": o["k_mer"], "EC_MPOS": o["m_pos"], "EC_SMER": o["s_mer"], "EC_SCM_COV": o["cov"],
           "EC_SCM_DEL": o["del"], "EC_SCM_OCC_OFF": o["occ_off"], "EC_SCM_OCC": o["occ"], "stats": o["stats"].astype(np.uint64)}
    return (res, o["blocks"]) if blocks else res


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.fixture(scope="module")
def runs(hip):
    reads = case_reads(hip)
    ref = None
    seq, off, lens = pack_reads(reads)
    if R.available():
        from test_gpu_dropin import device_dbs
        db, scm = device_dbs(hip, reads, K, S)            # the device's scan + count, resident, and as the reference's structs
    else:
        hip.scan_host(seq, off, lens, K, S)
        hip.count()
    n_scm = hip.fetch("N_SCM")
    hip.ec_graph()
    seg = correct(hip)
    work = hip.fetch("EC_BLOCK_WORK").reshape(-1, 12)
    out = hip.fetch("EC_BLOCK_OUT").reshape(-1, 12)
    orc, blocks = oracle(hip, off, blocks=True)
    if R.available():
        from test_gpu_ec_routes import reference_run
        ref = reference_run(db, scm, K, S, EDIST, C_MIN, 10 * C_MIN, C_MIN, ARC_F)
    return {"reads": reads, "n_scm": n_scm, "seg": seg, "oracle": orc, "blocks": blocks, "work": work, "out": out, "ref": ref}


def test_descriptors_give_what_the_walk_gives(runs):
    """(the walk is the oracle's: oracle/ec.c walks every chain as syncerr.c does)"""
    assert_same(runs["oracle"], runs["seg"], "descriptors against the oracle's walk")
    assert int(runs["seg"]["EC_N_SCM"].sum()) == len(runs["seg"]["EC_KMER"]) > 0


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
def test_descriptors_give_what_the_reference_gives(runs):
    sr1, sc1, summary, marks = runs["ref"]
    for name, got in (("seg", runs["seg"]),):
        assert np.array_equal(got["EC_N_SCM"], sr1["n_scm"]), name
        assert np.array_equal(got["EC_KMER"], sr1["k_mer"]), name
        assert np.array_equal(got["EC_MPOS"], sr1["m_pos"]), name
        assert np.array_equal(got["EC_SMER"], sr1["s_mer"]), name
        assert np.array_equal(got["EC_SCM_COV"], sc1["cov"]), name
        assert np.array_equal(got["EC_SCM_DEL"], sc1["del"]), name
        assert np.array_equal(got["EC_SCM_OCC"], sc1["occ"]), name
        st = got["stats"]
        assert int(st[0] + st[5] + st[10]) == summary["total"] and int(st[2] + st[7]) == summary["corrected"], name


def block_table(runs):
    w, o = runs["work"], runs["out"]
    return {"read": w[:, 4].astype(np.int64), "r": w[:, 7] != 0, "open": (w[:, 2] == 0xFFFFFFFF) & (w[:, 3] == 0xFFFFFFFF),
            "solved": o[:, 0] == 1, "np": o[:, 1].astype(np.int64)}


def test_cases_are_present(runs):
    n_scm, n_reads = runs["n_scm"].astype(np.int64), len(runs["reads"])
    b = block_table(runs)
    nb = np.bincount(b["read"], minlength=n_reads)
    assert n_reads % 4 != 0
    # the work list is in read order, a read's blocks in chain order: the leading block first, an open one last
    assert np.all(np.diff(b["read"]) >= 0)
    first = np.flatnonzero(np.r_[True, np.diff(b["read"]) != 0])
    last = np.r_[first[1:], len(b["read"])] - 1
    assert np.all(b["r"][first]) and np.count_nonzero(b["r"]) == len(first) and np.all(b["open"][last]) and np.all(nb[nb > 0] >= 2)
    # no block: no good syncmer (with and without syncmers); such a read keeps its chain
    none = np.flatnonzero(nb == 0)
    assert np.any(n_scm[none] > 0) and np.any(n_scm[none] == 0)
    assert np.array_equal(runs["seg"]["EC_N_SCM"][none], runs["n_scm"][none])
    # end blocks only
    assert np.any(nb == 2)
    # 64 and 65 syncmers, with blocks inside; more than 64 blocks
    for n in (64, 65):
        assert np.any((n_scm == n) & (nb == 2)) and np.any((n_scm == n) & (nb > 2)), n
    assert nb.max() > 64
    # solved next to unsolved within a read of at most 64 syncmers, both orders; solved paths of 1, 2 and more entries, none of 0
    same = (b["read"][1:] == b["read"][:-1]) & (n_scm[b["read"][1:]] <= 64)
    assert np.any(same & b["solved"][1:] & ~b["solved"][:-1]) and np.any(same & ~b["solved"][1:] & b["solved"][:-1])
    nps = b["np"][b["solved"] & (n_scm[b["read"]] <= 64)]
    assert np.any(nps == 1) and np.any(nps == 2) and np.any(nps > 3) and not np.any(nps == 0)
    # solved and unsolved leading and closing blocks
    for kind in ("r", "open"):
        assert np.any(b[kind] & b["solved"]) and np.any(b[kind] & ~b["solved"]), kind
    # the corrected chains differ from the originals in length, both ways
    d = runs["seg"]["EC_N_SCM"].astype(np.int64) - n_scm
    assert np.any(d > 0) and np.any(d < 0)


@pytest.mark.parametrize("drop", [1, 2, 3])
def test_last_workgroup_partly_filled(hip, drop):
    """the last workgroup of the wave-per-read kernels holds fewer than its four reads: the full set leaves a remainder, and without its last one, two and three
    reads every other remainder is seen"""
    reads = case_reads(hip)[:-drop]
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    hip.count()
    hip.ec_graph()
    assert_same(oracle(hip, off), correct(hip), "drop %d" % drop)


def test_sid0_above_zero(hip, runs):
    reads = runs["reads"]
    seq, off, lens = pack_reads(reads)
    sid0 = 70001
    hip.scan_host(seq, off, lens, K, S, sid0=sid0)
    hip.count()
    hip.ec_graph()
    seg = correct(hip)
    # the same chains as at sid0 = 0 (which test_descriptors_give_what_the_walk_gives holds to the oracle), the occurrences' read ids moved by sid0
    for k in ("EC_N_SCM", "EC_SCM_OFF", "EC_KMER", "EC_MPOS", "EC_SMER", "EC_SCM_COV", "EC_SCM_DEL", "EC_SCM_OCC_OFF", "stats"):
        assert np.array_equal(seg[k], runs["seg"][k]), k
    assert np.array_equal(seg["EC_SCM_OCC"], runs["seg"]["EC_SCM_OCC"] + (np.uint64(sid0) << np.uint64(32)))


def test_appended_batch(hip, runs):
    reads = runs["reads"]
    cuts = (0, 1, 203, 204, len(reads))
    piece, main = HipSyncasm(0), HipSyncasm(0)
    try:
        main.scan_begin(K, S)
        for a, b in zip(cuts[:-1], cuts[1:]):
            sq, of, ln = pack_reads(reads[a:b])
            piece.scan_host(sq, of, ln, K, S, sid0=a)
            main.scan_append(piece)
        main.count()
        main.ec_graph()
        seg = correct(main)
        assert_same(runs["oracle"], seg, "appended against the oracle's round on these reads")
        assert_same(seg, runs["seg"], "appended against one scan")
    finally:
        piece.close()
        main.close()
