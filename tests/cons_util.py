"""Helpers for the base-space consensus tests: flat read views, oracle (oracle/consensus.c) and compiled-reference calls."""
import ctypes as C

import numpy as np

import oracle_lib as O


class ReadsView(C.Structure):
    _fields_ = [("sid0", C.c_uint64), ("scm_off", C.c_void_p), ("k_mer", C.c_void_p), ("m_pos", C.c_void_p), ("hs_off", C.c_void_p),
                ("hoco_s", C.c_void_p), ("rl_off", C.c_void_p), ("ho_rl", C.c_void_p), ("lrl_off", C.c_void_p), ("ho_l_rl", C.c_void_p)]


def make_view(sr, sid0=0):
    """sr: flat image of the reads (hoco_l, hoco_s, ho_rl, ho_l_rl, n_scm, k_mer, m_pos) -> (ReadsView, keep-alive dict)"""
    hl = sr["hoco_l"].astype(np.uint64)
    n = len(hl)
    k = {}
    k["scm_off"] = np.concatenate([[0], np.cumsum(sr["n_scm"].astype(np.uint64))]).astype(np.uint64)
    k["hs_off"] = np.concatenate([[0], np.cumsum((hl + 3) // 4)])[:n].astype(np.uint64)
    k["rl_off"] = np.concatenate([[0], np.cumsum(hl)]).astype(np.uint64)
    is255 = (sr["ho_rl"] == 255).astype(np.uint64)
    c255 = np.concatenate([[0], np.cumsum(is255)]).astype(np.uint64)
    k["lrl_off"] = c255[k["rl_off"][:n].astype(np.int64)].astype(np.uint64)
    k["rl_off"] = k["rl_off"][:n].copy()
    for f in ("k_mer", "m_pos", "hoco_s", "ho_rl"):
        k[f] = np.ascontiguousarray(sr[f])
    k["ho_l_rl"] = np.ascontiguousarray(sr["ho_l_rl"] if len(sr["ho_l_rl"]) else np.zeros(1, np.uint32))
    v = ReadsView(sid0, *[k[f].ctypes.data for f in ("scm_off", "k_mer", "m_pos", "hs_off", "hoco_s", "rl_off", "ho_rl", "lrl_off", "ho_l_rl")])
    return v, k


def oracle_rl(view, occ, K):
    L = O.lib()
    L.orc_consensus_rl.argtypes = [C.POINTER(ReadsView), C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    tot = np.zeros(K, np.uint64)
    m, first = C.c_uint32(), C.c_uint64()
    occ = np.ascontiguousarray(occ, np.uint64)
    L.orc_consensus_rl(C.byref(view), len(occ), occ.ctypes.data, K, tot.ctypes.data, C.byref(m), C.byref(first))
    return tot, m.value, first.value


def oracle_string(view, tot, m_seq, first, K, rev, beg, hoco):
    L = O.lib()
    L.orc_consensus_string.restype = C.c_int64
    L.orc_consensus_string.argtypes = [C.POINTER(ReadsView), C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_char_p]
    cap = (abs(beg) + K + 8) + int(tot.sum() // max(m_seq, 1)) + 2 * K + 64
    buf = C.create_string_buffer(cap)
    n = L.orc_consensus_string(C.byref(view), tot.ctypes.data, m_seq, first, K, rev, beg, hoco, buf)
    return n, buf.raw[:n]


def reference_string(db, scm, sid, rev, beg, hoco, cap=1 << 20):
    import ref_lib as R
    L = R.lib()
    L.refx_syncmer_consensus.restype = C.c_int64
    L.refx_syncmer_consensus.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int64, C.c_int, C.c_char_p, C.c_int64]
    buf = C.create_string_buffer(cap)
    n = L.refx_syncmer_consensus(db.handle, scm.handle, sid, rev, beg, hoco, buf, cap)
    return n, buf.raw[:n]


def long_run_reads(seed, K):
    """HiFi-like reads over a genome that holds homopolymers of 300 and 700 bases (run lengths beyond the 255 escape of ho_rl)
    and plenty of short ones; reads disagree on run lengths, so the consensus has something to average"""
    import adversarial as A
    rng = np.random.default_rng(seed)
    g = bytearray(A.rand_dna(rng, 40 * K))
    for at, ln, ch in ((9 * K, 300, b"A"), (21 * K + 11, 700, b"C"), (30 * K, 260, b"T")):
        g[at:at + ln] = ch * ln
    g = bytes(g)
    reads = []
    for _ in range(200):
        st = int(rng.integers(0, len(g) - 12 * K))
        ln = int(rng.integers(8 * K, 12 * K))
        r = bytearray(g[st:st + ln])
        # homopolymer length errors, the dominant HiFi error: lengthen or shorten some runs
        for p in sorted(rng.integers(1, len(r) - 1, size=30).tolist(), reverse=True):
            if rng.integers(0, 2):
                r.insert(p, r[p])
            elif r[p] == r[p - 1]:
                del r[p]
        r = bytes(r)
        reads.append(A.revcomp(r) if rng.integers(0, 2) else r)
    return reads


def late_run_reads(seed, K, n_reads=150):
    """reads for k above 1024: HiFi-like reads of 8-10 k bases (hoco length several k) over a genome of about 30 k bases where a homopolymer
    of 260-700 bases follows every k/3 random bases -- so syncmers have runs beyond the 255 escape past their position 1024, and reads of
    both strands cover each; run-length errors give the consensus something to average"""
    import adversarial as A
    rng = np.random.default_rng(seed)
    g = bytearray()
    j = 0
    while len(g) < 30 * K:
        ln = (260, 300, 450, 700)[j % 4]
        g += A.rand_dna(rng, K // 3) + b"ACGT"[j % 4:j % 4 + 1] * ln
        j += 1
    g = bytes(g)
    reads = []
    for i in range(n_reads):
        ln = int(rng.integers(8 * K, 10 * K))
        st = int(rng.integers(0, len(g) - ln))
        r = bytearray(g[st:st + ln])
        for p in sorted(rng.integers(1, len(r) - 1, size=30).tolist(), reverse=True):
            if rng.integers(0, 2):
                r.insert(p, r[p])
            elif r[p] == r[p - 1]:
                del r[p]
        r = bytes(r)
        reads.append(A.revcomp(r) if i & 1 else r)
    return reads


def _jitter_runs(rng, r, n):
    """run-length errors only, as in long_run_reads: lengthen a run, or shorten one that has at least 2 bases -- the hoco string stays what it was"""
    for p in sorted(rng.integers(1, len(r) - 1, size=n).tolist(), reverse=True):
        if rng.integers(0, 2):
            r.insert(p, r[p])
        elif r[p] == r[p - 1]:
            del r[p]
    return r


def _hoco_len(b):
    return 1 + sum(b[i] != b[i - 1] for i in range(1, len(b)))


def tandem_reads(seed, K, n_reads, m, extra=(), S=None):
    """reads that are tandem arrays: one random unit of 3 k bases, a homopolymer of 300 bases (beyond the 255 escape of ho_rl) put in at offset k/2,
    repeated m times per read; run-length errors only, every odd-numbered read reverse-complemented; each entry e of `extra` appends one forward
    read of e units.  A syncmer whose window fits inside the unit occurs exactly n_reads * m + sum(extra) times, the ones across the unit's end once
    less per read: occurrence lists of a chosen length (consensus.hpp: CONS_CHUNK).  With S given, units are drawn until the long run lies in a
    syncmer of the first kind, so that the longest lists are the ones that hold it -- and, at k above 1024, until it also lies past position 1024
    of some syncmer, where a later pass of cons_rl_kernel looks it up."""
    import adversarial as A
    rng = np.random.default_rng(seed)
    while True:
        u = A.rand_dna(rng, 3 * K)
        run = b"ACGT"[(b"ACGT".index(u[K // 2:K // 2 + 1]) + 1) & 3:][:1]
        if run == u[K // 2 - 1:K // 2]:
            run = b"ACGT"[(b"ACGT".index(run) + 2) & 3:][:1]                 # neither neighbour's base: the run stays 300 long
        unit = u[:K // 2] + run * 300 + u[K // 2:]
        if S is None:
            break
        q, P = _hoco_len(unit[:K // 2]), _hoco_len(unit)                       # the run's hoco position, the unit's hoco length
        mp = O.scan([unit * 3], K, S)["m_pos"]
        mp = mp[(mp >> 1) < P].tolist()
        # position of the run in the stored (forward) orientation of each syncmer of the first period that holds it
        t = [(q - (x >> 1)) % P if x & 1 == 0 else K - 1 - (q - (x >> 1)) % P for x in mp if (q - (x >> 1)) % P < K]
        if unit[0] != unit[-1] and any(x >> 1 <= q and q < (x >> 1) + K <= P for x in mp) and (K <= 1024 or max(t) >= 1024):
            break
    reads = []
    for i in range(n_reads):
        r = bytes(_jitter_runs(rng, bytearray(unit * m), len(unit) * m // 100))
        reads.append(A.revcomp(r) if i & 1 else r)
    return reads + [unit * e for e in extra]


# tandem_reads(5, 101, ...) at s = 11: (n_reads, m, extra) and the occurrence-list lengths that come of it, on both sides of 1024 and of 2048;
# at k = 1101, s = 31 both loops of cons_rl_kernel (positions, occurrences) run more than once
TANDEM_SEED = 5
TANDEM_CASES = [((32, 32, ()), {992, 1024}), ((32, 32, (1,)), {992, 1025}), ((64, 32, ()), {1984, 2048}), ((64, 32, (1,)), {1984, 2049}),
                ((40, 60, (1,)), {2360, 2401})]
TANDEM_BIG_K = (1101, 31, (32, 33, (2,)), {1025, 1058})


SHARD_FRAC = (0.0, 0.9, 1.0)      # the (40, 60, (1,)) reads over two handles: 37 reads, and 3 with the extra one


def shard_bounds(n, frac=SHARD_FRAC):
    return [int(round(f * n)) for f in frac]


def shard_lengths(reads, K, S, frac=SHARD_FRAC):
    """the longest occurrence list of the first shard's reads and of the last shard's, each shard scanned and counted on its own"""
    b = shard_bounds(len(reads), frac)
    first = np.diff(O.scan_and_count(reads[b[0]:b[1]], K, S)[1]["occ_off"].astype(np.int64))
    last = np.diff(O.scan_and_count(reads[b[-2]:b[-1]], K, S)[1]["occ_off"].astype(np.int64))
    return int(first.max()), int(last.max())


def deep_locus_reads(seed, K, n_bad, n_good, lo, hi):
    """n_bad + n_good reads of one whole genome of 8 k bases (a run of 300 bases put in at offset k), with run-length errors, every third one
    reverse-complemented; each of the first n_bad carries 3 substitutions at distinct positions of [lo, hi).  With [lo, hi) inside one syncmer's
    k-mer the correction rewrites that stretch of nearly every bad read: long occurrence lists whose head is corrected entries"""
    import adversarial as A
    rng = np.random.default_rng(seed)
    g = A.rand_dna(rng, 8 * K)
    run = b"ACGT"[(b"ACGT".index(g[K:K + 1]) + 1) & 3:][:1]
    if run == g[K - 1:K]:
        run = b"ACGT"[(b"ACGT".index(run) + 2) & 3:][:1]
    g = g[:K] + run * 300 + g[K:]
    reads = []
    for i in range(n_bad + n_good):
        r = bytearray(g)
        if i < n_bad:
            for p in rng.choice(np.arange(lo, hi), 3, replace=False).tolist():
                r[p] = b"ACGT"[(b"ACGT".index(bytes(r[p:p + 1])) + 1 + int(rng.integers(0, 3))) & 3]
        r = bytes(_jitter_runs(rng, r, len(r) // 100))
        reads.append(A.revcomp(r) if i % 3 == 2 else r)
    return reads


def list_flags(sr, occ):
    """the `corrected` bits (k_mer & 1) of the chain entries an occurrence list names; sr: n_scm and k_mer of the chains"""
    scm_off = np.concatenate([[0], np.cumsum(sr["n_scm"].astype(np.int64))])
    rd = (occ >> np.uint64(32)).astype(np.int64)
    idx = ((occ >> np.uint64(1)) & np.uint64(0x7FFFFFFF)).astype(np.int64)
    return (sr["k_mer"][scm_off[rd] + idx] & np.uint64(1)).astype(bool)


def list_strands(sr, occ):
    """the strand bits (m_pos & 1) of the chain entries an occurrence list names, as a set"""
    scm_off = np.concatenate([[0], np.cumsum(sr["n_scm"].astype(np.int64))])
    rd = (occ >> np.uint64(32)).astype(np.int64)
    idx = ((occ >> np.uint64(1)) & np.uint64(0x7FFFFFFF)).astype(np.int64)
    return set((sr["m_pos"][scm_off[rd] + idx] & 1).tolist())


def chunk_shapes(sr, cov, dele, occ_off, occ, c, chunk=1024):
    """what the corrected lists longer than one chunk look like, among live syncmers of coverage >= c: ids whose whole first chunk is corrected
    entries while a later chunk holds a live one (`head`), and ids with corrected and live entries inside one chunk (`mixed`)"""
    head, mixed = [], []
    for i in np.nonzero((dele == 0) & (cov >= c) & (np.diff(occ_off.astype(np.int64)) > chunk))[0].tolist():
        f = list_flags(sr, occ[int(occ_off[i]):int(occ_off[i + 1])])
        if f[:chunk].all() and not f[chunk:].all():
            head.append(i)
        if any(f[a:a + chunk].any() and not f[a:a + chunk].all() for a in range(0, len(f), chunk)):
            mixed.append(i)
    return head, mixed


DEEP = dict(K=101, S=11, c=30, n_bad=1030, n_good=200)


def deep_locus_case(seed=5, spare=40):
    """the reads of deep_locus_reads in two passes: the oracle's round (no device) runs once on n_bad + spare bad reads, the bad reads it leaves
    uncorrected are dropped, and of the rest the first n_bad stay -- so that the first 1024 entries of some live list are all corrected.  Whether they
    are is for the caller to assert (chunk_shapes): dropping reads changes the coverage the second round sees.  Returns (reads, K, S, c)."""
    import ec_util as E
    K, S, c, n_bad, n_good = (DEEP[k] for k in ("K", "S", "c", "n_bad", "n_good"))
    reads = deep_locus_reads(seed, K, n_bad + spare, n_good, 4 * K + 300, 4 * K + 340)
    got, cnt = O.scan_and_count(reads, K, S)
    res = E.oracle_round_on(got, cnt, K, c, 0.02, 0.35)
    scm_off = np.concatenate([[0], np.cumsum(res["n_scm"].astype(np.int64))])
    fixed = np.add.reduceat(np.append(res["k_mer"] & np.uint64(1), np.uint64(0)), scm_off[:-1])[:n_bad + spare] > 0
    bad = [reads[i] for i in np.nonzero(fixed)[0][:n_bad].tolist()]
    assert len(bad) == n_bad, "the spare bad reads do not make up for the uncorrected ones"
    return bad + reads[n_bad + spare:], K, S, c
