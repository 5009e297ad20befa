"""GPU: the device path at k above 1024, up to oatk_hip_max_k().  Kernels that walk the k positions of a syncmer in passes of 1024
(consensus.hpp: CONS_Q * 64) run their later passes only here; the scan switches from its fast kernel to the general one at these k, and at
the largest k a k-mer spans about 126 words of the hash and of the count's sequence comparison.  Every comparison is exact, element for
element, against the oracle (pinned to the compiled reference at these k by tests/test_oracle_vs_ref.py and tests/test_oracle_consensus.py)
or against the compiled reference itself."""
import ctypes as C

import numpy as np
import pytest

import adversarial as A
import cons_util as CU
import oracle_lib as O
import ref_lib as R
from test_gpu_consensus import compare_with_oracle
from test_gpu_dropin import _KString, device_dbs, host_lib
from test_gpu_scan import compare_scan, run_hip

pytestmark = pytest.mark.gpu

MAX_K = None                      # oatk_hip_max_k(), read from the library inside the test
KS = [(1024, 31), (1025, 31), (1501, 31), (2048, 21), (2049, 21), (MAX_K, 31)]
PASS = 1024                       # positions per pass of cons_rl_kernel


def occ_lists(hip, after_ec):
    if after_ec:
        return hip.fetch("EC_SCM_OCC_OFF"), hip.fetch("EC_SCM_OCC")
    c = hip.fetch_count()
    return c["occ_off"], c["occ"]


def k_of(hip, K):
    return hip.L.oatk_hip_max_k() if K is MAX_K else K


def strands_of(keep, occ):
    """the strand bits (m_pos & 1) of a syncmer's occurrences; keep: the flat read view of cons_util.make_view"""
    rd = (occ >> np.uint64(32)).astype(np.int64)
    idx = ((occ >> np.uint64(1)) & np.uint64(0x7FFFFFFF)).astype(np.int64)
    return set((keep["m_pos"][keep["scm_off"][rd].astype(np.int64) + idx] & 1).tolist())


@pytest.mark.parametrize("K,S", KS)
def test_scan_and_count_match_oracle(hip, K, S):
    K = k_of(hip, K)
    reads = A.reads(K, S, seed=K, scale=0.5) + A.hifi_like(40, 120000, 20000, seed=K + 1)
    got, _ = run_hip(hip, reads, K, S)
    hip.count()
    c = hip.fetch_count()
    want_scan, want = O.scan_and_count(reads, K, S, mode=0)
    compare_scan(got, want_scan)
    assert int(got["n_scm"].sum()) > 100
    assert c["n_scm"] == want["n_scm"]
    for f in ["h", "s", "cov", "occ_off", "occ", "k_id"]:
        assert np.array_equal(c[f], want[f]), f
    assert int(want["cov"].max()) > 1                              # the sequence comparison of equal k-mers ran


@pytest.mark.parametrize("after_ec", [False, True])
@pytest.mark.parametrize("K,S", KS)
def test_consensus_matches_oracle(hip, K, S, after_ec):
    """every CONS_* array of every selected syncmer; homopolymers beyond the 255 escape fall past position 1024 of syncmers seen on both strands"""
    K = k_of(hip, K)
    reads = CU.late_run_reads(K, K)
    D, view, keep, n_long = compare_with_oracle(hip, reads, K, S, after_ec, 2)
    rl = D["RL"].reshape(len(D["SEL"]), K)
    if K > PASS:
        assert int((rl[:, PASS:] > 0).sum()) > 0                   # a later pass wrote rounded means, not zeros
    if K >= 1501:
        late = np.nonzero((rl[:, PASS:] >= 255).any(axis=1))[0]    # long runs looked up in a later pass
        assert len(late) > 0
        occ_off, occ = occ_lists(hip, after_ec)
        seen = set()
        for s_i in late.tolist():
            i = int(D["SEL"][s_i])
            seen |= strands_of(keep, occ[int(occ_off[i]):int(occ_off[i + 1])])
        assert seen == {0, 1}


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("with_ec", [False, True])
@pytest.mark.parametrize("K,S", [(1025, 31), (1501, 31), (2049, 21), (MAX_K, 31)])
def test_syncmer_consensus_strings_equal_the_reference(hip, K, S, with_ec):
    """oatk_scg_syncmer_consensus (device totals, host strings) against the compiled reference's scg_syncmer_consensus on the very same structs,
    both strands, hoco and base space, `beg` on both sides of 1024"""
    K = k_of(hip, K)
    cov = 2
    L, H = R.lib(), host_lib()
    H.oatk_read_error_correction.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_double, C.c_void_p]
    H.oatk_consensus_fetch.restype = C.c_void_p
    H.oatk_consensus_fetch.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    H.oatk_consensus_destroy.argtypes = [C.c_void_p]
    H.oatk_scg_syncmer_consensus.restype = C.c_int64
    H.oatk_scg_syncmer_consensus.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int64, C.POINTER(_KString), C.c_int]
    L.refx_syncmer_consensus.restype = C.c_int64
    L.refx_syncmer_consensus.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int64, C.c_int, C.c_char_p, C.c_int64]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    db, scm = device_dbs(hip, CU.late_run_reads(K + 7, K), K, S)
    if with_ec:
        st = np.zeros(12, np.uint64)
        assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, 4, 40, 4, 0.35, st.ctypes.data) == 0
        assert int(st[2] + st[7]) > 0
    rc = C.c_int(0)
    cs = H.oatk_consensus_fetch(hip.h, cov, K, C.byref(rc))
    assert rc.value == 0 and cs
    rscm = object.__new__(R.ScmDb)
    rscm._h = scm
    sc = rscm.flatten()
    ids = np.nonzero((sc["cov"] >= cov) & (sc["del"] == 0))[0]
    assert len(ids) >= 5
    buf = C.create_string_buffer(1 << 22)
    for i in ids.tolist():
        for rev in (0, 1):
            for beg in [b for b in (0, 9, PASS - 1, PASS, PASS + 1, K - 1, -4) if b < K]:      # (scg_syncmer_consensus asserts beg < k)
                for hoco in (0, 1):
                    ks = _KString(0, 0, None)
                    n = H.oatk_scg_syncmer_consensus(cs, db, i, rev, beg, C.byref(ks), hoco)
                    got = C.string_at(ks.s, ks.l) if ks.l else b""
                    libc.free(ks.s)
                    nr = L.refx_syncmer_consensus(db, scm, i, rev, beg, hoco, buf, len(buf))
                    assert n == nr and got == buf.raw[:nr], (i, rev, beg, hoco)
    H.oatk_consensus_destroy(cs)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)


def copies_reads(K, counts, seed):
    """one short read per entry of `counts`, repeated that many times on mixed strands, with run-length changes in some copies: every syncmer
    of read j occurs exactly counts[j] times.  The first copy of each, and a few more, carry substitutions in their middle, which the correction
    puts right: those occurrences of the middle syncmers are corrected entries at the head of the list"""
    rng = np.random.default_rng(seed)
    reads = []
    for n in counts:
        # hoco length about 3 k; runs of 3, 153 and 303 bases (beyond the 255 escape)
        base = b"".join(A.rand_dna(rng, K // 2) + b"ACGT"[u % 4:u % 4 + 1] * (3 + 150 * (u % 3)) for u in range(8))
        bad = set([0] + rng.choice(np.arange(1, n), 7, replace=False).tolist())
        for c in range(n):
            r = bytearray(base)
            if c % 5 == 1:                                         # run-length changes: lengthen or shorten some runs
                for p in sorted(rng.integers(1, len(r) - 1, size=8).tolist(), reverse=True):
                    if rng.integers(0, 2):
                        r.insert(p, r[p])
                    elif r[p] == r[p - 1]:
                        del r[p]
            if c in bad:
                p = len(r) // 2 + int(rng.integers(-50, 50))
                r[p] = b"ACGT"[(b"ACGT".index(bytes([r[p]])) + 1 + int(rng.integers(0, 3))) & 3]
            r = bytes(r)
            reads.append(A.revcomp(r) if (c * 7 + 3) % 11 < 5 else r)
    return reads


@pytest.mark.parametrize("after_ec", [False, True])
@pytest.mark.parametrize("K,S", [(101, 11), (1501, 31)])
def test_multi_chunk_consensus_matches_oracle(hip, K, S, after_ec):
    """syncmers of 1024, 1025, 2048, 2049 and 3000 occurrences: one workgroup, or several that add into a shared row (cons_finish_shared_kernel)"""
    counts = (1024, 1025, 2048, 2049, 3000)
    D, view, keep, _ = compare_with_oracle(hip, copies_reads(K, counts, K), K, S, after_ec, 2)
    occ_off, occ = occ_lists(hip, after_ec)
    n_occ = np.diff(occ_off.astype(np.int64))[D["SEL"]]
    for n in counts:
        assert (n_occ == n).any(), n                               # each chunk boundary is met exactly
    if after_ec:
        head = occ[occ_off[D["SEL"]].astype(np.int64)]
        cut = (n_occ > PASS) & (D["MSEQ"] < n_occ) & (D["FIRST"] != head)
        assert cut.any()                                           # corrected occurrences left out of a shared row, its head among them
