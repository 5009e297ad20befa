"""GPU: occurrence lists longer than one chunk of cons_rl_kernel (consensus.hpp: CONS_CHUNK = 1024).  Such a syncmer gets several workgroups that add
into one row with global atomics -- cleared before (cons_zero_shared_kernel), rounded and its first live occurrence resolved after
(cons_finish_shared_kernel) -- where a shorter list is summed, rounded and written by one workgroup.  Checked here, exactly, against the oracle
(oracle/consensus.c): lists of 1024, 1025, 2048, 2049 and 2401 entries as scanned; a live list whose whole first chunk is corrected entries; k above
1024, where the kernel's loop over positions runs more than once as well; a second and third call on one handle, which reuse the rows; a
caller-chosen list of ids (oatk_hip_consensus_ids); and reads sharded so that a row takes one path on one rank and the other on the next
(oatk_hip_consensus_sharded).  tests/test_cons_chunk_reads.py holds the read sets to these shapes without a device; every test here asserts its own
shape again on what the device holds, so none can pass on lists of 1024 or fewer."""
import threading

import numpy as np
import pytest
import torch

import cons_util as CU
from oatk_amd import HipSyncasm, _lib, pack_reads
from test_gpu_consensus import check_consensus, compare_with_oracle, device_consensus, load_reads

pytestmark = pytest.mark.gpu

CHUNK = 1024
K0, S0 = 101, 11
ROW = ("TOT", "RL", "MSEQ", "FIRST")


def lists_of(D, occ_off, occ):
    """the occurrence list of every selected syncmer"""
    return [occ[int(occ_off[i]):int(occ_off[i + 1])] for i in D["SEL"].tolist()]


def assert_long_rows(D, K, sr, lists):
    """some selected syncmer with a list over one chunk has a run length behind the 255 escape and occurrences of both strands"""
    tot = D["TOT"].reshape(len(D["SEL"]), K)
    ok = [len(o) > CHUNK and int(D["MSEQ"][s]) > 0 and int(tot[s].max()) // int(D["MSEQ"][s]) >= 255 and CU.list_strands(sr, o) == {0, 1}
          for s, o in enumerate(lists)]
    assert any(ok)


@pytest.mark.parametrize("shape,lengths", CU.TANDEM_CASES)
def test_chunk_edges_as_scanned(hip, shape, lengths):
    """(32, 32, ()) stays on the one-workgroup path at exactly 1024; (32, 32, (1,)) has unshared rows (992) and shared rows (1025) in one launch"""
    reads = CU.tandem_reads(CU.TANDEM_SEED, K0, *shape, S=S0)
    sr, cov, occ, occ_off, dele = load_reads(hip, reads, K0, S0, False)
    D, view, keep, n_long = check_consensus(hip, K0, 1, sr, cov, occ, occ_off, dele)
    lists = lists_of(D, occ_off, occ)
    assert set(len(o) for o in lists) == lengths and len(lists) == len(cov)
    assert n_long > 0
    if max(lengths) > CHUNK:
        assert_long_rows(D, K0, sr, lists)
    tot = D["TOT"].reshape(len(lists), K0)
    assert any(((tot[s] % np.uint64(len(o))) * np.uint64(2) >= np.uint64(len(o))).any() for s, o in enumerate(lists) if len(o) >= CHUNK)      # a mean that rounds up


def test_corrected_first_chunk(hip):
    """after the correction: a live list of 1230 entries whose first 1024 are corrected (its first chunk adds nothing, neither to the count nor to the
    first occurrence, which lies in the second chunk), and lists where corrected and live entries share a chunk"""
    reads, K, S, c = CU.deep_locus_case()
    sr, cov, occ, occ_off, dele = load_reads(hip, reads, K, S, True, c_ec=c)
    D, view, keep, _ = check_consensus(hip, K, c, sr, cov, occ, occ_off, dele)
    head, mixed = CU.chunk_shapes(sr, cov, dele, occ_off, occ, c, CHUNK)
    assert head and set(mixed) - {head[0]}
    for i in head:
        o = occ[int(occ_off[i]):int(occ_off[i + 1])]
        f = CU.list_flags(sr, o)
        at = int(np.argmin(f))
        assert len(o) > CHUNK and f[:CHUNK].all() and CHUNK <= at < 2 * CHUNK
        s = int(D["SLOT"][i])
        assert int(D["MSEQ"][s]) == int((~f).sum()) > 0 and int(D["FIRST"][s]) == int(o[at])
    for i in mixed:
        assert int(D["MSEQ"][int(D["SLOT"][i])]) == int((~CU.list_flags(sr, occ[int(occ_off[i]):int(occ_off[i + 1])])).sum())


def test_k_above_1024_and_chunked(hip):
    """lists of 1025 and 1058 entries at k = 1101: the loop over positions and the chunks of the list both go round more than once"""
    K, S, shape, lengths = CU.TANDEM_BIG_K
    reads = CU.tandem_reads(CU.TANDEM_SEED, K, *shape, S=S)
    sr, cov, occ, occ_off, dele = load_reads(hip, reads, K, S, False)
    D, view, keep, n_long = check_consensus(hip, K, 1, sr, cov, occ, occ_off, dele)
    lists = lists_of(D, occ_off, occ)
    assert set(len(o) for o in lists) == lengths and min(lengths) > CHUNK
    assert_long_rows(D, K, sr, lists)
    rl = D["RL"].reshape(len(lists), K)
    assert (rl[:, CHUNK:] > 0).any() and (rl[:, CHUNK:] >= 255).any()             # rounded means and a long run past position 1024


def test_rows_are_cleared_between_calls(hip):
    """consensus(1), consensus(1000), consensus(1) on one handle: the second call selects the shared rows only, so they move to the front of the
    buffers the first call filled; totals, counts or first occurrences left over in a shared row would be added to.  Two tandem arrays, so that
    the ids of the shared rows (the table is in hash order) are no prefix of all ids"""
    shape, lengths = (32, 32, (1,)), {992, 1025}
    reads = CU.tandem_reads(CU.TANDEM_SEED, K0, *shape, S=S0) + CU.tandem_reads(CU.TANDEM_SEED + 1, K0, *shape, S=S0)
    tables = load_reads(hip, reads, K0, S0, False)
    sr, cov, occ, occ_off, dele = tables
    assert set(np.diff(occ_off.astype(np.int64)).tolist()) == lengths
    first = device_consensus(hip, 1)
    D, view, keep, n_long = check_consensus(hip, K0, 1000, *tables)
    assert 0 < len(D["SEL"]) < len(first["SEL"]) and not np.array_equal(D["SEL"], first["SEL"][:len(D["SEL"])])      # rows shifted
    assert all(len(o) == 1025 for o in lists_of(D, occ_off, occ))
    third = device_consensus(hip, 1)
    for k in first:
        assert np.array_equal(first[k], third[k]), k
    check_consensus(hip, K0, 1, *tables)


@pytest.mark.parametrize("shape", [(40, 60, (1,)), (32, 32, (1,))])
def test_consensus_ids(hip, shape):
    """oatk_hip_consensus_ids on a permuted subset of the ids, given as a device tensor: its rows equal those of oatk_hip_consensus and the oracle's.
    (40, 60, (1,)): every list has three chunks; (32, 32, (1,)): lists of one chunk and of two in one call"""
    reads = CU.tandem_reads(CU.TANDEM_SEED, K0, *shape, S=S0)
    sr, cov, occ, occ_off, dele = load_reads(hip, reads, K0, S0, False)
    D, view, keep, _ = check_consensus(hip, K0, 1, sr, cov, occ, occ_off, dele)
    n = len(cov)
    ids = np.random.default_rng(11).permutation(n)[:n - 1].astype(np.int32)
    assert len(ids) >= 4 and not np.array_equal(ids, np.sort(ids))
    n_occ = np.diff(occ_off.astype(np.int64))[ids]
    assert (n_occ > CHUNK).any()
    if shape == (32, 32, (1,)):
        assert (n_occ <= CHUNK).any()
    d_ids = torch.from_numpy(ids).to("cuda:%d" % hip.device)
    torch.cuda.synchronize()
    hip.consensus_ids(d_ids.data_ptr(), len(ids))
    G = {k: hip.fetch("CONS_" + k) for k in ROW}
    assert np.array_equal(hip.fetch("CONS_SEL"), ids.astype(np.uint32))
    slot = D["SLOT"][ids].astype(np.int64)
    for k in ("TOT", "RL"):
        assert np.array_equal(G[k].reshape(len(ids), K0), D[k].reshape(n, K0)[slot]), k
    for k in ("MSEQ", "FIRST"):
        assert np.array_equal(G[k], D[k][slot]), k
    for j, i in enumerate(ids.tolist()):
        tot, m, first = CU.oracle_rl(view, occ[int(occ_off[i]):int(occ_off[i + 1])], K0)
        assert m == int(G["MSEQ"][j]) > 0 and first == int(G["FIRST"][j]), i
        assert np.array_equal(G["TOT"].reshape(len(ids), K0)[j], tot), i
        assert np.array_equal(G["RL"].reshape(len(ids), K0)[j], np.floor(tot.astype(np.float64) / m + 0.5).astype(np.uint32)), i


CONS = ["CONS_SEL", "CONS_SLOT", "CONS_RL", "CONS_MSEQ", "CONS_FIRST"]


def sharded_consensus(reads, bounds, K, S, c, a):
    """scan, count, merge, correction and consensus of reads[bounds[r]:bounds[r + 1]] on rank r; the ranks are threads of this process, each with its
    own handle on device 0, over the in-process communicator group.  Returns the CONS_* arrays of every rank."""
    L = _lib.load()
    world = len(bounds) - 1
    grp = L.oatk_comm_group_create(world)
    assert grp
    out, errs = [None] * world, []

    def work(rank):
        try:
            h = HipSyncasm(0)
            comm = L.oatk_comm_group_rank(grp, rank)
            seq, off, lens = pack_reads(reads[bounds[rank]:bounds[rank + 1]])
            h.scan_host(seq, off, lens, K, S, sid0=bounds[rank])
            h.count()
            h.merge_counts(comm)
            h.ec_sharded(comm, 0.02, c, a)
            h.consensus_sharded(comm, c)
            out[rank] = {k: h.fetch(k) for k in CONS}
            L.oatk_comm_destroy(comm)
            h.close()
        except Exception as ex:                          # noqa: BLE001
            errs.append((rank, ex))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    alive = any(t.is_alive() for t in th)
    if not alive:
        L.oatk_comm_group_destroy(grp)
    assert not alive, "a rank hangs in a collective"
    assert not errs, errs
    return out


@pytest.mark.parametrize("which", ["tandem", "deep_locus"])
def test_sharded_rows_chunked_on_one_rank_only(hip, which):
    """two handles with 90 % and 10 % of the reads: a row is added up by several workgroups on rank 0, by one on rank 1, and by several where one
    handle holds all reads; after oatk_hip_consensus_sharded every rank has what that one handle has.  deep_locus: rank 0's first chunk of a row is
    all corrected entries, and the correction itself crosses the ranks"""
    a = 0.35
    if which == "tandem":
        K, S, c = K0, S0, 30
        reads = CU.tandem_reads(CU.TANDEM_SEED, K, 40, 60, (1,), S=S)
    else:
        reads, K, S, c = CU.deep_locus_case()
    bounds = CU.shard_bounds(len(reads))
    lo, hi = CU.shard_lengths(reads, K, S)
    assert lo > CHUNK and 0 < hi <= CHUNK
    out = sharded_consensus(reads, bounds, K, S, c, a)
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    hip.count()
    hip.ec_graph(light_c=c)
    hip.ec(0.02, c, a)
    hip.consensus(c)
    ref = {k: hip.fetch(k) for k in CONS}
    n_occ = np.diff(hip.fetch("EC_SCM_OCC_OFF").astype(np.int64))[ref["CONS_SEL"]]
    assert len(n_occ) > 0 and (n_occ > CHUNK).any()
    if which == "deep_locus":
        assert (ref["CONS_MSEQ"][n_occ > CHUNK] < n_occ[n_occ > CHUNK]).any()      # corrected entries were left out of a chunked row
    for r in out:
        for k in CONS:
            assert np.array_equal(r[k], ref[k]), k
