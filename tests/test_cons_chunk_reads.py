"""The read sets of tests/test_gpu_consensus_chunks.py have the shapes those tests are about, checked on the oracle alone (no device): occurrence
lists of exactly the lengths on both sides of a chunk of cons_rl_kernel (consensus.hpp: CONS_CHUNK = 1024), with long runs and both strands in a
list of more than one chunk; and, after the oracle's correction round, a live list whose whole first chunk is corrected entries."""
import numpy as np
import pytest

import cons_util as CU
import ec_util as E
import oracle_lib as O

CHUNK = 1024


def scanned(reads, K, S):
    got, cnt = O.scan_and_count(reads, K, S)
    sr = dict(got)
    sr["k_mer"] = cnt["k_id"]
    return sr, cnt


def long_rows(sr, cnt, K):
    """per syncmer with a list over one chunk: (list length, long run taking part, strands in the list, long run past position 1024)"""
    view, keep = CU.make_view(sr)
    out = []
    for i in np.nonzero(np.diff(cnt["occ_off"].astype(np.int64)) > CHUNK)[0].tolist():
        occ = cnt["occ"][int(cnt["occ_off"][i]):int(cnt["occ_off"][i + 1])]
        tot, m, _ = CU.oracle_rl(view, occ, K)
        out.append((len(occ), m > 0 and int(tot.max()) // m >= 255, CU.list_strands(sr, occ), m > 0 and int(tot[CHUNK:].max(initial=0)) // m >= 255))
    return out


@pytest.mark.parametrize("shape,lengths", CU.TANDEM_CASES)
def test_tandem_reads_give_the_list_lengths(shape, lengths):
    K, S = 101, 11
    reads = CU.tandem_reads(CU.TANDEM_SEED, K, *shape, S=S)
    assert sum(len(r) for r in reads) <= 1_500_000
    sr, cnt = scanned(reads, K, S)
    assert set(np.diff(cnt["occ_off"].astype(np.int64)).tolist()) == lengths
    rows = long_rows(sr, cnt, K)
    if max(lengths) > CHUNK:
        assert any(n == max(lengths) and esc and strands == {0, 1} for n, esc, strands, _ in rows)
    else:
        assert not rows                                            # exactly one chunk: nothing may take the shared-row path


def test_tandem_reads_at_k_above_1024():
    K, S, shape, lengths = CU.TANDEM_BIG_K
    reads = CU.tandem_reads(CU.TANDEM_SEED, K, *shape, S=S)
    assert sum(len(r) for r in reads) <= 4_000_000
    sr, cnt = scanned(reads, K, S)
    assert set(np.diff(cnt["occ_off"].astype(np.int64)).tolist()) == lengths and min(lengths) > CHUNK
    rows = long_rows(sr, cnt, K)
    assert any(n == max(lengths) and esc and strands == {0, 1} for n, esc, strands, _ in rows)
    assert any(late and strands == {0, 1} for _, _, strands, late in rows)      # looked up in the second pass over the positions


def test_tandem_reads_run_lengths_differ_between_occurrences():
    """the consensus has something to round: totals that are no multiple of the count, some of them with a fraction of a half or more"""
    K, S = 101, 11
    sr, cnt = scanned(CU.tandem_reads(CU.TANDEM_SEED, K, 32, 32, (1,), S=S), K, S)
    view, keep = CU.make_view(sr)
    up = 0
    for i in np.nonzero(np.diff(cnt["occ_off"].astype(np.int64)) > CHUNK)[0].tolist():
        tot, m, _ = CU.oracle_rl(view, cnt["occ"][int(cnt["occ_off"][i]):int(cnt["occ_off"][i + 1])], K)
        up += int(((tot % np.uint64(m)) * np.uint64(2) >= np.uint64(m)).sum())
    assert up > 0


def test_two_tandem_arrays_interleave_short_and_long_lists():
    """what the repeated calls of test_rows_are_cleared_between_calls need: the lists of 1025 are not the first ids, so selecting them alone moves rows"""
    K, S = 101, 11
    reads = CU.tandem_reads(CU.TANDEM_SEED, K, 32, 32, (1,), S=S) + CU.tandem_reads(CU.TANDEM_SEED + 1, K, 32, 32, (1,), S=S)
    ln = np.diff(O.scan_and_count(reads, K, S)[1]["occ_off"].astype(np.int64))
    assert set(ln.tolist()) == {992, 1025}
    long_ids = np.nonzero(ln >= 1000)[0]
    assert not np.array_equal(long_ids, np.arange(len(long_ids)))


@pytest.mark.parametrize("which", ["tandem", "deep_locus"])
def test_sharded_split_has_rows_chunked_on_one_rank_only(which):
    K, S = 101, 11
    reads = CU.tandem_reads(CU.TANDEM_SEED, K, 40, 60, (1,), S=S) if which == "tandem" else CU.deep_locus_case()[0]
    lo, hi = CU.shard_lengths(reads, K, S, CU.SHARD_FRAC)
    assert lo > CHUNK and 0 < hi <= CHUNK
    assert int(np.diff(O.scan_and_count(reads, K, S)[1]["occ_off"].astype(np.int64)).max()) > CHUNK


def test_deep_locus_reads_have_a_corrected_first_chunk():
    reads, K, S, c = CU.deep_locus_case()
    assert len(reads) == CU.DEEP["n_bad"] + CU.DEEP["n_good"] and sum(len(r) for r in reads) <= 1_500_000
    got, cnt = O.scan_and_count(reads, K, S)
    res = E.oracle_round_on(got, cnt, K, c, 0.02, 0.35)
    head, mixed = CU.chunk_shapes(res, res["cov"], res["del"], res["occ_off"], res["occ"], c, CHUNK)
    # a live list over 1024 whose first 1024 entries are all corrected, its first uncorrected entry in the second chunk ...
    assert head
    f = CU.list_flags(res, res["occ"][int(res["occ_off"][head[0]]):int(res["occ_off"][head[0] + 1])])
    assert len(f) > CHUNK and f[:CHUNK].all() and CHUNK <= int(np.argmin(f)) < 2 * CHUNK
    # ... and another with corrected and live entries inside one chunk
    assert set(mixed) - {head[0]}
    # its live entries, all behind the first chunk, are of both strands
    assert CU.list_strands(res, res["occ"][int(res["occ_off"][head[0]]):int(res["occ_off"][head[0] + 1])][~f]) == {0, 1}


def test_oracle_round_on_is_what_oracle_round_runs():
    """the part of ec_util.oracle_round that needs no handle: the wrapper hands it the handle's scan and count and nothing else"""
    class Handle:
        def __init__(self, got, cnt):
            self.got, self.cnt = got, cnt

        def fetch_scan(self, off, with_hash=True):
            assert not with_hash
            return self.got

        def fetch_count(self):
            return self.cnt

    K, S, c = 101, 11, 30
    reads = CU.deep_locus_reads(3, K, 60, 60, 4 * K + 300, 4 * K + 340)
    got, cnt = O.scan_and_count(reads, K, S)
    a, b = E.oracle_round_on(got, cnt, K, c, 0.02, 0.35, blocks=True), E.oracle_round(Handle(got, cnt), None, K, c, 0.02, 0.35, blocks=True)
    assert int(a["stats"][7]) > 0 and a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
