"""GPU: the k-mer hash kernel's workgroups of 64 records (kmer_hash.hpp: four waves prepare sixteen records each, the first wave then runs all
64 chains and places the records).  What changes with the shape of a workgroup is tested here against the CPU oracle, bit for bit, with the
checks of test_gpu_record_path.py: shards that hold many full workgroups and a last one of every size (a wave with no record to prepare, a chain
wave with idle lanes), shards with fewer than sixteen records, reads shorter than k beside them, and k-mers whose Murmur input is a whole number of
8-byte blocks, has a tail block, or is one block only -- the LDS rows of the records are an odd number of words apart at each of them."""
import numpy as np
import pytest

import adversarial as A
import test_gpu_record_path as RP
from oatk_amd import pack_reads

pytestmark = pytest.mark.gpu


def short_reads(K, n, seed):
    rng = np.random.default_rng(seed)
    return [A.rand_dna(rng, int(rng.integers(1, max(K - 1, 2)))) for _ in range(n)]


# (K, S): 8-byte Murmur blocks of the k-mer's ceil(K / 4) bytes -- full blocks, tail bytes
#   (32, 7): 1, 0    (33, 7): 1, 1    (125, 11): 4, 0    (257, 15): 8, 1    (997, 31): 31, 2    (1001, 31): 31, 3    (1021, 31): 32, 0
@pytest.mark.parametrize("K,S", [(32, 7), (33, 7), (125, 11), (257, 15), (997, 31), (1001, 31), (1021, 31)])
def test_full_and_tail_workgroups(hip, K, S):
    """a read's records all land in one shard: long reads give shards of hundreds of records (full workgroups and a tail of whatever size), the
    short ones between them hold the reads' shards apart and give none"""
    long_len = 200 * K                  # some three hundred records a read at every k
    reads = []
    for i, r in enumerate(A.hifi_like(24, 4 * long_len, long_len, seed=K)):
        reads.append(r)
        reads.extend(short_reads(K, 1 + i % 3, seed=K + i))
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    n_scm = hip.fetch("N_SCM")
    assert int(n_scm.max()) > 128 and int((n_scm == 0).sum()) >= 24
    # tails of different sizes among the reads' shards, some under a wave's sixteen records and some over
    tails = set(int(x) % 64 for x in n_scm if x)
    assert len(tails) > 4 and min(tails) < 16 < max(tails)
    RP.check(hip, off, *RP.oracle(reads, K, S))


def test_shards_with_a_handful_of_records(hip):
    """more reads than shards, each a little over k long: every shard holds a few records of several reads, one tail workgroup each"""
    K, S = 301, 21
    reads = A.hifi_like(2500, 200000, 420, seed=3, err=0.0)
    seq, off, lens = pack_reads(reads)
    hip.scan_host(seq, off, lens, K, S)
    n_scm = hip.fetch("N_SCM")
    assert 0 < int(n_scm.sum()) < 16 * 1024
    RP.check(hip, off, *RP.oracle(reads, K, S))


def test_masked_hashes_over_full_workgroups(hip):
    K, S = 101, 11
    reads = A.hifi_like(40, 60000, 12000, seed=8)
    seq, off, lens = pack_reads(reads)
    hip.debug_hash_mask(0xFFF)
    try:
        hip.scan_host(seq, off, lens, K, S)
        assert int(hip.fetch("N_SCM").max()) > 128
        RP.check(hip, off, *RP.oracle(reads, K, S, 0xFFF))
    finally:
        hip.debug_hash_mask(RP.FULL)
    hip.scan_host(seq, off, lens, K, S)
    RP.check(hip, off, *RP.oracle(reads, K, S))
