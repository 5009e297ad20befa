"""GPU: coverage, forward-strand counts and marks of the refreshed syncmer table in ONE pass over the sorted (key, occurrence) pairs (oatk_amd/csrc/ec.hpp:
ec_cov_runs_kernel; r20) against plain counting.  A wave finds the runs of equal keys in its tile of 64 entries; runs inside a tile are stored, the runs at a tile's two edges are added atomically.
So the cases are about tile edges: runs that begin or end exactly at one, a run longer than one tile and one longer than two, a single key, all keys distinct,
keys that no entry has, a last tile that is not full, more than one workgroup (256 entries) -- through oatk_hip_debug_cov_runs, which takes the pairs as they
are; then whole corrections against the compiled reference, where oracle/_ref is built."""
import numpy as np
import pytest

import test_gpu_ec_memo as M

pytestmark = pytest.mark.gpu

TILE = 64


def pairs(lengths, gaps=None, seed=1):
    """runs of the given lengths, run r on key r (+ the keys that `gaps` leaves without an entry); strands at random, a few runs all reverse"""
    rng = np.random.default_rng(seed)
    keys, k = [], 0
    for r, n in enumerate(lengths):
        k += 1 + (gaps[r] if gaps else 0)
        keys += [k] * n
    key = np.array(keys, np.uint32)
    occ = rng.integers(0, 1 << 40, len(key)).astype(np.uint64)
    for r in np.unique(key)[::5]:
        occ[key == r] |= np.uint64(1)                          # no forward occurrence: the syncmer is marked
    return key, occ, k + 3


CASES = {
    "runs that end at a tile's edge": [64, 64, 30, 34, 128, 1, 63],
    "runs that begin at a tile's edge": [10, 54, 70, 58, 64, 5],
    "a run longer than one tile": [20, 100, 7],
    "a run longer than two tiles": [33, 200, 64, 3],
    "a run longer than a workgroup": [5, 700, 1, 1, 60],
    "a single key": [1],
    "a single key over tiles": [333],
    "all keys distinct": [1] * 300,
    "a run in the last lane and one in the first": [63, 1, 1, 63, 2],
    "two entries": [1, 1],
    "many": list(np.random.default_rng(7).integers(1, 90, 400)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_pass_against_the_passes_it_replaced(hip, name):
    """(the passes it replaced are gone: plain counting is what it is held to)"""
    lengths = [int(x) for x in CASES[name]]
    key, occ, nv = pairs(lengths, gaps=[(3 * r) % 4 for r in range(len(lengths))], seed=len(lengths))
    starts = np.concatenate([[0], np.cumsum(lengths)])
    if "end at" in name:
        assert (starts[1:] % TILE == 0).sum() >= 3
    if "begin at" in name:
        assert (starts[:-1] % TILE == 0).sum() >= 3
    want_cov = np.bincount(key, minlength=nv).astype(np.uint32)
    want_fwd = np.bincount(key[(occ & np.uint64(1)) == 0], minlength=nv).astype(np.uint32)
    got = hip.cov_runs(key, occ, nv)
    assert np.array_equal(got[0], want_cov), (name, "cov")
    assert np.array_equal(got[1], want_fwd), (name, "fwd")
    assert np.array_equal(got[2], (want_fwd == 0).astype(np.uint8)), (name, "del")
    assert int((want_cov > 0).sum()) == len(lengths) and int(((want_fwd == 0) & (want_cov > 0)).sum()) >= 1


def test_no_entries(hip):
    cov, fwd, dl = hip.cov_runs(np.zeros(0, np.uint32), np.zeros(0, np.uint64), 5)
    assert not cov.any() and not fwd.any() and dl.all()


@pytest.mark.parametrize("name", ["assemble", "diploid-tiers", "k1001"])
def test_corrections_with_the_switch_on_and_off(hip, monkeypatch, name):
    """(the switch is gone with the passes it chose: the table of a whole correction is held to plain counting over the chains the correction left, and to the
    compiled reference where it is built)"""
    M.clean(hip, monkeypatch)
    K, S, c, reads, env = M.read_sets(hip)[name]()
    dbs = M.resident(hip, reads, K, S)
    on, st = M.correct(hip, monkeypatch, c, env)
    assert int(on["EC_SCM_COV"].sum()) > TILE * 4 and int(on["EC_SCM_DEL"].sum()) > 0
    cov, fwd = np.bincount((on["EC_KMER"] >> np.uint64(1)).astype(np.int64), minlength=len(on["EC_SCM_COV"])), (on["EC_MPOS"] & 1) == 0
    assert np.array_equal(on["EC_SCM_COV"], cov)
    assert np.array_equal(on["EC_SCM_DEL"], np.bincount((on["EC_KMER"] >> np.uint64(1)).astype(np.int64)[fwd], minlength=len(cov)) == 0)
    M.against_reference(hip, st, dbs, K, S, c)
