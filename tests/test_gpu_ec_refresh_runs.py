"""GPU: coverage, forward-strand counts and marks of the refreshed syncmer table in ONE pass over the sorted (key, occurrence) pairs (oatk_amd/csrc/ec.hpp:
ec_cov_runs_kernel; r20) against the passes it replaced (ec_fwd_flag_kernel, an inclusive scan, ec_cov_sorted_kernel: OATK_DEBUG_EC_REFRESH_RUNS=0) and against
plain counting.  A wave finds the runs of equal keys in its tile of 64 entries; runs inside a tile are stored, the runs at a tile's two edges are added atomically.
So the cases are about tile edges: runs that begin or end exactly at one, a run longer than one tile and one longer than two, a single key, all keys distinct,
keys that no entry has, a last tile that is not full, more than one workgroup (256 entries) -- through oatk_hip_debug_cov_runs, which takes the pairs as they
are; then whole corrections with the switch on and off."""
import numpy as np
import pytest

import test_gpu_ec_memo as M

pytestmark = pytest.mark.gpu

TILE = 64
SWITCH = "OATK_DEBUG_EC_REFRESH_RUNS"


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
    lengths = [int(x) for x in CASES[name]]
    key, occ, nv = pairs(lengths, gaps=[(3 * r) % 4 for r in range(len(lengths))], seed=len(lengths))
    starts = np.concatenate([[0], np.cumsum(lengths)])
    if "end at" in name:
        assert (starts[1:] % TILE == 0).sum() >= 3
    if "begin at" in name:
        assert (starts[:-1] % TILE == 0).sum() >= 3
    want_cov = np.bincount(key, minlength=nv).astype(np.uint32)
    want_fwd = np.bincount(key[(occ & np.uint64(1)) == 0], minlength=nv).astype(np.uint32)
    new, old = hip.cov_runs(key, occ, nv, runs=True), hip.cov_runs(key, occ, nv, runs=False)
    for got, what in ((new, "one pass"), (old, "three passes")):
        assert np.array_equal(got[0], want_cov), (name, what, "cov")
        assert np.array_equal(got[1], want_fwd), (name, what, "fwd")
        assert np.array_equal(got[2], (want_fwd == 0).astype(np.uint8)), (name, what, "del")
    assert int((want_cov > 0).sum()) == len(lengths) and int(((want_fwd == 0) & (want_cov > 0)).sum()) >= 1


def test_no_entries(hip):
    for runs in (True, False):
        cov, fwd, dl = hip.cov_runs(np.zeros(0, np.uint32), np.zeros(0, np.uint64), 5, runs=runs)
        assert not cov.any() and not fwd.any() and dl.all()


@pytest.mark.parametrize("name", ["assemble", "diploid-tiers", "k1001"])
def test_corrections_with_the_switch_on_and_off(hip, monkeypatch, name):
    M.clean(hip, monkeypatch)
    K, S, c, reads, env = M.read_sets(hip)[name]()
    dbs = M.resident(hip, reads, K, S)
    off, _ = M.correct(hip, monkeypatch, c, dict(env, **{SWITCH: "0"}))
    on, st = M.correct(hip, monkeypatch, c, dict(env, **{SWITCH: None}))
    assert int(off["EC_SCM_COV"].sum()) > TILE * 4 and int(off["EC_SCM_DEL"].sum()) > 0
    M.assert_same(on, off, name + ", the refreshed table in one pass against three")
    M.against_reference(hip, st, dbs, K, S, c)
