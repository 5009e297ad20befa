"""GPU: the wave solver with its alignment's lanes following the last diagonal alive (oatk_amd/csrc/ec_wave.hpp: ecw_step) and with larger batches
taken from its queues (ECW_BATCH; a wave's memo lives as long as a batch).  Neither may change a result: on the read sets of
tests/test_gpu_ec_memo.py, and on reads with one long error-dense stretch each -- blocks of 3 .. 6 kb, routed to the second tier --, the default is
compared with OATK_DEBUG_EC_REGROUP=0 and with OATK_DEBUG_EC_BATCH=16, 32 and 64: the eleven statistics, the corrected chains and the refreshed table
(test_gpu_ec_assemble.OUT) and every block's EcBlockOut -- status, np, flags, short_block, tried, n_path, wf_steps, wf_diag, tier; path_off and ticks
are left out as elsewhere.  The optimum paths themselves lie in a pool that no buffer id exposes: they are compared through what is made of them, the
corrected chains (every replaced block's entries are its path's vertices) and, with oatk_hip_ec_keep_seq, the corrected sequences.  Where
oracle/_ref is built the default is held against the compiled reference as test_gpu_ec_memo.py holds it.  The extension turns that
OATK_DEBUG_EC_STAGES reports show that the switch does switch."""
import re

import numpy as np
import pytest

import adversarial as A
import test_gpu_ec_memo as M

pytestmark = pytest.mark.gpu

REGROUP, BATCH = "OATK_DEBUG_EC_REGROUP", "OATK_DEBUG_EC_BATCH"
OLD = {REGROUP: "0", BATCH: "16"}                              # the solver as it was before either
VARIANTS = [("the default", {REGROUP: None, BATCH: None}), ("regroup alone", {REGROUP: None, BATCH: "16"}), ("batch 32", {REGROUP: None, BATCH: "32"}),
            ("batch 64", {REGROUP: None, BATCH: "64"}), ("batch 64, regroup off", {REGROUP: "0", BATCH: "64"})]
T0_DEFAULT = 3072                                              # longest block of the first tier (include/oatk_hip_ec.h: oatk_hip_debug_ec_tiers)
DENSE_K, DENSE_S, DENSE_C = 1001, 31, 4


def dense_reads():
    """a homopolymer-free genome (so that every edit below survives the compression) at ~20x in reads with two lone errors each -- blocks of one to two thousand bases,
    the first tier's --, and six reads that carry one stretch of 3.5 .. 4.5 kb with an error every 300 .. 399 bases: no k-mer of a stretch is clean, so it is ONE
    block, of 3 .. 6 kb, whose path of a dozen vertices fits the second tier"""
    rng = np.random.default_rng(2020)
    n = 40000
    g = A.rand_nohp(rng, n)
    gg = g + g
    reads = []

    def damaged(r, at, stretch):
        r = bytearray(r)
        p, edits = at, []
        while p < at + stretch:
            edits.append((p, len(edits) % 3))
            p += 300 + int(rng.integers(0, 100))
        for p, kind in reversed(edits):
            if kind == 0:
                r[p] = [x for x in b"ACGT" if x not in (r[p - 1], r[p], r[p + 1])][0]
            elif kind == 1:
                r.insert(p, [x for x in b"ACGT" if x not in (r[p - 1], r[p])][p & 1])
            else:
                del r[p]
        return bytes(r)
    for i in range(64):
        st = (i * n) // 64 + int(rng.integers(0, 100))
        r = damaged(damaged(gg[st:st + 12000 + 37 * (i % 5)], 2500 + 41 * i, 1), 8000 + 23 * i, 1)
        reads.append(A.revcomp(r) if i % 3 == 0 else r)
    for i, stretch in enumerate((3500, 3700, 3900, 4100, 4300, 4500)):
        st = 1000 + 5300 * i
        r = damaged(gg[st:st + 2500 + stretch + 2500], 2500, stretch)
        reads.append(A.revcomp(r) if i % 2 else r)
    return reads


def turns(err):
    """extension turns of every launch of the wave solver: [(tier, blocks, batch, turns)]"""
    return [tuple(int(x) for x in m) for m in
            re.findall(r"\[ec stages\] wave solver, tier (\d), (\d+) blocks: batch (\d+), \d+ levels reused, \d+ blocks started at their sink, (\d+) extension turns", err)]


def run_variants(hip, monkeypatch, c, env, name):
    old, _ = M.correct(hip, monkeypatch, c, dict(env, **OLD))
    assert len(old["EC_BLOCK_OUT"]) > 0 and int(old["EC_BLOCK_OUT"][:, 6].sum()) > 0          # blocks, and wavefront steps
    st = None
    for what, v in VARIANTS:
        got, s = M.correct(hip, monkeypatch, c, dict(env, **v))
        M.assert_same(got, old, "%s, %s against regroup off and batch 16" % (name, what))
        if st is None:
            st = s
    return old, st


@pytest.mark.parametrize("name", ["assemble", "diploid-tiers", "diploid-classes", "k1001", "repeats"])
def test_regroup_and_batches_change_nothing(hip, monkeypatch, name):
    M.clean(hip, monkeypatch)
    K, S, c, reads, env = M.read_sets(hip)[name]()
    dbs = M.resident(hip, reads, K, S)
    _, st = run_variants(hip, monkeypatch, c, env, name)
    M.against_reference(hip, st, dbs, K, S, c)


def test_blocks_of_the_second_tier(hip, monkeypatch, capfd):
    M.clean(hip, monkeypatch)
    dbs = M.resident(hip, dense_reads(), DENSE_K, DENSE_S)
    env = {"OATK_DEBUG_EC_HEAVY": "0"}
    old, st = run_variants(hip, monkeypatch, DENSE_C, env, "dense stretches")
    work = hip.fetch("EC_BLOCK_WORK").reshape(-1, 12)
    long_l = work[:, 6].astype(np.int64)
    second = (long_l > T0_DEFAULT) & (long_l <= 2 * T0_DEFAULT)
    assert int(second.sum()) >= 4, sorted(long_l.tolist())[-8:]                              # blocks of the second tier ...
    assert int((old["EC_BLOCK_OUT"][second, 0] == 1).sum()) >= 3                               # ... that it corrected (EC_SUCCESS)
    assert int(old["EC_BLOCK_OUT"][second, 6].min()) > 8                                       # ... over a wavefront step per error at least (nine or more in 3.5 kb)
    M.against_reference(hip, st, dbs, DENSE_K, DENSE_S, DENSE_C)
    # the switch switches: the same steps in fewer turns, in the first tier's launch and in the second's
    seen = {}
    for reg in (None, "0"):
        capfd.readouterr()
        M.correct(hip, monkeypatch, DENSE_C, dict(env, **{"OATK_DEBUG_EC_STAGES": "1", REGROUP: reg, BATCH: None}))
        seen[reg] = turns(capfd.readouterr().err)
        print("regroup %s: (tier, blocks, batch, turns) %s" % (reg, seen[reg]))
    assert [x[:3] for x in seen[None]] == [x[:3] for x in seen["0"]] and {0, 1} <= {x[0] for x in seen[None]}
    for on, off in zip(seen[None], seen["0"]):
        assert on[3] < off[3] if on[0] <= 1 else on[3] <= off[3], (on, off)
    monkeypatch.delenv("OATK_DEBUG_EC_STAGES", raising=False)


def test_sequences(hip, monkeypatch):
    M.clean(hip, monkeypatch)
    M.resident(hip, dense_reads(), DENSE_K, DENSE_S, ref=False)
    raw = {}
    for what, v in (("old", OLD), ("new", {REGROUP: None, BATCH: None})):
        got, _ = M.correct(hip, monkeypatch, DENSE_C, dict(v, **{"OATK_DEBUG_EC_HEAVY": "0"}), keep_seq=True)
        hip.corrected_reads()
        raw[what] = dict(got, **{k: hip.fetch(k) for k in ("EC_BLOCK_QEND", "EC_CSEQ", "EC_CSEQ_LEN", "EC_CSEQ_OFF")})
    hip.ec_keep_seq(False)
    assert int((raw["old"]["EC_BLOCK_QEND"] > T0_DEFAULT).sum()) >= 3                          # long blocks were replaced
    M.assert_same(raw["new"], raw["old"], "sequences, the default against regroup off and batch 16")
