"""GPU: the wave solver's queues in source order and what a wave keeps from one block to the next (oatk_amd/csrc/ec_wave.hpp: EcwMemo;
api_ec.inc: ec_queue_sort).  None of it may change a result: every correction below is run with the memo on (the default), with its levels
alone (OATK_DEBUG_EC_MEMO=1) and off (=0) and compared array by array -- the block statistics, the corrected chains and the refreshed table
(test_gpu_ec_assemble.OUT) and every block's outcome and effort (EC_BLOCK_OUT: status, np, flags, short_block, tried, n_path, wf_steps,
wf_diag, tier; path_off and ticks are left out as elsewhere) -- and, where oracle/_ref is built, held against the compiled reference.

Read sets (of existing modules): short reads with every kind of block (K = 101); a diploid genome, whose bubbles make frames, on the tiers
and on the classes; K = 1001; repeats with ambiguous paths; and long blocks on the shipping caps, where blocks that a tier gives up midway
and a larger tier runs again sit between blocks of one source.  Then the queue's order (OATK_DEBUG_EC_QUEUE_SORT=0) and the serial tiers,
the counters OATK_DEBUG_EC_STAGES prints, and the sequence buffers of oatk_hip_ec_keep_seq."""
import re

import numpy as np
import pytest

import ref_lib as R
import test_gpu_ec as G
import test_gpu_ec_assemble as AS
import test_gpu_ec_routes as RT
from oatk_amd import pack_reads
from test_gpu_ec_seq import OUT_COLS

pytestmark = pytest.mark.gpu

EDIST, ARC_F = 0.02, 0.35
MEMO, SORT = "OATK_DEBUG_EC_MEMO", "OATK_DEBUG_EC_QUEUE_SORT"
KNOBS = ("OATK_DEBUG_EC_HEAVY", "OATK_DEBUG_EC_SERIAL_TIERS", "OATK_DEBUG_EC_STEP_BUDGET", "OATK_DEBUG_EC_FUSED_MIN_NW", "OATK_DEBUG_EC_HEAVY_CAP2",
         "OATK_DEBUG_EC_HEAVY_FL", "OATK_DEBUG_EC_STAGES", MEMO, SORT)


def resident(hip, reads, K, S, ref=True):
    """scan + count + EC graph of `reads` on the device; with `ref`, where the reference is built, its structs of the same batch (reference_run frees them)"""
    dbs = None
    if ref and R.available():
        from test_gpu_dropin import device_dbs
        dbs = device_dbs(hip, reads, K, S)
    else:
        seq, off, lens = pack_reads(reads)
        hip.scan_host(seq, off, lens, K, S)
        hip.count()
    hip.ec_graph()
    return dbs


def correct(hip, monkeypatch, c, env, keep_seq=False):
    """one correction of the resident batch under `env` (None: unset) and everything it left"""
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    st = hip.ec(EDIST, c, ARC_F, keep_seq=keep_seq)
    got = {k: hip.fetch(k) for k in AS.OUT}
    got["stats"] = np.array(st[:11], np.uint64)
    got["EC_BLOCK_OUT"] = hip.fetch("EC_BLOCK_OUT").reshape(-1, 12)[:, OUT_COLS].copy()
    return got, st


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def against_reference(hip, st, dbs, K, S, c):
    if dbs is None:
        return
    got = {k: G.fetch_ec(hip, k) for k in G.EC_BUF}
    RT.assert_matches(st, got, RT.reference_run(dbs[0], dbs[1], K, S, EDIST, c, 10 * c, c, ARC_F))


def clean(hip, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, 0, 0), "oatk_hip_debug_ec_tiers")          # the shipping caps


def memo_lines(err):
    """(tier, blocks, batch, levels reused, blocks started at their sink) of every launch of the wave solver"""
    return [tuple(int(x) for x in m) for m in
            re.findall(r"\[ec stages\] wave solver, tier (\d), (\d+) blocks: batch (\d+), (\d+) levels reused, (\d+) blocks started at their sink", err)]


def read_sets(hip):
    return {
        "assemble": lambda: (AS.K, AS.S, AS.C_MIN, AS.case_reads(hip), {}),
        "diploid-tiers": lambda: G.CASES[0][:3] + (G.CASES[0][3](), {"OATK_DEBUG_EC_HEAVY": "0"}),
        "diploid-classes": lambda: G.CASES[0][:3] + (G.CASES[0][3](), {"OATK_DEBUG_EC_HEAVY": "1"}),
        "k1001": lambda: G.CASES[2][:3] + (G.CASES[2][3](), {}),
        "repeats": lambda: G.CASES[4][:3] + (G.CASES[4][3](), {}),
    }


@pytest.mark.parametrize("name", ["assemble", "diploid-tiers", "diploid-classes", "k1001", "repeats"])
def test_memo_on_against_off(hip, monkeypatch, name):
    clean(hip, monkeypatch)
    K, S, c, reads, env = read_sets(hip)[name]()
    dbs = resident(hip, reads, K, S)
    off, _ = correct(hip, monkeypatch, c, dict(env, **{MEMO: "0"}))
    levels, _ = correct(hip, monkeypatch, c, dict(env, **{MEMO: "1"}))
    on, st = correct(hip, monkeypatch, c, dict(env, **{MEMO: None}))
    assert len(off["EC_BLOCK_OUT"]) > 0 and int(off["EC_BLOCK_OUT"][:, 4].sum()) > 0          # blocks, and arcs tried
    assert_same(levels, off, name + ", levels reused against the memo off")
    assert_same(on, off, name + ", the memo on against off")
    against_reference(hip, st, dbs, K, S, c)


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")       # (the planned blocks are laid out with the reference's syncmers)
def test_memo_with_blocks_handed_from_tier_to_tier(hip, monkeypatch, capfd):
    clean(hip, monkeypatch)
    K = 1001
    reads, plan, S = RT.long_block_reads(K, EDIST)
    c = RT.LONG_C
    dbs = resident(hip, reads, K, S)
    env = {"OATK_DEBUG_EC_HEAVY": "0", "OATK_DEBUG_EC_STAGES": "1"}
    off, _ = correct(hip, monkeypatch, c, dict(env, **{MEMO: "0"}))
    capfd.readouterr()
    on, st = correct(hip, monkeypatch, c, dict(env, **{MEMO: None}))
    err = capfd.readouterr().err
    assert_same(on, off, "long blocks, the memo on against off")
    tiers = set(int(t) for t in on["EC_BLOCK_OUT"][:, 8])
    assert {RT.T_LDS, RT.T_HYBRID, RT.T_SLAB} <= tiers                      # every tier finished blocks
    # a routed list shorter than sixteen blocks per wave is taken a block at a time
    sc = RT.stage_counts(err)
    lines = memo_lines(err)
    routed = [n for t in (1, 2) for n, how in sc["tier"].get(t, []) if how == "routed by length"]
    assert routed and lines
    for tier, n, batch, _, _ in lines:
        if tier > 0:
            assert batch == 1, (tier, n, batch)                             # (a few dozen long blocks: every list here is that short)
    assert any(tier > 0 and n in routed for tier, n, _, _, _ in lines)
    against_reference(hip, st, dbs, K, S, c)


def test_queue_in_source_order_against_read_order(hip, monkeypatch):
    clean(hip, monkeypatch)
    K, S, c, mk = G.CASES[2]
    dbs = resident(hip, mk(), K, S)
    plain, _ = correct(hip, monkeypatch, c, {SORT: "0", MEMO: "0"})
    unsorted_memo, _ = correct(hip, monkeypatch, c, {SORT: "0", MEMO: None})
    srt, st = correct(hip, monkeypatch, c, {SORT: None, MEMO: None})
    assert_same(unsorted_memo, plain, "read order, the memo on against off")
    assert_same(srt, plain, "source order against read order")
    against_reference(hip, st, dbs, K, S, c)


def test_serial_tiers(hip, monkeypatch):
    clean(hip, monkeypatch)
    K, S, c, mk = G.CASES[0]
    dbs = resident(hip, mk(), K, S)
    hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, 48, 160), "oatk_hip_debug_ec_tiers")       # most blocks outgrow the first tier and are run again
    try:
        env = {"OATK_DEBUG_EC_HEAVY": "0", "OATK_DEBUG_EC_SERIAL_TIERS": "1"}
        off, _ = correct(hip, monkeypatch, c, dict(env, **{MEMO: "0"}))
        on, st = correct(hip, monkeypatch, c, dict(env, **{MEMO: None}))
        assert_same(on, off, "serial tiers, the memo on against off")
        assert int(st[11]) > 0                                                                 # blocks did fall through
        against_reference(hip, st, dbs, K, S, c)
    finally:
        hip._check(hip.L.oatk_hip_debug_ec_tiers(hip.h, 0, 0), "oatk_hip_debug_ec_tiers")


def test_engagement(hip, monkeypatch, capfd):
    clean(hip, monkeypatch)
    K, S, c, mk = G.CASES[2]
    resident(hip, mk(), K, S, ref=False)
    seen = {}
    for memo in (None, "0"):
        capfd.readouterr()
        correct(hip, monkeypatch, c, {"OATK_DEBUG_EC_STAGES": "1", MEMO: memo})
        lines = memo_lines(capfd.readouterr().err)
        assert any(tier == 0 and batch > 1 for tier, _, batch, _, _ in lines)  # the first tier, in batches
        seen[memo] = (sum(x[3] for x in lines), sum(x[4] for x in lines))
        print("memo %s: %d levels reused, %d blocks started at their sink" % ((memo,) + seen[memo]))
    assert seen[None][0] > 0 and seen[None][1] > 0
    assert seen["0"] == (0, 0)
    monkeypatch.delenv("OATK_DEBUG_EC_STAGES", raising=False)
    capfd.readouterr()
    correct(hip, monkeypatch, c, {})
    assert "[ec stages]" not in capfd.readouterr().err


def test_sequences(hip, monkeypatch):
    clean(hip, monkeypatch)
    K, S, c, mk = G.CASES[2]
    resident(hip, mk(), K, S, ref=False)
    raw = {}
    for memo in ("0", None):
        got, _ = correct(hip, monkeypatch, c, {MEMO: memo}, keep_seq=True)
        seqs = hip.corrected_reads()
        raw[memo] = dict(got, **{k: hip.fetch(k) for k in ("EC_BLOCK_QEND", "EC_CSEQ", "EC_CSEQ_LEN", "EC_CSEQ_OFF")})
        raw[memo]["n"] = np.array([len(seqs)])
    hip.ec_keep_seq(False)
    assert int((raw["0"]["EC_BLOCK_QEND"] > 0).sum()) > 0                    # blocks were replaced
    assert_same(raw[None], raw["0"], "sequences, the memo on against off")
