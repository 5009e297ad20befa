"""GPU parity of the mini-circle repeat units (include/oatk_hip_racov.h: oatk_hip_ra_minicircle_units; include/oatk_syncasm.h: oatk_extract_minicircles) with
the Python model of tests/minicircle_util.py, which restates extract_minicircles_with_anchor (path_finder.c:539-730) line by line and is pinned to hand-derived
cases by tests/test_minicircle_model.py -- the function is static in a unit the oracle recipe does not compile, so there is no compiled reference to call.
Every comparison is exact: MC_UNIT per record, the distinct paths, their order and the number of records behind each."""
import ctypes as C

import numpy as np
import pytest

import adversarial as A
import minicircle_util as MC
import multiplex_util as MX
import ref_lib as R
import test_gpu_align as GA
from racov_util import Scg
from test_gpu_dropin import device_dbs
from oatk_amd import HipSyncasm, _lib

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")

RESIDENT_ALN = 2
BUFS = ["MC_UNIT", "MC_PATH_OFF", "MC_PATH_V", "MC_PATH_CNT"]


def check(got, model, what):
    unit, p_off, p_v, p_cnt = got
    mcs, paths, cnt = model
    assert np.array_equal(unit, mcs), (what, np.flatnonzero(unit != mcs)[:10])
    w_off, w_v = MC.flat_paths(paths)
    assert np.array_equal(p_off, w_off) and np.array_equal(p_v, w_v), (what, len(p_off) - 1, len(paths))
    assert p_cnt.tolist() == cnt, what
    assert int(p_cnt.sum()) == int((mcs != np.uint64(MC.NONE)).sum())


def run(hip, records, anchor, what):
    off, uid = MC.flat_records(records)
    model = MC.extract(off, uid, anchor)
    check(hip.ra_minicircle_units(anchor, {"off": off, "uid": uid}), model, what)
    return model


def test_the_hand_derived_table(hip):
    mcs, paths, cnt = run(hip, [r[0] for r in MC.TABLE], MC.ANCHOR, "table")
    assert list(zip(paths, cnt)) == MC.TABLE_PATHS


LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1100]


def edge_records(n):
    """records of n fragments round anchor 5: periodic ones of period 1, 2, 3 and 64, each also with one fragment changed at j = 0, at j = n - 1 and on either
    side of every chunk boundary, and with its last hit turned round; and records whose only hits lie in the last chunk"""
    out = []
    for p in (1, 2, 3, 64):
        unit = [10] + [14 + 4 * t for t in range(1, p)]
        for phase in (0, p // 2):
            base = [unit[(j + phase) % p] for j in range(n)]
            out.append(base)
            for j in sorted({0, n - 1} | {b + d for b in range(64, n, 64) for d in (-1, 0)}):
                if 0 <= j < n:
                    out.append(base[:j] + [base[j] ^ 2] + base[j + 1:])
            hits = [j for j in range(n) if base[j] >> 1 == 5]
            if hits:
                out.append(base[:hits[-1]] + [base[hits[-1]] ^ 1] + base[hits[-1] + 1:])
    last = (n - 1) // 64 * 64 if n else 0
    for hits in ([last, n - 1], [n - 2, n - 1], [last, last + 1, n - 1]):
        if all(0 <= j < n for j in hits):
            rec = [14] * n
            for j in hits:
                rec[j] = 11
            out.append(rec)
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_record_lengths_round_the_chunk_and_the_length_class(hip, n):
    records = edge_records(n)
    mcs, paths, cnt = run(hip, records, 5, n)
    n_valid = int((mcs != np.uint64(MC.NONE)).sum())
    print("n", n, "records", len(records), "valid", n_valid, "paths", len(paths))
    if n >= 3:
        assert 0 < n_valid < len(records)
    if n >= 66:                                     # period 64: paths longer than one lane walks (128 where the changed fragment was the middle hit of three)
        assert max(len(p) for p in paths) >= 64


def random_records(seed, count):
    """over 6 unitigs, lengths 0-40, about a third built periodic round the anchor (unitig 2) at any phase; a fifth of those spoiled"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(0, 41))
        if rng.integers(0, 3) == 0 and n:
            p = int(rng.integers(1, min(n, 6) + 1))
            unit = [4 | int(rng.integers(0, 2))] + [int(x) for x in rng.choice([0, 1, 2, 3, 6, 7, 8, 9, 10, 11], p - 1)]
            ph = int(rng.integers(0, p))
            rec = [unit[(j + ph) % p] for j in range(n)]
            if rng.integers(0, 5) == 0:
                rec[int(rng.integers(0, n))] ^= int(rng.integers(1, 4))
        else:
            rec = [int(x) for x in rng.integers(0, 12, n)]
        out.append(rec)
    return out


@pytest.fixture(scope="module")
def random_set():
    records = random_records(20241, 20000)
    off, uid = MC.flat_records(records)
    model = MC.extract(off, uid, 2)
    n_valid = int((model[0] != np.uint64(MC.NONE)).sum())
    assert n_valid >= 1000 and len(model[1]) >= 20, (n_valid, len(model[1]))
    return off, uid, model


def test_random_records_equal_the_model(hip, random_set):
    off, uid, model = random_set
    check(hip.ra_minicircle_units(2, {"off": off, "uid": uid}), model, "random")
    assert max(model[2]) >= 2 and min(model[2]) == 1


def test_results_do_not_depend_on_the_hash_bits(hip, random_set):
    off, uid, model = random_set
    paths = model[1]
    groups = {}
    for p in paths:
        groups.setdefault(MC.path_hash(p, 2), []).append(p)
    assert max(len(g) for g in groups.values()) >= 2, "two different paths share a group of the 2-bit hash"
    try:
        for bits in (64, 8, 2, 0):
            hip.debug_mc_hash_bits(bits)
            check(hip.ra_minicircle_units(2, {"off": off, "uid": uid}), model, ("bits", bits))
            rounds = hip.ra_minicircle_times()[1]
            want = {}
            for p in paths:
                want[MC.path_hash(p, bits)] = want.get(MC.path_hash(p, bits), 0) + 1
            print("bits", bits, "groups", len(want), "rounds", rounds)
            assert rounds == max(want.values()), (bits, rounds)         # a round settles one path per group: the device keyed the paths as this test does
    finally:
        hip.debug_mc_hash_bits(0)


def test_refusals_leave_the_resident_results_alone(hip):
    off, uid = MC.flat_records([r[0] for r in MC.TABLE])
    first = hip.ra_minicircle_units(MC.ANCHOR, {"off": off, "uid": uid})
    before = [hip.fetch(b).tobytes() for b in BUFS]
    ptrs = [hip.buffer(b) for b in BUFS]

    def refused(aln, anchor, code):
        keep = [np.ascontiguousarray(aln["off"], np.uint64), np.ascontiguousarray(aln["uid"], np.uint64)]
        a = _lib.RacovAln(len(keep[0]) - 1, len(keep[1]), None, keep[0].ctypes.data, None, keep[1].ctypes.data, None, None, None, None)
        n = [C.c_uint64(99), C.c_uint64(98), C.c_uint64(97)]
        rc = hip.L.oatk_hip_ra_minicircle_units(hip.h, C.byref(a), anchor, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]))
        assert rc == code, (rc, hip.L.oatk_hip_last_error(hip.h))
        assert [x.value for x in n] == [99, 98, 97]
        assert [hip.buffer(b) for b in BUFS] == ptrs and [hip.fetch(b).tobytes() for b in BUFS] == before

    good = {"off": off, "uid": uid}
    refused(good, 1 << 31, _lib.E_ARG)
    refused(good, 1 << 63, _lib.E_ARG)
    for bad_off in (np.array([1, 3, 5], np.uint64), np.array([0, 4, 3, 5], np.uint64), np.array([0, 2, 4], np.uint64), np.array([0, 2, 6], np.uint64)):
        refused({"off": bad_off, "uid": np.array([10, 14, 10, 14, 10], np.uint64)}, 5, _lib.E_ARG)
    # a uid of 2^32 or more inside a unit; forward, reverse, and in a path a wave writes (over 32 elements)
    big = (1 << 32) | 14
    refused({"off": [0, 3], "uid": [10, big, 10]}, 5, _lib.E_ARG)
    refused({"off": [0, 2, 5], "uid": [10, 10, 11, big | 1, 11]}, 5, _lib.E_ARG)
    long_unit = [10] + [14 + 4 * t for t in range(1, 40)]
    refused({"off": [0, 81], "uid": (long_unit[:20] + [big] + long_unit[21:]) * 2 + [10]}, 5, _lib.E_ARG)
    # the same uid outside any unit is nobody's business: the record gives none
    ok = hip.ra_minicircle_units(5, {"off": [0, 3], "uid": [10, big, 14]})
    assert ok[0].tolist() == [MC.NONE] and len(ok[3]) == 0 and ok[1].tolist() == [0]
    # a second identical call gives identical bytes
    again = hip.ra_minicircle_units(MC.ANCHOR, good)
    assert all(np.array_equal(x, y) for x, y in zip(first, again)) and [hip.fetch(b).tobytes() for b in BUFS] == before
    # no records at all: zeros
    n = [C.c_uint64(99), C.c_uint64(98), C.c_uint64(97)]
    a = _lib.RacovAln()
    assert hip.L.oatk_hip_ra_minicircle_units(hip.h, C.byref(a), 5, C.byref(n[0]), C.byref(n[1]), C.byref(n[2])) == 0
    assert [x.value for x in n] == [0, 0, 0]
    assert [len(hip.fetch(b)) for b in BUFS] == [0, 1, 0, 0] and hip.fetch("MC_PATH_OFF").tolist() == [0]


def test_resident_alignments_are_refused_before_any_alignment():
    h = HipSyncasm(0)
    try:
        n = [C.c_uint64(99), C.c_uint64(98), C.c_uint64(97)]
        assert h.L.oatk_hip_ra_minicircle_units(h.h, None, 5, C.byref(n[0]), C.byref(n[1]), C.byref(n[2])) == _lib.E_STATE
        assert [x.value for x in n] == [99, 98, 97]
        p, b = C.c_void_p(), C.c_uint64()
        assert h.L.oatk_hip_buffer(h.h, _lib.BUF["MC_UNIT"], C.byref(p), C.byref(b)) == _lib.E_STATE
    finally:
        h.close()


# ---- through the pipeline: two mini-circles that share a conserved core ----
CORE, VAR1, VAR2, TURNS = 900, 700, 800, 6


def minicircle_reads(seed=77, n_reads=150, n_cross=8, read_len=4200):
    """the conserved core C followed by one of two variable segments: reads sampled from the tandem texts (C V1)^m and (C V2)^m, and a few that run from one
    text into the other (C V1 C V2 ...): those walk round the anchor without repeating one unit"""
    rng = np.random.default_rng(seed)
    c, v1, v2 = (A.rand_dna(rng, n) for n in (CORE, VAR1, VAR2))
    t1, t2 = (c + v1) * TURNS, (c + v2) * TURNS
    reads = []
    for t in (t1, t2):
        for _ in range(n_reads):
            st = int(rng.integers(0, len(t) - read_len))
            reads.append(t[st:st + read_len])
    cross = (c + v1) * 2 + (c + v2) * 2 + c
    for _ in range(n_cross):
        st = int(rng.integers(0, CORE // 2))
        reads.append(cross[st:st + len(cross) - CORE // 2])
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    return [r if i % 2 == 0 else r.translate(comp)[::-1] for i, r in enumerate(reads)]


def graph_for_stats(g):
    """what path_finder.c:696-727 reads from scg->utg_asmg, through the layout mirrors"""
    a = C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents
    nu, na = int(a.n_vtx), int(a.n_arc)
    return {"idx_p": np.frombuffer(C.string_at(a.idx_p, 16 * nu), np.uint64), "idx_n": np.frombuffer(C.string_at(a.idx_n, 16 * nu), np.uint64),
            "arc_w": np.array([a.arc[i].w for i in range(na)], np.uint64), "arc_ls": np.array([a.arc[i].ls for i in range(na)], np.uint64),
            "arc_del": np.array([a.arc[i].del_ for i in range(na)], np.uint8), "vtx_len": np.array([a.vtx[i].len for i in range(nu)], np.uint64),
            "vtx_cov": np.array([a.vtx[i].cov for i in range(nu)], np.uint32)}


def pick_anchor(aln, n_utg):
    """the unitig holding the core: the one both circles run through, so the one with the most fragments"""
    return int(np.bincount((aln["uid"] >> np.uint64(1)).astype(np.int64), minlength=n_utg).argmax())


@needs_ref
def test_two_circles_through_the_pipeline(hip):
    K, S, c, _ = GA.CASES[2]
    L, H = GA.setup_libs()
    vp = C.c_void_p
    L.refx_consensus.argtypes = [vp, vp, C.c_int, C.c_int]
    H.oatk_extract_minicircles.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint, C.POINTER(_lib.McPaths)]
    H.oatk_mc_paths_free.restype = None
    H.oatk_mc_paths_free.argtypes = [C.POINTER(_lib.McPaths)]
    db, scm = device_dbs(hip, minicircle_reads(), K, S)
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    g = L.refx_make_graph(db, scm, c, 0.35)
    assert g
    L.refx_process_unitigs(g)
    L.refx_consensus(db, g, 0, 0)                          # vtx.len and arc.ls, as parse_organelle_minicircle has them (path_finder.c:818)
    v = L.refx_ra_new()
    nsk = C.c_uint64(0)
    assert H.oatk_scg_read_alignment(hip.h, db, v, g, 0, C.byref(nsk), None) == 0, hip.L.oatk_hip_last_error(hip.h)      # leaves the alignments resident
    aln = MX.flat_aln(GA.flatten(L, v))
    G = graph_for_stats(g)
    anchor = pick_anchor(aln, len(G["vtx_len"]))
    model = MC.extract(aln["off"], aln["uid"], anchor)
    mcs, paths, cnt = model
    print("anchor", anchor, "records", len(mcs), "valid", int((mcs != np.uint64(MC.NONE)).sum()), "paths", list(zip(paths, cnt)))
    # both circles are there: two paths of the anchor and one more unitig each, different ones; and a read that changes circles is rejected for its period
    two = [p for p in paths if len(p) == 2]
    assert len({p[1] >> 1 for p in two}) >= 2 and all(p[0] == anchor << 1 for p in paths)
    off = aln["off"].astype(np.int64)
    period_rejects = 0
    for i in np.flatnonzero(mcs == np.uint64(MC.NONE)):
        rec = [int(x) for x in aln["uid"][off[i]:off[i + 1]]]
        hits = [x for x in rec if x >> 1 == anchor]
        period_rejects += len(hits) >= 2 and len({x & 1 for x in hits}) == 1
    assert period_rejects >= 1
    # the device: resident, and the same alignments downloaded and uploaded again
    check(hip.ra_minicircle_units(anchor), model, "resident")
    check(hip.ra_minicircle_units(anchor, aln), model, "uploaded")
    # the adaptor, both ways, against the model and a restatement of :696-727
    want = [(len(p), p) + MC.path_stats(G, p) + (n, ) for p, n in zip(paths, cnt)]
    for flags in (RESIDENT_ALN, 0):
        out = _lib.McPaths()
        assert H.oatk_extract_minicircles(hip.h, v, g, anchor, flags, C.byref(out)) == 0, hip.L.oatk_hip_last_error(hip.h)
        got = [(out.a[i].nv, [out.a[i].v[t] for t in range(out.a[i].nv)], out.a[i].len, out.a[i].wlen, out.a[i].cnt) for i in range(out.n)]
        H.oatk_mc_paths_free(C.byref(out))
        assert got == want, (flags, got, want)
    assert all(w[2] > 0 and w[3] > 0 for w in want)
    L.refx_ra_destroy(v)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)
