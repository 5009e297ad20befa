"""GPU parity of the spanning-triplet scores of scg_multiplex (include/oatk_hip_racov.h: oatk_hip_ra_triplet_scores) and of the decisions taken
from them (include/oatk_syncasm.h: oatk_scg_multiplex_plan) against the Python model of tests/multiplex_util.py -- which
tests/test_multiplex_model.py pins to the compiled reference -- and, through the pipeline, against the COMPILED REFERENCE's scg_multiplex
itself (syncasm.c:1090): `updated` is its return value.  Every comparison of doubles is exact.  The device runs twice each time: on the
alignments resident in the handle, and with everything uploaded -- through the pipeline, where oatk_hip_read_alignment leaves them there;
the hand-made records of the synthetic set can only be uploaded."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import multiplex_util as MX
import ref_lib as R
import test_gpu_align as GA
from racov_util import Scg
from test_gpu_dropin import device_dbs
from oatk_amd import _lib

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")

RESIDENT_ALN = 2


def libs():
    L, H = GA.setup_libs()
    vp = C.c_void_p
    H.oatk_scg_multiplex_plan.argtypes = [vp, vp, vp, C.c_uint, C.c_uint32, C.c_double, C.c_double, vp, C.POINTER(C.c_int), C.POINTER(_lib.TripletTable)]
    H.oatk_triplet_table_free.restype = None
    H.oatk_triplet_table_free.argtypes = [C.POINTER(_lib.TripletTable)]
    return L, H


def plan(H, hip, v, g, n_vtx, flags, max_n_scm, min_n_r, min_d_f, want_rc=0):
    """oatk_scg_multiplex_plan: (multi_vtx, updated, [(l_in, l_out, value)])"""
    mv = np.full(max(n_vtx, 1), 9, np.uint8)
    upd = C.c_int(-5)
    tab = _lib.TripletTable()
    rc = H.oatk_scg_multiplex_plan(hip.h, v, g, flags, max_n_scm, min_n_r, min_d_f, mv.ctypes.data, C.byref(upd), C.byref(tab))
    assert rc == want_rc, (rc, hip.L.oatk_hip_last_error(hip.h))
    if rc:
        return mv[:n_vtx], upd.value, None
    ent = [(tab.l_in[k], tab.l_out[k], tab.val[k]) for k in range(tab.n)]
    H.oatk_triplet_table_free(C.byref(tab))
    return mv[:n_vtx], upd.value, ent


def check_plan(got, m, what):
    mv, upd, ent = got
    assert upd == m["updated"], (what, upd, m["updated"])
    assert np.array_equal(mv, m["multi_vtx"]), (what, mv, m["multi_vtx"])
    k = np.flatnonzero(m["have"])
    assert [(int(a), int(b)) for a, b, _ in ent] == [(int(m["pair_in"][i]), int(m["pair_out"][i])) for i in k], what
    assert MX.same_doubles([x for _, _, x in ent], m["score"][k]), what


@needs_ref
@pytest.mark.parametrize("case", [2, 3])
def test_plan_matches_reference_through_the_pipeline(hip, case):
    """test_gpu_align.CASES driven like the coverage tests drive them: in every unzip round the plan is made BEFORE the reference's
    scg_multiplex on the same graph and alignments"""
    K, S, c, mk = GA.CASES[case]
    L, H = libs()
    db, scm = device_dbs(hip, mk(), K, S)
    st = np.zeros(12, np.uint64)
    assert H.oatk_read_error_correction(hip.h, db, scm, None, 0.02, c, 10 * c, c, 0.35, st.ctypes.data) == 0
    g = L.refx_make_graph(db, scm, c, 0.35)
    assert g
    v = L.refx_ra_new()

    def align(for_unzip):
        nsk = C.c_uint64(0)
        rc = H.oatk_scg_read_alignment(hip.h, db, v, g, for_unzip, C.byref(nsk), None)
        assert rc == 0, hip.L.oatk_hip_last_error(hip.h)

    align(0)
    L.refx_process_unitigs(g)
    align(0)
    max_n_scm = int(math.ceil(30000.0 / K))
    seen = {"rounds": 0, "updated": 0, "have": 0, "records": 0}
    for _ in range(3):
        align(1)
        L.refx_update_utg_cov(g)
        graph, aln = MX.flatten_graph(g), MX.flat_aln(GA.flatten(L, v))
        m = MX.model(graph, aln, max_n_scm, 10.0, 0.3)
        nu = len(graph["vtx_del"])
        for flags, a in ((RESIDENT_ALN, None), (0, aln)):
            MX.assert_same_scores(hip.ra_triplet_scores(graph, a), m, (case, flags))
            check_plan(plan(H, hip, v, g, nu, flags, max_n_scm, 10.0, 0.3), m, (case, flags))
        updated = L.refx_multiplex(g, v, max_n_scm, 10.0, 0.3)
        assert m["updated"] == updated
        seen["rounds"] += 1
        seen["updated"] += updated > 0
        seen["have"] += int(m["have"].sum())
        seen["records"] += MX.triplet_records(aln)[0]
        if updated == 0:
            break
    print("case", case, seen)
    assert seen["updated"] > 0 and seen["have"] > 0 and seen["records"] > 0
    L.refx_ra_destroy(v)
    L.refx_scg_destroy(g)
    L.refx_scmdb_destroy(scm)
    L.refx_srdb_destroy(db)


# ---- the synthetic set: fourteen unitigs, each on the list for one of the cases below ----
A_, B_, C_, D_, E_, F_, G_, H_, P_, Q0, Q1, Q2, S_, T_ = range(14)
N_UTG, N_SCM, F_LEN = 14, 600, 3001
MAX_N_SCM, MIN_N_R, MIN_D_F = 20, 5.0, 0.3


def utg_list(u):
    """positions 0..4 hold syncmers 0..4, which every unitig holds; 5..9 the unitig's own.  F: 3000 shared positions, then its only own one"""
    if u == F_:
        return [p % 5 for p in range(F_LEN - 1)] + [500]
    return [0, 1, 2, 3, 4] + [100 + 10 * u + p for p in range(5)]


def fw(u):
    return u << 1


def rv(u):
    return u << 1 | 1


# (v, w, link_id, comp, del); a pair of complementary arcs shares its link id
ARCS = sorted([
    (fw(A_), fw(B_), 0, 0, 0), (rv(B_), rv(A_), 0, 1, 0),
    (fw(C_), fw(B_), 1, 0, 0), (rv(B_), rv(C_), 1, 1, 0),
    (fw(B_), fw(D_), 2, 0, 0), (rv(D_), rv(B_), 2, 1, 0),
    (fw(B_), fw(E_), 3, 0, 0), (rv(E_), rv(B_), 3, 1, 0),
    (fw(E_), rv(E_), 4, 0, 0),                                          # self-complementary
    (fw(A_), fw(E_), 5, 0, 1), (rv(E_), rv(A_), 5, 1, 1),               # deleted (asmg_arc still finds them)
    (fw(D_), fw(G_), 6, 0, 0), (rv(G_), rv(D_), 6, 1, 0),
    (fw(G_), fw(H_), 7, 0, 0), (rv(H_), rv(G_), 7, 1, 0),
    (fw(C_), fw(F_), 8, 0, 0), (rv(F_), rv(C_), 8, 1, 0),
    (fw(F_), fw(H_), 9, 0, 0), (rv(H_), rv(F_), 9, 1, 0),
    (fw(A_), fw(F_), 10, 0, 0), (rv(F_), rv(A_), 10, 1, 0),
    (fw(P_), fw(P_), 11, 0, 0), (rv(P_), rv(P_), 11, 1, 0),             # a live arc of P onto itself
    (fw(Q0), fw(Q1), 12, 0, 0), (rv(Q1), rv(Q0), 12, 1, 0),
    (fw(Q1), fw(Q2), 12, 1, 0), (rv(Q2), rv(Q1), 12, 0, 0),             # the link id of Q0 -> Q1 once more: (24, 25) is its own mirror
], key=lambda a: a[0])

F7, F1 = math.modf(7 + 1 / 3)[0], math.modf(1 + 1 / 3)[0]              # what modf leaves of the scores of reads with three alignments


def U(v):
    """a fragment over the unitig's own syncmers"""
    return (v, 5, 9, 0, 4)


def N(v):
    """a fragment over shared syncmers only"""
    return (v, 0, 4, 0, 4)


def synthetic_reads():
    """per read its records (score, [(uid, u_beg, u_end, s_beg, s_end), ...]), in ra_v order"""
    one = lambda s, *f: [(s, list(f))]
    rd = []
    # a path of five fragments: the keys slide along it
    rd += [one(20.0, U(fw(A_)), U(fw(B_)), U(fw(D_)), U(fw(G_)), U(fw(H_)))] * 4
    # exactly three fragments; (BD, DG) reaches min_n_r exactly
    rd += [one(12.0, U(fw(B_)), U(fw(D_)), U(fw(G_)))]
    # two fragments: ignored
    rd += [one(9.0, U(fw(A_)), U(fw(B_)))] * 2
    # (AB, BD) crossed on both strands in turn, integral
    rd += [one(8.0, U(fw(A_)), U(fw(B_)), U(fw(D_))), one(8.0, U(rv(D_)), U(rv(B_)), U(rv(A_)))] * 3
    # (CB, BD) crossed on both strands in turn, integral and fractional scores mixed: reads with two and three alignments
    rd += [[(1 + 1 / 3, [U(fw(C_)), U(fw(B_)), U(fw(D_))]), (1 + 1 / 3, [U(fw(A_))]), (1 + 1 / 3, [U(fw(C_))])]]
    rd += [one(11.0, U(rv(D_)), U(rv(B_)), U(rv(C_)))]
    rd += [[(6.5, [U(fw(C_)), U(fw(B_)), U(fw(D_))]), (6.5, [N(fw(B_))])]]
    rd += [[(4.5, [U(rv(D_)), U(rv(B_)), U(rv(C_))]), (4.5, [U(fw(A_)), U(fw(B_))])]]
    rd += [[(1 + 1 / 3, [U(fw(C_)), U(fw(B_)), U(fw(D_))]), (1 + 1 / 3, [U(fw(H_))]), (1 + 1 / 3, [U(fw(G_)), U(fw(H_))])]]
    rd += [[(7 + 1 / 3, [U(rv(D_)), U(rv(B_)), U(rv(C_))]), (7 + 1 / 3, [U(fw(A_))]), (7 + 1 / 3, [U(fw(C_))])]]
    # (AB, BE) = 3 and (CB, BE) = 12: 3 / 10 is min_d_f exactly on the incoming side, 3 / 12 below it on the outgoing side
    rd += [one(7.0, U(fw(A_)), U(fw(B_)), U(fw(E_)))] * 3
    rd += [one(7.0, U(fw(C_)), U(fw(B_)), U(fw(E_)))] * 12
    # through the self-complementary arc and back: the second triplet's key is the first one's mirror
    rd += [one(16.0, U(fw(B_)), U(fw(E_)), U(rv(E_)), U(rv(B_)))] * 3
    # through the deleted arc A+ -> E+: no pair, no error
    rd += [one(12.0, U(fw(A_)), U(fw(E_)), U(rv(E_)))] * 2
    # (DG, GH) stays just under min_n_r: 4 + .5 + .333; the .5 record's middle fragment has its only unique syncmer at u_end, and one more
    # record's middle fragment has none (no event)
    rd += [[(3.5, [U(fw(D_)), (fw(G_), 0, 5, 0, 5), U(fw(H_))]), (3.5, [N(fw(D_)), N(fw(G_))])]]
    rd += [[(7 + 1 / 3, [U(fw(D_)), U(fw(G_)), U(fw(H_))]), (7 + 1 / 3, [N(fw(A_))]), (7 + 1 / 3, [N(fw(C_))])]]
    rd += [[(3.5, [U(fw(D_)), N(fw(G_)), U(fw(H_))]), (3.5, [N(fw(D_)), N(fw(G_))])]]
    # the long unitig F (over max_n_scm): six integral records, a fragment over all its 3001 positions whose unique syncmer is the last,
    # the same fragment one position shorter (no event), and a key that is seen once only
    rd += [one(30.0, U(fw(C_)), (fw(F_), 0, F_LEN - 1, 0, 4), U(fw(H_)))] * 6
    rd += [[(30.5, [U(fw(C_)), (fw(F_), 0, F_LEN - 1, 0, 4), U(fw(H_))]), (30.5, [N(fw(C_))])]]
    rd += [[(30.5, [U(fw(C_)), (fw(F_), 0, F_LEN - 2, 0, 4), U(fw(H_))]), (30.5, [N(fw(C_))])]]
    rd += [one(30.0, U(fw(A_)), (fw(F_), 0, F_LEN - 1, 0, 4), U(fw(H_)))]
    # the arc of P onto itself, on both strands
    rd += [one(9.0, U(fw(P_)), U(fw(P_)), U(fw(P_)))] * 3 + [one(9.0, U(rv(P_)), U(rv(P_)), U(rv(P_)))] + [one(9.0, U(fw(P_)), U(fw(P_)), U(fw(P_)))] * 2
    # the key that is its own mirror: the first event leaves the score, every later one adds it twice (1 + 2 + 2 = min_n_r)
    rd += [one(9.0, U(fw(Q0)), U(fw(Q1)), U(fw(Q2))), one(9.0, U(rv(Q2)), U(rv(Q1)), U(rv(Q0))), one(9.0, U(fw(Q0)), U(fw(Q1)), U(fw(Q2)))]
    return rd


# the pairs in the reference's lookup order -- (l_in, l_out): score -- and the marks of the fourteen unitigs
MIX = F1 + 1.0 + 0.5 + 0.5 + F1 + F7                # (CB, BD) in record order; Python adds from the left
assert (F1, F7, MIX) == (float.fromhex("0x1.5555555555554p-2"), float.fromhex("0x1.5555555555550p-2"), 2.999999999999999)
WANT = [((0, 4), 10.0), ((0, 6), 3.0), ((2, 4), MIX), ((2, 6), 12.0),          # B
        ((4, 12), 5.0),                                                          # D: at min_n_r
        ((6, 8), 6.0),                                                           # E: twice per read through the self-complementary arc
        ((16, 18), 6.5), ((20, 18), 1.0),                                        # F
        ((12, 14), 4.0 + 0.5 + F7),                                              # G: just under min_n_r
        ((22, 22), 6.0),                                                         # P
        ((24, 25), 5.0)]                                                         # Q1: 1 + 2 + 2
WANT_VTX = [0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 2, 0]
WANT_UPDATED = 1                                 # (CB, BD): below min_d_f of both its arcs' best


def flatten_reads(reads):
    sid, off, s, uid, ub, ue, sb, se = [], [0], [], [], [], [], [], []
    for i, recs in enumerate(reads):
        for sc, frags in recs:
            sid.append(i), s.append(sc)
            for f in frags:
                uid.append(f[0]), ub.append(f[1]), ue.append(f[2]), sb.append(f[3]), se.append(f[4])
            off.append(len(uid))
    return {"sid": np.array(sid, np.uint32), "off": np.array(off, np.uint64), "s": np.array(s, np.float64), "uid": np.array(uid, np.uint64),
            "u_beg": np.array(ub, np.uint32), "u_end": np.array(ue, np.uint32), "s_beg": np.array(sb, np.uint32), "s_end": np.array(se, np.uint32)}


def synthetic_graph():
    lists = [utg_list(u) for u in range(N_UTG)]
    su = [[] for _ in range(N_SCM)]
    for u, lst in enumerate(lists):
        for p, x in enumerate(lst):
            su[x].append((u << 1, p))
    idx_p, idx_n = np.zeros(2 * N_UTG, np.uint64), np.zeros(2 * N_UTG, np.uint64)
    for i, a in enumerate(ARCS):
        if idx_n[a[0]] == 0:
            idx_p[a[0]] = i
        idx_n[a[0]] += 1
    vtx_del = np.zeros(N_UTG, np.uint8)
    vtx_del[T_] = 1
    return {"n_scm": N_SCM, "su_off": np.concatenate([[0], np.cumsum([len(x) for x in su])]).astype(np.uint64),
            "su_uid": np.array([e[0] for x in su for e in x], np.uint64), "su_pos": np.array([e[1] for x in su for e in x], np.uint32),
            "scm_cov": np.full(N_SCM, 20, np.uint32), "utg_off": np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64),
            "utg_a": np.array([x << 1 for lst in lists for x in lst], np.uint64), "idx_p": idx_p, "idx_n": idx_n,
            "arc_v": np.array([a[0] for a in ARCS], np.uint64), "arc_w": np.array([a[1] for a in ARCS], np.uint64),
            "arc_link": np.array([a[2] for a in ARCS], np.uint64), "arc_comp": np.array([a[3] for a in ARCS], np.uint8),
            "arc_del": np.array([a[4] for a in ARCS], np.uint8), "vtx_del": vtx_del}


class Synthetic:
    """the graph above as a scg_t of the reference's (refx_scg_from_flat; vtx[].a, link_id, comp and del through the layout mirrors) and the
    reads' records as its scg_ra_v.  Never handed to scg_multiplex itself: its rewrite frees arrays that live here."""

    def __init__(self, L, reads):
        self.L = L
        vp = C.c_void_p
        L.refx_fake_scmdb.restype = vp
        L.refx_fake_scmdb.argtypes = [C.c_uint64, vp, vp]
        L.refx_fake_dbs_free.argtypes = [vp, vp]
        L.refx_scg_from_flat.restype = vp
        L.refx_scg_from_flat.argtypes = [vp, C.c_uint64, C.c_uint64] + [vp] * 10
        L.refx_scg_flat_destroy.argtypes = [vp]
        L.refx_ra_build.restype = vp
        L.refx_ra_build.argtypes = [C.c_uint64] + [vp] * 8
        G = self.graph = synthetic_graph()
        self.scm = L.refx_fake_scmdb(N_SCM, G["scm_cov"].ctypes.data, np.zeros(N_SCM, np.uint8).ctypes.data)
        utg_n = np.diff(G["utg_off"].astype(np.int64)).astype(np.uint32)
        self.g = L.refx_scg_from_flat(self.scm, N_UTG, len(ARCS), G["su_off"].ctypes.data, G["su_uid"].ctypes.data, G["su_pos"].ctypes.data, utg_n.ctypes.data,
                                      G["idx_p"].ctypes.data, G["idx_n"].ctypes.data, G["arc_v"].ctypes.data, G["arc_w"].ctypes.data,
                                      np.zeros(len(ARCS), np.uint64).ctypes.data, G["arc_del"].ctypes.data)
        self.lists = [np.ascontiguousarray(G["utg_a"][int(G["utg_off"][u]):int(G["utg_off"][u + 1])]) for u in range(N_UTG)]
        ag = C.cast(self.g, C.POINTER(Scg)).contents.utg_asmg.contents
        for u, x in enumerate(self.lists):
            ag.vtx[u].a = x.ctypes.data
            ag.vtx[u].del_ = int(G["vtx_del"][u])
        for i, a in enumerate(ARCS):
            ag.arc[i].link_id, ag.arc[i].comp = a[2], a[3]
        self.aln = flatten_reads(reads)
        a = self.aln
        cols = [a["sid"].astype(np.uint64), np.diff(a["off"].astype(np.int64)).astype(np.uint32), a["s"], a["uid"], a["u_beg"].astype(np.uint64),
                a["u_end"].astype(np.uint64), a["s_beg"], a["s_end"]]
        self.v = L.refx_ra_build(len(a["sid"]), *[x.ctypes.data for x in cols])

    def close(self):
        self.L.refx_ra_destroy(self.v)
        self.L.refx_scg_flat_destroy(self.g)
        self.L.refx_fake_dbs_free(None, self.scm)


@needs_ref
def test_synthetic_cases_match_the_constants_and_the_model(hip):
    L, H = libs()
    reads = synthetic_reads()
    syn = Synthetic(L, reads)
    try:
        aln = syn.aln
        assert len(aln["sid"]) <= 200
        n = np.diff(aln["off"].astype(np.int64))
        assert (n == 2).any() and (n == 3).any() and (n >= 5).any()
        trace = []
        tab = MX.triplet_table(syn.graph, aln, trace)
        m = MX.decide(syn.graph, tab, MAX_N_SCM, MIN_N_R, MIN_D_F)
        # the constants against the model
        assert [(int(a), int(b)) for a, b in zip(m["pair_in"], m["pair_out"])] == [k for k, _ in WANT]
        assert MX.same_doubles(m["score"], [x for _, x in WANT]) and m["have"].all()
        assert list(m["multi_vtx"]) == WANT_VTX and m["updated"] == WANT_UPDATED
        # what makes the cases live: the mixed key is crossed on both strands in turn and its sum depends on the order ...
        mix = [(A, sc) for _, A, _, sc in trace if A in ((2, 4), (5, 3))]
        assert [A for A, _ in mix] == [(2, 4), (5, 3)] * 3
        assert any(sum(p) != MIX for p in itertools.permutations([sc for _, sc in mix]))
        # ... the key through the deleted arc is put but never read, the self-mirrored key and the once-only key exist ...
        assert (10, 8) in tab and (10, 8) not in set(zip(m["pair_in"].tolist(), m["pair_out"].tolist()))
        assert sum(1 for _, A, M, _ in trace if A == M) == 3 and sum(1 for _, A, _, _ in trace if A == (20, 18)) == 1
        # ... and the records without an event are the two that lack a unique syncmer in their middle fragment
        with_event = {i for i, _, _, _ in trace}
        assert sum(1 for i in range(len(n)) if n[i] >= 3 and i not in with_event) == 2
        # the device, uploaded: the raw scores and the plan
        got = hip.ra_triplet_scores(syn.graph, aln)
        print("pairs", list(zip(got["pair_in"].tolist(), got["pair_out"].tolist(), got["score"].tolist(), got["have"].tolist())))
        MX.assert_same_scores(got, m, "synthetic")
        check_plan(plan(H, hip, syn.v, syn.g, N_UTG, 0, MAX_N_SCM, MIN_N_R, MIN_D_F), m, "synthetic plan")
        # a graph passed without vtx_del reads as "no unitig is deleted": T has no arc, so it turns into a singleton and nothing else moves
        g2 = dict(syn.graph)
        del g2["vtx_del"]
        MX.assert_same_scores(hip.ra_triplet_scores(g2, aln), m, "no vtx_del")
    finally:
        syn.close()


@needs_ref
def test_refusals_write_nothing(hip):
    """no arc between fragments 0 and 1 of a record of three whose fragments have no unique syncmer (no event would come of it, the
    reference still dereferences NULL): OATK_E_ARG; too little room for the pairs: an error and the number needed"""
    L, H = libs()
    bad = synthetic_reads() + [[(2.5, [N(fw(D_)), N(fw(A_)), N(fw(B_))]), (2.5, [N(fw(C_))])]]
    syn = Synthetic(L, bad)
    try:
        g, keep_g = hip._racov_graph(syn.graph)
        a, keep_a = hip._racov_aln(syn.aln)
        off, n = np.full(N_UTG + 1, 77, np.uint64), C.c_uint64(99)
        p_in, p_out, sc, hv = np.full(16, 77, np.uint64), np.full(16, 77, np.uint64), np.full(16, -7.0), np.full(16, 7, np.uint8)
        args = lambda cap: (hip.h, C.byref(g), C.byref(a), off.ctypes.data, cap, C.byref(n), p_in.ctypes.data, p_out.ctypes.data, sc.ctypes.data, hv.ctypes.data)
        assert hip.L.oatk_hip_ra_triplet_scores(*args(16)) == _lib.E_ARG
        assert n.value == 99 and (off == 77).all() and (p_in == 77).all() and (p_out == 77).all() and (sc == -7.0).all() and (hv == 7).all()
        mv, upd, _ = plan(H, hip, syn.v, syn.g, N_UTG, 0, MAX_N_SCM, MIN_N_R, MIN_D_F, want_rc=_lib.E_ARG)
        assert (mv == 9).all() and upd == -5
    finally:
        syn.close()
    syn = Synthetic(L, synthetic_reads())
    try:
        g, keep_g = hip._racov_graph(syn.graph)
        a, keep_a = hip._racov_aln(syn.aln)
        rc = hip.L.oatk_hip_ra_triplet_scores(hip.h, C.byref(g), C.byref(a), off.ctypes.data, len(WANT) - 1, C.byref(n), p_in.ctypes.data, p_out.ctypes.data,
                                              sc.ctypes.data, hv.ctypes.data)
        assert rc == _lib.E_NOMEM and n.value == len(WANT)
        assert (off == 77).all() and (p_in == 77).all() and (sc == -7.0).all() and (hv == 7).all()
        assert hip.L.oatk_hip_ra_triplet_scores(*args(16)) == 0 and n.value == len(WANT) and MX.same_doubles(sc[:len(WANT)], [x for _, x in WANT])
    finally:
        syn.close()


@needs_ref
def test_no_triplets_at_all(hip):
    """every record has fewer than three fragments: no pair has a score, nothing is dropped"""
    L, H = libs()
    reads = [[(sc, fr[:2]) for sc, fr in recs] for recs in synthetic_reads()]
    syn = Synthetic(L, reads)
    try:
        m = MX.model(syn.graph, syn.aln, MAX_N_SCM, MIN_N_R, MIN_D_F)
        got = hip.ra_triplet_scores(syn.graph, syn.aln)
        MX.assert_same_scores(got, m, "no triplets")
        assert len(got["have"]) == len(WANT) and not got["have"].any() and not got["score"].any()
        mv, upd, ent = plan(H, hip, syn.v, syn.g, N_UTG, 0, MAX_N_SCM, MIN_N_R, MIN_D_F)
        assert upd == 0 and ent == [] and list(mv) == [0] * 12 + [2, 0]
    finally:
        syn.close()
