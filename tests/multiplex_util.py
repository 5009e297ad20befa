"""A plain Python model of scg_multiplex up to its rewrite of the graph (syncasm.c:1110-1302) over flattened arrays, and the flattening of
the reference's scg_t / scg_ra_v through the layout mirrors of racov_util.py.  The spanning-triplet table is a dict keyed by (l0, l1),
updated in record order exactly as the reference's kh_dbl table is: a Python float is the same IEEE double, and every += rounds once."""
import ctypes as C
import math
import sys

import numpy as np

import align_util as AU
from racov_util import Scg

EPS = sys.float_info.epsilon


def flatten_graph(g):
    """scg_t of the compiled reference -> dict shaped like oatk_racov_graph_t (include/oatk_hip_racov.h), vtx_del included"""
    G = AU.ref_ra_graph(g)
    a = C.cast(g, C.POINTER(Scg)).contents.utg_asmg.contents
    nu, na = int(a.n_vtx), int(a.n_arc)
    lists = [np.frombuffer(C.string_at(a.vtx[i].a, 8 * a.vtx[i].n), np.uint64) if a.vtx[i].n else np.zeros(0, np.uint64) for i in range(nu)]
    out = {"n_scm": G["n_scm"], "su_off": G["su_off"], "su_uid": G["su_uid"], "su_pos": G["su_pos"], "scm_cov": np.zeros(G["n_scm"], np.uint32),
           "utg_off": np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64),
           "utg_a": np.concatenate(lists + [np.zeros(0, np.uint64)]).astype(np.uint64), "idx_p": G["idx_p"], "idx_n": G["idx_n"],
           "arc_v": np.array([a.arc[i].v for i in range(na)], np.uint64), "arc_w": np.array([a.arc[i].w for i in range(na)], np.uint64),
           "arc_link": np.array([a.arc[i].link_id for i in range(na)], np.uint64), "arc_comp": np.array([a.arc[i].comp for i in range(na)], np.uint8),
           "arc_del": np.array([a.arc[i].del_ for i in range(na)], np.uint8), "vtx_del": np.array([a.vtx[i].del_ for i in range(nu)], np.uint8)}
    return out


def flat_aln(f):
    """test_gpu_align.flatten's dict (per-record fragment counts) -> the dict of offsets the device binding takes"""
    return {"sid": f["sid"].astype(np.uint32), "off": np.concatenate([[0], np.cumsum(f["n"].astype(np.uint64))]).astype(np.uint64), "s": f["s"],
            "uid": f["uid"], "u_beg": f["u_beg"].astype(np.uint32), "u_end": f["u_end"].astype(np.uint32), "s_beg": f["s_beg"], "s_end": f["s_end"]}


class MissingArc(Exception):
    """two consecutive fragments without an arc: the reference dereferences NULL"""


def arc_id(G, x):
    return int(G["arc_link"][x]) << 1 | int(G["arc_comp"][x])


def comp_arc_id(G, x):
    v, w = int(G["arc_v"][x]), int(G["arc_w"][x])
    return arc_id(G, x) ^ 1 if (v ^ 1) != w or (w ^ 1) != v else arc_id(G, x)


def find_arc(G, v, w):
    """asmg_arc: the first arc v -> w in array order, deleted or not"""
    p, n = int(G["idx_p"][v]), int(G["idx_n"][v])
    for x in range(p, p + n):
        if int(G["arc_w"][x]) == w:
            return x
    raise MissingArc((v, w))


def triplet_table(G, aln, trace=None):
    """syncasm.c:1110-1166: {(l0, l1): double}; trace (a list) receives (record, key, mirror key, score) of every event"""
    su_n = np.diff(G["su_off"].astype(np.int64))
    utg_a, utg_off = G["utg_a"], G["utg_off"].astype(np.int64)
    uniq_pos = su_n[(utg_a >> np.uint64(1)).astype(np.int64)] == 1 if len(utg_a) else np.zeros(0, bool)
    tab = {}
    off = aln["off"].astype(np.int64)
    for i in range(len(aln["sid"])):
        f0, m = int(off[i]), int(off[i + 1] - off[i])
        if m < 3:
            continue
        score = math.modf(float(aln["s"][i]))[0]
        if score < EPS:
            score = 1.0
        uid = [int(x) for x in aln["uid"][f0:f0 + m]]
        if score < .99:
            uniq = []
            for j in range(m):
                b = int(utg_off[uid[j] >> 1])
                uniq.append(bool(uniq_pos[b + int(aln["u_beg"][f0 + j]):b + int(aln["u_end"][f0 + j]) + 1].any()))
        else:
            uniq = [True] * m
        x = find_arc(G, uid[0], uid[1])
        l0, c0 = arc_id(G, x), comp_arc_id(G, x)
        for j in range(2, m):
            x = find_arc(G, uid[j - 1], uid[j])
            l1, c1 = arc_id(G, x), comp_arc_id(G, x)
            if uniq[j - 2] and uniq[j - 1] and uniq[j]:
                A, M = (l0, l1), (c1, c0)
                if trace is not None:
                    trace.append((i, A, M, score))
                if A not in tab:
                    tab[A] = score
                    tab[M] = score
                else:
                    tab[A] += score
                    tab[M] = tab.get(M, 0.0) + score
            l0, c0 = l1, c1
    return tab


def live_arcs(G, v):
    p, n = int(G["idx_p"][v]), int(G["idx_n"][v])
    return [x for x in range(p, p + n) if not G["arc_del"][x]]


def decide(G, tab, max_n_scm, min_n_r, min_d_f):
    """syncasm.c:1181-1302: the pairs in lookup order with their scores, multi_vtx and updated"""
    nu = len(G["utg_off"]) - 1
    vtx_del = G.get("vtx_del", np.zeros(nu, np.uint8))
    pair_off, p_in, p_out, score, have = [0], [], [], [], []
    multi_vtx = np.zeros(nu, np.uint8)
    updated = 0
    for i in range(nu):
        if vtx_del[i]:
            pair_off.append(len(p_in))
            continue
        v1 = i << 1
        a_in, a_out = live_arcs(G, v1 ^ 1), live_arcs(G, v1)
        if not a_in and not a_out:
            multi_vtx[i] = 2
        if not a_in or not a_out:
            pair_off.append(len(p_in))
            continue
        l_in, l_out = [comp_arc_id(G, x) for x in a_in], [arc_id(G, x) for x in a_out]
        s_all = [[tab.get((li, lo), .001) for lo in l_out] for li in l_in]
        for li in l_in:
            for lo in l_out:
                p_in.append(li), p_out.append(lo), have.append(int((li, lo) in tab)), score.append(tab.get((li, lo), 0.0))
        pair_off.append(len(p_in))
        s_in = [max([.0] + row) for row in s_all]
        s_out = [max([.0] + [row[t] for row in s_all]) for t in range(len(l_out))]
        s_max = max([.0] + s_in)
        loop = any(int(G["arc_w"][x]) == v1 for x in a_out)
        n_scm = int(G["utg_off"][i + 1]) - int(G["utg_off"][i])
        if n_scm > max_n_scm or loop or s_max < min_n_r:
            continue
        for s in range(len(l_in)):
            for t in range(len(l_out)):
                if s_all[s][t] / s_in[s] < min_d_f and s_all[s][t] / s_out[t] < min_d_f:
                    updated += 1
        multi_vtx[i] = 1
    return {"pair_off": np.array(pair_off, np.uint64), "pair_in": np.array(p_in, np.uint64), "pair_out": np.array(p_out, np.uint64),
            "score": np.array(score, np.float64), "have": np.array(have, np.uint8), "multi_vtx": multi_vtx, "updated": updated}


def model(G, aln, max_n_scm, min_n_r, min_d_f):
    return decide(G, triplet_table(G, aln), max_n_scm, min_n_r, min_d_f)


def triplet_records(aln):
    n = np.diff(aln["off"].astype(np.int64))
    return int((n >= 3).sum()), int(np.maximum(n - 2, 0).sum())


def same_doubles(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same_scores(got, want, what):
    for k in ("pair_off", "pair_in", "pair_out", "have"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k][:20], want[k][:20])
    assert same_doubles(got["score"], want["score"]), (what, "score", np.flatnonzero(got["score"] != want["score"])[:10])
