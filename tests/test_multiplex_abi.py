"""The spanning-triplet scores of scg_multiplex (include/oatk_hip_racov.h: oatk_hip_ra_triplet_scores[_sharded]; include/oatk_syncasm.h:
oatk_scg_multiplex_plan; include/oatk_multi.h: oatk_multi_scg_multiplex_plan): exported by the two libraries with the declared signatures,
listed by the Python binding, and without a device or without handles they return an error and write nothing."""
import ctypes as C
import os
import re

import numpy as np

from oatk_amd import _lib

import multiplex_util as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_SYMS = ["oatk_hip_ra_triplet_scores", "oatk_hip_ra_triplet_scores_sharded"]
HOST_SYMS = ["oatk_scg_multiplex_plan", "oatk_multi_scg_multiplex_plan", "oatk_triplet_table_free"]


def test_entry_points_are_exported():
    assert os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.HOST_LIB_PATH), "build with __graft_entry__.build()"
    L, H = C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.HOST_LIB_PATH)
    for n in HIP_SYMS:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n
    for n in HOST_SYMS:
        assert hasattr(H, n), n
        assert n in _lib.HOST_EXPORTS, n


def declared(header, name):
    """the parameter types of `name` as the header declares them, spaces and parameter names dropped"""
    src = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"\b%s\(([^;]*?)\);" % name, src, re.S)
    assert m, (header, name)
    out = []
    for p in m.group(1).split(","):
        p = re.sub(r"/\*.*?\*/", "", p, flags=re.S).strip()
        t = re.sub(r"\b\w+$", "", p).strip()              # drop the parameter's name
        out.append(re.sub(r"\s+", " ", t).replace(" *", "*"))
    return out


CTYPE = {"oatk_hip_ctx*": C.c_void_p, "oatk_comm*": C.c_void_p, "oatk_multi*": C.c_void_p, "const oatk_scg_ra_v*": C.c_void_p, "const oatk_scg_t*": C.c_void_p,
         "const oatk_racov_graph_t*": C.POINTER(_lib.RacovGraph), "const oatk_racov_aln_t*": C.POINTER(_lib.RacovAln), "uint64_t": C.c_uint64,
         "unsigned": C.c_uint, "uint32_t": C.c_uint32, "double": C.c_double, "int*": C.POINTER(C.c_int), "oatk_triplet_table*": C.POINTER(_lib.TripletTable)}
PLAIN = {"uint64_t*": (C.c_void_p, C.POINTER(C.c_uint64)), "double*": (C.c_void_p, ), "uint8_t*": (C.c_void_p, )}


def test_the_binding_declares_the_headers_signatures():
    L, H = _lib.load(), _lib.load_host()
    for lib, header, name in ((L, "oatk_hip_racov.h", "oatk_hip_ra_triplet_scores"), (L, "oatk_hip_racov.h", "oatk_hip_ra_triplet_scores_sharded"),
                              (H, "oatk_syncasm.h", "oatk_scg_multiplex_plan"), (H, "oatk_multi.h", "oatk_multi_scg_multiplex_plan")):
        want, got = declared(header, name), getattr(lib, name).argtypes
        assert len(want) == len(got), (name, want, got)
        for w, t in zip(want, got):
            assert t in PLAIN[w] if w in PLAIN else t is CTYPE[w] or t == CTYPE[w], (name, w, t)
    # the graph struct ends with the unitigs' del flags, after everything the coverage calls read
    assert _lib.RacovGraph._fields_[-1][0] == "vtx_del" and _lib.RacovGraph._fields_[-2][0] == "arc_del"
    assert C.sizeof(_lib.RacovGraph) == 8 * 17


def test_the_binding_has_the_methods():
    from oatk_amd import HipSyncasm
    assert callable(HipSyncasm.ra_triplet_scores) and callable(HipSyncasm.ra_triplet_scores_sharded)


def test_without_a_device_the_calls_refuse_and_write_nothing():
    L, H = _lib.load(), _lib.load_host()
    off, n = np.full(4, 77, np.uint64), C.c_uint64(99)
    buf = np.full(4, 77, np.uint64)
    sc, hv = np.full(4, -7.0), np.full(4, 7, np.uint8)
    assert L.oatk_hip_ra_triplet_scores(None, None, None, off.ctypes.data, 4, C.byref(n), buf.ctypes.data, buf.ctypes.data, sc.ctypes.data, hv.ctypes.data) == _lib.E_NODEV
    assert L.oatk_hip_ra_triplet_scores_sharded(None, None, None, None, off.ctypes.data, 4, C.byref(n), buf.ctypes.data, buf.ctypes.data, sc.ctypes.data,
                                                hv.ctypes.data) == _lib.E_NODEV
    mv, upd = np.full(4, 9, np.uint8), C.c_int(-5)
    assert H.oatk_scg_multiplex_plan(None, None, None, 0, 20, 10.0, 0.3, mv.ctypes.data, C.byref(upd), None) == _lib.E_NODEV
    assert H.oatk_multi_scg_multiplex_plan(None, None, None, 20, 10.0, 0.3, mv.ctypes.data, C.byref(upd), None) == _lib.E_NODEV
    assert n.value == 99 and (off == 77).all() and (buf == 77).all() and (sc == -7.0).all() and (hv == 7).all() and (mv == 9).all() and upd.value == -5


def test_the_model_on_a_two_arc_graph():
    """A+ -> B+ -> C+ with complements, three reads across it: the model's table, pairs and marks, worked by hand"""
    arcs = sorted([(0, 2, 0, 0), (3, 1, 0, 1), (2, 4, 1, 0), (5, 3, 1, 1)])
    idx_p, idx_n = np.zeros(6, np.uint64), np.zeros(6, np.uint64)
    for i, a in enumerate(arcs):
        if idx_n[a[0]] == 0:
            idx_p[a[0]] = i
        idx_n[a[0]] += 1
    G = {"n_scm": 6, "su_off": np.arange(7, dtype=np.uint64), "su_uid": np.array([0, 0, 2, 2, 4, 4], np.uint64), "su_pos": np.array([0, 1] * 3, np.uint32),
         "utg_off": np.array([0, 2, 4, 6], np.uint64), "utg_a": np.arange(6, dtype=np.uint64) << np.uint64(1), "idx_p": idx_p, "idx_n": idx_n,
         "arc_v": np.array([a[0] for a in arcs], np.uint64), "arc_w": np.array([a[1] for a in arcs], np.uint64),
         "arc_link": np.array([a[2] for a in arcs], np.uint64), "arc_comp": np.array([a[3] for a in arcs], np.uint8), "arc_del": np.zeros(4, np.uint8)}
    aln = {"sid": np.arange(3, dtype=np.uint32), "off": np.array([0, 3, 6, 8], np.uint64), "s": np.array([6.0, 6.5, 4.0]),
           "uid": np.array([0, 2, 4, 5, 3, 1, 0, 2], np.uint64), "u_beg": np.zeros(8, np.uint32), "u_end": np.ones(8, np.uint32)}
    tab = MX.triplet_table(G, aln)
    assert tab == {(0, 2): 1.5, (3, 1): 1.5}
    m = MX.decide(G, tab, 20, 1.5, 0.3)
    assert m["pair_off"].tolist() == [0, 0, 1, 1] and (m["pair_in"].tolist(), m["pair_out"].tolist(), m["score"].tolist()) == ([0], [2], [1.5])
    assert m["multi_vtx"].tolist() == [0, 1, 0] and m["updated"] == 0
    assert MX.decide(G, tab, 20, 1.6, 0.3)["multi_vtx"].tolist() == [0, 0, 0]
