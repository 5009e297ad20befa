"""The coverage estimates from read alignments (include/oatk_hip_racov.h, oatk_scg_ra_utg_coverage / oatk_scg_ra_arc_coverage of
include/oatk_syncasm.h): exported by both libraries, and without a device the adaptor returns an error and writes nothing -- there is no
CPU restatement to fall back on."""
import ctypes as C
import os

from oatk_amd import _lib

from racov_util import Arc, Asmg, Scg, Vtx

HIP_SYMS = ["oatk_hip_ra_utg_coverage", "oatk_hip_ra_arc_coverage", "oatk_hip_debug_racov_cap"]
HOST_SYMS = ["oatk_scg_ra_utg_coverage", "oatk_scg_ra_arc_coverage"]


def test_entry_points_are_exported():
    assert os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.HOST_LIB_PATH), "build with __graft_entry__.build()"
    L, H = C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.HOST_LIB_PATH)
    for n in HIP_SYMS:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n
    for n in HOST_SYMS:
        assert hasattr(H, n), n


def test_without_a_device_the_adaptor_refuses_and_writes_nothing():
    H = C.CDLL(_lib.HOST_LIB_PATH)
    L = _lib.load()
    vp = C.c_void_p
    for f in HOST_SYMS:
        getattr(H, f).argtypes = [vp, vp, vp, vp, C.c_uint, C.c_int]
    # a graph of two unitigs and one arc, covs set; the adaptor must leave them as they are
    vtx = (Vtx * 2)()
    arc = (Arc * 1)()
    a0 = (C.c_uint64 * 2)(2, 4)
    vtx[0].n, vtx[0].a, vtx[0].cov = 2, C.cast(a0, vp), 17
    vtx[1].n, vtx[1].a, vtx[1].cov = 2, C.cast(a0, vp), 23
    arc[0].v, arc[0].w, arc[0].cov = 0, 2, 9
    idx = (C.c_uint64 * 4)(0, 0, 0, 0)
    ag = Asmg(2, 2, C.cast(vtx, C.POINTER(Vtx)), 1, 1, C.cast(arc, C.POINTER(Arc)), C.cast(idx, vp), C.cast(idx, vp))
    g = Scg(None, C.pointer(ag), None, None)
    ra = (C.c_uint64 * 3)(0, 0, 0)          # oatk_scg_ra_v {n, m, a}: empty
    for f in HOST_SYMS:
        rc = getattr(H, f)(None, None, C.cast(ra, vp), C.cast(C.pointer(g), vp), 0, 0)
        assert rc == _lib.E_NODEV, (f, rc)
        assert (vtx[0].cov, vtx[1].cov, arc[0].cov) == (17, 23, 9), f
    # the device entry points themselves
    assert L.oatk_hip_ra_utg_coverage(None, None, None, None, 0, None, None) == _lib.E_NODEV
    assert L.oatk_hip_ra_arc_coverage(None, None, None, None) == _lib.E_NODEV
    assert L.oatk_hip_debug_racov_cap(None, 0) == _lib.E_NODEV
