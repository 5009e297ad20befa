"""The coverage estimates from read alignments over several handles (include/oatk_hip_racov.h: oatk_hip_ra_*_coverage_sharded;
include/oatk_multi.h: oatk_multi_scg_ra_*_coverage): exported by the two libraries, listed by the Python binding, and without a device or
without handles they return an error and write nothing."""
import ctypes as C
import os

from oatk_amd import _lib

from racov_util import Arc, Asmg, Scg, Vtx

HIP_SYMS = ["oatk_hip_ra_utg_coverage_sharded", "oatk_hip_ra_arc_coverage_sharded"]
HOST_SYMS = ["oatk_multi_scg_ra_utg_coverage", "oatk_multi_scg_ra_arc_coverage"]


def test_entry_points_are_exported():
    assert os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.HOST_LIB_PATH), "build with __graft_entry__.build()"
    L, H = C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.HOST_LIB_PATH)
    for n in HIP_SYMS:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n
    for n in HOST_SYMS:
        assert hasattr(H, n), n
        assert n in _lib.HOST_EXPORTS, n


def test_the_binding_has_the_sharded_methods():
    from oatk_amd import HipSyncasm
    assert callable(HipSyncasm.ra_utg_coverage_sharded) and callable(HipSyncasm.ra_arc_coverage_sharded)


def test_without_handles_the_calls_refuse_and_write_nothing():
    H = _lib.load_host()                    # declares the argtypes of the N-handle calls
    L = _lib.load()
    vp = C.c_void_p
    for f in HOST_SYMS:
        assert getattr(H, f).argtypes == [vp, vp, vp, vp, C.c_int], f
    # a graph of two unitigs and one arc, covs set; the calls must leave them as they are
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
        rc = getattr(H, f)(None, None, C.cast(ra, vp), C.cast(C.pointer(g), vp), 0)
        assert rc == _lib.E_NODEV, (f, rc)
        assert (vtx[0].cov, vtx[1].cov, arc[0].cov) == (17, 23, 9), f
    # the device entry points themselves: no handle, whatever the communicator
    out = (C.c_double * 2)(1.5, 2.5)
    it = C.c_uint64(7)
    assert L.oatk_hip_ra_utg_coverage_sharded(None, None, None, None, None, 0, C.cast(out, vp), C.byref(it)) == _lib.E_NODEV
    assert L.oatk_hip_ra_arc_coverage_sharded(None, None, None, None, C.cast(out, vp)) == _lib.E_NODEV
    assert (out[0], out[1], it.value) == (1.5, 2.5, 7)


def test_the_synthetic_set_admits_cuts_where_the_boundary_matters():
    """CPU arithmetic on the read list of tests/test_gpu_racov.py, by the reference's rules: cuts by read exist that split a unitig's fractional
    (multi-member-block) contributions, a link's duplets, and the self-complementary arc's first event from a later one -- tests/test_gpu_racov_sharded.py
    runs every cut and asserts that it met them"""
    import racov_sharded_util as T
    reads = T.RC.synthetic_reads()
    facts = [T.boundary_facts(reads, b) for b in range(len(reads) + 1)]
    assert any(f[0] for f in facts) and any(f[1] for f in facts) and any(f[2] for f in facts)
    assert [b for b, f in enumerate(facts) if f[2]] == [146, 147]            # the three reads over the self-complementary arc are 145, 146, 147
