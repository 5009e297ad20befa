"""The mini-circle repeat units (include/oatk_hip_racov.h: oatk_hip_ra_minicircle_units, oatk_hip_ra_minicircle_times, oatk_hip_debug_mc_hash_bits;
include/oatk_syncasm.h: oatk_extract_minicircles, oatk_mc_path_stats, oatk_mc_paths_free): exported by the two libraries with the declared signatures,
listed by the Python binding with the four buffer ids the header declares, and without a device they return an error and write nothing."""
import ctypes as C
import os
import re

import numpy as np

from oatk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_SYMS = ["oatk_hip_ra_minicircle_units", "oatk_hip_ra_minicircle_times", "oatk_hip_debug_mc_hash_bits"]
HOST_SYMS = ["oatk_extract_minicircles", "oatk_mc_path_stats", "oatk_mc_paths_free"]
BUFS = ["MC_UNIT", "MC_PATH_OFF", "MC_PATH_V", "MC_PATH_CNT"]


def test_entry_points_are_exported():
    assert os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.HOST_LIB_PATH), "build with __graft_entry__.build()"
    L, H = C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.HOST_LIB_PATH)
    for n in HIP_SYMS:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n
    for n in HOST_SYMS:
        assert hasattr(H, n), n
        assert n in _lib.HOST_EXPORTS, n


def test_the_header_declares_the_four_buffer_ids_and_the_binding_has_them():
    src = open(os.path.join(ROOT, "include", "oatk_hip_racov.h")).read()
    m = re.search(r"enum\s*\{\s*OATK_BUF_MC_UNIT\s*=\s*(\d+)\s*,\s*OATK_BUF_MC_PATH_OFF\s*,\s*OATK_BUF_MC_PATH_V\s*,\s*OATK_BUF_MC_PATH_CNT\s*\}", src)
    assert m, "enum { OATK_BUF_MC_UNIT = ..., OATK_BUF_MC_PATH_OFF, OATK_BUF_MC_PATH_V, OATK_BUF_MC_PATH_CNT }"
    base = int(m.group(1))
    assert [_lib.BUF[b] for b in BUFS] == [base, base + 1, base + 2, base + 3]
    others = [v for k, v in _lib.BUF.items() if k not in BUFS]
    assert not set(range(base, base + 4)) & set(others), "the ids are taken"
    from oatk_amd import device
    assert [np.dtype(device._DTYPES[b]).itemsize for b in BUFS] == [8, 8, 4, 8]


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


CTYPE = {"oatk_hip_ctx*": (C.c_void_p, ), "const oatk_scg_ra_v*": (C.c_void_p, ), "const oatk_scg_t*": (C.c_void_p, ), "const oatk_asmg_t*": (C.c_void_p, ),
         "const oatk_racov_aln_t*": (C.POINTER(_lib.RacovAln), ), "uint64_t": (C.c_uint64, ), "unsigned": (C.c_uint, ), "uint64_t*": (C.POINTER(C.c_uint64), ),
         "float*": (C.POINTER(C.c_float), ), "oatk_mc_paths*": (C.POINTER(_lib.McPaths), )}


def test_the_binding_declares_the_headers_signatures():
    L, H = _lib.load(), _lib.load_host()
    for lib, header, name in [(L, "oatk_hip_racov.h", n) for n in HIP_SYMS] + [(H, "oatk_syncasm.h", n) for n in HOST_SYMS]:
        want, got = declared(header, name), getattr(lib, name).argtypes
        assert len(want) == len(got), (name, want, got)
        for w, t in zip(want, got):
            assert any(t is c or t == c for c in CTYPE[w]), (name, w, t)
    # oatk_mc_path: nv, v, len, wlen, cnt as the C compiler lays them out (4 + pad, 8, 4 + pad, 8, 8)
    assert [f[0] for f in _lib.McPath._fields_] == ["nv", "v", "len", "wlen", "cnt"] and C.sizeof(_lib.McPath) == 40 and C.sizeof(_lib.McPaths) == 24


def test_the_binding_has_the_method():
    from oatk_amd import HipSyncasm
    assert callable(HipSyncasm.ra_minicircle_units) and callable(HipSyncasm.debug_mc_hash_bits)


def test_without_a_device_the_calls_refuse_and_write_nothing():
    L, H = _lib.load(), _lib.load_host()
    n = [C.c_uint64(99), C.c_uint64(98), C.c_uint64(97)]
    assert L.oatk_hip_ra_minicircle_units(None, None, 5, C.byref(n[0]), C.byref(n[1]), C.byref(n[2])) == _lib.E_NODEV
    assert L.oatk_hip_debug_mc_hash_bits(None, 8) == _lib.E_NODEV
    assert L.oatk_hip_ra_minicircle_times(None, None, None) == _lib.E_NODEV
    out = _lib.McPaths(7, 7, None)
    assert H.oatk_extract_minicircles(None, None, None, 5, 0, C.byref(out)) == _lib.E_NODEV
    assert [x.value for x in n] == [99, 98, 97] and out.n == 7 and out.m == 7
    H.oatk_mc_paths_free(None)                     # a no-op
    assert H.oatk_mc_path_stats(None, C.byref(out)) == _lib.E_ARG
