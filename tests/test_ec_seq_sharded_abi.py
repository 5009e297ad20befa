"""The corrected reads' sequences over several handles (include/oatk_multi.h: oatk_multi_read_error_correction_fo): exported, declared, listed with its
signature, and without a device it answers OATK_E_NODEV and writes nothing -- there is no CPU restatement to fall back on.  The ABI version stays what
tests/test_abi.py pins: the device entry points are the ones a single handle has, and no buffer id is new."""
import ctypes as C
import os
import re

from oatk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "oatk_multi_read_error_correction_fo"


def test_entry_point_is_exported_declared_and_listed():
    assert os.path.exists(_lib.HOST_LIB_PATH), "build with __graft_entry__.build()"
    H = C.CDLL(_lib.HOST_LIB_PATH)
    assert hasattr(H, SYM) and hasattr(H, "oatk_multi_read_error_correction")
    hdr = open(os.path.join(ROOT, "include", "oatk_multi.h")).read()
    decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % SYM, hdr)
    assert decl, "not declared in include/oatk_multi.h"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 10 and args[0].startswith("oatk_multi *") and args[8].startswith("FILE *") and args[9].startswith("uint64_t *")
    assert SYM in _lib.HOST_EXPORTS
    assert len(_lib.load_host().oatk_multi_read_error_correction_fo.argtypes) == 10


def test_without_a_device_it_refuses_and_writes_nothing(tmp_path):
    H = _lib.load_host()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    path = tmp_path / "out.fo"
    fo = libc.fopen(str(path).encode(), b"w")
    assert fo
    try:
        assert H.oatk_multi_read_error_correction_fo(None, None, None, 0.02, 3, 30, 3, 0.35, fo, None) == _lib.E_NODEV
        assert H.oatk_multi_read_error_correction_fo(None, None, None, 0.02, 3, 30, 3, 0.35, None, None) == _lib.E_NODEV
    finally:
        libc.fclose(fo)
    assert os.path.getsize(path) == 0


def test_abi_version_is_unchanged():
    assert _lib.load().oatk_hip_abi_version() == 1
