"""The corrected reads' sequences (include/oatk_hip_ec.h: oatk_hip_ec_keep_seq, oatk_hip_ec_corrected_reads and the EC_CSEQ buffers; include/oatk_syncasm.h:
oatk_read_error_correction_fo): exported, listed, and without a device they answer OATK_E_NODEV -- there is no CPU restatement to fall back on.  The ABI version
stays what tests/test_abi.py pins."""
import ctypes as C
import os
import re

from oatk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_SYMS = ["oatk_hip_ec_keep_seq", "oatk_hip_ec_corrected_reads"]
HOST_SYMS = ["oatk_read_error_correction_fo", "oatk_read_error_correction"]
BUFS = ["EC_CSEQ_LEN", "EC_CSEQ_OFF", "EC_CSEQ", "EC_BLOCK_QEND"]


def test_entry_points_are_exported_and_listed():
    assert os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.HOST_LIB_PATH), "build with __graft_entry__.build()"
    L, H = C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.HOST_LIB_PATH)
    for n in HIP_SYMS:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n
    for n in HOST_SYMS:
        assert hasattr(H, n), n


def test_buffer_ids_follow_block_out():
    """the ids the header's enum gives the new buffers are the ones the Python side uses, right behind OATK_BUF_EC_BLOCK_OUT"""
    hdr = open(os.path.join(ROOT, "include", "oatk_hip_ec.h")).read()
    body = re.search(r"enum \{\s*OATK_BUF_EC_N_SCM = 100,(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = ["EC_N_SCM"] + [x.strip()[len("OATK_BUF_"):] for x in body.split(",") if x.strip()]
    assert names[-5:] == ["EC_BLOCK_OUT"] + BUFS
    for i, n in enumerate(names):
        assert _lib.BUF[n] == 100 + i, n
    from oatk_amd import device
    for n in BUFS:
        assert n in device._DTYPES, n


def test_without_a_device_they_refuse():
    L, H = _lib.load(), C.CDLL(_lib.HOST_LIB_PATH)
    assert L.oatk_hip_ec_keep_seq(None, 1) == _lib.E_NODEV
    n = C.c_uint64(7)
    assert L.oatk_hip_ec_corrected_reads(None, C.byref(n)) == _lib.E_NODEV and n.value == 7
    vp = C.c_void_p
    H.oatk_read_error_correction_fo.argtypes = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, vp, vp]
    assert H.oatk_read_error_correction_fo(None, None, None, None, 0.02, 3, 30, 3, 0.35, None, None) == _lib.E_NODEV
