"""The strings of scg_consensus for reads sharded over several handles (include/oatk_hip_multi.h: oatk_hip_consensus_strings_sharded; include/oatk_multi.h:
oatk_multi_consensus, oatk_multi_scg_consensus): exported, declared, listed with their signatures; the new buffer id is the header's and no other buffer's; and
without a device the calls refuse and write nothing -- there is no CPU restatement to fall back on.  The ABI version stays what tests/test_abi.py pins."""
import ctypes as C
import os
import re

from oatk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header, name):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert decl, "%s is not declared in include/%s" % (name, header)
    return [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]


def test_entry_points_are_exported_declared_and_listed():
    assert os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.HOST_LIB_PATH), "build with __graft_entry__.build()"
    L, H = C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.HOST_LIB_PATH)
    for n in ("oatk_hip_consensus_strings_sharded", "oatk_hip_consensus_kmer_time"):
        assert hasattr(L, n) and n in _lib.EXPORTS, n
    for n in ("oatk_multi_consensus", "oatk_multi_scg_consensus"):
        assert hasattr(H, n) and n in _lib.HOST_EXPORTS, n
    a = declared("oatk_hip_multi.h", "oatk_hip_consensus_strings_sharded")
    assert len(a) == 6 and a[0].startswith("oatk_hip_ctx *") and a[1].startswith("oatk_comm *") and a[2].startswith("const oatk_cons_plan_t *") and a[3].startswith("int ")
    assert len(_lib.load().oatk_hip_consensus_strings_sharded.argtypes) == 6
    a = declared("oatk_multi.h", "oatk_multi_scg_consensus")
    one = declared("oatk_syncasm.h", "oatk_scg_consensus")
    names = lambda args: [x.split()[-1].lstrip("*") for x in args]                      # noqa: E731
    assert len(a) == 7 and a[0].startswith("oatk_multi *") and names(a)[1:] == names(one)[1:]      # oatk_scg_consensus' arguments behind the handles
    assert a[1].startswith("const oatk_overlap_t *") and a[6].startswith("FILE *")
    assert len(_lib.load_host().oatk_multi_scg_consensus.argtypes) == 7
    assert declared("oatk_multi.h", "oatk_multi_consensus") == ["oatk_multi *m", "uint32_t min_cov"]


def test_the_buffer_id_is_the_headers_and_nobody_elses():
    hdr = open(os.path.join(ROOT, "include", "oatk_hip_multi.h")).read()
    m = re.search(r"OATK_BUF_CONS_KMER\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.BUF["CONS_KMER"]
    ids = sorted(_lib.BUF.values())
    assert len(ids) == len(set(ids))
    from oatk_amd import device
    assert device._DTYPES["CONS_KMER"] == device.np.uint8


def test_without_a_device_they_refuse_and_write_nothing(tmp_path):
    L, H = _lib.load(), _lib.load_host()
    tot, ref = C.c_uint64(7), C.c_uint64(7)
    assert L.oatk_hip_consensus_strings_sharded(None, None, None, 0, C.byref(tot), C.byref(ref)) == _lib.E_NODEV
    assert (tot.value, ref.value) == (7, 7)
    assert L.oatk_hip_consensus_kmer_time(None, None, None) == _lib.E_NODEV
    assert H.oatk_multi_consensus(None, 4) == _lib.E_NODEV
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    path = tmp_path / "out.gfa"
    fo = libc.fopen(str(path).encode(), b"w")
    assert fo
    try:
        assert H.oatk_multi_scg_consensus(None, None, None, None, 0, 1, fo) == _lib.E_ARG      # (as oatk_scg_consensus answers missing arguments)
    finally:
        libc.fclose(fo)
    assert os.path.getsize(path) == 0


def test_abi_version_is_unchanged():
    assert _lib.load().oatk_hip_abi_version() == 1
