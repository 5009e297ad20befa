"""CPU: the C-ABI libraries load and export every symbol their headers declare (no compute: there is no GPU here)."""
import ctypes
import os
import re

import pytest

from oatk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header, prefix):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % prefix, txt)))


def test_hip_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = sum((declared(h, "oatk_hip_") for h in sorted(os.listdir(os.path.join(ROOT, "include"))) if h.startswith("oatk_hip")), [])   # one library
    names += declared("oatk_hip_multi.h", "oatk_comm_")
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), n
    assert set(_lib.EXPORTS) <= set(names)
    assert L.oatk_hip_abi_version() == 1


def test_host_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.HOST_LIB_PATH)
    L = ctypes.CDLL(_lib.HOST_LIB_PATH)
    # (oatk_dropin.h belongs to the static archive that is linked into the CLI: tests/test_cli_fallback.py checks its symbols)
    for hdr in [h for h in os.listdir(os.path.join(ROOT, "include")) if h not in ("oatk_hip.h", "oatk_dropin.h") and h.endswith(".h")]:
        for n in declared(hdr, "oatk_"):
            if n.startswith("oatk_hip_") or n.startswith("oatk_comm_"):
                continue
            assert hasattr(L, n), (hdr, n)


def test_no_silent_fallback_without_a_gpu():
    """without a device the product path raises; it never computes on the CPU"""
    L = _lib.load()
    if L.oatk_hip_device_count() > 0:
        pytest.skip("a GPU is visible")
    from oatk_amd import HipSyncasm, OatkHipError
    with pytest.raises(OatkHipError):
        HipSyncasm(0)


def test_product_does_not_import_the_oracle():
    """only tests/, bench.py's cpu_baseline leg and __graft_entry__.smoke may touch oracle/"""
    for base, _, files in list(os.walk(os.path.join(ROOT, "oatk_amd"))) + list(os.walk(os.path.join(ROOT, "tools"))) + list(os.walk(os.path.join(ROOT, "include"))):
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hip", ".hpp", ".inc", ".sh")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                assert "oracle_lib" not in txt and "ref_lib" not in txt and "liboatk_oracle" not in txt and "oracle/" not in txt, f


def test_the_scale_model_of_bench_is_plain_arithmetic_on_its_inputs():
    """bench.py `scale_model`: the predicted strong-scaling step is compute(reads / N) + latencies + bytes over links -- more GPUs
    never predict a slower compute part, what is predicted is printed with its parts, and the parts add up."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    tr1, tr8 = [40, 3000, 6, 5 * 10**8, 8, 4 * 10**8, 6, 12 * 10**8], [40, 3000, 6, 7 * 10**7, 8, 39 * 10**7, 6, 15 * 10**7]
    m = b.scale_model(2_000_000, 95.0, tr1, 250_000, 14.0, tr8, 30 * 10**9, 90.0)
    assert m["measured"]["collectives_per_step"] == 60
    prev = None
    for n in ("2", "4", "8"):
        p = m["predicted"][n]
        assert abs(sum(p["parts_ms"].values()) - p["ms_per_step"]) < 0.02
        assert prev is None or p["parts_ms"]["compute"] < prev
        prev = p["parts_ms"]["compute"]
        assert abs(p["speedup_over_1"] - 90.0 / p["ms_per_step"]) < 0.01


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_a_plain_bench_run_measures_the_headline_only(monkeypatch):
    """bench.py without --full leaves every leg beyond the headline out; --full brings them back, and --no-extras / --no-cpu-baseline still narrow it"""
    import sys
    b = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "1"])
    a = b.parse_args()
    assert (a.full, a.no_extras, a.no_cpu_baseline, a.steps, a.warmup, a.dump_outputs) == (False, True, True, 3, 1, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = b.parse_args()
    assert (a.full, a.no_extras, a.no_cpu_baseline, a.dump_outputs) == (True, False, False, "d")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    a = b.parse_args()
    assert (a.no_extras, a.no_cpu_baseline) == (False, True)


def test_bench_dump_outputs_are_exact_float64_and_repeatable(tmp_path):
    """--dump-outputs: float64 files that hold every value exactly (u64 hashes as two halves), the same sample on every run, within 64 MB"""
    import numpy as np
    b = _bench_module()
    rng = np.random.default_rng(5)
    n_reads, n_vtx = 20000, 3000
    n = rng.integers(0, 40, n_reads).astype(np.uint32)
    off = np.zeros(n_reads + 1, np.uint64)
    off[1:] = np.cumsum(n)
    tot = int(off[-1])
    bufs = {"EC_N_SCM": n, "EC_SCM_OFF": off, "EC_KMER": (rng.integers(0, n_vtx, tot).astype(np.uint64) << np.uint64(1)) | np.uint64(1),
            "EC_MPOS": rng.integers(0, 1 << 31, tot).astype(np.uint32), "EC_SMER": rng.integers(0, 1 << 63, tot, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
            "EC_SCM_COV": rng.integers(0, 100, n_vtx).astype(np.uint32), "EC_SCM_DEL": rng.integers(0, 2, n_vtx).astype(np.uint8)}

    class FakeHip:
        def sync(self):
            pass

        def fetch(self, name):
            return bufs[name].copy()
    st = np.arange(12, dtype=np.uint64)
    b.dump_outputs(FakeHip(), st, str(tmp_path / "a"))
    b.dump_outputs(FakeHip(), st, str(tmp_path / "b"))
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(os.listdir(str(tmp_path / "b"))) and "ec_stats.npy" in names and "ec_n_scm.npy" in names
    total = 0
    for f in names:
        x, y = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert x.dtype == np.float64 and np.array_equal(x, y), f
        total += x.nbytes
    assert total <= 64 << 20
    ld = lambda f: np.load(str(tmp_path / "a" / (f + ".npy")))      # noqa: E731
    reads = ld("sample_reads").astype(np.int64)
    assert len(reads) == b.DUMP_SAMPLE_READS and np.all(np.diff(reads) > 0)
    idx = np.concatenate([np.arange(int(off[r]), int(off[r + 1])) for r in reads])
    smer = (ld("sample_smer_hi").astype(np.uint64) << np.uint64(32)) | ld("sample_smer_lo").astype(np.uint64)
    assert np.array_equal(smer, bufs["EC_SMER"][idx])
    assert np.array_equal(ld("sample_kmer").astype(np.uint64), bufs["EC_KMER"][idx])
    assert np.array_equal(ld("ec_n_scm"), n.astype(np.float64)) and np.array_equal(ld("ec_stats"), st.astype(np.float64))
    assert np.array_equal(ld("scm_cov"), bufs["EC_SCM_COV"].astype(np.float64))     # a small table goes whole
