"""The Python model of scg_multiplex's decisions (tests/multiplex_util.py) pinned to the COMPILED REFERENCE: the reference's own pipeline up to
the unzip rounds on the two read sets of the committed alignment vectors, and before every scg_multiplex the graph and the alignments are
flattened and the model's `updated` must be what the reference then returns.  No device takes part."""
import ctypes as C
import math

import pytest

import ec_util as E
import multiplex_util as MX
import ref_lib as R
import test_gpu_align as GA
from test_oracle_align import ref_flatten

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")


def reference_rounds(reads, K, S, c, max_rounds=3):
    """[(flattened graph, flattened alignments, the reference's scg_multiplex return value)] of the unzip rounds (run_syncasm.c:219-232)"""
    L = R.lib()
    vp = C.c_void_p
    L.refx_ra_new.restype = vp
    L.refx_ra_destroy.argtypes = [vp]
    L.refx_read_alignment.argtypes = [vp, vp, vp, C.c_int, C.c_int]
    L.refx_process_unitigs.argtypes = [vp]
    L.refx_update_utg_cov.argtypes = [vp]
    L.refx_multiplex.argtypes = [vp, vp, C.c_uint32, C.c_double, C.c_double]
    db = R.SrDb.from_reads(reads, K, S, threads=2)
    scm = R.ScmDb(db)
    g, _ = E.ref_graph(db, scm)
    E.reference_ec(db, scm, g, 0.02, c, 0.35)
    L.refx_scg_destroy(g)
    g = L.refx_make_graph(db.handle, scm.handle, c, 0.35)
    v = L.refx_ra_new()
    L.refx_read_alignment(db.handle, v, g, 3, 0)
    L.refx_process_unitigs(g)
    L.refx_read_alignment(db.handle, v, g, 3, 0)
    rounds = []
    for _ in range(max_rounds):
        L.refx_read_alignment(db.handle, v, g, 3, 1)
        L.refx_update_utg_cov(g)
        graph, aln = MX.flatten_graph(g), MX.flat_aln(ref_flatten(L, v))
        updated = L.refx_multiplex(g, v, int(math.ceil(30000.0 / K)), 10.0, 0.3)
        rounds.append((graph, aln, updated))
        if updated == 0:
            break
    L.refx_ra_destroy(v)
    L.refx_scg_destroy(g)
    scm.close()
    db.close()
    return rounds


# records of three or more fragments and triplet slots per unzip round, as counted from tests/golden/align_*.npz
EXPECT = {"align_diploid_k101": [(304, 1425)], "align_repeats_k301": [(109, 248), (66, 66)]}


@needs_ref
@pytest.mark.parametrize("case", sorted(GA.GOLDEN))
def test_model_updated_equals_the_reference(case):
    K, S, c, mk = GA.GOLDEN[case]
    rounds = reference_rounds(mk(), K, S, c)
    assert len(rounds) >= len(EXPECT[case])
    for r, (graph, aln, updated) in enumerate(rounds):
        m = MX.model(graph, aln, int(math.ceil(30000.0 / K)), 10.0, 0.3)
        n_rec, n_slot = MX.triplet_records(aln)
        print(case, "round", r, "records >= 3 fragments", n_rec, "slots", n_slot, "pairs", len(m["have"]), "with a score", int(m["have"].sum()),
              "updated", updated, "model", m["updated"])
        assert m["updated"] == updated, (case, r)
        if r < len(EXPECT[case]):
            assert (n_rec, n_slot) == EXPECT[case][r], (case, r)
            assert n_rec > 0 and updated > 0 and m["have"].sum() > 0, (case, r)
