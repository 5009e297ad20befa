"""CPU: the Python model of extract_minicircles_with_anchor (tests/minicircle_util.py) reproduces, literally, the cases derived by hand from
path_finder.c:545-693 with anchor 5 (A+ = 10, A- = 11, B = 14/15, C = 18/19): every record's unit and path, and the distinct paths of the whole
table in path_cmpfunc order with their multiplicities.  The statistics of :696-727 on a hand-computed three-unitig graph."""
import numpy as np
import pytest

import minicircle_util as MC


@pytest.mark.parametrize("uids,unit,path", MC.TABLE, ids=["-".join(map(str, r[0])) or "empty" for r in MC.TABLE])
def test_the_record_gives_the_unit_and_path_of_the_table(uids, unit, path):
    mc = MC.unit_of(uids, MC.ANCHOR)
    if unit is None:
        assert mc == MC.NONE
        return
    beg, end, rev = unit
    assert mc == (beg << 33 | end << 1 | rev)
    assert MC.path_of(uids, mc) == path


def test_the_distinct_paths_of_the_whole_table():
    off, uid = MC.flat_records([r[0] for r in MC.TABLE])
    mcs, paths, cnt = MC.extract(off, uid, MC.ANCHOR)
    assert [int(x) for x in mcs] == [MC.NONE if r[1] is None else (r[1][0] << 33 | r[1][1] << 1 | r[1][2]) for r in MC.TABLE]
    assert list(zip(paths, cnt)) == MC.TABLE_PATHS


def test_the_compare_is_by_length_first():
    assert MC.path_cmp([10, 99], [10, 14, 18]) < 0 and MC.path_cmp([10, 18, 14], [10, 14, 18]) > 0 and MC.path_cmp([10], [10]) == 0


def test_the_hash_is_a_sum_over_the_elements():
    """what lets the lanes of a wave add their shares in any order; the mask keeps the low bits"""
    p = [10, 14, 18]
    h = MC.path_hash(p)
    assert h == (MC.mix64(3) + sum(MC.mix64((t << 32 | e) + 0x9E3779B97F4A7C15) for t, e in reversed(list(enumerate(p))))) & MC.M64
    assert MC.path_hash(p, 8) == h & 0xFF and MC.path_hash(p, 64) == h and MC.path_hash([10, 18, 14]) != h


def three_unitig_graph():
    """A (len 1000, cov 30), B (len 400, cov 10), C (len 250, cov 7); live arcs A+ -> B+ (ls 100), B+ -> A+ (ls 50), A+ -> A+ (ls 20), B+ -> C+ (ls 30), C+ -> A+ (ls 40);
    A+ -> C+ exists but is deleted"""
    arcs = sorted([(10, 14, 100, 0), (14, 10, 50, 0), (10, 10, 20, 0), (14, 18, 30, 0), (18, 10, 40, 0), (10, 18, 60, 1)])
    nv = 10
    idx_p, idx_n = np.zeros(2 * nv, np.uint64), np.zeros(2 * nv, np.uint64)
    for i, a in enumerate(arcs):
        if idx_n[a[0]] == 0:
            idx_p[a[0]] = i
        idx_n[a[0]] += 1
    ln, cov = np.zeros(nv, np.uint64), np.zeros(nv, np.uint32)
    ln[[5, 7, 9]], cov[[5, 7, 9]] = [1000, 400, 250], [30, 10, 7]
    return {"idx_p": idx_p, "idx_n": idx_n, "arc_w": np.array([a[1] for a in arcs], np.uint64), "arc_ls": np.array([a[2] for a in arcs], np.uint64),
            "arc_del": np.array([a[3] for a in arcs], np.uint8), "vtx_len": ln, "vtx_cov": cov}


def test_the_statistics_of_three_paths_worked_by_hand():
    G = three_unitig_graph()
    # [A]: len = 1000 - 20 = 980; wlen = 30 * 1000 - 30 * 20 = 29400
    assert MC.path_stats(G, [10]) == (980, 29400.0)
    # [A, B]: closing arc B -> A (ls 50): len = 1000 - 50 + 400 - 100 = 1250; wlen = 30000 - 30 * 50 + 10 * 400 - 10 * 100 = 31500
    assert MC.path_stats(G, [10, 14]) == (1250, 31500.0)
    # [A, B, C]: closing arc C -> A (ls 40): len = 1000 - 40 + 400 - 100 + 250 - 30 = 1480; wlen = 30000 - 1200 + 4000 - 1000 + 1750 - 210 = 33340
    assert MC.path_stats(G, [10, 14, 18]) == (1480, 33340.0)
    # [A, C]: A -> C is deleted: asmg_arc1 finds nothing, the reference asserts
    assert MC.path_stats(G, [10, 18]) is None
