"""The graph recipes of align_util (tandem, pieces, ladder, gapped, ugapped, singletons, compose) do what they announce: on synthetic chains with distinct
syncmer ids, oracle/align.c gives every read exactly the planned number of alignments, fragments per alignment and score, at every value the GPU
tests sweep (tests/test_gpu_align_big.py), laid down forward and flipped.  No GPU."""
import numpy as np
import pytest

import align_util as AU


def synthetic_chains(lens, seed=0):
    """reads that share no syncmer: ids in read order, random strand bits (and random bits where the aligner must not look)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.uint32)
    tot = int(lens.sum())
    ids = rng.permutation(tot).astype(np.uint64)
    k_mer = ids << np.uint64(1) | rng.integers(0, 2, tot).astype(np.uint64)
    m_pos = (rng.integers(0, 1000, tot).astype(np.uint32) << np.uint32(1)) | rng.integers(0, 2, tot).astype(np.uint32)
    return (lens, k_mer, m_pos), tot


def sweep_plans():
    """(name, syncmers of the read, plan): every recipe at every swept value"""
    P = []
    for n in (20, 23):                                                     # hits one step either side of 160, by a trimmed last copy
        for hits in (159, 160, 161):
            P.append(("tandem hits %d" % hits, n, AU.tandem(n, hits // n, hits % n)))
    P.append(("tandem no loop", 20, AU.tandem(20, 9, 0, loop=False)))
    P.append(("tandem trim 1", 20, AU.tandem(20, 3, 1)))
    for f in (128, 129):                                                   # fragments: singletons on the chain's own unitig, and on unitigs of their own
        P.append(("tail frags %d" % f, 21, AU.tandem(21, 1, tail=f - 1)))
        P.append(("singletons frags %d" % f, 21, AU.compose(AU.tandem(21, 1), AU.singletons(21, f - 1))))
        P.append(("both frags %d" % f, 21, AU.compose(AU.tandem(21, 1, tail=60), AU.singletons(21, f - 61))))
    P.append(("singletons alone", 20, AU.singletons(20, 50)))
    for depth in (2, 47, 48, 49):                                          # the walk: fragments per alignment
        P.append(("pieces depth %d" % depth, 52, AU.pieces(52, range(1, depth))))
        P.append(("pieces depth %d ovl" % depth, 110, AU.pieces(110, range(2, 2 * depth, 2), [i & 1 for i in range(depth - 1)])))
    P.append(("pieces dead arcs", 30, AU.pieces(30, [5, 11, 12, 20], [0, 1, 0, 1], dead=True)))
    for w in (6, 7, 32, 33):                                               # predecessors per fragment: RaSmall::PREV and RAB_PREV
        P.append(("ladder w %d" % w, 20, AU.ladder(20, [9], w)))
        P.append(("ladder w %d ovl" % w, 20, AU.ladder(20, [9], w, 1)))
    for w in (6, 7):
        P.append(("ladder w %d d 2" % w, 21, AU.ladder(21, [7, 14], w, [1, 0], dead=True)))
        P.append(("ladder 1-%d-1" % w, 22, AU.ladder(22, [20, 21], [w, 1, 1])))
    P.append(("ladder 2^9", 45, AU.ladder(45, range(5, 45, 5), 2)))
    P.append(("ladder 2^9 ovl", 45, AU.ladder(45, range(5, 45, 5), 2, [0, 1] * 4)))
    for c, g in ((10, 1), (10, 2), (10, 4), (10, 5), (10, 6), (3, 1)):    # the gapped fragment's score: c - 2g = 8, 6, 2, 0, -2, 1
        P.append(("gapped c %d g %d" % (c, g), 24, AU.gapped(24, c, g)))
    for c, g in ((12, 1), (12, 2), (4, 2), (4, 1), (6, 3)):
        P.append(("gapped alone c %d g %d" % (c, g), 24, AU.gapped(24, c, g, late=False)))
    for c, x in ((3, 1), (10, 3), (12, 11)):                               # the unitig's gap instead of the read's
        P.append(("ugapped c %d x %d" % (c, x), 24, AU.ugapped(24, c, x)))
    P.append(("ugapped + short tandem", 24, AU.compose(AU.ugapped(24, 10, 2), AU.tandem(21, 8, n_read=24))))
    P.append(("ladder over two waves of fragments", 20, AU.ladder(20, [2, 4, 6, 8], [30, 2, 30, 1, 2])))
    for n, n_read in ((18, 20), (17, 20), (45, 50), (44, 50)):             # 90 % of the read, one syncmer either side
        P.append(("pieces %d of %d" % (n, n_read), n_read, AU.pieces(n, [n // 3, n // 2], n_read=n_read)))
        P.append(("tandem %d of %d" % (n, n_read), n_read, AU.tandem(n, 10, 3, n_read=n_read)))
    P.append(("tandem + ladder", 20, AU.compose(AU.tandem(20, 9), AU.ladder(20, [4, 11], 3, [1, 0]))))
    P.append(("tandem + ladder 2^9", 45, AU.compose(AU.tandem(45, 4, 7), AU.ladder(45, range(5, 45, 5), 2))))
    P.append(("tandem + gapped", 24, AU.compose(AU.tandem(24, 7), AU.gapped(24, 10, 1))))           # the tandem's score n beats the gapped n - 1
    P.append(("gapped + short tandem", 24, AU.compose(AU.gapped(24, 10, 1), AU.tandem(22, 8, n_read=24))))
    return P


PLANS = sweep_plans()


def test_closed_forms_of_the_sweep():
    """the swept values really are one step either side of each limit"""
    by = {name: p["exp"] for name, _, p in PLANS}
    assert [by["tandem hits %d" % h]["hits"] for h in (159, 160, 161)] == [159, 160, 161]
    assert [by["tail frags %d" % f]["frags"] for f in (128, 129)] == [128, 129] and by["tail frags 129"]["hits"] <= 160
    assert [by["singletons frags %d" % f]["frags"] for f in (128, 129)] == [128, 129] and by["singletons frags 129"]["hits"] <= 160
    assert [by["both frags %d" % f]["frags"] for f in (128, 129)] == [128, 129] and by["both frags 129"]["hits"] <= 160
    assert [by["pieces depth %d" % d]["depth"] for d in (47, 48, 49)] == [47, 48, 49]
    assert [by["ladder w %d" % w]["prev"] for w in (6, 7, 32, 33)] == [6, 7, 32, 33]
    assert by["ladder w 7"]["hits"] <= 160 and by["ladder w 7 ovl"]["hits"] <= 160 and by["ladder w 32"]["aln"] == {2: 1024}
    assert by["ladder 2^9"]["aln"] == {9: 512} and not AU.over_small(by["ladder 2^9"]) and AU.over_small(by["tandem + ladder 2^9"])
    assert by["pieces 18 of 20"]["aln"] and not by["pieces 17 of 20"]["aln"] and by["tandem 45 of 50"]["aln"] and not by["tandem 44 of 50"]["aln"]
    over = {name for name, e in by.items() if AU.over_small(e)}
    assert {"tandem hits 161", "tail frags 129", "pieces depth 49", "ladder w 7", "ladder w 32", "ladder w 33"} <= over
    assert not {"tandem hits 160", "tail frags 128", "pieces depth 48", "ladder w 6", "ladder 2^9", "gapped c 10 g 1"} & over
    assert [name for name, e in by.items() if AU.over_big(e)] == ["ladder w 33", "ladder w 33 ovl"]


@pytest.mark.parametrize("flip", [0, 1, 2])
def test_oracle_gives_what_the_recipes_announce(flip):
    """every plan on a read of its own (plus reads without a plan, which must stay unaligned); flip 2 alternates the orientation"""
    lens = [n for _, n, _ in PLANS] + [20, 33]
    chains, n_scm = synthetic_chains(lens, seed=flip)
    jobs = [(r, p, (flip == 1) if flip < 2 else bool(r & 1)) for r, (_, _, p) in enumerate(PLANS)]
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    hits = AU.graph_hits(chains, G)
    assert [int(h) for h in hits] == [p["exp"]["hits"] for _, _, p in PLANS] + [0, 0]
    out = AU.oracle_align(*chains, G)
    AU.assert_as_planned(out, exps, len(lens))
    assert out["n_mapped"] == sum(1 for e in exps.values() if e["aln"]) and out["n_unique"] == sum(1 for e in exps.values() if sum(e["aln"].values()) == 1)
    # the strand bit of every hit follows the lay-down: a flipped read's fragments are on orientation 1 of its unitigs
    fl = np.array([f for _, _, f in jobs] + [0, 0])
    assert np.array_equal(out["uid"] & np.uint64(1), fl[np.repeat(out["sid"].astype(np.int64), out["n"])].astype(np.uint64))


def test_old_ra_threshold_on_the_planned_score():
    """a read is aligned iff bit 0 of old_ra is set and max_score >= old_ra >> 1 (alignment.c:225, :505)"""
    names = ("tandem hits 161", "ladder w 7", "gapped c 10 g 1", "tandem + ladder")
    sel = [(n, p) for name, n, p in PLANS if name in names]
    lens = [n for n, _ in sel for _ in range(4)]
    chains, n_scm = synthetic_chains(lens, seed=5)
    jobs = [(4 * i + t, p, bool(t & 1)) for i, (_, p) in enumerate(sel) for t in range(4)]
    G, exps = AU.recipe_graph(n_scm, chains, jobs)
    old = np.array([(p["exp"]["score"] + d) << 1 | b for _, p in sel for d, b in ((-1, 1), (0, 1), (1, 1), (0, 0))], np.int64)
    out = AU.oracle_align(*chains, G, old)
    AU.assert_as_planned(out, exps, len(lens), skipped={r for r in range(len(lens)) if r % 4 >= 2})
    assert len(out["sid"]) > 0
