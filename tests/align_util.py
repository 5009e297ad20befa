"""Helpers for the read-alignment parity tests: the reference's scg_t flattened the way scg_ra_analysis_thread reads it, the oracle's
alignment (oracle/align.c), the old_ra filter of alignment.c:610-634 restated, the device result as arrays."""
import ctypes as C
import math
import sys

import numpy as np

import oracle_lib as O
import ref_lib as R

GRAPH_FIELDS = (("su_off", np.uint64), ("su_uid", np.uint64), ("su_pos", np.uint32), ("utg_n", np.uint32), ("idx_p", np.uint64), ("idx_n", np.uint64),
                ("arc_w", np.uint64), ("arc_ln", np.uint64), ("arc_del", np.uint8))
OUT_FIELDS = ("sid", "n", "s", "uid", "u_beg", "u_end", "s_beg", "s_end")


class RaGraphT(C.Structure):
    _fields_ = [("n_scm", C.c_uint64), ("n_utg", C.c_uint64), ("n_arc", C.c_uint64)] + [(k, C.c_void_p) for k, _ in GRAPH_FIELDS]


class RaOutT(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_aln", "n_frg", "m_aln", "m_frg", "n_mapped", "n_unique")] + [
        ("sid", C.POINTER(C.c_uint64)), ("n", C.POINTER(C.c_uint32)), ("s", C.POINTER(C.c_double)), ("uid", C.POINTER(C.c_uint64)),
        ("u_beg", C.POINTER(C.c_uint64)), ("u_end", C.POINTER(C.c_uint64)), ("s_beg", C.POINTER(C.c_uint32)), ("s_end", C.POINTER(C.c_uint32))]


def ref_ra_graph(g):
    """scg_t of the compiled reference -> dict of arrays shaped like oatk_ra_graph_t"""
    L = R.lib()
    L.refx_ra_graph_dims.argtypes = [C.c_void_p] * 5
    L.refx_ra_graph_flatten.argtypes = [C.c_void_p] * 10
    d = [C.c_uint64() for _ in range(4)]
    L.refx_ra_graph_dims(g, *[C.byref(x) for x in d])
    ns, nsu, nu, na = (x.value for x in d)
    G = {"n_scm": ns, "su_off": np.zeros(ns + 1, np.uint64), "su_uid": np.zeros(max(nsu, 1), np.uint64), "su_pos": np.zeros(max(nsu, 1), np.uint32),
         "utg_n": np.zeros(max(nu, 1), np.uint32), "idx_p": np.zeros(max(2 * nu, 1), np.uint64), "idx_n": np.zeros(max(2 * nu, 1), np.uint64),
         "arc_w": np.zeros(max(na, 1), np.uint64), "arc_ln": np.zeros(max(na, 1), np.uint64), "arc_del": np.zeros(max(na, 1), np.uint8)}
    L.refx_ra_graph_flatten(g, *[G[k].ctypes.data for k, _ in GRAPH_FIELDS])
    G["su_uid"], G["su_pos"] = G["su_uid"][:nsu], G["su_pos"][:nsu]
    G["utg_n"], G["idx_p"], G["idx_n"] = G["utg_n"][:nu], G["idx_p"][:2 * nu], G["idx_n"][:2 * nu]
    G["arc_w"], G["arc_ln"], G["arc_del"] = G["arc_w"][:na], G["arc_ln"][:na], G["arc_del"][:na]
    return G


def old_ra_filter(prev, n_reads, for_unzip):
    """alignment.c:610-634: which reads the next call aligns and the score they must reach; `prev` = flattened previous alignments"""
    old = np.zeros(n_reads, np.int64)
    if for_unzip and len(prev["sid"]):
        for sid, n, s in zip(prev["sid"].tolist(), prev["n"].tolist(), prev["s"].tolist()):
            if n > 2 and (old[sid] & 1) == 0:
                frac, whole = math.modf(s)
                if frac < sys.float_info.epsilon:
                    whole -= 1
                old[sid] = int(whole) << 1 | 1
    else:
        old[:] = 1
    return old


def oracle_align(n_scm, k_mer, m_pos, G, old_ra=None):
    L = O.lib()
    L.orc_read_alignment.restype = C.POINTER(RaOutT)
    L.orc_read_alignment.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RaGraphT), C.c_void_p]
    L.orc_ra_out_free.argtypes = [C.POINTER(RaOutT)]
    keep = [np.ascontiguousarray(G[k], dtype=dt) for k, dt in GRAPH_FIELDS]
    gs = RaGraphT(int(G["n_scm"]), len(G["utg_n"]), len(G["arc_w"]), *[a.ctypes.data for a in keep])
    a = [np.ascontiguousarray(n_scm, dtype=np.uint32), np.ascontiguousarray(k_mer, dtype=np.uint64), np.ascontiguousarray(m_pos, dtype=np.uint32)]
    o = None if old_ra is None else np.ascontiguousarray(old_ra, dtype=np.int64)
    p = L.orc_read_alignment(len(a[0]), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, C.byref(gs), None if o is None else o.ctypes.data)
    r = p.contents
    na, nf = r.n_aln, r.n_frg
    out = {"sid": O._arr(r.sid, na, np.uint64), "n": O._arr(r.n, na, np.uint32), "s": O._arr(r.s, na, np.float64), "uid": O._arr(r.uid, nf, np.uint64),
           "u_beg": O._arr(r.u_beg, nf, np.uint64), "u_end": O._arr(r.u_end, nf, np.uint64), "s_beg": O._arr(r.s_beg, nf, np.uint32),
           "s_end": O._arr(r.s_end, nf, np.uint32), "n_mapped": r.n_mapped, "n_unique": r.n_unique}
    L.orc_ra_out_free(p)
    return out


def device_align(hip, G, old_ra=None):
    """oatk_hip_read_alignment on the resident chains; result shaped like the flattened scg_ra_v"""
    na, nf, st = hip.read_alignment(G, old_ra)
    off = hip.fetch("RA_ALN_OFF")
    out = {"sid": hip.fetch("RA_ALN_SID").astype(np.uint64), "n": np.diff(off).astype(np.uint32), "s": hip.fetch("RA_ALN_S"),
           "uid": hip.fetch("RA_FRG_UID"), "u_beg": hip.fetch("RA_FRG_UBEG").astype(np.uint64), "u_end": hip.fetch("RA_FRG_UEND").astype(np.uint64),
           "s_beg": hip.fetch("RA_FRG_SBEG"), "s_end": hip.fetch("RA_FRG_SEND"), "n_mapped": int(st[0]), "n_unique": int(st[1]), "skipped": int(st[2])}
    assert len(out["sid"]) == na and len(out["uid"]) == nf
    return out


def assert_same(got, want, what=""):
    for k in OUT_FIELDS:
        assert len(got[k]) == len(want[k]), (what, k, len(got[k]), len(want[k]))
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def random_graph(rng, n_scm, chains, n_src, max_len, p_overlap, p_noise):
    """unitigs cut out of the chains of n_src random reads (pieces of 1..max_len syncmers, consecutive pieces joined by an arc, with probability
    p_overlap sharing one syncmer across an arc of ln = 1), so other reads of the same region hit several unitigs at once; plus random arcs
    and a few deleted ones.  Nothing an assembler would build, but every path of the aligner gets walked: ties, many predecessors, several
    best chains, chains that miss the 90 % mark"""
    n_chain, k_mer, m_pos = chains
    starts = np.cumsum(n_chain, dtype=np.int64) - n_chain
    hits = [[] for _ in range(n_scm)]
    utg_n, arcs = [], {}
    for r in rng.choice(len(n_chain), size=min(n_src, len(n_chain)), replace=False).tolist():
        n = int(n_chain[r])
        ids = (k_mer[starts[r]:starts[r] + n] >> np.uint64(1)).astype(np.int64)
        rev = (m_pos[starts[r]:starts[r] + n] & 1).astype(np.int64)
        flip = int(rng.integers(0, 2))                   # lay the read down in either orientation
        if flip:
            ids, rev = ids[::-1], 1 - rev[::-1]
        j, prev_u = 0, None
        while j < n:
            ln = int(rng.integers(1, max_len + 1))
            ovl = 1 if (prev_u is not None and j > 0 and rng.random() < p_overlap) else 0
            seg = list(range(j - ovl, min(j - ovl + ln + ovl, n)))
            u = len(utg_n)
            for q, t in enumerate(seg):
                hits[int(ids[t])].append((u << 1 | int(rev[t]), q))
            utg_n.append(len(seg))
            if prev_u is not None:
                arcs[(prev_u << 1, u << 1)] = ovl
                arcs[(u << 1 | 1, prev_u << 1 | 1)] = ovl
            prev_u, j = u, seg[-1] + 1
    n_utg = len(utg_n)
    for _ in range(int(p_noise * n_utg)):
        v, w = int(rng.integers(0, 2 * n_utg)), int(rng.integers(0, 2 * n_utg))
        if (v, w) not in arcs:
            arcs[(v, w)] = arcs[(w ^ 1, v ^ 1)] = int(rng.integers(0, 3))
    keys = sorted(arcs)
    su_off = np.zeros(n_scm + 1, np.uint64)
    su_uid, su_pos = [], []
    for sid in range(n_scm):
        hs = sorted(hits[sid], key=lambda t: (t[0] & 1, t[0] >> 1, t[1]))            # scg_scm_utg_index orders by (rev, utg, pos)
        su_uid += [h[0] for h in hs]
        su_pos += [h[1] for h in hs]
        su_off[sid + 1] = len(su_uid)
    idx_p, idx_n = np.zeros(2 * n_utg, np.uint64), np.zeros(2 * n_utg, np.uint64)
    for i, (v, w) in enumerate(keys):
        if idx_n[v] == 0:
            idx_p[v] = i
        idx_n[v] += 1
    return {"n_scm": n_scm, "su_off": su_off, "su_uid": np.array(su_uid, np.uint64), "su_pos": np.array(su_pos, np.uint32), "utg_n": np.array(utg_n, np.uint32),
            "idx_p": idx_p, "idx_n": idx_n, "arc_v": np.array([v for v, _ in keys], np.uint64), "arc_w": np.array([w for _, w in keys], np.uint64), "arc_ln": np.array([arcs[k] for k in keys], np.uint64),
            "arc_del": (rng.random(len(keys)) < 0.03).astype(np.uint8)}


# ---- graph recipes: per read, a piece of a unitig graph whose hit, fragment, predecessor and alignment counts are known in closed form ----
#
# A recipe works in READ SPACE: a unitig is the array of read positions it carries, in the read's direction, and an arc (a, b, ln, dead) joins unitig a
# to unitig b of the same plan in that direction.  piece() turns a plan into syncmer ids and strand bits for one read's chain, forward or flipped
# (flipped: every unitig reversed and complemented, so the read's hits carry strand bit 1 and take the `utg_n - p - 1` branch; the closed forms do not
# change), and combine() concatenates the pieces of many reads into one graph shaped like random_graph's.  A plan carries what it expects, `exp`:
#   hits   positions of the read's syncmers on the plan's unitigs          frags  fragments of score >= 0 (chains and singletons)
#   prev   most predecessors ever recorded for one fragment                depth  fragments of the longest chain walked from a fragment of maximal score
#   score  max_score                                                       aln    {fragments per alignment: alignments}; each scores score + 1 / n_aln
# `n` is the number of syncmers laid (positions 0 .. n-1 of the chain), `n_read` the read's (the 90 % rule, min_a_frac, divides by it).
SMALL_LIMITS = {"hits": 160, "frags": 128, "prev": 6, "depth": 48}          # RaSmall (align.hpp): a read over any of them leaves the lane-per-read tier
BIG_PREV, BIG_MAX_HITS = 32, 1 << 21                                        # RAB_PREV, RAB_MAX_HITS (align_big.hpp)


def _covers(s_cnt, n_read):
    return not (float(s_cnt) / float(n_read) < 0.9)


def _plan(utg, arcs, **exp):
    return {"utg": [np.asarray(u, np.int64) for u in utg], "arcs": list(arcs), "exp": exp}


def tandem(n, m, trim=0, tail=0, loop=True, n_read=None):
    """ONE unitig carrying the chain m times, then its first `trim` syncmers once more (0 <= trim < n), then `tail` copies of syncmer 0; with `loop`
    a self-arc of ln = 0 from the unitig's end to its start.
    hits = m n + trim + tail.  A hit links to the same copy's next syncmer (the closest larger unitig position), so every copy is one chained fragment
    of score n (the trimmed one: trim), and every tail copy a singleton on the chains' own unitig: frags = m + (trim > 0) + tail.  The copies tie on
    (s_beg, s_end); only the unitig's last fragment reaches its end and only copy 0 starts at 0, and the self-arc joins them at read positions that do
    not meet (p1 + u_ovl = 0 != p + 1), so the arc loop runs and records nothing: prev = 0, m co-optimal alignments of one fragment, in copy order."""
    assert m >= 1 and 0 <= trim < n and not (trim and tail)
    n_read = n_read or n
    u = np.concatenate([np.tile(np.arange(n), m), np.arange(trim), np.zeros(tail, np.int64)])
    return _plan([u], [(0, 0, 0, 0)] if loop else [], hits=m * n + trim + tail, frags=m + (trim > 0) + tail, prev=0, depth=1, score=n,
                 aln={1: m} if _covers(n, n_read) else {})


def _levels(n, cuts, ovl):
    cuts = list(cuts)
    ovl = [ovl] * len(cuts) if np.isscalar(ovl) else list(ovl)
    assert len(ovl) == len(cuts) and all(0 < c < n for c in cuts) and all(a < b for a, b in zip(cuts, cuts[1:]))
    beg = [0] + [c - o for c, o in zip(cuts, ovl)]
    end = cuts + [n]
    assert all(e - b >= 1 + o for b, e, o in zip(beg, end, [0] + ovl)), "a piece behind an arc of ln = 1 needs two syncmers: the shared one scores nothing"
    return beg, end, ovl


def ladder(n, cuts, widths, ovl=0, dead=False, n_read=None):
    """the chain cut at `cuts` into len(cuts) + 1 consecutive pieces (level i+1 starts ovl[i] in {0, 1} syncmers before the cut: the shared syncmer of an
    arc of ln = ovl[i]), level i present on widths[i] duplicate unitigs, arcs from every duplicate of a level to every duplicate of the next.  With
    `dead` every live arc stands behind a DELETED arc between the same two unitigs whose ln is the wrong one (asmg_arc1 takes the first that is alive).
    hits = sum widths[i] len_i (sum len_i = n + sum ovl), frags = sum widths.  The duplicates of a level tie on (s_beg, s_end) and come in unitig order;
    each of level i+1 gets score_i + len_{i+1} - ovl from every duplicate of level i: the first raises it, the others tie and are appended, so
    prev = max(widths[:-1]); the last level holds max_score = n, prod(widths) alignments of len(widths) fragments each."""
    n_read = n_read or n
    beg, end, ovl = _levels(n, cuts, ovl)
    widths = [widths] * len(beg) if np.isscalar(widths) else list(widths)
    assert len(widths) == len(beg)
    utg, first, arcs = [], [], []
    for b, e, w in zip(beg, end, widths):
        first.append(len(utg))
        utg += [np.arange(b, e)] * w
    for i, o in enumerate(ovl):
        for a in range(first[i], first[i] + widths[i]):
            for b in range(first[i + 1], first[i + 1] + widths[i + 1]):
                if dead:
                    arcs.append((a, b, 1 - o, 1))
                arcs.append((a, b, o, 0))
    n_aln = int(np.prod([int(w) for w in widths], dtype=object))
    return _plan(utg, arcs, hits=sum(w * (e - b) for b, e, w in zip(beg, end, widths)), frags=sum(widths), prev=max(widths[:-1]) if len(widths) > 1 else 0,
                 depth=len(widths), score=n, aln={len(widths): n_aln} if _covers(n + sum(ovl), n_read) else {})


def pieces(n, cuts, ovl=0, dead=False, n_read=None):
    """the chain cut into consecutive unitigs joined by arcs of ln = ovl[i] (ladder of width 1): hits = n + sum ovl, len(cuts) + 1 fragments with one
    predecessor each, ONE alignment of len(cuts) + 1 fragments and score n -- or none where n + sum ovl is under 90 % of the read (n < n_read)"""
    return ladder(n, cuts, 1, ovl, dead, n_read)


def gapped(n, c, g, late=True, n_read=None):
    """unitig GAP carries positions 0 and 1+g .. c-1 of the piece [0, c) (s_gap = g > u_gap = 0: one chained fragment (0, c-1) of c - g syncmers and score
    c - 2g; below 0 it is no fragment), unitig LATE (with `late`) the complete positions 1 .. c-1 (score c - 1), unitig B the rest c .. n-1; arcs of ln = 0
    from GAP and LATE to B.  Sorted: GAP, LATE, B.  GAP reaches B first: with c - 2g > 0 it raises B to c - 2g + n - c and is recorded (at 0 it ties with
    B's own score and prev_n = 0: not recorded); LATE then raises B to n - 1 and the list starts again: prev = 1, one alignment LATE + B of n - 1
    syncmers and score n - 1.  Without `late`: GAP + B, n - g syncmers, score n - 2g, where c - 2g > 0; else B stays alone and covers too little."""
    n_read = n_read or n
    assert g >= 1 and 1 + g < c < n
    sg = c - 2 * g
    utg = [np.concatenate([[0], np.arange(1 + g, c)])] + ([np.arange(1, c)] if late else []) + [np.arange(c, n)]
    arcs = [(a, len(utg) - 1, 0, 0) for a in range(len(utg) - 1)]
    hits, frags = sum(len(u) for u in utg), len(utg) - (sg < 0)
    if late:
        return _plan(utg, arcs, hits=hits, frags=frags, prev=1, depth=2, score=n - 1, aln={2: 1} if _covers(n - 1, n_read) else {})
    if sg > 0:
        return _plan(utg, arcs, hits=hits, frags=frags, prev=1, depth=2, score=n - 2 * g, aln={2: 1} if _covers(n - g, n_read) else {})
    assert n - c > sg and not _covers(n - c, n_read)
    return _plan(utg, arcs, hits=hits, frags=frags, prev=0, depth=1, score=n - c, aln={})


def ugapped(n, c, x, n_read=None):
    """unitig A carries the piece [0, c) with x copies of its LAST syncmer c-1 pushed in behind position 0, unitig B the rest, one arc of ln = 0.  The
    chain on A steps over the x copies (u_gap = x > s_gap = 0): one fragment (0, c-1) of c syncmers and score c - x; nothing points to the copies and
    they point nowhere (no hit of a later read position lies behind them): x singletons in the middle of the unitig that chain with nothing.
    hits = n + x, frags = 2 + x, prev = 1, one alignment A + B of n syncmers and score n - x."""
    n_read = n_read or n
    assert 3 <= c < n and 1 <= x < c
    A = np.concatenate([[0], np.full(x, c - 1), np.arange(1, c)])
    return _plan([A, np.arange(c, n)], [(0, 1, 0, 0)], hits=n + x, frags=2 + x, prev=1, depth=2, score=n - x, aln={2: 1} if _covers(n, n_read) else {})


def singletons(n, f, n_read=None):
    """f one-syncmer unitigs (unitig i carries position i mod n) and no arc: f hits, f fragments of score 1 that all tie for max_score = 1 and none of
    which covers 90 % of a read of two syncmers or more: no alignment.  Composed with a chain they are what fills the fragment array."""
    n_read = n_read or n
    assert n_read >= 2
    return _plan([np.array([i % n]) for i in range(f)], [], hits=f, frags=f, prev=0, depth=1, score=1 if f else 0, aln={})


def compose(*plans):
    """several recipes for ONE read, side by side (no arcs between them): hits and fragments add up, the alignments are those of the plans that reach the
    largest max_score"""
    utg, arcs = [], []
    for p in plans:
        arcs += [(a + len(utg), b + len(utg), ln, d) for a, b, ln, d in p["arcs"]]
        utg += p["utg"]
    E = [p["exp"] for p in plans]
    score = max(e["score"] for e in E)
    aln = {}
    for e in E:
        if e["score"] == score:
            for k, v in e["aln"].items():
                aln[k] = aln.get(k, 0) + v
    return _plan(utg, arcs, hits=sum(e["hits"] for e in E), frags=sum(e["frags"] for e in E), prev=max(e["prev"] for e in E),
                 depth=max(e["depth"] for e in E if e["score"] == score), score=score, aln=aln)


def over_small(e):
    return e["hits"] > SMALL_LIMITS["hits"] or e["frags"] > SMALL_LIMITS["frags"] or e["prev"] > SMALL_LIMITS["prev"] or e["depth"] > SMALL_LIMITS["depth"]


def over_big(e):
    return e["hits"] >= BIG_MAX_HITS or e["prev"] > BIG_PREV


def read_chains(chains):
    """(n_scm, k_mer, m_pos) of all reads -> per read (syncmer ids, strand bits)"""
    n_chain, k_mer, m_pos = chains
    ids, rev = (np.asarray(k_mer) >> np.uint64(1)).astype(np.int64), (np.asarray(m_pos) & 1).astype(np.int64)
    cut = np.cumsum(np.asarray(n_chain, np.int64))[:-1]
    return list(zip(np.split(ids, cut), np.split(rev, cut)))


def piece(chain, plan, flip):
    """the plan laid down for one read's chain: (per unitig ids, per unitig strand bits, arcs between oriented local unitigs, reverse complements included)"""
    ids, rev = chain
    if not flip:
        uu = [(ids[u], rev[u]) for u in plan["utg"]]
        arcs = [x for a, b, ln, d in plan["arcs"] for x in ((a << 1, b << 1, ln, d), (b << 1 | 1, a << 1 | 1, ln, d))]
    else:
        uu = [(ids[u[::-1]], 1 - rev[u[::-1]]) for u in plan["utg"]]
        arcs = [x for a, b, ln, d in plan["arcs"] for x in ((a << 1 | 1, b << 1 | 1, ln, d), (b << 1, a << 1, ln, d))]
    return uu, arcs


def combine(n_scm, parts):
    """pieces of many reads -> one graph (the dict random_graph returns): unitig ids offset piece by piece, su_* in (rev, utg, pos) order per syncmer,
    a vertex's arcs in the order the pieces list them"""
    utg_ids = [i for uu, _ in parts for i, _ in uu]
    utg_rev = [r for uu, _ in parts for _, r in uu]
    utg_n = np.array([len(i) for i in utg_ids], np.int64)
    n_utg = len(utg_n)
    ids = np.concatenate(utg_ids) if n_utg else np.zeros(0, np.int64)
    rev = np.concatenate(utg_rev) if n_utg else np.zeros(0, np.int64)
    uid = np.repeat(np.arange(n_utg, dtype=np.int64), utg_n)
    pos = np.arange(len(ids), dtype=np.int64) - np.repeat(np.cumsum(utg_n) - utg_n, utg_n)
    order = np.lexsort((pos, uid, rev, ids))                                           # scg_scm_utg_index: per syncmer by (rev, utg, pos)
    su_off = np.zeros(n_scm + 1, np.uint64)
    su_off[1:] = np.cumsum(np.bincount(ids, minlength=n_scm))
    base = np.cumsum([0] + [len(uu) for uu, _ in parts])
    A = np.array([(v + 2 * int(base[i]), w + 2 * int(base[i]), ln, d) for i, (_, arcs) in enumerate(parts) for v, w, ln, d in arcs], np.int64).reshape(-1, 4)
    if len(A) == 0:
        A = np.zeros((1, 4), np.int64)                                                 # (no vertex lists it)
        idx_n = np.zeros(2 * n_utg, np.int64)
    else:
        A = A[np.argsort(A[:, 0], kind="stable")]
        idx_n = np.bincount(A[:, 0], minlength=2 * n_utg)
    idx_p = np.where(idx_n > 0, np.cumsum(idx_n) - idx_n, 0)
    return {"n_scm": n_scm, "su_off": su_off, "su_uid": (uid << 1 | rev)[order].astype(np.uint64), "su_pos": pos[order].astype(np.uint32),
            "utg_n": utg_n.astype(np.uint32), "idx_p": idx_p.astype(np.uint64), "idx_n": idx_n.astype(np.uint64), "arc_v": A[:, 0].astype(np.uint64),
            "arc_w": A[:, 1].astype(np.uint64), "arc_ln": A[:, 2].astype(np.uint64), "arc_del": A[:, 3].astype(np.uint8)}


def recipe_graph(n_scm, chains, jobs):
    """jobs: [(read, plan, flip)], at most one per read -> (graph, {read: exp})"""
    ch = read_chains(chains)
    assert len({r for r, _, _ in jobs}) == len(jobs)
    return combine(n_scm, [piece(ch[r], p, f) for r, p, f in jobs]), {r: p["exp"] for r, p, _ in jobs}


def graph_hits(chains, G):
    """hits per read: positions of its syncmers on the unitigs"""
    n_chain, k_mer, _ = chains
    per = np.diff(G["su_off"].astype(np.int64))[(np.asarray(k_mer) >> np.uint64(1)).astype(np.int64)]
    return np.bincount(np.repeat(np.arange(len(n_chain)), np.asarray(n_chain, np.int64)), weights=per, minlength=len(n_chain)).astype(np.int64)


def assert_as_planned(out, exps, n_reads, skipped=()):
    """an alignment result holds, for every read, exactly the alignments its plan announces: how many, of how many fragments, their score"""
    sid = out["sid"].astype(np.int64)
    cnt = np.bincount(sid, minlength=n_reads)
    for r in range(n_reads):
        e = exps.get(r)
        want = {} if e is None or r in skipped else e["aln"]
        na = sum(want.values())
        assert cnt[r] == na, (r, int(cnt[r]), na, e)
        if na:
            sel = sid == r
            assert {int(k): int(v) for k, v in zip(*np.unique(out["n"][sel], return_counts=True))} == want, (r, e)
            assert np.all(out["s"][sel] == 1.0 / na + float(e["score"])), (r, e)
