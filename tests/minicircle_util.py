"""A plain Python model of extract_minicircles_with_anchor (path_finder.c:539-730) over flat alignments (off, uid), a record at a time in the
reference's loop order, with the line it restates beside every step.  That function is static in a unit the oracle recipe does not compile,
so this model -- pinned to the hand-derived cases of tests/test_minicircle_model.py -- is what the device results are compared with.
Python ints stand for the reference's unsigned integers: every place where the reference's width matters is masked explicitly."""
import functools

import numpy as np

NONE = (1 << 64) - 1
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def unit_of(uid, sid):
    """minicircle_analysis_thread (:545-607) for one record: beg << 33 | end << 1 | rev, or NONE"""
    nfrg = len(uid)
    if nfrg < 2:                                                    # :557
        return NONE
    beg = end = rev = None                                          # :563 (UINT32_MAX)
    for j in range(nfrg):                                           # :564
        u = int(uid[j])
        if u >> 1 != sid:                                           # :566
            continue
        if beg is None:                                             # :568
            beg = j
        elif end is None:                                           # :570
            end = j - 1
        if rev is None:                                             # :572
            rev = u & 1
        elif rev != (u & 1):                                        # :574
            rev = None
            break
    if beg is None or end is None or rev is None:                   # :581
        return NONE
    valid = True
    if beg > 0 or end < nfrg - 2:                                   # :589
        r = end - beg
        if beg > r:                                                 # :591
            valid = False
        else:
            k = r - beg                                             # :594
            k += 1
            if k > r:                                               # :595
                k = 0
            for j in range(nfrg):                                   # :596
                if int(uid[j]) != int(uid[beg + k]):                # :597
                    valid = False
                    break
                k += 1
                if k > r:                                           # :601
                    k = 0
    return (beg << 33 | end << 1 | rev) if valid else NONE          # :606


def path_of(uid, mc):
    """:657-668: the unit's vertices as 32-bit values; a reverse unit with elements 1 .. reversed, then every element ^ 1"""
    vt = [int(uid[j]) & M32 for j in range(mc >> 33, ((mc >> 1) & M32) + 1)]       # :661-662
    if mc & 1:                                                      # :663
        vt[1:] = vt[1:][::-1]                                       # :665
        vt = [x ^ 1 for x in vt]                                    # :666-667
    return vt


def path_cmp(x, y):
    """path_cmpfunc (:620-638)"""
    if len(x) != len(y):
        return (len(x) > len(y)) - (len(x) < len(y))
    for a, b in zip(x, y):
        if a != b:
            return (a > b) - (a < b)
    return 0


def extract(off, uid, sid):
    """:640-693: (mcs per record as uint64, the distinct paths in path_cmpfunc order, the number of records behind each)"""
    off = np.asarray(off, np.uint64).astype(np.int64)
    nr = max(len(off), 1) - 1
    mcs = np.full(nr, NONE, np.uint64)
    paths = []
    for i in range(nr):                                             # :647, :649
        rec = uid[int(off[i]):int(off[i + 1])]
        mc = unit_of(rec, sid)
        mcs[i] = mc
        if mc == NONE:                                              # :650
            continue
        paths.append(path_of(rec, mc))                              # :657-671
    paths.sort(key=functools.cmp_to_key(path_cmp))                  # :678
    out, cnt = [], []
    for p in paths:                                                 # :681-692
        if out and path_cmp(p, out[-1]) == 0:
            cnt[-1] += 1
        else:
            out.append(p)
            cnt.append(1)
    return mcs, out, cnt


def flat_paths(paths):
    """paths as the device keeps them: (MC_PATH_OFF, MC_PATH_V)"""
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.uint64)
    v = np.array([x for p in paths for x in p], np.uint32)
    return off, v


def find_arc1(G, v, w):
    """asmg_arc1 (graph.h:193-205) over a dict with idx_p, idx_n, arc_w, arc_del (and arc_ls): the first live arc v -> w, None if there is none"""
    p, n = int(G["idx_p"][v]), int(G["idx_n"][v])
    for x in range(p, p + n):
        if int(G["arc_w"][x]) == w and not int(G["arc_del"][x]):
            return x
    return None


def path_stats(G, vt):
    """:703-726 for one path: (len as uint32, wlen as double); G has vtx_len, vtx_cov, arc_ls beside find_arc1's fields.  A missing arc: None"""
    nv = len(vt)
    a = find_arc1(G, vt[nv - 1], vt[0])                             # :707
    if a is None:                                                   # :708
        return None
    ln = int(G["vtx_len"][vt[0] >> 1]) & M32                        # :709 (uint32_t len)
    cov = int(G["vtx_cov"][vt[0] >> 1])                             # :710
    wlen = float(cov) * ln                                          # :711
    ln = (ln - int(G["arc_ls"][a])) & M32                           # :712
    wlen -= float((cov * int(G["arc_ls"][a])) & M64)                # :712: an integer product, then a double
    for j in range(1, nv):                                          # :714
        len1 = int(G["vtx_len"][vt[j] >> 1]) & M32                  # :715
        cov = int(G["vtx_cov"][vt[j] >> 1])                         # :716
        ln = (ln + len1) & M32                                      # :717
        wlen += float(cov) * len1                                   # :718
        a = find_arc1(G, vt[j - 1], vt[j])                          # :719
        if a is None:                                               # :720
            return None
        ln = (ln - int(G["arc_ls"][a])) & M32                       # :721
        wlen -= float(cov) * float(int(G["arc_ls"][a]))             # :722
    return ln, wlen


# ---- the grouping key of the device's distinct-path step (oatk_amd/csrc/minicircle_core.hpp: mix64, hash_seed, hash_term, hash_mask) ----
def mix64(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    return x ^ (x >> 33)


def path_hash(vt, bits=0):
    h = mix64(len(vt))
    for t, e in enumerate(vt):
        h = (h + mix64((t << 32 | e) + 0x9E3779B97F4A7C15)) & M64
    return h if bits == 0 or bits >= 64 else h & ((1 << bits) - 1)


# ---- the table of the issue: anchor 5 (A+ = 10, A- = 11), B = 14/15, C = 18/19 ----
ANCHOR = 5
TABLE = [
    ([], None, None), ([10], None, None), ([10, 14], None, None),
    ([10, 10], (0, 0, 0), [10]),
    ([10, 14, 10], (0, 1, 0), [10, 14]),
    ([10, 14, 11], None, None), ([10, 14, 10, 14, 11], None, None),
    ([14, 10, 14, 10], (1, 2, 0), [10, 14]),
    ([18, 10, 14, 10], None, None),
    ([14, 18, 10, 14, 10], None, None),
    ([18, 14, 10, 18, 14, 10, 18], (2, 4, 0), [10, 18, 14]),
    ([11, 15, 11], (0, 1, 1), [10, 14]),
    ([11, 19, 15, 11], (0, 2, 1), [10, 14, 18]),
    ([10, 14, 18, 10], (0, 2, 0), [10, 14, 18]),
    ([10, 14, 10, 18, 10], None, None),
]
TABLE_PATHS = [([10], 1), ([10, 14], 3), ([10, 14, 18], 2), ([10, 18, 14], 1)]


def flat_records(records):
    """lists of uids -> (off uint64[n + 1], uid uint64[])"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.uint64)
    uid = np.array([x for r in records for x in r], np.uint64)
    return off, uid
