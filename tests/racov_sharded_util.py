"""Shared by tests/test_gpu_racov_sharded.py and tests/test_racov_sharded_abi.py: the synthetic set of tests/test_gpu_racov.py cut by read
into per-rank slices, and what a shard boundary cuts through -- derived from the read list by the reference's rules (syncasm.c:1756-1878 for
the blocks, :2083-2129 for the duplets), restated here because the reference exposes no per-read counts."""
import math

import numpy as np

import test_gpu_racov as RC


def cut_slices(reads, bounds):
    """per rank: (aln, chains) of reads[bounds[r]:bounds[r + 1]] -- this rank's records in the order of the whole set, sid = index into its own chains"""
    out = []
    for r in range(len(bounds) - 1):
        part = reads[bounds[r]:bounds[r + 1]]
        sid, off, s, uid, ub, ue, sb, se = [], [0], [], [], [], [], [], []
        for i, (_, recs) in enumerate(part):
            for sc, frags in recs:
                sid.append(i), s.append(sc)
                for f in frags:
                    uid.append(f[0]), ub.append(f[1]), ue.append(f[2]), sb.append(f[3]), se.append(f[4])
                off.append(len(uid))
        aln = {"sid": np.array(sid, np.uint32), "off": np.array(off, np.uint64), "s": np.array(s, np.float64), "uid": np.array(uid, np.uint64),
               "u_beg": np.array(ub, np.uint32), "u_end": np.array(ue, np.uint32), "s_beg": np.array(sb, np.uint32), "s_end": np.array(se, np.uint32)}
        n = np.array([len(c) for c, _ in part], np.uint64)
        chains = (np.concatenate([[0], np.cumsum(n)]).astype(np.uint64), np.array([x << 1 for c, _ in part for x in c], np.uint64))
        out.append((aln, chains))
    return out


def whole(reads):
    return cut_slices(reads, [0, len(reads)])[0]


# what the shard boundary has to cut through, from the inputs alone (the reference's rules restated on the read list):
SU_COUNT = {}
for _u, _lst in enumerate(RC.UTG):
    for _s in _lst:
        SU_COUNT[_s] = SU_COUNT.get(_s, 0) + 1
ARC_OF = {(a[0], a[1]): a for a in RC.ARCS}


def fractional_unitigs(read):
    """unitigs that receive fractional (multi-member-block) contributions from this read for sure: it has two or more records, each of one
    fragment whose stretch of the read equals the unitig's stretch (one LCS block per record, so make_ma_block yields blocks of all records)"""
    chain, recs = read
    if len(recs) < 2:
        return set()
    us = set()
    for _, frags in recs:
        if len(frags) != 1:
            return set()
        uid, ub, ue, sb, se = frags[0]
        lst = RC.UTG[uid >> 1][ub:ue + 1]
        if uid & 1:
            lst = lst[::-1]
        if chain[sb:se + 1] != lst:
            return set()
        us.add(uid >> 1)
    return us if len(us) >= 2 else set()


def duplet_events(read):
    """(link id, self-complementary) of every duplet this read puts (syncasm.c:2083-2129)"""
    ev = []
    for sc, frags in read[1]:
        if len(frags) < 2:
            continue
        score = math.modf(sc)[0]
        if score < np.finfo(np.float64).eps:
            score = 1.0
        uniq = [score >= .99 or any(SU_COUNT[x] == 1 for x in RC.UTG[f[0] >> 1][f[1]:f[2] + 1]) for f in frags]
        for j in range(1, len(frags)):
            a = ARC_OF[(frags[j - 1][0], frags[j][0])]
            if uniq[j - 1] and uniq[j]:
                ev.append((a[2], (a[0] ^ 1) == a[1]))
    return ev


def boundary_facts(reads, b):
    """for the cut reads[:b] | reads[b:]: unitigs with fractional contributions from both ranks, links with events from both ranks, and
    whether the self-complementary arc's first event and a later one lie on different ranks"""
    fr = [set().union(*[fractional_unitigs(r) for r in part]) if part else set() for part in (reads[:b], reads[b:])]
    ev = [[e for r in part for e in duplet_events(r)] for part in (reads[:b], reads[b:])]
    links = {l for l, _ in ev[0]} & {l for l, _ in ev[1]}
    self_split = any(s for _, s in ev[0]) and any(s for _, s in ev[1])
    return fr[0] & fr[1], links, self_split
