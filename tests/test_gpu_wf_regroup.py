"""GPU: the wave solver's alignment step with its lanes following the last diagonal alive (oatk_amd/csrc/ec_wave.hpp: ecw_step; r20).

A wavefront of n <= 32 diagonals gives each G = 64 / next_pow2(n) lanes, sixteen bases a lane and turn.  After an error all diagonals but one die in
their first window; from then on every lane compares for the survivor, 1024 bases a turn.  Which lanes compared which windows cannot change how far a
diagonal matches, so every result below is held against the CPU oracle (oracle_lib.Wavefront, as tests/test_gpu_levdist.py does) with the regrouping
on and off (oatk_hip_debug_wf_ed_turns), and the TURNS are held against a model of the step's loop (`Model`, pinned to the oracle's results without a
device): equal in both forms, and fewer with the regrouping wherever a lone survivor of a wavefront of 2 .. 64 diagonals is more than one turn of its
group from the end of its run -- which is what shows that the new path ran.

Directed jobs: targets of 300, 600, 1100, 2100, 3000 and a few of 6000 bases; 1 .. 4 substitutions, insertions and deletions (the survivor is the
middle, the highest, the lowest diagonal) at base 0, at 16 j +- 1, 256 j +- 1, 1024 j +- 1 and in the last sixteen bases; a query that runs past the
target and one that ends before it (an end is reached in a regrouped turn: the lowest-diagonal rule); period-2 and period-4 repeats, where several
diagonals live for many turns before one is left; queries lengthened two or three times; bands 2, 6, 12, 40 with jobs cut off by the band."""
import functools

import numpy as np
import pytest

import adversarial as A
import oracle_lib as O

pytestmark = pytest.mark.gpu

INT_MIN = -(1 << 31)
CODE = np.full(256, 255, np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    CODE[_ch] = _i


class Model:
    """ecw_step on the CPU: the wavefront, what it returns, and the extension turns it takes with the lanes regrouped (`on`) and not (`off`)"""

    def __init__(self, ts, bw):
        self.t, self.tl, self.bw = CODE[np.frombuffer(ts, np.uint8)], len(ts), bw
        self.k, self.d0, self.score = [-1], 0, 0
        self.t_end = self.q_end = -1
        self.on = self.off = 0
        self.must_gain = False        # a lone survivor of 2 .. 64 diagonals with more than a turn of its group left
        self.shared = 0               # turns that two or more diagonals of a wavefront of up to 64 survived

    def _runs(self, q, ql):
        """per diagonal: (active at entry, furthest k)"""
        out = []
        for j, kk in enumerate(self.k):
            dd = self.d0 + j
            act = not (kk >= self.tl or kk + dd >= ql)
            lim = min(ql - dd, self.tl) - 1
            if act and lim > kk:
                ne = np.flatnonzero(self.t[kk + 1:lim + 1] != q[kk + dd + 1:lim + dd + 1])
                kk += int(ne[0]) if len(ne) else lim - kk
            out.append((act, kk))
        return out

    def _count(self, runs):
        n = len(self.k)
        adv = [(kk - k0) for (act, kk), k0 in zip(runs, self.k) if act]
        if n > 64:                    # one lane a diagonal, four rounds of 64 side by side: ends are looked for round by round (of 256)
            for base in range(0, n, 256):
                part = [(kk - k0) for (act, kk), k0 in list(zip(runs, self.k))[base:base + 256] if act]
                t = max((a // 16 + 1 for a in part), default=0)
                self.on, self.off = self.on + t, self.off + t
                if any(self._reached(j, runs) for j in range(base, min(n, base + 256))):
                    break
            return
        if not adv:
            return
        G = 64 if n <= 1 else (64 >> (n - 1).bit_length() if n <= 32 else 1)
        turns = sorted(a // (16 * G) + 1 for a in adv)
        self.off += turns[-1]
        on = turns[-1]
        for t in range(1, turns[-1]):
            alive = [a for a in adv if a // (16 * G) + 1 > t]
            if len(alive) == 1 and G < 64:
                left = alive[0] - 16 * G * t
                on = t + left // 1024 + 1
                self.must_gain |= left > 16 * G
                break
            self.shared += 1
        self.on += on

    def _reached(self, j, runs):
        act, kk = runs[j]
        return act and (kk + self.d0 + j == self._ql - 1 or kk == self.tl - 1)

    def step(self, qs):
        """wf_ed_core resumed with the query qs (ecw_wf_ed_kernel's loop): (score, t_end, q_end)"""
        q, ql = CODE[np.frombuffer(qs, np.uint8)], len(qs)
        self._ql = ql
        while True:
            runs = self._runs(q, ql)
            self._count(runs)
            n = len(self.k)
            hit = [j for j in range(n) if self._reached(j, runs)]
            if hit:
                jf = hit[0]
                for j in range(jf):
                    if runs[j][0]:
                        self.k[j] = runs[j][1]
                self.t_end, self.q_end = runs[jf][1], runs[jf][1] + self.d0 + jf
                break
            k = [kk if act else k0 for (act, kk), k0 in zip(runs, self.k)]
            nk = []
            for i in range(n + 2):
                jj = i - 1
                v = k[jj - 1] if jj - 1 >= 0 else INT_MIN
                if 0 <= jj < n and k[jj] + 1 > v:
                    v = k[jj] + 1
                if jj + 1 < n and k[jj + 1] + 1 > v:
                    v = k[jj + 1] + 1
                nk.append(v)
            st, en, nd0 = 0, n + 2, self.d0 - 1
            if self.bw < 0 or n < 2 * self.bw + 1:
                st += nd0 < -self.tl
                en -= nd0 + n + 1 > ql
            else:
                lo, hi = max(-self.bw, -self.tl), max(self.bw, ql)
                while nd0 + st < lo:
                    st += 1
                while nd0 + en - 1 > hi:
                    en -= 1
            self.k, self.d0 = nk[st:en], nd0 + st
            self.t_end = self.q_end = -1
            self.score += 1
            if self.bw >= 0 and self.score > self.bw:
                break
        return (self.score, self.t_end + 1, self.q_end + 1)


def edit(ts, edits):
    """the query: `ts` with (position, kind) applied from the back -- 0 a substitution, 1 a base inserted in the query, 2 a base of the target left out"""
    q = bytearray(ts)
    for p, kind in sorted(set(edits), reverse=True):
        if kind == 0:
            q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1 + p % 3) % 4]
        elif kind == 1:
            q.insert(p, b"ACGT"[(b"ACGT".index(q[p]) + 2) % 4])
        else:
            del q[p]
    return bytes(q)


def places(tl):
    ps = {0, tl - 16, tl - 9, tl - 2}
    for unit, js in ((16, (1, 2, 7)), (256, (1, 2, 3, 5, 8, 11)), (1024, (1, 2, 3, 5))):
        for j in js:
            ps |= {unit * j - 1, unit * j + 1}
    return sorted(p for p in ps if 0 <= p < tl - 1)


def steps_of(it, ql):
    """the query in one go, or lengthened two or three times"""
    if it % 3 == 0:
        return [ql]
    cuts = [ql * 2 // 5, ql * 7 // 10] if it % 3 == 1 else [max(1, ql // 4), ql // 2, ql - 3]
    return sorted(set(c for c in cuts if 1 <= c < ql)) + [ql]


@functools.lru_cache(maxsize=None)
def cases():
    """(jobs, the oracle's results, the models): built once, shared, never changed"""
    rng = np.random.default_rng(2020)
    raw = []                                                    # (target, query, band, tag)
    it = 0
    for tl in (300, 600, 1100, 2100, 3000):
        ps = places(tl)
        for i in range(36):
            ts = A.rand_dna(rng, tl)
            n_ed = 1 + i % 4
            first = ps[(5 * i + tl) % len(ps)]
            rest = [int(rng.integers(0, tl - 1)) if (i + e) % 2 else ps[(7 * i + 3 * e) % len(ps)] for e in range(n_ed - 1)]
            edits = [(p, (i + e) % 3) for e, p in enumerate([first] + rest)]
            q = edit(ts, edits)
            if i % 6 == 1:
                q = q + A.rand_dna(rng, 40 + 7 * i)             # the query runs past the target
            elif i % 6 == 4:
                q = q[:len(q) - 20 - 9 * i]                     # the target runs past the query
            raw.append((ts, q, (2, 6, 12, 40)[(i + i // 4) % 4], "edits"))              # (every band with every number of edits: three or four edits in a band of 2 are cut off)
            it += 1
    for i in range(8):                                          # a handful of 6000
        ts = A.rand_dna(rng, 6000)
        ps = places(6000)
        edits = [(ps[(11 * i + 5 * e) % len(ps)], (i + e) % 3) for e in range(1 + i % 4)]
        q = edit(ts, edits)
        q = q + A.rand_dna(rng, 100) if i % 4 == 1 else (q[:-700] if i % 4 == 3 else q)
        raw.append((ts, q, (6, 12, 40, 2)[i % 4], "long"))
    for i in range(16):                                         # repeats: the diagonals a period apart match as long as the repeat lasts
        unit = (b"AC", b"ACGT")[i % 2]
        rep = (300, 700, 1300, 2200)[i // 4]
        ts = A.rand_dna(rng, 40) + unit * (rep // len(unit)) + A.rand_dna(rng, (500, 1500)[(i // 2) % 2])
        # as many substitutions as the period: the last far behind the others (which are neighbours), so that the diagonals a period off run from the first ones to the last beside diagonal 0
        edits = [(45 + e + (16 * i) % 64, 0) for e in range(len(unit) - 1)] + [(40 + rep * 2 // 3 + i, 0)] + ([(len(ts) - 100, 1 + i % 2)] if i % 4 >= 2 else [])
        raw.append((ts, edit(ts, edits), (12, 40, 6)[i % 3], "repeat"))
    for i in range(8):                                          # error-dense behind a clean stretch: the wavefront grows past 32 and past 64 diagonals, or the band cuts it off
        ts = A.rand_dna(rng, (600, 2100)[i % 2])
        q = ts[:300 + 100 * i] + A.rand_dna(rng, 300)
        raw.append((ts, q, (2, 6, 12, 40)[i % 4] if i < 6 else 100, "dense"))
    jobs, want, models, tags = [], [], [], []
    for it, (ts, q, bw, tag) in enumerate(raw):
        w, m = O.Wavefront(ts, bw), Model(ts, bw)
        steps, res = [], []
        for ql in steps_of(it, len(q)):
            r = w.step(q[:ql])
            assert m.step(q[:ql]) == r, (it, tag, bw, ql)      # the model is the oracle's wavefront
            steps.append(ql), res.append(r)
            if r[0] > bw:
                break
        w.close()
        jobs.append((ts, q, bw, steps)), want.append(res), models.append(m), tags.append(tag)
    return jobs, want, models, tags


def test_regrouped_lanes_change_no_result_and_save_turns(hip):
    jobs, want, models, tags = cases()
    assert 190 <= len(jobs) <= 240
    on, t_on = hip.wf_ed_turns(jobs, regroup=True)
    off, t_off = hip.wf_ed_turns(jobs, regroup=False)
    plain = hip.wf_ed(jobs)                                     # (the entry point without the switch runs what ships)
    n_gain = 0
    for j, m in enumerate(models):
        what = (j, tags[j], jobs[j][2], jobs[j][3])
        assert on[j] == want[j] and off[j] == want[j] and plain[j] == want[j], (what, on[j], off[j], plain[j], want[j])
        assert t_on[j] <= t_off[j], (what, t_on[j], t_off[j])
        if m.must_gain:
            assert t_on[j] < t_off[j], (what, t_on[j], t_off[j])
            n_gain += 1
        assert (t_on[j], t_off[j]) == (m.on, m.off), (what, t_on[j], t_off[j], m.on, m.off)
    print("turns: %d regrouped, %d not, over %d jobs (%d with a lone survivor far from its end)" % (sum(t_on), sum(t_off), len(jobs), n_gain))
    assert n_gain > len(jobs) // 2


def test_the_cases_are_what_they_are_meant_to_be():
    """(no device needed beyond the module's mark: what the directed jobs contain)"""
    jobs, want, models, tags = cases()
    cut = [j for j, (job, w) in enumerate(zip(jobs, want)) if w[-1][0] > job[2]]
    assert len(cut) >= 10 and {jobs[j][2] for j in cut} >= {2, 6, 12}                            # cut off by the band
    assert sum(1 for j in jobs if len(j[3]) >= 3) > 40 and sum(1 for j in jobs if len(j[3]) == 1) > 40
    assert any(w[-1][0] > 32 for w in want) and any(w[-1][0] > 64 for w in want)                # one lane a diagonal, and the path that is not touched
    rep = [m for m, t in zip(models, tags) if t == "repeat"]
    assert sum(1 for m in rep if m.shared >= 2 and m.must_gain) >= 6                             # several survivors for turns, then one
    ends = [j for j, (job, w) in enumerate(zip(jobs, want)) if w[-1][0] <= job[2] and (w[-1][1] < len(job[0]) or w[-1][2] < len(job[1]))]
    assert len(ends) >= 20                                                                       # one string runs past the other
    assert any(models[j].must_gain and models[j].off - models[j].on >= 8 for j in range(len(jobs)) if len(jobs[j][0]) >= 3000)
