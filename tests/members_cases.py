"""One small batch on which the four consumers of "a CpG member" (include/hifimeth_hip.h) must agree -- the motif-0 records, the
windows of `pileup -E`, MOD / CANON of `pileup -M` and the pairs of `pileup -L` -- and the derivation of the last three from the
first (plain module, imported by test_pileup_members_cpu.py and test_gpu_pileup_members.py).

    genome()    mA (3300 b) and mB (2800 b), CpGs planted one by one at A_CPGS / B_CPGS
    reads()     four records in input order, HP none, 1, 2, 1; 4550 aligned columns in one batch:
                  fwd_tile   mA 0 .. 1599 forward, column == reference offset: the C of 1023 is the last column of the projection's
                             first 1024-column tile, 1010 .. 1040 lie on both sides of it
                  rev_gaps   mA from 1700, reverse, S5 M200 I2 M150 D2 M200 N10 M700 S4: 1899 | 1900 split by the I, the D removes
                             the CpG 2050, 2251 is the last column before the N, 2262 the first behind it, 2961 the alignment's last
                  end_on_c   mB 100 .. 999 forward, mapq 10: ends on the C of the CpG 999
                  mm_on_g    mB 1100 .. 1899 forward: a stored mismatch on the G of the CpG 1150, 40 more over 1252 .. 1291 (94.9 %
                             identity); its columns 345 | 346 (the CpG 1445) are the batch's columns 4095 | 4096
    FILTERS     (min_mapq, min_pi) that drop end_on_c by -q and mm_on_g by -f and nothing else
    derive(members, chrs, ...)   from [(hp, {gpos: ML byte})] per record and the reference text alone: n_mod / n_canon per
                reference CpG and set, the k = 2 window counts, the four pair counts per distance
"""
import numpy as np

import bedmethyl_cases as B
from patterns_cases import _background

A_CPGS = (100, 104, 110, 160, 600, 640, 1010, 1018, 1023, 1030, 1040, 1500, 1560, 1750, 1790, 1830, 1899, 2000, 2040, 2050, 2056, 2100,
          2251, 2262, 2300, 2350, 2390, 2900, 2950, 2961)
B_CPGS = (150, 152, 200, 260, 500, 540, 999, 1150, 1200, 1230, 1260, 1400, 1440, 1445, 1800)
THR = 128
K = 2
MAX_DIST = 64
HPS = (0, 1, 2, 1)
FILTERS = (20, 97.0)
_CACHE = {}


def genome():
    if "genome" not in _CACHE:
        rng = np.random.default_rng(6101)
        out = []
        for name, n, cpgs in (("mA", 3300, A_CPGS), ("mB", 2800, B_CPGS)):
            s = _background(rng, n)
            for g in cpgs:
                s[g], s[g + 1] = "C", "G"
            out.append((name, "".join(s)))
        _CACHE["genome"] = out
    return _CACHE["genome"]


def reads():
    if "reads" not in _CACHE:
        rng = np.random.default_rng(6102)
        g = genome()
        mk = lambda *a, **kw: B.make_read(*a, rng, chroms=g, **kw)
        _CACHE["reads"] = [
            mk("fwd_tile", 0, 0, 0, [("M", 1600)], probs={1010: THR, 1018: THR - 1, 1023: 255, 1030: 0, 1040: THR}, drop=(600,)),
            mk("rev_gaps", 16, 0, 1700, [("S", 5), ("M", 200), ("I", 2), ("M", 150), ("D", 2), ("M", 200), ("N", 10), ("M", 700), ("S", 4)],
               probs={1750: THR, 1790: THR - 1, 2262: THR, 2300: THR - 1}, hp=1),
            mk("end_on_c", 0, 1, 100, [("M", 900)], mapq=10, probs={150: THR - 1, 152: THR}, hp=2),
            mk("mm_on_g", 0, 1, 1100, [("M", 51), ("X", 1), ("M", 100), ("X", 40), ("M", 608)], probs={1440: THR, 1445: THR - 1}, hp=1)]
    return _CACHE["reads"]


def as_dict(r):
    return dict(flag=r.flag, tid=r.tid, pos=r.pos, mapq=r.mapq, cigar=r.cigar, seq=r.seq, mm=r.mm, ml=r.ml)


def offsets(chrs):
    return np.concatenate([[0], np.cumsum([len(s) for _n, s in chrs])])


def reference_cpgs(chrs):
    """concatenated offsets of the C of every CG that lies in one sequence, ascending, and the sequence of each"""
    off = offsets(chrs)
    pos, sid = [], []
    for i, (_n, s) in enumerate(chrs):
        b = np.frombuffer(s.encode(), np.uint8)
        at = np.nonzero((b[:-1] == 67) & (b[1:] == 71))[0]
        pos.append(at + off[i])
        sid.append(np.full(len(at), i))
    return np.concatenate(pos), np.concatenate(sid)


def derive(members, chrs, thr=THR, span=150, max_dist=MAX_DIST):
    """members: [(hp, {gpos: ML byte})] per record -> (bed, pat, link):
    bed[s] = {gpos: (n_mod, n_canon)} of the reference CpGs with a member in set s (0 all, 1 / 2 the records of that hp);
    pat = {gpos of the first locus: [4 counts]} over the pairs of adjacent reference CpGs of one sequence at most `span` apart,
    pattern bit i = locus i methylated; link = {d: [UU, UM, MU, MM]}, 2 <= d <= max_dist, first letter = the lower coordinate"""
    cpg, sid = reference_cpgs(chrs)
    is_cpg = set(int(g) for g in cpg)
    bed = [{}, {}, {}]
    pat, link = {}, {}
    win = np.nonzero((sid[1:] == sid[:-1]) & (cpg[1:] - cpg[:-1] <= span))[0]
    for hp, mem in members:
        assert set(mem) <= is_cpg
        for g, p in mem.items():
            for s in {0, hp}:
                c = bed[s].setdefault(g, [0, 0])
                c[0 if p >= thr else 1] += 1
        for r in win:
            a, b = int(cpg[r]), int(cpg[r + 1])
            if a in mem and b in mem:
                pat.setdefault(a, [0, 0, 0, 0])[(mem[a] >= thr) + 2 * (mem[b] >= thr)] += 1
        g = np.array(sorted(mem), np.int64)
        m = np.array([mem[int(x)] >= thr for x in g], np.int64)
        for i in range(len(g)):
            d = g[i + 1:] - g[i]
            for j in np.nonzero((d >= 2) & (d <= max_dist))[0]:
                link.setdefault(int(d[j]), [0, 0, 0, 0])[2 * m[i] + m[i + 1 + j]] += 1
    return [{g: tuple(c) for g, c in b.items()} for b in bed], pat, link
