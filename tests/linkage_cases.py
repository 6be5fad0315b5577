"""Hand-built inputs for `pileup -L` beyond patterns_cases (plain module, imported by test_pileup_linkage_cpu.py and
test_gpu_pileup_linkage.py), one per way the pair kernels can go wrong.

    genome()    patterns_cases.genome() (chr1 .. chr3) + lk (600 b, CpGs at LK) + big (20 kb, CpGs at big_cpgs())
    reads()     patterns_cases.reads() + the records below, sorted by (tid, pos); long_f stays the first record, so in a batch that
                starts with it column == reference offset: the members 1018 | 1030 of chr1 pair across the projection's 1024-column
                tile edge, and the batch's column 4096 (the selection's block edge) falls inside the third record
    crowd()     300 copies of eq_f, a record with all five members of lk: every pair's three atomics meet 299 others

lk, with MAX_DIST = 400: 50 | 52 are the nearest two CpGs can be (d = 2), 50 | 450 lie exactly MAX_DIST apart, 60 | 461 one more.
  adj_a, adj_b    two overlapping records (40 .. 54 and 53 .. 472) next to each other in the input: the last member of one (52) and
                  the first of the next (60) must not pair
  twin            the same two alignments under ONE read name (primary + supplementary): still no pair between them
  single          a record with one member
  reach           all five members in one run: d == MAX_DIST counts, MAX_DIST + 1 does not
  gapD, gapN      members on both sides of a 300-base D / N: pairs whose loci lie in different runs
  eq              ML bytes THR, THR, THR - 1, THR - 1, 255 at the five loci: pa == pb on either side of the threshold, pa == t next to
                  pb == t - 1 (MU)
each on both strands.  big: two records (one per strand) of 17 kb on 20 kb: d reaches 16 384 (100 | 16484, 102 | 16486) and passes
it (100 | 16486).
"""
import numpy as np

import patterns_cases as K
from hifimeth_amd.synth import AlignedRead, revcomp
from pileup_cases import build_seq

LK = (50, 52, 60, 450, 461)
MAX_DIST = 400
THR = K.THR
LK_TID, BIG_TID = 3, 4
_BIG_FIXED = (100, 102, 16484, 16486, 16600)
_CACHE = {}


def big_cpgs():
    if "big_cpgs" not in _CACHE:
        rng = np.random.default_rng(4201)
        c = set(_BIG_FIXED)
        for g in rng.integers(200, 19000, 110):
            if all(abs(int(g) - x) >= 2 for x in c):
                c.add(int(g))
        _CACHE["big_cpgs"] = tuple(sorted(c))
    return _CACHE["big_cpgs"]


def genome():
    if "genome" not in _CACHE:
        rng = np.random.default_rng(4202)
        out = list(K.genome())
        for name, n, cpgs in (("lk", 600, LK), ("big", 20000, big_cpgs())):
            s = K._background(rng, n)
            for g in cpgs:
                s[g], s[g + 1] = "C", "G"
            out.append((name, "".join(s)))
        _CACHE["genome"] = out
    return _CACHE["genome"]


def make_read(name, flag, tid, pos, spec, rng, mapq=60, probs=None):
    """patterns_cases.make_read on this genome: a 5mC call on every C of the forward strand, ML random, except
    probs = {reference offset of a CpG's C: ML byte}"""
    seq = build_seq(genome()[tid][1], pos, spec, rng)
    L, rev = len(seq), bool(flag & 16)
    fwd = revcomp(seq) if rev else seq
    q = K._qidx(spec, pos)
    fixed = {((L - 1 - (q[g] + 1)) if rev else q[g]): p for g, p in (probs or {}).items()}
    ml = [fixed.get(i, int(rng.integers(0, 256))) for i, ch in enumerate(fwd) if ch == "C"]
    return AlignedRead(name, flag, tid, pos, mapq, [(it[0], it[1]) for it in spec], seq, "C+m" + ",0" * len(ml) + ";", np.array(ml, np.uint8))


def own_reads():
    """the records this module adds, in input order"""
    if "own" in _CACHE:
        return _CACHE["own"]
    rng = np.random.default_rng(4203)
    EQ = {50: THR, 52: THR, 60: THR - 1, 450: THR - 1, 461: 255}
    out = []
    for flag, t in ((0, "f"), (16, "r")):
        out += [make_read("reach_" + t, flag, LK_TID, 40, [("M", 440)], rng),
                make_read("gapD_" + t, flag, LK_TID, 40, [("M", 30), ("D", 300), ("M", 110)], rng),
                make_read("gapN_" + t, flag, LK_TID, 40, [("M", 30), ("N", 300), ("M", 110)], rng),
                make_read("eq_" + t, flag, LK_TID, 40, [("M", 440)], rng, probs=EQ),
                make_read("single_" + t, flag, LK_TID, 440, [("M", 15)], rng),
                make_read("big_" + t, flag, BIG_TID, 50, [("M", 17000)], rng)]
    for flag, t in ((0, "f"), (16, "r")):            # the last records at 40 ...
        out += [make_read("twin_" + t, flag, LK_TID, 40, [("M", 15)], rng), make_read("adj_a_" + t, flag, LK_TID, 40, [("M", 15)], rng)]
    for flag, t in ((0, "f"), (16, "r")):            # ... and the only ones at 53: adj_a_r | adj_b_f are neighbours after the sort
        out += [make_read("adj_b_" + t, flag, LK_TID, 53, [("M", 420)], rng), make_read("twin_" + t, flag | 2048, LK_TID, 53, [("M", 420)], rng)]
    _CACHE["own"] = out
    return out


def reads():
    if "reads" not in _CACHE:
        out = sorted(K.reads() + own_reads(), key=lambda r: (r.tid, r.pos))      # stable
        assert out[0].name == "long_f"
        _CACHE["reads"] = out
    return _CACHE["reads"]


def crowd(n=300):
    if ("crowd", n) not in _CACHE:
        _CACHE[("crowd", n)] = [next(r for r in own_reads() if r.name == "eq_f")] * n
    return _CACHE[("crowd", n)]


as_dict = K.as_dict
