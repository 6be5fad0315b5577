"""Hand-built inputs for `pileup -M` (plain module, imported by test_pileup_bedmethyl_cpu.py and test_gpu_pileup_bedmethyl.py): a
genome whose CpGs are planted one by one, and reads that each put one rule of the definition on a known CpG.

    genome()    chr1 (1600 b): CpGs at CHR1, a G behind the one at 200 (reference CGG); ends in C.  chr2 (300 b): begins with G
                (chr1's last C + this G spell no CpG); its CpG at 250 is only ever seen deleted.  chr3 (500 b): CpGs at CHR3, the last one on the last two bases of the job.
    reads()     sorted by (tid, pos); the first is a forward read of all of chr1 that lost its calls at 1023 and 1030, so in a batch
                that starts with it column == reference offset and those two lie on both sides of the projection's 1024-column tile
                edge (the C of 1023 is the tile's last column); the second, also 1600 columns, has a mismatch on the G of 447, whose C
                is column 2047
    dense()     10 kb of CGCGCG.. (5000 reference CpGs: more than one 4096 block of ranks) and a few 4 kb reads on it
"""
import numpy as np

from hifimeth_amd.synth import AlignedRead, revcomp
from pileup_cases import build_seq

CHR1 = (0, 100, 104, 110, 120, 200, 300, 447, 455, 1023, 1030, 1400)
CHR2 = (150, 250)
CHR3 = (50, 60, 75, 90, 498)
THR = 128
_CACHE = {}


def _background(rng, n):
    s = ["ACGT"[int(x)] for x in rng.integers(0, 4, n)]
    for i in range(1, n):
        if s[i - 1] == "C" and s[i] == "G":
            s[i] = "A"
    return s


def genome():
    if "genome" not in _CACHE:
        rng = np.random.default_rng(5201)
        out = []
        for name, n, cpgs in (("chr1", 1600, CHR1), ("chr2", 300, CHR2), ("chr3", 500, CHR3)):
            s = _background(rng, n)
            for g in cpgs:
                s[g], s[g + 1] = "C", "G"
                if g + 2 < n and s[g + 2] == "G":      # no CGG by chance
                    s[g + 2] = "A"
                if g and s[g - 1] == "C":              # the planted C makes no CC G.. run into a second CpG; and no CCG by chance
                    s[g - 1] = "A"
            out.append([name, s])
        out[0][1][202] = "G"                           # CGG at 200: a reverse read's CHG
        out[0][1][-1] = "C"
        out[0][1][-2] = "A"
        out[1][1][0] = "G"
        _CACHE["genome"] = [(n, "".join(s)) for n, s in out]
    return _CACHE["genome"]


def _qidx(spec, pos):
    """reference offset -> index in SEQ as stored, for the columns of the M / = / X ops (the walk of pileup_cases.build_seq)"""
    out, q, si = {}, 0, pos
    for k, item in enumerate(spec):
        op, n = item[0], item[1]
        if op == "S":
            q += n if k == 0 else 0
        elif op in "M=X":
            for _ in range(n):
                out[si] = q
                q += 1
                si += 1
        elif op == "I":
            q += n
        elif op in "DN":
            si += n
    return out


def make_read(name, flag, tid, pos, spec, rng, mapq=60, probs=None, drop=(), chroms=None, calls=True, hp=None):
    """a record with a 5mC call (C+m) on every C of its forward strand, ML random, except: probs = {reference offset of a CpG's C:
    ML byte} sets the call the projection looks up for that locus, drop = those loci lose their call; calls=False: no MM / ML"""
    chroms = chroms or genome()
    seq = build_seq(chroms[tid][1], pos, spec, rng)
    L, rev = len(seq), bool(flag & 16)
    fwd = revcomp(seq) if rev else seq
    q = _qidx(spec, pos)
    at = lambda g: (L - 1 - (q[g] + 1)) if rev else q[g]
    fixed = {at(g): p for g, p in (probs or {}).items()}
    gone = {at(g) for g in drop}
    deltas, ml, skipped = [], [], 0
    for i, ch in enumerate(fwd):
        if ch != "C":
            continue
        if i in gone:
            skipped += 1
            continue
        deltas.append(skipped)
        skipped = 0
        ml.append(fixed.get(i, int(rng.integers(0, 256))))
    ok = calls and deltas
    mm = "C+m" + "".join(",%d" % d for d in deltas) + ";" if ok else None
    return AlignedRead(name, flag, tid, pos, mapq, [(it[0], it[1]) for it in spec], seq, mm, np.array(ml, np.uint8) if ok else None, hp)


def reads():
    if "reads" in _CACHE:
        return _CACHE["reads"]
    rng = np.random.default_rng(5202)
    A = {100: THR, 104: THR - 1, 110: 255, 120: 0}
    out = [make_read("long_nocall", 0, 0, 0, [("M", 1600)], rng, drop=(1023, 1030)),
           make_read("long_mmG448", 0, 0, 0, [("M", 448), ("X", 1), ("M", 1151)], rng),
           make_read("long_r", 16, 0, 0, [("M", 1600)], rng),
           make_read("head", 0, 0, 0, [("M", 50)], rng)]
    for flag, t in ((0, "f"), (16, "r")):
        out += [make_read("A_eq_" + t, flag, 0, 80, [("M", 100)], rng, probs=A),
                make_read("A_nocall110_" + t, flag, 0, 80, [("M", 100)], rng, drop=(110,)),
                make_read("A_mmC104_" + t, flag, 0, 80, [("M", 24), ("X", 1), ("M", 75)], rng),
                make_read("A_mmG105_" + t, flag, 0, 80, [("M", 25), ("X", 1), ("M", 74)], rng),
                make_read("A_ins_" + t, flag, 0, 80, [("M", 25), ("I", 3), ("M", 75)], rng),
                make_read("A_delG_" + t, flag, 0, 80, [("M", 25), ("D", 1), ("M", 74)], rng),
                make_read("A_delC_" + t, flag, 0, 80, [("M", 24), ("D", 1), ("M", 75)], rng),
                make_read("A_delCG_" + t, flag, 0, 80, [("M", 24), ("D", 2), ("M", 74)], rng),
                make_read("A_del3_" + t, flag, 0, 80, [("M", 19), ("D", 13), ("M", 68)], rng),
                make_read("A_skipCG_" + t, flag, 0, 80, [("M", 24), ("N", 2), ("M", 74)], rng),
                make_read("A_skipG_" + t, flag, 0, 80, [("M", 25), ("N", 1), ("M", 74)], rng),
                make_read("A_mix_" + t, flag, 0, 80, [("=", 15), ("X", 1), ("M", 9), ("D", 0), ("M", 11), ("=", 64)], rng),
                make_read("A_endC_" + t, flag, 0, 80, [("M", 31)], rng),
                make_read("A_endC_I_more_" + t, flag, 0, 80, [("M", 31), ("I", 2), ("M", 50)], rng),
                make_read("A_endC_I_" + t, flag, 0, 80, [("M", 31), ("I", 2)], rng),
                make_read("A_beginG_" + t, flag, 0, 105, [("M", 50)], rng),
                make_read("A_clip_" + t, flag, 0, 80, [("S", 5), ("M", 100), ("S", 4)], rng),
                make_read("A_secondary_" + t, flag | 256, 0, 80, [("M", 100)], rng),
                make_read("A_noentries_" + t, flag, 0, 80, [("M", 100)], rng, calls=False),
                make_read("A_mapq10_" + t, flag, 0, 80, [("M", 100)], rng, mapq=10),
                make_read("A_lowid_" + t, flag, 0, 80, [("M", 10), ("X", 4), ("M", 86)], rng),       # 96 %
                make_read("cgg_" + t, flag, 0, 190, [("M", 120)], rng),
                make_read("c1end_" + t, flag, 0, 1380, [("M", 220)], rng),
                make_read("c2_" + t, flag, 1, 0, [("M", 200)], rng),
                make_read("c2del_" + t, flag, 1, 220, [("M", 20), ("D", 20), ("M", 30)], rng),
                make_read("c3_" + t, flag, 2, 30, [("M", 100)], rng),
                make_read("c3del_" + t, flag, 2, 30, [("M", 15), ("D", 50), ("M", 35)], rng),        # 45 .. 94: four CpGs
                make_read("c3end_" + t, flag, 2, 400, [("M", 100)], rng)]
    out.append(AlignedRead("unmapped", 4, 0, 80, 0, [("M", 100)], out[4].seq, out[4].mm, out[4].ml))
    out.sort(key=lambda r: (r.tid, r.pos))      # stable: the long reads stay the first records
    assert out[0].name == "long_nocall" and out[1].name == "long_mmG448"
    _CACHE["reads"] = out
    return out


def as_dict(r):
    return dict(flag=r.flag, tid=r.tid, pos=r.pos, mapq=r.mapq, cigar=r.cigar, seq=r.seq, mm=r.mm, ml=r.ml)


def with_hp(rs):
    """the same reads tagged HP 1, HP 2, none, in turn"""
    import dataclasses
    return [dataclasses.replace(r, hp=(1, 2, None)[i % 3]) for i, r in enumerate(rs)]


def dense():
    """-> (genome, reads): one 10 kb sequence of CG repeats; six 4 kb reads: clean ones on both strands, one with a 3 kb deletion
    (1500 reference CpGs in one D), one without calls on its first kilobase, one mismatched at every 50th G"""
    if "dense" not in _CACHE:
        g = [("cg", "CG" * 5000)]
        rng = np.random.default_rng(5204)
        mm50 = [("M", 49), ("X", 1)] * 80
        out = [make_read("dense_f", 0, 0, 0, [("M", 4000)], rng, chroms=g),
               make_read("dense_r", 16, 0, 1000, [("M", 4000)], rng, chroms=g),
               make_read("dense_del", 0, 0, 3001, [("M", 500), ("D", 3000), ("M", 500)], rng, chroms=g),
               make_read("dense_nocall", 16, 0, 5000, [("M", 4000)], rng, chroms=g, drop=range(5000, 6000, 2)),
               make_read("dense_mm", 0, 0, 6000, mm50, rng, chroms=g),
               make_read("dense_tail", 16, 0, 6000, [("M", 4000)], rng, chroms=g)]
        _CACHE["dense"] = (g, out)
    return _CACHE["dense"]
