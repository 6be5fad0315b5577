"""Hand-built inputs for `pileup -E` (plain module, imported by test_pileup_patterns_cpu.py and test_gpu_pileup_patterns.py): a
genome whose CpGs are planted one by one, and reads that each put one condition of the definition on a known window.

    genome()    chr1 (1600 b): CpGs at CHR1; ends in C.  chr2 (300 b): begins with G (chr1's last C + this G spell no CpG), one
                CpG: fewer than any k.  chr3 (500 b): CpGs at CHR3, the last one on the last two bases of the job.
    reads()     sorted by (tid, pos); the first is a clean forward read of all of chr1, so in a batch that starts with it column
                == reference offset and the loci 1010 .. 1040 lie on both sides of the projection's 1024-column tile edge (the C of
                1023 is the tile's last column)
    dense()     10 kb of CGCGCG.. (5000 reference CpGs: more than one 4096 block of ranks) and 4 kb reads on it
"""
import numpy as np

from hifimeth_amd.synth import AlignedRead, revcomp
from pileup_cases import build_seq

CHR1 = (0, 100, 104, 110, 120, 300, 450, 601, 1010, 1018, 1023, 1030, 1040, 1400)
CHR2 = (150,)
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
        rng = np.random.default_rng(4101)
        out = []
        for name, n, cpgs in (("chr1", 1600, CHR1), ("chr2", 300, CHR2), ("chr3", 500, CHR3)):
            s = _background(rng, n)
            for g in cpgs:
                s[g], s[g + 1] = "C", "G"
            out.append([name, s])
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


def make_read(name, flag, tid, pos, spec, rng, mapq=60, probs=None, drop=()):
    """a record with a 5mC call (C+m) on every C of its forward strand, ML random, except: probs = {reference offset of a CpG's C:
    ML byte} sets the call the projection looks up for that locus, drop = those loci lose their call"""
    chroms = genome()
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
    mm = "C+m" + "".join(",%d" % d for d in deltas) + ";" if deltas else None
    return AlignedRead(name, flag, tid, pos, mapq, [(it[0], it[1]) for it in spec], seq, mm, np.array(ml, np.uint8) if deltas else None)


def reads():
    if "reads" in _CACHE:
        return _CACHE["reads"]
    rng = np.random.default_rng(4102)
    A = {100: THR, 104: THR - 1, 110: 255, 120: 0}
    out = [make_read("long_f", 0, 0, 0, [("M", 1600)], rng),
           make_read("long_r", 16, 0, 0, [("M", 1600)], rng),
           make_read("long_f2", 0, 0, 0, [("M", 1600)], rng, probs={1010: 200, 1018: 10, 1023: 200, 1030: 10, 1040: 200}),
           make_read("head", 0, 0, 0, [("M", 50)], rng)]
    for flag, t in ((0, "f"), (16, "r")):
        out += [make_read("A_eq_" + t, flag, 0, 80, [("M", 100)], rng, probs=A),
                make_read("A_del110_" + t, flag, 0, 80, [("M", 28), ("D", 4), ("M", 68)], rng),
                make_read("A_mmC104_" + t, flag, 0, 80, [("M", 24), ("X", 1), ("M", 75)], rng),
                make_read("A_mmG105_" + t, flag, 0, 80, [("M", 25), ("X", 1), ("M", 74)], rng),
                make_read("A_miss110_" + t, flag, 0, 80, [("M", 100)], rng, drop=(110,)),
                make_read("A_ins_" + t, flag, 0, 80, [("M", 26), ("I", 3), ("M", 74)], rng),
                make_read("A_brk120_" + t, flag, 0, 80, [("M", 41), ("I", 1), ("M", 59)], rng),
                make_read("A_end111_" + t, flag, 0, 80, [("M", 32)], rng),
                make_read("A_end110_" + t, flag, 0, 80, [("M", 31)], rng),
                make_read("A_clip_" + t, flag, 0, 80, [("S", 5), ("M", 100), ("S", 4)], rng),
                make_read("A_secondary_" + t, flag | 256, 0, 80, [("M", 100)], rng),
                make_read("A_mapq10_" + t, flag, 0, 80, [("M", 100)], rng, mapq=10),
                make_read("A_lowid_" + t, flag, 0, 80, [("M", 10), ("X", 4), ("M", 86)], rng),       # 96 %
                make_read("span_" + t, flag, 0, 290, [("M", 330)], rng),
                make_read("tile_" + t, flag, 0, 1000, [("M", 60)], rng),
                make_read("c1end_" + t, flag, 0, 1380, [("M", 220)], rng),
                make_read("c2_" + t, flag, 1, 0, [("M", 200)], rng),
                make_read("c3_" + t, flag, 2, 30, [("M", 100)], rng),
                make_read("c3end_" + t, flag, 2, 400, [("M", 100)], rng)]
    out.append(AlignedRead("unmapped", 4, 0, 80, 0, [("M", 100)], out[4].seq, out[4].mm, out[4].ml))
    out.sort(key=lambda r: (r.tid, r.pos))      # stable: long_f stays the first record
    assert out[0].name == "long_f"
    _CACHE["reads"] = out
    return out


def as_dict(r):
    return dict(flag=r.flag, tid=r.tid, pos=r.pos, mapq=r.mapq, cigar=r.cigar, seq=r.seq, mm=r.mm, ml=r.ml)


def crowd(n=300):
    """n reads on the window 100 .. 120: three distinct records, each n / 3 times"""
    if ("crowd", n) not in _CACHE:
        rng = np.random.default_rng(4103)
        base = [make_read("crowd%d" % i, (0, 16, 0)[i], 0, 80, [("M", 100)], rng) for i in range(3)]
        _CACHE[("crowd", n)] = [base[i % 3] for i in range(n)]
    return _CACHE[("crowd", n)]


def dense():
    """-> (genome, reads): one 10 kb sequence of CG repeats; 140 reads of 4 kb (four distinct records), 1999 windows each at k = 2"""
    if "dense" not in _CACHE:
        g = [("cg", "CG" * 5000)]
        rng = np.random.default_rng(4104)
        base = []
        for i, pos in enumerate((0, 1000, 3000, 6000)):
            seq = g[0][1][pos:pos + 4000]
            flag = 16 if i & 1 else 0
            n = (revcomp(seq) if flag else seq).count("C")
            base.append(AlignedRead("dense%d" % i, flag, 0, pos, 60, [("M", 4000)], seq, "C+m" + ",0" * n + ";",
                                    rng.integers(0, 256, n).astype(np.uint8)))
        _CACHE["dense"] = (g, sorted([base[i % 4] for i in range(140)], key=lambda r: r.pos))
    return _CACHE["dense"]
