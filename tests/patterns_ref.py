"""Textbook restatement of `pileup -E` (include/hifimeth_hip.h has the definition): plain module, Python ints and loops, imported by
test_pileup_patterns_cpu.py and test_gpu_pileup_patterns.py.  Per record the set of member loci is what oracle.pileup_oracle
projects for it as CpG records; everything behind that -- reference CpGs, windows, patterns, counts, rows, statistics, BED text --
is restated here from the definition, with no knowledge of runs, tiles or ranks.

    reference_cpgs(chrs)                   [[offsets of C of CG] per sequence], upper-case bytes only
    member_loci(rec, chrs, ...)            {(sid, soff): prob} of one record
    windows(records, chrs, k, ...)         {(sid, soff of the first locus): [2^k counts]}, valid windows with a contributing record
    rows(records, chrs, k, ...)            [(gstart, gend, counts[16], n, k)] ascending, the rows hm_pileup_fetch_patterns returns
    stats(counts, k)                       (entropy, epipolymorphism, pdr, level) by the direct formulas
    bed_text(rows, chrs)                   the text of <prefix>.patterns.CpG.bed
"""
import math

_MEMBERS = {}


def reference_cpgs(chrs):
    return [[g for g in range(len(s) - 1) if s[g] == "C" and s[g + 1] == "G"] for _n, s in chrs]


def member_loci(rec, chrs, min_mapq=0, min_pi=0.0):
    """the loci where the record contributes a motif-0 record to the counters, with the call's ML byte; cached by the record's
    content (a test may hold hundreds of copies of one read)"""
    from oracle import pileup_oracle as P
    key = (rec["flag"], rec["tid"], rec["pos"], rec["mapq"], tuple(rec["cigar"]), rec["seq"], rec.get("mm"),
           None if rec.get("ml") is None else bytes(bytearray(int(x) for x in rec["ml"])), min_mapq, min_pi, id(chrs))
    if key not in _MEMBERS:
        _hist, recs = P.read_contribution(rec, chrs, min_mapq, min_pi)
        out = {}
        for sid, soff, prob, motif in recs:
            if motif == 0:
                assert (sid, soff) not in out
                out[(sid, soff)] = prob
        _MEMBERS[key] = out
    return _MEMBERS[key]


def windows(records, chrs, k, max_span=150, thr=128, min_mapq=0, min_pi=0.0):
    cpgs = reference_cpgs(chrs)
    counts = {}
    for rec in records:
        mem = member_loci(rec, chrs, min_mapq, min_pi)
        if not mem:
            continue
        for sid, c in enumerate(cpgs):
            for j in range(len(c) - k + 1):
                loci = c[j:j + k]
                if loci[-1] - loci[0] > max_span or any((sid, g) not in mem for g in loci):
                    continue
                pattern = sum(1 << i for i, g in enumerate(loci) if mem[(sid, g)] >= thr)
                counts.setdefault((sid, loci[0]), [0] * (1 << k))[pattern] += 1
    return counts


def rows(records, chrs, k, max_span=150, thr=128, min_reads=1, min_mapq=0, min_pi=0.0):
    cpgs = reference_cpgs(chrs)
    off = [0]
    for _n, s in chrs:
        off.append(off[-1] + len(s))
    w = windows(records, chrs, k, max_span, thr, min_mapq, min_pi)
    out = []
    for (sid, first), cnt in sorted(w.items()):
        n = sum(cnt)
        if n < min_reads:
            continue
        j = cpgs[sid].index(first)
        out.append((off[sid] + first, off[sid] + cpgs[sid][j + k - 1] + 2, tuple(cnt) + (0,) * (16 - len(cnt)), n, k))
    return out


def stats(counts, k):
    c = [int(x) for x in counts[:1 << k]]
    n = sum(c)
    entropy = -sum(x / n * math.log2(x / n) for x in c if x) / k
    epi = 1.0 - sum((x / n) ** 2 for x in c if x)
    pdr = 1.0 - (c[0] + c[-1]) / n
    level = 100.0 * sum(bin(b).count("1") * x for b, x in enumerate(c)) / (k * n)
    return entropy + 0.0, epi, pdr, level


def bed_text(rows_, chrs, stats_of=None):
    """stats_of(counts16, n, k) -> the four statistics; default: the formulas above"""
    off = [0]
    for _n, s in chrs:
        off.append(off[-1] + len(s))
    text = []
    for start, end, cnt, n, k in rows_:
        sid = max(i for i in range(len(chrs)) if off[i] <= start and len(chrs[i][1]))
        st = stats_of(cnt, n, k) if stats_of else stats(cnt, k)
        text.append("%s\t%d\t%d\t%d\t%.6g\t%.6g\t%.6g\t%.6g\t%s\n" % (chrs[sid][0], start - off[sid], end - off[sid], n, *st,
                                                                  ",".join("%d" % x for x in cnt[:1 << k])))
    return "".join(text)
