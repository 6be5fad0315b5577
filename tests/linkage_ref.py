"""Textbook restatement of `pileup -L` (include/hifimeth_hip.h has the definition): plain module, Python ints and loops, imported by
test_pileup_linkage_cpu.py and test_gpu_pileup_linkage.py.  Per record the member loci are those of patterns_ref.member_loci (what
oracle.pileup_oracle projects for it as CpG records); every pair of them is classed and counted directly, with no knowledge of
histograms, lists or runs.

    pairs(records, chrs, max_dist, ...)    {d: [UU, UM, MU, MM]} over the pairs of member loci of one record, 2 <= d <= max_dist
    rows(records, chrs, max_dist, ...)     [(d, UU, UM, MU, MM)] ascending, the rows hm_pileup_fetch_linkage returns
    stats(uu, um, mu, mm)                  (concordance, r) by the direct formulas on Python ints
    tsv_text(rows)                         the text of <prefix>.linkage.CpG.tsv
"""
import math

from patterns_ref import member_loci

HEADER = "#dist\tn\tn_uu\tn_um\tn_mu\tn_mm\tconcordance\tr\n"


def pairs(records, chrs, max_dist, thr=128, min_mapq=0, min_pi=0.0):
    counts = {}
    for rec in records:
        mem = sorted(member_loci(rec, chrs, min_mapq, min_pi).items())   # [((sid, soff), prob)]: one record lies on one sequence
        for i, ((sa, a), pa) in enumerate(mem):
            for (sb, b), pb in mem[i + 1:]:
                assert sa == sb and a < b
                d = b - a
                if 2 <= d <= max_dist:
                    counts.setdefault(d, [0, 0, 0, 0])[2 * (pa >= thr) + (pb >= thr)] += 1   # UU, UM, MU, MM: first letter = lower
    return counts


def rows(records, chrs, max_dist, thr=128, min_pairs=1, min_mapq=0, min_pi=0.0):
    got = pairs(records, chrs, max_dist, thr, min_mapq, min_pi)
    return [(d, *got.get(d, [0, 0, 0, 0])) for d in range(2, max_dist + 1) if sum(got.get(d, [0])) >= min_pairs]


def stats(uu, um, mu, mm):
    n = uu + um + mu + mm
    den = (mm + mu) * (um + uu) * (mm + um) * (mu + uu)
    return (uu + mm) / n, (mm * uu - mu * um) / math.sqrt(den) if den else float("nan")


def tsv_text(rows_, stats_of=None):
    """stats_of(uu, um, mu, mm) -> the two statistics; default: the formulas above.  A row without pairs has none: nan"""
    text = [HEADER]
    for d, uu, um, mu, mm in rows_:
        n = uu + um + mu + mm
        st = (stats_of or stats)(uu, um, mu, mm) if n else (float("nan"), float("nan"))
        text.append("%d\t%d\t%d\t%d\t%d\t%d\t%.6g\t%.6g\n" % (d, n, uu, um, mu, mm, *st))
    return "".join(text)
