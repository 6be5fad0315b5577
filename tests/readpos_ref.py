"""Plain-Python restatement of `pileup -P` / `pileup -I` (include/hifimeth_hip.h: methylation by position in the read, end trimming)
over test records (dict(flag, tid, pos, mapq, cigar, seq, mm, ml), as pileup_cases.as_dict gives them).  Plain module, imported by
test_pileup_readpos_cpu.py and test_gpu_pileup_readpos.py.

The alignment walk, the motif tests and the MM / ML parser are the CPU oracle's (oracle/pileup_oracle.py: their (qoff, soff) pairs
carry the read position the definition speaks of); everything the definition adds is restated here: trimming by DELETING entries
before anything else looks at them, the bin of a projected record, the threshold-free table and its rows.  Nothing here is shared
with the library, and nothing is read from any other project: the definition in the header is the specification.
"""
from oracle import pileup_oracle as P

CTX = ("CpG", "CHG", "CHH")
ENDS = ("5p", "3p", "interior")


def entries(rec):
    """the record's MM / ML entries [(qoff, strand, unmod_base, code, prob)], qoff in the read's original orientation"""
    fwd, _ = P.fwd_rev(rec["seq"], rec["flag"])
    return P.parse_mods(fwd, rec.get("mm"), rec.get("ml"))


def trim_entries(mods, L, n5, n3):
    """`-I n5:n3`: the entries at p < n5 or p > L - 1 - n3 are deleted"""
    return [m for m in mods if n5 <= m[0] <= L - 1 - n3]


def projected(rec, chrs, min_mapq=0, min_pi=0.0, trim=(0, 0)):
    """the records the projection emits for one input record -> [(motif, p, L, ML byte, sid, soff)]"""
    if rec["flag"] & 4:
        return []
    L = len(rec["seq"])
    mods = entries(rec)
    if not mods:                                      # a record without entries is not submitted
        return []
    mods = trim_entries(mods, L, *trim)
    a = P.map_info(rec["flag"], rec["pos"], rec["cigar"], rec["seq"], chrs[rec["tid"]][1])
    if rec["mapq"] < min_mapq or a["pi"] < min_pi:
        return []
    at = {}
    for q, _strand, _ub, code, prob in mods:          # the last 5mC entry of a position wins
        if code == "m":
            at[q] = prob
    out = []
    for motif, pairs in ((0, P.cpg_records(a, L)), (1, P.chg_records(a, L)), (2, P.chh_mapped_samples(a, L))):
        out += [(motif, p, L, at[p], rec["tid"], soff) for p, soff in pairs if p in at]
    return out


def bin_of(p, L, D):
    """-> (end, dist): 0 = 5', 1 = 3', 2 = interior (dist 0); ties go to 5'"""
    d5, d3 = p, L - 1 - p
    if min(d5, d3) >= D:
        return 2, 0
    return (0, d5) if d5 <= d3 else (1, d3)


def histograms(records, chrs, D, **kw):
    """H[(motif, end, dist)][ML byte], the non-empty rows only"""
    H = {}
    for rec in records:
        for motif, p, L, prob, _sid, _soff in projected(rec, chrs, **kw):
            row = H.setdefault((motif, *bin_of(p, L, D)), [0] * 256)
            row[prob] += 1
    return H


def rows(records, chrs, D, thr, min_calls=1, **kw):
    """-> [(motif, end, dist, n_m, n_u, sum_ml)] in fetch order: by motif, 5' by ascending dist, 3' by ascending dist, interior;
    thr = the three thresholds of the last count, a call is methylated iff its ML byte >= thr[motif]"""
    H = histograms(records, chrs, D, **kw)
    order = [(0, d) for d in range(D)] + [(1, d) for d in range(D)] + [(2, 0)]
    out = []
    for motif in range(3):
        for end, dist in order:
            h = H.get((motif, end, dist), [0] * 256)
            n_m = sum(h[thr[motif]:])
            n_u = sum(h[:thr[motif]])
            if n_m + n_u >= min_calls:
                out.append((motif, end, dist, n_m, n_u, sum(v * c for v, c in enumerate(h))))
    return out


def tsv_text(rws):
    text = ["#context\tend\tdist\tn\tn_m\tn_u\tpercent\tmean_ml\n"]
    for motif, end, dist, n_m, n_u, sum_ml in rws:
        n = n_m + n_u
        st = (100.0 * n_m / n, sum_ml / n) if n else (float("nan"), float("nan"))
        text.append("%s\t%s\t%d\t%d\t%d\t%d\t%g\t%.6g\n" % (CTX[motif], ENDS[end], dist, n, n_m, n_u, *st))
    return "".join(text)


def surviving_entries(rec, n5, n3):
    """the entries of the record that `-I n5:n3` leaves, for a direct submission (hm_mod_t: qoff, strand, unmod_base, code, prob):
    the test's own deletion.  A record all of whose entries go stays in the input with one entry the engine ignores (A+a on base
    0): a record without entries is not submitted at all, while a trimmed record still takes part -- it covers its CpGs without a
    call.  A record that had no entry to begin with gives none."""
    import numpy as np
    hm_mod_t = np.dtype([("qoff", "<i4"), ("strand", "u1"), ("unmod_base", "S1"), ("code", "S1"), ("prob", "u1")])
    mods = entries(rec)
    keep = trim_entries(mods, len(rec["seq"]), n5, n3)
    if mods and not keep:
        keep = [(0, 0, "A", "a", 0)]
    out = np.zeros(len(keep), hm_mod_t)
    for i, (q, strand, ub, code, prob) in enumerate(keep):
        out[i] = (q, strand, ub.encode(), code.encode(), prob)
    return out
