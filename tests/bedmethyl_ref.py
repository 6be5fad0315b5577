"""Textbook restatement of `pileup -M` (include/hifimeth_hip.h has the definition): plain module, Python ints and loops, imported by
test_pileup_bedmethyl_cpu.py and test_gpu_pileup_bedmethyl.py.  Per record the member loci (MOD / CANON) are what
oracle.pileup_oracle projects for it as CpG records, and whether it takes part comes from the oracle's identity and the record's
mapq; NOCALL, DIFF, DELETE and "nothing" come from a walk of the CIGAR of its own (the oracle's alignment strings do not tell D
from N), with no knowledge of tiles or ranks.

    reference_cpgs(chrs)                        [[offsets of C of CG] per sequence], upper-case bytes only
    takes_part(rec, chrs, min_mapq, min_pi)     the record has entries, is mapped and passes -q / -f
    classes(rec, chrs, min_mapq, min_pi)        {(sid, soff): ("member", prob) | "nocall" | "diff" | "delete" | "end"} of one record;
                                                "end" = the alignment ends on the C: nothing is counted
    counters(records, chrs, thr, hps, ...)      [{(sid, soff): [n_mod, n_canon, n_nocall, n_diff, n_delete]}] for the sets 0, 1, 2
    rows(records, chrs, thr, min_valid, ...)    [(gpos, n_mod, n_canon, n_nocall, n_diff, n_delete)] ascending: hm_pileup_fetch_bedmethyl
    bed_text(rows, chrs)                        the text of <prefix>.bedmethyl.CpG.bed
"""
import bisect

_CLASSES = {}
_CPGS = {}


def reference_cpgs(chrs):
    if id(chrs) not in _CPGS:
        _CPGS[id(chrs)] = (chrs, [[g for g in range(len(s) - 1) if s[g] == "C" and s[g + 1] == "G"] for _n, s in chrs])
    return _CPGS[id(chrs)][1]


def takes_part(rec, chrs, min_mapq=0, min_pi=0.0):
    from oracle import pileup_oracle as P
    if rec["flag"] & 4:
        return False
    fwd, _ = P.fwd_rev(rec["seq"], rec["flag"])
    if not P.parse_mods(fwd, rec.get("mm"), rec.get("ml")):
        return False
    a = P.map_info(rec["flag"], rec["pos"], rec["cigar"], rec["seq"], chrs[rec["tid"]][1])
    return rec["mapq"] >= min_mapq and not a["pi"] < min_pi


def walk(rec):
    """the CIGAR by the definition -> (match, deleted, last): match = {reference offset: (index in SEQ as stored, run number)} of the
    M / = / X columns, a run closed by every I, D or N of non-zero length; deleted = the offsets inside a D; last = the offset of the
    last column of the last run (None without one)"""
    cigar = list(rec["cigar"])
    q, s, run = 0, rec["pos"], 0
    if cigar and cigar[0][0] == "S":
        q = cigar[0][1]
    match, deleted, last = {}, set(), None
    for k, (op, n) in enumerate(cigar):
        if op in "M=X":
            for _ in range(n):
                match[s] = (q, run)
                last = s
                q += 1
                s += 1
        elif op == "I":
            q += n
            run += 1 if n else 0
        elif op in "DN":
            if op == "D":
                deleted.update(range(s, s + n))
            s += n
            run += 1 if n else 0
        else:
            assert op in "SHP"
    return match, deleted, last


def classes(rec, chrs, min_mapq=0, min_pi=0.0):
    from oracle import pileup_oracle as P
    key = (rec["flag"], rec["tid"], rec["pos"], rec["mapq"], tuple(rec["cigar"]), rec["seq"], rec.get("mm"),
           None if rec.get("ml") is None else bytes(bytearray(int(x) for x in rec["ml"])), min_mapq, min_pi, id(chrs))
    if key in _CLASSES:
        return _CLASSES[key]
    out = {}
    if takes_part(rec, chrs, min_mapq, min_pi):
        sid, stored, L = rec["tid"], rec["seq"], len(rec["seq"])
        members = {soff: prob for t, soff, prob, motif in P.read_contribution(rec, chrs, min_mapq, min_pi)[1] if motif == 0}
        fwd, _ = P.fwd_rev(stored, rec["flag"])
        called = {m[0] for m in P.parse_mods(fwd, rec.get("mm"), rec.get("ml")) if m[3] == "m"}   # forward-strand offsets with a 5mC entry
        match, deleted, last = walk(rec)
        cpgs = reference_cpgs(chrs)[sid]
        end = max(list(match) + list(deleted) + [rec["pos"]]) + 1
        for g in cpgs[bisect.bisect_left(cpgs, rec["pos"]):bisect.bisect_left(cpgs, end)]:
            if g in match:
                q, run = match[g]
                pair = g + 1 in match and match[g + 1][1] == run
                intact = pair and stored[q] == "C" and stored[q + 1] == "G"
                entry = intact and ((L - 1 - (q + 1)) if rec["flag"] & 16 else q) in called
                assert entry == (g in members)
                if entry:
                    out[(sid, g)] = ("member", members[g])
                elif intact:
                    out[(sid, g)] = "nocall"
                elif g == last:
                    out[(sid, g)] = "end"
                else:
                    out[(sid, g)] = "diff"
            elif g in deleted:
                out[(sid, g)] = "delete"
        assert set(members) <= {g for (_s, g) in out}
    _CLASSES[key] = out
    return out


def column_of(cls, thr):
    if isinstance(cls, tuple):
        return 0 if cls[1] >= thr else 1
    return {"nocall": 2, "diff": 3, "delete": 4, "end": None}[cls]


def counters(records, chrs, thr=128, hps=None, min_mapq=0, min_pi=0.0):
    sets = [{}, {}, {}]
    for i, rec in enumerate(records):
        hp = hps[i] if hps is not None and hps[i] in (1, 2) else 0
        for locus, cls in classes(rec, chrs, min_mapq, min_pi).items():
            col = column_of(cls, thr)
            if col is None:
                continue
            for s in {0, hp}:
                sets[s].setdefault(locus, [0] * 5)[col] += 1
    return sets


def rows(records, chrs, thr=128, min_valid=1, part=0, hps=None, min_mapq=0, min_pi=0.0):
    off = [0]
    for _n, s in chrs:
        off.append(off[-1] + len(s))
    c = counters(records, chrs, thr, hps, min_mapq, min_pi)[part]
    return [(off[sid] + g, *n) for (sid, g), n in sorted(c.items()) if sum(n) >= 1 and n[0] + n[1] >= min_valid]


def bed_text(rows_, chrs):
    off = [0]
    for _n, s in chrs:
        off.append(off[-1] + len(s))
    text = []
    for gpos, n_mod, n_canon, n_nocall, n_diff, n_delete in rows_:
        sid = max(i for i in range(len(chrs)) if off[i] <= gpos and len(chrs[i][1]))
        k, valid = gpos - off[sid], n_mod + n_canon
        cols = [chrs[sid][0], k, k + 1, "m", min(1000, valid), ".", k, k + 1, "255,0,0", valid,
                "%.2f" % (100.0 * n_mod / valid if valid else 0.0), n_mod, n_canon, 0, n_delete, 0, n_diff, n_nocall]
        text.append("\t".join(str(x) for x in cols) + "\n")
    return "".join(text)
