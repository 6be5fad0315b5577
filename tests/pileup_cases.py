"""Hand-built edge inputs for the `pileup` kernels (plain module, imported by test_pileup_edges_cpu.py, test_gpu_pileup_edges.py
and tools/make_golden.py): a small genome whose chromosome joints would complete motifs if a kernel looked across them, and
five classes of AlignedRead lists that hifimeth_amd.synth.synth_alignments never produces.

    genome()            three chromosomes: chr1 begins CGG.. and ends ..CAC, chr2 begins GG.. and ends ..TCG, chr3 begins TG.. and
                        ends ..CA; every chromosome carries a CGG / CCG cluster, chr1 and chr2 a run of reference N
    cigar_zoo()         every CIGAR op, clips in odd places, zero-length ops, lying =/X, runs of 1-2 columns, both strands
    boundaries()        reads on the first / last base of every chromosome, whole chromosomes, odd and even l_qseq, N on N
    tiny_crowd()        a few hundred alignments of 1-70 columns, sorted: many reads per wavefront and per 1024-column tile
    foreign_tags()      the same alignments with MM/ML as other callers write them
    identity_ties()     reads whose identity is exactly the -f value, and one match above / below

Every function asserts, with the CPU oracle, that its class holds what it is for (conditions, not measurements).  Nothing
here is random beyond a seeded generator; names are stable.

REFUSED lists, by name, the records the engine legitimately refuses at submit time -- none of the classes above holds one:
the malformed records (illegal SEQ nibbles, CIGAR op B, modification offsets outside the read, alignments past the
chromosome end) are built by `bad_records()` and the GPU test asserts their return code and message.

REF_UNDEFINED names the records that are left out of tests/golden/align_edges.json: with an empty CIGAR the reference's
cigar_to_alignment reads cigar[0] of an empty array (bam_info.cpp:282), so its qb is whatever follows in memory; its
alignment is empty either way, which is what the oracle gives.

Not covered (said in the issue): references above 2^32 bases (the 8 high bits of PRec.hi) need more than 50 GB of planes.
"""
import dataclasses

import numpy as np

from hifimeth_amd.synth import AlignedRead, revcomp, synth_genome

REFUSED = ()
REF_UNDEFINED = ("zoo_empty_cigar_f", "zoo_empty_cigar_r")
TIE_VALUES = (97.5, 98.5)          # 39/40 and 197/200: 100.0 * m / as_size is exact in binary floating point

# a CGG / CCG cluster: CpG next to both CHG spellings, CHH of both strands, runs of C and of G
CLUSTER = ("CGGCCGCAGCTGCCGGACGCGGTCCGGCTGCAGCCCGGGACCATCTTGGAGTGATGCGCCGGCGCAGCTGTACGG"
           "CCGGCCGGCAGCAGCTGCTGCCCAGGGTCACTAATGGTGAGCGCGCCGGTTCCGGAACCGGCAGCGCTGCCGG")
CLUSTER_AT = 300
N_RUN = (288, 300)                 # right in front of the cluster


def genome():
    g = [(n, list(s)) for n, s in synth_genome(n_chr=3, length=600, seed=101, n_frac=0.0)]
    for _n, s in g:
        s[CLUSTER_AT:CLUSTER_AT + len(CLUSTER)] = CLUSTER
    for k in (0, 1):
        g[k][1][N_RUN[0]:N_RUN[1]] = "N" * (N_RUN[1] - N_RUN[0])
    g[0][1][:6] = "CGGCAG"
    g[0][1][-7:] = "ACGTCAC"          # CAC on the last three bases; its last C + chr2's G would spell CG, AC + G -> CHG-like
    g[1][1][:5] = "GGACG"
    g[1][1][-6:] = "CCATCG"           # CG on the last base pair; CG + chr3's T.. / G + TG would need chr3
    g[2][1][:5] = "TGGCA"
    g[2][1][-6:] = "GTCTCA"           # CA + (nothing): the last chromosome
    return [(n, "".join(s)) for n, s in g]


# ---- building blocks ----------------------------------------------------------------------------------------------
_OTHER = {"A": "C", "C": "T", "G": "A", "T": "G", "N": "A"}


def _rand(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def build_seq(chrom, pos, spec, rng):
    """SEQ as stored for a CIGAR spec [(op, n) | (op, n, 'm' | 'x')] laid out the way the reference walks it
    (cigar_to_alignment, bam_info.cpp:262-371): a leading S consumes query bases, S / H / P anywhere else consume nothing;
    M and = copy the chromosome ('m'), X places a different base ('x') unless told otherwise; I inserts random bases.  The
    bases of the S ops that the walk does not consume are appended, so l_qseq is what a BAM writer would store."""
    q, si, tail = [], pos, 0
    for k, item in enumerate(spec):
        op, n = item[0], item[1]
        mode = item[2] if len(item) > 2 else ("x" if op == "X" else "m")
        if op == "S":
            if k == 0:
                q.append(_rand(rng, n))
            else:
                tail += n
        elif op in "M=X":
            ref = chrom[si:si + n]
            assert len(ref) == n, "spec runs past the chromosome"
            q.append(ref if mode == "m" else "".join(_OTHER[c] for c in ref))
            si += n
        elif op == "I":
            q.append(_rand(rng, n))
        elif op in "DN":
            si += n
    return "".join(q) + _rand(rng, tail)


def all_cg_mods(fwd, rng, lo=0, hi=256):
    """every C as C+m and every G as G-m (contexts or not: the C at L-1 / L-2, the G at 0 / 1), ML drawn from [lo, hi)"""
    parts, n = [], 0
    for base, head in (("C", "C+m"), ("G", "G-m")):
        k = fwd.count(base)
        if k:
            parts.append(head + ",0" * k + ";")
            n += k
    if not parts:
        return None, None
    ml = rng.integers(lo, hi, n).astype(np.uint8)
    ml[::7] = 255
    ml[3::7] = 0
    return "".join(parts), ml


def make_read(name, flag, tid, pos, spec, chroms, rng, mapq=60, seq=None):
    cigar = [(it[0], it[1]) for it in spec]
    if seq is None:
        seq = build_seq(chroms[tid][1], pos, spec, rng)
    fwd = revcomp(seq) if flag & 16 else seq
    mm, ml = all_cg_mods(fwd, rng)
    return AlignedRead(name, flag, tid, pos, mapq, cigar, seq, mm, ml)


def as_dict(r):
    return dict(flag=r.flag, tid=r.tid, pos=r.pos, mapq=r.mapq, cigar=r.cigar, seq=r.seq, mm=r.mm, ml=r.ml)


def _oracle():
    from oracle import pileup_oracle
    return pileup_oracle


def _records(reads, chroms, **kw):
    P = _oracle()
    return [P.read_contribution(as_dict(r), chroms, **kw)[1] for r in reads]


# ---- cigar_zoo ----------------------------------------------------------------------------------------------------
def cigar_zoo():
    g = genome()
    rng = np.random.default_rng(201)
    c0 = CLUSTER_AT
    tick = [("M", 1), ("I", 1), ("M", 1), ("D", 1), ("M", 2), ("I", 1), ("M", 2), ("D", 1), ("M", 3), ("D", 1), ("M", 1), ("I", 1),
            ("M", 2), ("D", 1), ("M", 3), ("I", 1), ("M", 1), ("D", 1), ("M", 2), ("I", 1)]
    specs = [
        ("all_ops", c0, [("S", 4), ("M", 8), ("I", 2), ("=", 6), ("D", 3), ("X", 1), ("=", 5), ("N", 5), ("M", 7), ("P", 2), ("M", 8),
                         ("S", 3), ("H", 5)]),
        ("H_then_S", c0, [("H", 5), ("S", 10), ("M", 20)]),
        ("S_lead_I", c0 + 3, [("S", 3), ("I", 2), ("M", 15)]),
        ("D_lead", c0, [("D", 2), ("M", 15)]),
        ("zero_ops", c0, [("M", 6), ("I", 0), ("M", 6), ("D", 0), ("M", 6), ("M", 0), ("=", 6), ("X", 0), ("=", 5)]),
        ("zero_first", c0, [("M", 0), ("M", 12), ("S", 0)]),
        ("N_skip", c0, [("M", 10), ("N", 8), ("M", 12)]),
        ("P_mid", c0, [("M", 9), ("P", 2), ("M", 10), ("S", 3), ("H", 2)]),
        ("S_mid", c0, [("M", 8), ("S", 4), ("M", 9), ("H", 3), ("M", 7)]),
        ("all_S", c0, [("S", 4)]),
        ("all_I", c0, [("I", 4)]),
        ("all_H", c0, [("H", 9)]),
        ("S_then_I_only", c0, [("S", 2), ("I", 6), ("S", 2)]),
        ("empty_cigar", c0, []),
        ("eq_lies", c0, [("=", 8, "m"), ("=", 3, "x"), ("=", 8, "m"), ("X", 4, "m"), ("=", 6, "m"), ("X", 2, "x"), ("X", 8, "m")]),
        ("eqx_true", c0, [("=", 6), ("X", 2), ("=", 6), ("X", 1), ("=", 20)]),
        ("tick0", c0, tick),
        ("tick1", c0 + 1, tick),
        ("tick2", c0 + 2, tick),
        ("pairs", c0, [("M", 2), ("D", 1)] * 8),
        ("pairs_I", c0 + 1, [("M", 2), ("I", 1)] * 8),
        ("triples", c0, [("M", 3), ("I", 1), ("M", 3), ("D", 1)] * 3),
        ("singles", c0, [("M", 1), ("D", 1)] * 5),
        ("over_N", N_RUN[0] - 8, [("M", 12), ("I", 1), ("M", 14)]),
    ]
    reads = []
    for name, pos, spec in specs:
        for flag, tag in ((0, "f"), (16, "r")):
            tid = len(reads) % 3 if name not in ("over_N",) else 0
            seq = None
            if name in ("all_S", "all_I", "S_then_I_only", "empty_cigar", "all_H"):
                seq = CLUSTER[:{"all_S": 4, "all_I": 4, "S_then_I_only": 10}.get(name, 12)]
            r = make_read(f"zoo_{name}_{tag}", flag, tid, pos, spec, g, rng, seq=seq)
            reads.append(r)
    # not vacuous: every op letter, every read carries calls, records from both strands, and the runs of 1-2 columns give records
    ops = {op for r in reads for op, _n in r.cigar}
    assert ops == set("MIDNSHP=X"), ops
    assert all(r.mm for r in reads)
    recs = _records(reads, g)
    by = dict(zip((r.name for r in reads), recs))
    assert sum(len(x) for x in recs) > 100
    for nm in ("pairs", "tick0", "tick1", "tick2", "triples", "H_then_S", "eq_lies", "zero_ops"):
        assert by[f"zoo_{nm}_f"] and by[f"zoo_{nm}_r"], nm
    assert {m for x in (by["zoo_pairs_f"] + by["zoo_pairs_r"]) for *_a, m in [x]} == {0}      # two columns hold a CpG only
    for nm in ("all_S", "all_I", "all_H", "empty_cigar", "singles", "S_then_I_only"):
        assert not by[f"zoo_{nm}_f"] and not by[f"zoo_{nm}_r"], nm
    return reads


# ---- boundaries ---------------------------------------------------------------------------------------------------
def joint_traps(g):
    """(sid, soff, motif) of the records a projection would make if it took a chromosome's neighbour in the concatenated
    reference for its continuation: motifs whose columns straddle a joint."""
    P = _oracle()
    cat = "".join(s for _n, s in g)
    off = np.concatenate([[0], np.cumsum([len(s) for _n, s in g])])
    traps = set()
    for j in off[1:-1]:
        j = int(j)
        sid = int(np.searchsorted(off, j, side="right") - 1)          # the chromosome that starts at j
        for a in (j - 2, j - 1):                                       # first column of a window that crosses j
            two, three = cat[a:a + 2], cat[a:a + 3]
            where = lambda p: (sid - 1, p - int(off[sid - 1])) if p < j else (sid, p - j)  # noqa: E731
            if a == j - 1 and two == "CG":
                traps.add((*where(a), 0))
            if three in P.FWD_CHG or three == "CGG":
                traps.add((*where(a), 1))
            if three in P.FWD_CHH:
                traps.add((*where(a), 2))
            if three in P.REV_CHH:
                traps.add((*where(a + 2), 2))
    return traps


def boundaries():
    g = genome()
    rng = np.random.default_rng(202)
    reads = []
    for tid, (_n, s) in enumerate(g):
        L = len(s)
        nxt = g[tid + 1][1][:6] if tid + 1 < len(g) else "GGCGGC"
        prv = g[tid - 1][1][-6:] if tid else "CCGCCG"
        for flag, tag in ((0, "f"), (16, "r")):
            reads.append(make_read(f"bnd_whole{tid}_{tag}", flag, tid, 0, [("M", L)], g, rng))
            for n in (1, 2, 3, 4, 7, 64, 65):                        # odd and even l_qseq, on the first and on the last base
                reads.append(make_read(f"bnd_head{tid}_{n}{tag}", flag, tid, 0, [("=", n)], g, rng))
                reads.append(make_read(f"bnd_tail{tid}_{n}{tag}", flag, tid, L - n, [("M", n)], g, rng))
            # soft clips that continue with the neighbour's bases: what a read spanning the joint would really hold
            tail = s[L - 16:] + nxt
            reads.append(make_read(f"bnd_tailclip{tid}_{tag}", flag, tid, L - 16, [("M", 16), ("S", 6)], g, rng, seq=tail))
            head = prv + s[:17]
            reads.append(make_read(f"bnd_headclip{tid}_{tag}", flag, tid, 0, [("S", 6), ("M", 17)], g, rng, seq=head))
            reads.append(make_read(f"bnd_tail_del{tid}_{tag}", flag, tid, L - 14, [("M", 8), ("D", 4), ("M", 2)], g, rng))
            reads.append(make_read(f"bnd_tail_D{tid}_{tag}", flag, tid, L - 12, [("M", 9), ("I", 2), ("D", 3)], g, rng))
        if tid < 2:
            a = N_RUN[0]
            reads.append(make_read(f"bnd_N_on_N{tid}_f", 0, tid, a - 9, [("M", 9 + 12 + 10)], g, rng))
            reads.append(make_read(f"bnd_N_on_N{tid}_r", 16, tid, a - 8, [("=", 8), ("M", 12), ("=", 9)], g, rng))
    # conditions
    assert any("N" in r.seq for r in reads)
    assert {r.l_qseq & 1 for r in reads} == {0, 1}
    recs = _records(reads, g)
    flat = {(sid, soff, m) for x in recs for sid, soff, _p, m in x}
    last_pair = [(sid, soff) for sid, soff, m in flat if soff == len(g[sid][1]) - 2 and m == 0]
    assert last_pair, "no CpG record on the last base pair of a chromosome"
    assert any(soff == len(g[sid][1]) - 3 for sid, soff, _m in flat)            # a 3-column motif ending on the last base
    assert any(soff == 0 for _sid, soff, _m in flat)
    traps = joint_traps(g)
    assert len(traps) >= 3 and {m for *_x, m in traps} == {0, 1, 2}, traps
    assert not (flat & traps)
    # the reads do cover the trap columns, with a call on them, so that a look across the joint would make a record
    for sid, soff, _m in traps:
        assert any(r.tid == sid and r.pos <= soff < r.pos + sum(n for op, n in r.cigar if op in "M=X") for r in reads)
    return reads


# ---- tiny_crowd ---------------------------------------------------------------------------------------------------
def tiny_crowd(n=360):
    g = genome()
    rng = np.random.default_rng(203)
    reads = []
    while len(reads) < n:
        i = len(reads)
        tid = int(rng.integers(0, 3))
        L = len(g[tid][1])
        kind = i % 6
        if kind < 3:                                                  # a single run of 1-3 columns
            spec = [("M=X"[i % 2] if kind else "M", kind + 1)]
        elif kind == 3:
            spec = [("M", int(rng.integers(1, 4))), ("DI"[i % 2], 1), ("M", int(rng.integers(1, 4)))]
        else:
            a = int(rng.integers(4, 71))
            b = int(rng.integers(1, a))
            spec = [("=", b), ("I", 1), ("=", a - b)] if kind == 4 else [("M", a)]
        span = sum(n_ for op, n_ in spec if op in "M=XD")
        near = int(rng.integers(0, 3))
        pos = (int(rng.integers(CLUSTER_AT, CLUSTER_AT + len(CLUSTER) - span)) if near else int(rng.integers(0, L - span + 1)))
        spec = [(op, n_, "m") for op, n_ in spec]
        flag = 16 if rng.random() < 0.5 else 0
        r = make_read(f"tiny{i}", flag, tid, pos, spec, g, rng, mapq=int(rng.integers(0, 61)))
        if r.mm is None:
            continue                                                  # no C / G in it: draw again (every read carries calls)
        reads.append(r)
    reads.sort(key=lambda r: (r.tid, r.pos))
    cols = [sum(n_ for op, n_ in r.cigar if op in "M=X") for r in reads]
    assert all(r.mm for r in reads) and max(cols) <= 70 and min(cols) == 1
    assert sum(c <= 3 for c in cols) >= n // 3
    assert sum(cols) / len(cols) < 32                                 # more than two reads per wavefront on average
    assert sum(len(x) for x in _records(reads, g)) > 300
    return reads


# ---- foreign_tags -------------------------------------------------------------------------------------------------
def _positions_mm(fwd, base, head, keep=None):
    """MM list `head` over the occurrences of `base` in fwd selected by keep(k-th occurrence, offset) -> (text, offsets)"""
    deltas, qs, skipped = [], [], 0
    for k, q in enumerate(i for i, c in enumerate(fwd) if c == base):
        if keep is None or keep(k, q):
            deltas.append(skipped)
            qs.append(q)
            skipped = 0
        else:
            skipped += 1
    if not qs:
        return "", []
    return head + "".join(f",{d}" for d in deltas) + ";", qs


def foreign_tags():
    g = genome()
    rng = np.random.default_rng(204)
    c0 = CLUSTER_AT
    body = [("M", 40), ("I", 1), ("M", 30), ("D", 2), ("M", 50)]
    aln = [("f", 0, 0, c0, body), ("r", 16, 1, c0 + 5, body), ("fs", 0x800, 2, c0 + 2, body), ("rs", 16 | 0x100, 0, c0 + 9, body),
           ("fN", 0, 0, N_RUN[0] - 2, [("M", 44)]), ("rN", 16, 1, N_RUN[0] - 3, [("M", 44)]),
           ("fclip", 0, 2, c0, [("S", 2), ("M", 60), ("S", 2)]), ("rodd", 16, 1, c0 + 1, [("M", 61)])]
    reads = []
    for tag, flag, tid, pos, spec in aln:
        base = make_read("x", flag, tid, pos, spec, g, rng)
        fwd = revcomp(base.seq) if flag & 16 else base.seq
        nC, nG = fwd.count("C"), fwd.count("G")
        assert nC > 5 and nG > 5
        ml = lambda n: rng.integers(0, 256, n).astype(np.uint8)  # noqa: E731
        allC = "C+m" + ",0" * nC + ";"
        third, _q = _positions_mm(fwd, "C", "C+m", lambda k, q: k % 3 == 1)
        dialects = {
            "allCG": (allC + "G-m" + ",0" * nG + ";", ml(nC + nG)),
            "mh": ("C+mh" + ",0" * nC + ";", ml(2 * nC)),
            "hm_G": ("G-hm" + ",0" * nG + ";" + third, ml(2 * nG + len(_q))),
            "h_only": ("C+h" + ",0" * nC + ";G-h" + ",0" * nG + ";", ml(nC + nG)),
            "chebi": ("C+27551" + ",0" * nC + ";G-76792" + ",0" * nG + ";", ml(nC + nG)),
            "flags": ("C+m?" + ",0" * nC + ";G-m." + ",0" * nG + ";", ml(nC + nG)),
            "A_a": ("A+a" + ",0" * fwd.count("A") + ";" + allC + "T-a,1,0;", ml(fwd.count("A") + nC + 2)),
            "dup": (allC + allC, np.concatenate([np.full(nC, 250, np.uint8), np.full(nC, 5, np.uint8)])),
            "dup3": (third + allC + third + "G-m,0;", np.concatenate([np.full(len(_q), 0, np.uint8), ml(nC), np.full(len(_q), 255, np.uint8),
                                                                  np.array([255], np.uint8)])),
            "edges": (allC + "G-m" + ",0" * nG + ";", np.tile(np.array([0, 255, 128, 127], np.uint8), nC + nG)[:nC + nG]),
        }
        if "N" in fwd:
            dialects["N_m"] = ("N+m" + ",0" * fwd.count("N") + ";" + third, ml(fwd.count("N") + len(_q)))
            dialects["N_h"] = ("N+h,1;" + allC, ml(1 + nC))
            dialects["N_n"] = ("N+n" + ",0" * fwd.count("N") + ";" + third, ml(fwd.count("N") + len(_q)))  # the reference's own N code
        for dn, (mm, mlb) in dialects.items():
            reads.append(dataclasses.replace(base, name=f"tag_{tag}_{dn}", mm=mm, ml=mlb))
    reads.sort(key=lambda r: (r.tid, r.pos))
    # conditions
    P = _oracle()
    assert any(r.flag & 0x100 for r in reads) and any(r.flag & 0x800 for r in reads)
    assert any(r.name.endswith("N_m") for r in reads)
    assert {0, 255} <= {int(v) for r in reads for v in r.ml}
    # a histogram count that comes from a non-m code; none from N / A lists
    non_m = 0
    for r in reads:
        fwd = P.fwd_rev(r.seq, r.flag)[0]
        if not r.flag & 0x900:
            non_m += sum(1 for q, _s, ub, code, _p in P.parse_mods(fwd, r.mm, r.ml) if code != "m" and ub in "CG" and P.mod_context(fwd, q) >= 0)
    assert non_m > 100
    h_only = [r for r in reads if r.name.endswith("h_only")]
    assert all(P.read_contribution(as_dict(r), g)[0] for r in h_only if not r.flag & 0x900)
    assert not any(P.read_contribution(as_dict(r), g)[1] for r in h_only)
    # the later duplicate decides pcov / ncov
    dup = [r for r in reads if r.name.endswith("_dup")]
    first_only = [dataclasses.replace(r, mm=r.mm[:len(r.mm) // 2], ml=r.ml[:len(r.ml) // 2]) for r in dup]
    a, b = P.pileup([as_dict(r) for r in dup], g), P.pileup([as_dict(r) for r in first_only], g)
    assert a["loci"] and [l[:2] for l in a["loci"]] == [l[:2] for l in b["loci"]]
    assert any(x[2:4] != y[2:4] for x, y in zip(a["loci"], b["loci"]))
    assert all(l[2] == 0 for l in a["loci"]) and all(l[3] == 0 for l in b["loci"])
    return reads


# ---- identity_ties ------------------------------------------------------------------------------------------------
def identity_ties():
    g = genome()
    rng = np.random.default_rng(205)
    c0 = CLUSTER_AT
    mis = lambda n: ("M", n, "x")  # noqa: E731
    shapes = {                                                        # name: (spec, matches, as_size)
        "t40_39": ([("M", 22), mis(1), ("M", 17)], 39, 40),
        "t40_39i": ([("M", 37), ("I", 1), ("M", 2)], 39, 40),
        "t40_38": ([("M", 22), mis(2), ("M", 16)], 38, 40),
        "t40_40": ([("M", 40)], 40, 40),
        "t200_197": ([("M", 100), ("D", 3), ("M", 97)], 197, 200),
        "t200_197x": ([("=", 60), ("X", 1), ("=", 60), ("X", 2), ("=", 77)], 197, 200),
        "t200_196": ([("M", 100), ("D", 3), ("M", 57), mis(1), ("M", 39)], 196, 200),
        "t200_198": ([("M", 100), ("D", 2), ("M", 98)], 198, 200),
        "t80_78": ([("M", 30), ("I", 1), ("M", 48), ("D", 1)], 78, 80),         # 97.5 again, by gaps only
    }
    reads = []
    for k, (nm, (spec, m, n)) in enumerate(shapes.items()):
        for flag, tag in ((0, "f"), (16, "r")):
            r = make_read(f"tie_{nm}_{tag}", flag, (k + (flag >> 4)) % 3, c0 + k, spec, g, rng, mapq=int(10 + 5 * k))
            reads.append(r)
    reads.sort(key=lambda r: (r.tid, r.pos))
    P = _oracle()
    for r in reads:
        nm = r.name.split("_", 1)[1].rsplit("_", 1)[0]
        _spec, m, n = shapes[nm]
        a = P.map_info(r.flag, r.pos, r.cigar, r.seq, g[r.tid][1])
        assert a["as_size"] == n and a["pi"] == 100.0 * m / n, (r.name, a["pi"])
    for x in TIE_VALUES:
        up = float(np.nextafter(x, 200.0))
        tie = [r for r in reads if P.map_info(r.flag, r.pos, r.cigar, r.seq, g[r.tid][1])["pi"] == x]
        assert len(tie) >= 4
        for r in tie:                                                  # kept at -f x, dropped at the next double above
            assert P.read_contribution(as_dict(r), g, min_pi=x)[1]
            assert not P.read_contribution(as_dict(r), g, min_pi=up)[1]
    return reads


def fixture_reads():
    """the alignments recorded in tests/golden/align_edges.json, a sample that keeps the file small: the whole cigar_zoo (but
    REF_UNDEFINED); of the boundaries the reads of 1-7 columns on the first and last bases of chr2 (and two of chr1 / chr3), the
    clipped and gapped tails and one N on N; every 24th read of tiny_crowd.  With the reference built, the CPU test runs
    every read of every class through it."""
    def keep(nm):
        if nm.startswith(("bnd_head", "bnd_tail")) and nm[8].isdigit():
            n = int(nm[:-1].split("_")[2])
            return n <= 7 and (nm[8] == "1" or (n in (2, 3) and nm.endswith("f")))
        return nm.startswith(("bnd_tailclip", "bnd_tail_D", "bnd_tail_del2", "bnd_headclip0", "bnd_N_on_N0"))
    reads = cigar_zoo() + [r for r in boundaries() if keep(r.name)] + tiny_crowd()[::24]
    return [r for r in reads if r.name not in REF_UNDEFINED]


def fixture_tag_reads():
    """the records of tests/golden/modparse_edges.json: every dialect on one forward and one reverse read that hold N"""
    return [r for r in foreign_tags() if r.name.startswith(("tag_fN_", "tag_rN_"))]


CLASSES = dict(cigar_zoo=cigar_zoo, boundaries=boundaries, tiny_crowd=tiny_crowd, foreign_tags=foreign_tags,
               identity_ties=identity_ties)


def everything():
    """all classes in one coordinate-sorted list (stable: ties keep class order)"""
    reads = [r for f in CLASSES.values() for r in f()]
    reads.sort(key=lambda r: (r.tid, r.pos))
    return reads


# ---- records the engine must refuse -------------------------------------------------------------------------------
class RawRead:
    """AlignedRead-like with SEQ given as packed nibbles and the CIGAR as BAM words, for records no writer of ours makes"""

    def __init__(self, name, flag, tid, pos, mapq, cigar_words, seq, seq4, mm, ml):
        self.name, self.flag, self.tid, self.pos, self.mapq = name, flag, tid, pos, mapq
        self._cigar, self.seq, self.seq4, self.mm, self.ml, self.hp = cigar_words, seq, np.asarray(seq4, np.uint8), mm, ml, None

    def cigar_u32(self):
        return np.asarray(self._cigar, np.uint32)


def bad_records():
    """-> [(name, read, message)] over genome(): each must be refused with HM_EDATA and this message"""
    g = genome()
    good = make_read("good", 0, 0, CLUSTER_AT, [("M", 41)], g, np.random.default_rng(206))
    s4 = good.seq4
    out = []
    for v in (0, 3, 14):
        for where, idx, shift in (("high", 5, 4), ("low", 7, 0), ("last_odd", len(s4) - 1, 4)):
            b = s4.copy()
            b[idx] = (int(b[idx]) & (0xf0 >> shift)) | (v << shift)
            out.append((f"bad_nibble{v}_{where}", RawRead("n", 0, 0, CLUSTER_AT, 60, good.cigar_u32(), good.seq, b, good.mm, good.ml),
                        f"Illegal BAM base encoded value {v}"))
    out.append(("bad_cigar_B", RawRead("b", 0, 0, CLUSTER_AT, 60, [(20 << 4) | 0, (2 << 4) | 9, (21 << 4) | 0], good.seq, s4, good.mm, good.ml),
                "Unrecognised CIGAR operation"))
    L = len(g[1][1])
    past = make_read("past", 0, 1, L - 40, [("M", 40)], g, np.random.default_rng(207))
    out.append(("bad_past_end", dataclasses.replace(past, pos=L - 39), "alignment runs past the end of the reference sequence"))
    out.append(("bad_past_end_D", dataclasses.replace(past, cigar=[("M", 40), ("D", 1)]), "alignment runs past the end of the reference sequence"))
    return out
