"""Pileup on a reference that crosses 2^31 / 2^32 bases: the small job, the pad that puts it across a boundary, and the
translation of its results (shared by test_gpu_pileup_bigref.py and test_pileup_bigref_cpu.py).

The big job is the small job behind one contig of P times 'N': every locus moves by P, every sequence index by 1, and nothing
else may change.  P is chosen from the small job's own results so that a boundary B (2^31 or 2^32) falls

    cpg_at_B      on a covered CpG locus g* inside the middle contig (depth >= 3, a forward and a reverse match run around it)
    rev_chh_at_B  on the recorded locus of a reverse-strand CHH record (project_kernel records it at g + 2: the deciding
                  column lies below B, the record at B)
    contig_at_B   on the first base of the middle contig

Nothing here needs a GPU: the expectations come from the CPU oracle (oracle/pileup_oracle.py)."""
import dataclasses
import functools

import numpy as np

B31, B32 = 1 << 31, 1 << 32
BOUNDARIES = (B31, B32)
PLACEMENTS = ("cpg_at_B", "rev_chh_at_B", "contig_at_B")
CASES = [(B, pl) for B in BOUNDARIES for pl in PLACEMENTS]
CASE_IDS = ["2^%d-%s" % (B.bit_length() - 1, pl) for B, pl in CASES]
HOST_LEN = {B: B + 40000 for B in BOUNDARIES}      # the reference / label buffer of a boundary: every placement's total fits
MIN_PI = 97.0                                     # at err = 0.03 the reads' identities lie on both sides of it
RATES = (0.02, 0.05, 0.013)                       # of the binomial test's table
LABEL_SEED = 77


def as_dict(r):
    return dict(flag=r.flag, tid=r.tid, pos=r.pos, mapq=r.mapq, cigar=r.cigar, seq=r.seq, mm=r.mm, ml=r.ml)


def _perfect_read(name, genome, tid, pos, length, rev, seed):
    """a read equal to the reference over [pos, pos + length) of contig tid (N replaced), every C of its own strand called"""
    from hifimeth_amd.synth import AlignedRead, revcomp
    rng = np.random.default_rng(seed)
    ref = genome[tid][1][pos:pos + length]
    seq = "".join(c if c != "N" else "A" for c in ref)
    cigar = []
    for c in ref:                                  # '=' over ACGT, 'X' over a reference N
        op = "X" if c == "N" else "="
        if cigar and cigar[-1][0] == op:
            cigar[-1][1] += 1
        else:
            cigar.append([op, 1])
    fwd = revcomp(seq) if rev else seq
    n = fwd.count("C")
    return AlignedRead(name, 16 if rev else 0, tid, pos, 60, [(o, k) for o, k in cigar], seq, "C+m" + ",0" * n + ";",
                       rng.integers(0, 256, n).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def small_job():
    """-> (genome, reads): test_gpu_pileup.py::_data's set at err = 0.03 with the haplotype tags and extra secondary /
    supplementary flags of test_gpu_pileup_hp.py::_tagged_reads, plus two built reads that make the contig_at_B placement hold
    whatever the random set does: one ending on the last base of the first contig, one starting 3 bases into the middle one."""
    from hifimeth_amd.synth import synth_alignments, synth_genome
    genome = synth_genome(n_chr=3, length=12000, seed=7)
    reads = synth_alignments(genome, 60, seed=8, median_len=1500, err=0.03, eqx=True)
    rng = np.random.default_rng(9)
    out = []
    for r in reads:
        hp = [None, 1, 2, 3][int(rng.integers(0, 4))]
        flag = r.flag
        if not flag & 4 and rng.random() < 0.1:
            flag |= 0x100 if rng.random() < 0.5 else 0x800
        out.append(dataclasses.replace(r, hp=hp, flag=flag))
    n0 = len(genome[0][1])
    built = [dataclasses.replace(_perfect_read("tail0", genome, 0, n0 - 700, 700, False, 1), hp=1),
             dataclasses.replace(_perfect_read("head1", genome, 1, 3, 700, True, 2), hp=2)]
    mapped = sorted([r for r in out if not r.flag & 4] + built, key=lambda r: (r.tid, r.pos))
    return genome, mapped + [r for r in out if r.flag & 4]


def offsets_of(genome):
    return np.concatenate([[0], np.cumsum([len(s) for _, s in genome])]).astype(np.int64)


def shifted_reads(reads):
    """the big job's reads: the sequence index moves behind the pad, nothing else changes (unmapped records keep tid -1)"""
    return [r if r.flag & 4 else dataclasses.replace(r, tid=r.tid + 1) for r in reads]


@functools.lru_cache(maxsize=None)
def oracle_small():
    """-> (oracle result with MIN_PI, number of records without the filter)"""
    from oracle import pileup_oracle as P
    genome, reads = small_job()
    recs = [as_dict(r) for r in reads]
    return P.pileup(recs, genome, min_pi=MIN_PI), len(P.pileup(recs, genome)["records"])


@functools.lru_cache(maxsize=None)
def tested_loci():
    """small-job loci where both haplotypes have a counted call (the rows of the haplotype test at min_cov 1), ascending"""
    from oracle import pileup_oracle as P
    genome, reads = small_job()
    off = offsets_of(genome)
    cov = {1: set(), 2: set()}
    for r in reads:
        if r.hp in cov and not r.flag & 4:
            cov[r.hp].update(int(off[sid]) + soff for sid, soff, _p, _m in P.read_contribution(as_dict(r), genome, 0, MIN_PI)[1])
    return np.array(sorted(cov[1] & cov[2]), np.int64)


def match_runs(r):
    """maximal runs of M / = / X columns of a mapped read -> [(first reference offset in its contig, length)]"""
    runs, s, open_ = [], r.pos, False
    for op, n in r.cigar:
        if op in "M=X":
            if n == 0:
                continue
            if open_:
                runs[-1][1] += n
            else:
                runs.append([s, n])
            open_, s = True, s + n
        elif op == "I":
            open_ = open_ and n == 0
        elif op in "DN":
            s += n
            open_ = open_ and n == 0
    return [(a, n) for a, n in runs]


def small_labels(n):
    """the fixed-seed -1 / 0 / 1 truth labels over the small reference"""
    return np.random.default_rng(LABEL_SEED).integers(-1, 2, n).astype(np.int8)


def record_gpos(want, offsets):
    return np.array([offsets[sid] + soff for sid, soff, _p, _m in want["records"]], np.int64)


def loci_gpos(want, offsets):
    return np.array([offsets[sid] + soff for sid, soff, _p, _n, _m in want["loci"]], np.int64)


def placement(name, B, genome, reads, want):
    """-> (P, g): the pad length and the small-job locus that lands on B, with the placement's own preconditions asserted"""
    off = offsets_of(genome)
    lo, hi = int(off[1]) + 100, int(off[2]) - 100               # the interior of the middle contig
    if name == "contig_at_B":
        g = int(off[1])
        assert any(r.tid == 1 and not r.flag & 4 and r.pos <= 10 and r.mm is not None for r in reads)
    elif name == "cpg_at_B":
        g = None
        runs = [(r.flag & 16, int(off[r.tid]) + a, n) for r in reads if not r.flag & 4 and r.mm is not None for a, n in match_runs(r)]
        for sid, soff, pc, nc, motif in want["loci"]:
            x = int(off[sid]) + soff
            if motif != 0 or pc + nc < 3 or not lo <= x < hi or genome[sid][1][soff:soff + 2] != "CG":
                continue
            around = {bool(rev) for rev, a, n in runs if a <= x - 3 and a + n - 1 >= x + 3}
            if around == {False, True}:
                g = x
                break
        assert g is not None, "no covered CpG with depth >= 3 and a forward and a reverse run around it"
    elif name == "rev_chh_at_B":
        cand = sorted({int(off[sid]) + soff for sid, soff, _p, motif in want["records"]
                       if motif == 2 and genome[sid][1][soff] == "G" and lo <= off[sid] + soff < hi})
        assert cand, "no reverse-strand CHH record inside the middle contig"
        both = tested_loci()                                    # ... one with rows of the haplotype test within 5000 loci either side
        cand = [x for x in cand if ((both >= x - 5000) & (both < x)).sum() >= 20 and ((both >= x) & (both < x + 5000)).sum() >= 20]
        assert cand, "no reverse-strand CHH record with haplotype-tested loci around it"
        g = cand[len(cand) // 2]
        assert genome[1][1][g - int(off[1])] == "G"             # recorded at the G, two columns above the deciding one
    else:
        raise ValueError(name)
    return B - g, g


def check_preconditions(name, B, P, rec_gpos, locus_gpos):
    """what makes a case worth its memory, from the small job's loci alone (rec_gpos / locus_gpos: small coordinates)"""
    big_rec, big_loci = rec_gpos + P, locus_gpos + P
    assert (big_rec < B).sum() >= 1000 and (big_rec >= B).sum() >= 1000, "fewer than 1000 records on one side of B"
    assert ((big_loci >= B - 65) & (big_loci < B)).any(), "no covered locus within 64 below B"
    if name == "contig_at_B":
        assert ((big_loci >= B) & (big_loci <= B + 64)).any(), "no covered locus within 64 above B"
    else:
        assert (big_loci == B).any() and (big_rec == B).any(), "B itself is not a recorded, covered locus"
    for g in (big_rec, big_loci):                               # a kernel with a 32-bit locus cannot give the expected set:
        assert set(g.astype(np.int32).astype(np.int64).tolist()) != set(g.tolist())      # an int32 wraps from 2^31 on, ...
        assert B < B32 or set((g & 0xffffffff).tolist()) != set(g.tolist())              # ... a uint32 from 2^32 on


# ---- translation and the comparison every row fetch goes through ------------------------------------------------------------------
def translate(rows, P):
    """the small job's rows (any dtype with a gpos field) where the big job must have them"""
    out = rows.copy()
    out["gpos"] += P
    return out


def truncate32(rows, signed=False):
    """the defect class: the rows a 32-bit locus somewhere on the way would give"""
    out = rows.copy()
    g = out["gpos"] & 0xffffffff
    out["gpos"] = g.astype(np.uint32).view(np.int32).astype(np.int64) if signed else g
    return out


def same_rows(got, want):
    """exact: dtype, number, and every byte (floats as bits)"""
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def assert_same_rows(got, want, what=""):
    assert got.dtype == want.dtype, what
    assert len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        i = next(k for k in range(len(got)) if got[k:k + 1].tobytes() != want[k:k + 1].tobytes())
        raise AssertionError("%s: row %d is %r, expected %r" % (what, i, got[i], want[i]))


def sorted_records(g, p, m, o):
    """records() as one array sorted by (gpos, prob, motif, order)"""
    rec = np.zeros(len(g), [("gpos", "<i8"), ("prob", "u1"), ("motif", "u1"), ("order", "<u4")])
    rec["gpos"], rec["prob"], rec["motif"], rec["order"] = g, p, m, o
    return np.sort(rec, order=["gpos", "prob", "motif", "order"])


def ranges(B, P, n_small):
    """[(name, (big lo, big hi), (small lo, small hi))]: the whole reference, either side of B, the two loci around it, and
    5000 loci either side of it (B - 5000 is no multiple of 4096: the fetch's blocks do not line up with B)"""
    g, total = B - P, P + n_small
    assert (B - 5000) % 4096 and 0 <= g - 5000 and g + 5000 <= n_small
    return [("all", (0, total), (0, n_small)), ("below", (0, B), (0, g)), ("above", (B, total), (g, n_small)),
            ("around", (B - 1, B + 1), (g - 1, g + 1)), ("near", (B - 5000, B + 5000), (g - 5000, g + 5000))]


def oracle_locus_rows(want, offsets):
    """the oracle's loci as LOCUS_DTYPE rows in small coordinates"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    rows = np.zeros(len(want["loci"]), LOCUS_DTYPE)
    for i, (sid, soff, pc, nc, motif) in enumerate(want["loci"]):
        rows[i] = (offsets[sid] + soff, pc, nc, motif, 0)
    return rows
