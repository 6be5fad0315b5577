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
ASM_TAIL = 300                                    # small_job: the built haplotype reads cover this much of the first contig's end


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
    # ... and, for the allele-specific regions, two reads per haplotype and strand over the whole middle contig and over the last
    # 300 bases of the first, every call of haplotype 1 methylated and every call of haplotype 2 not: wherever B is placed in the
    # middle contig, its start included, the loci around it are hits of one sign (test_pileup_bigref_cpu.py asserts the chain)
    n1 = len(genome[1][1])
    for tid, pos, length in ((1, 0, n1), (0, n0 - ASM_TAIL, ASM_TAIL)):
        for hp, level in ((1, 255), (2, 0)):
            for rev in (False, True):
                for i in range(2):
                    r = _perfect_read("asm%d_%d_%d_%d" % (tid, hp, rev, i), genome, tid, pos, length, rev, 3)
                    built.append(dataclasses.replace(r, hp=hp, ml=np.full(len(r.ml), level, np.uint8)))
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
COORDS = ("gpos", "start", "end")                 # the fields that hold a global locus: loci, records, sites, asm, bedMethyl rows
                                                  # carry gpos; patterns, domains and asm regions start and end


def _coords_of(rows):
    names = [f for f in COORDS if f in (rows.dtype.names or ())]
    assert names, "rows without a coordinate field"
    return names


def translate(rows, P):
    """the small job's rows (any dtype with gpos, or start and end) where the big job must have them"""
    out = rows.copy()
    for f in _coords_of(out):
        out[f] += P
    return out


def wrap32(g, signed=False):
    """int64 coordinates as they come out of a 32-bit variable"""
    g = np.asarray(g, np.int64) & 0xffffffff
    return g.astype(np.uint32).view(np.int32).astype(np.int64) if signed else g


def truncate32(rows, signed=False):
    """the defect class: the rows a 32-bit locus somewhere on the way would give"""
    out = rows.copy()
    for f in _coords_of(out):
        out[f] = wrap32(out[f], signed)
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


# ---- the newer outputs of the small job, each from its own CPU restatement ---------------------------------------------------------------
THR = (128, 128, 128)                             # the oracle's thresholds for this job (expected_thresholds() asserts it)
PATTERN_SPAN, LINKAGE_DIST, PROFILE_D = 150, 2000, 1024
META = dict(bins=20, flank=2000, flank_bins=10)
REGION_MIN_COVS = (1, 2)
CONTEXT_FLANKS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def small_records():
    """-> (genome, the reads as the restatements take them, their haplotypes)"""
    genome, reads = small_job()
    return genome, [as_dict(r) for r in reads], [r.hp for r in reads]


@functools.lru_cache(maxsize=None)
def expected_thresholds():
    want, _n = oracle_small()
    assert tuple(want["thresholds"]) == THR
    return list(THR)


def _as(dtype, tuples):
    return np.array(tuples, dtype) if tuples else np.zeros(0, dtype)


@functools.lru_cache(maxsize=None)
def expected_patterns(k, min_reads=1):
    import patterns_ref
    from hifimeth_amd.pileup import PATTERN_DTYPE
    genome, recs, _hp = small_records()
    return _as(PATTERN_DTYPE, patterns_ref.rows(recs, genome, k, PATTERN_SPAN, expected_thresholds()[0], min_reads, 0, MIN_PI))


@functools.lru_cache(maxsize=None)
def expected_bedmethyl(min_valid, part=0):
    import bedmethyl_ref
    from hifimeth_amd.pileup import BEDMETHYL_DTYPE
    genome, recs, hps = small_records()
    rows = bedmethyl_ref.rows(recs, genome, expected_thresholds()[0], min_valid, part, hps, 0, MIN_PI)
    return _as(BEDMETHYL_DTYPE, [r + (0,) for r in rows])


@functools.lru_cache(maxsize=None)
def expected_bedmethyl_counters():
    import bedmethyl_ref
    genome, recs, hps = small_records()
    return bedmethyl_ref.counters(recs, genome, expected_thresholds()[0], hps, 0, MIN_PI)


@functools.lru_cache(maxsize=None)
def expected_linkage_pairs():
    import linkage_ref
    genome, recs, _hp = small_records()
    return linkage_ref.pairs(recs, genome, LINKAGE_DIST, expected_thresholds()[0], 0, MIN_PI)


@functools.lru_cache(maxsize=None)
def expected_linkage(min_pairs=0):
    import linkage_ref
    from hifimeth_amd.pileup import LINKAGE_DTYPE
    genome, recs, _hp = small_records()
    rows = linkage_ref.rows(recs, genome, LINKAGE_DIST, expected_thresholds()[0], min_pairs, 0, MIN_PI)
    return _as(LINKAGE_DTYPE, [(d, 0, *c) for d, *c in rows])


@functools.lru_cache(maxsize=None)
def expected_readpos(min_calls=0):
    import readpos_ref
    from hifimeth_amd.pileup import READPOS_DTYPE
    genome, recs, _hp = small_records()
    rows = readpos_ref.rows(recs, genome, PROFILE_D, expected_thresholds(), min_calls, min_pi=MIN_PI)
    return _as(READPOS_DTYPE, [(m, e, d, 0, n_m, n_u, s) for m, e, d, n_m, n_u, s in rows])


@functools.lru_cache(maxsize=None)
def expected_readpos_histograms():
    """uint64 [3, 2 D + 1, 256]: context, bin (5' 0 .. D - 1, 3' 0 .. D - 1, interior), ML byte"""
    import readpos_ref
    genome, recs, _hp = small_records()
    out = np.zeros((3, 2 * PROFILE_D + 1, 256), np.uint64)
    for (motif, end, dist), h in readpos_ref.histograms(recs, genome, PROFILE_D, min_pi=MIN_PI).items():
        out[motif, 2 * PROFILE_D if end == 2 else end * PROFILE_D + dist] = h
    return out


def linkage_straddlers(g):
    """pairs of member loci of one record, at most LINKAGE_DIST apart, with the lower member below the global small locus g and
    the upper at or above it: what a 32-bit locus in the pair kernel loses once g lies on the boundary"""
    import patterns_ref
    genome, recs, _hp = small_records()
    off = offsets_of(genome)
    n = 0
    for rec in recs:
        x = sorted(int(off[sid]) + soff for sid, soff in patterns_ref.member_loci(rec, genome, 0, MIN_PI))
        n += sum(1 for i, a in enumerate(x) for b in x[i + 1:] if a < g <= b and 2 <= b - a <= LINKAGE_DIST)
    return n


@functools.lru_cache(maxsize=None)
def oracle_loci():
    want, _n = oracle_small()
    genome, _reads = small_job()
    return oracle_locus_rows(want, offsets_of(genome))


@functools.lru_cache(maxsize=None)
def oracle_planes():
    """(pcov, ncov, key) over the small reference, from the oracle's loci"""
    import regions_ref
    genome, _reads = small_job()
    return regions_ref.planes_from_loci(oracle_loci(), int(offsets_of(genome)[-1]))


@functools.lru_cache(maxsize=None)
def _running(min_cov, base):
    import regions_ref
    return regions_ref.Running(*oracle_planes(), min_cov=min_cov, base=base)


def region_block():
    from hifimeth_amd.pileup import region_geometry
    return region_geometry()[0]


def _pairs(points):
    return np.array([(a, b) for a in points for b in points if a < b], np.int64).T


def intervals(g):
    """the fixed interval set of `-R` around the placed small locus g -> (start, end), small coordinates: every pair of the points
    g - 1, g, g + 1, g +- one block of the region index and g +- (one block + 1), each contig, and all three contigs at once"""
    genome, _reads = small_job()
    off = offsets_of(genome)
    blk = region_block()
    pts = sorted({g - blk - 1, g - blk, g - 1, g, g + 1, g + blk, g + blk + 1})
    assert pts[0] >= 0 and pts[-1] <= off[-1]
    start, end = _pairs(pts)
    start = np.concatenate([start, off[:-1], [0]])
    end = np.concatenate([end, off[1:], [off[-1]]])
    return start.astype(np.int64), end.astype(np.int64)


def meta_intervals():
    """the metaplot's intervals -> (start, end, seq_start, seq_end, strand), small coordinates: one within 500 bases of every
    contig's start and one within 500 of its end, so that a flank of 2000 is clamped to the sequence on either side; strands mixed"""
    genome, _reads = small_job()
    off = offsets_of(genome)
    rows = []
    for k, st in enumerate(("+-", "-.", ".+")):
        a, b = int(off[k]), int(off[k + 1])
        rows += [(a + 100 + 7 * k, a + 430 + k, a, b, st[0]), (b - 460 - k, b - 120 - 5 * k, a, b, st[1])]
    start, end, s0, s1 = (np.array([r[i] for r in rows], np.int64) for i in range(4))
    assert (((start - s0 < 500) | (s1 - end < 500)) & (end - start >= META["bins"])).all()
    return start, end, s0, s1, "".join(r[4] for r in rows).encode()


def expected_regions(start, end, min_cov=1, base=0, lo=None, hi=None):
    """int64 [n, 3, 4] for intervals in the coordinates of planes that begin at locus `base`"""
    import regions_ref
    return regions_ref.region_sums(_running(min_cov, base), start, end, lo, hi)


def expected_metaplot(start, end, s0, s1, strand, min_cov=1, base=0, lo=None, hi=None):
    """-> (int64 [3, bins + 2 flank_bins, 5]: n_regions, n_loci, pcov, ncov, ppm; n_used)"""
    import regions_ref
    return regions_ref.metaplot(_running(min_cov, base), start, end, s0, s1, strand.decode(), META["bins"], META["flank"],
                                META["flank_bins"], lo, hi)


def region_table(sums):
    """REGION_SUM_DTYPE [n, 3] -> int64 [n, 3, 4]"""
    import regions_ref
    return np.stack([sums[k] for k in regions_ref.QUANTITIES], axis=-1).astype(np.int64)


def meta_table(rows):
    """METABIN_DTYPE rows -> int64 [3, n_bins, 5] in expected_metaplot's order"""
    import regions_ref
    nb = META["bins"] + 2 * META["flank_bins"]
    assert rows["motif"].tolist() == [c for c in range(3) for _ in range(nb)] and rows["bin"].tolist() == list(range(nb)) * 3
    return np.stack([rows[k] for k in ("n_regions",) + regions_ref.QUANTITIES], axis=-1).astype(np.int64).reshape(3, nb, 5)


@functools.lru_cache(maxsize=8)
def expected_context(flank, lo=0, hi=None, min_cov=1):
    """int64 [3, 4^k + 1, 4] over the small loci [lo, hi) (at flank 3 a table is 25 MB: only a few are kept)"""
    import context_ref
    genome, _reads = small_job()
    return context_ref.context_table(*oracle_planes(), [s for _n, s in genome], flank, min_cov, 0, lo, hi)


def domain_scores_of(ctx):
    from hifimeth_amd.pileup import DOMAIN_LEVELS, domain_scores
    return domain_scores(*DOMAIN_LEVELS[ctx])


def expected_domains(loci, ctx, lo, hi):
    """-> (segments, R, (P0, N0, R0, P1, N1, R1)) of context ctx over the loci rows inside [lo, hi)"""
    import domains_ref
    from hifimeth_amd.pileup import DOMAIN_MAX_GAP
    rows = loci[(loci["gpos"] >= lo) & (loci["gpos"] < hi)]
    seg, R = domains_ref.domains(rows, ctx, *domain_scores_of(ctx), DOMAIN_MAX_GAP)
    sums = tuple(int(seg[f][seg["state"] == z].sum()) for z in (0, 1) for f in ("pcov", "ncov", "n_loci"))
    return seg, R, sums


# ---- allele-specific regions: the rows of the haplotype test from the oracle, the p-values exact -------------------------------------
ASM_MIN_COV = 1
ASM_MAX_P = 0.5                                   # the exact p-values of this job nearest to it are 0.4667 and 1: a table split 2 : 0
ASM_MAX_GAP, ASM_MIN_LOCI = 500, 2                # against 0 : 2 (p = 1/3) is a hit, an even one (p = 1) is none and breaks a chain


def option_sets(partitions):
    """the engine options of the cases that run the outputs which need one, and the number of bedMethyl sets they give"""
    return dict(patterns=2 if partitions else 4, bedmethyl=True, linkage=LINKAGE_DIST, profile=PROFILE_D), 3 if partitions else 1


OPTION_CASES = [(B32, "cpg_at_B"), (B32, "contig_at_B"), (B31, "cpg_at_B")]
OPTION_CASE_IDS = ["2^%d-%s-options" % (B.bit_length() - 1, pl) for B, pl in OPTION_CASES]


@functools.lru_cache(maxsize=None)
def expected_asm_rows():
    """the hm_asm_t rows at ASM_MIN_COV: counts per haplotype from the oracle's per-read contributions, diff as the host forms it,
    pvalue = the exact two-sided Fisher p rounded to fp64 (the device's differs from it in the last bits)"""
    from hifimeth_amd.pileup import ASM_DTYPE
    from oracle import pileup_oracle as P
    from test_gpu_pileup_asm import fisher_exact
    genome, recs, hps = small_records()
    want, _n = oracle_small()
    off, thr = offsets_of(genome), expected_thresholds()
    motif = {(sid, soff): m for sid, soff, _p, _n2, m in want["loci"]}
    cov = {1: {}, 2: {}}
    for rec, hp in zip(recs, hps):
        if hp in cov:
            for sid, soff, prob, m in P.read_contribution(rec, genome, 0, MIN_PI)[1]:
                cov[hp].setdefault((sid, soff), [0, 0])[0 if prob >= thr[m] else 1] += 1
    keys = [k for k in sorted(set(cov[1]) & set(cov[2])) if min(sum(cov[1][k]), sum(cov[2][k])) >= ASM_MIN_COV]
    rows = np.zeros(len(keys), ASM_DTYPE)
    cache = {}
    for r, k in zip(rows, keys):
        t = (*cov[1][k], *cov[2][k])
        if t not in cache:
            cache[t] = float(fisher_exact(*t))
        r["gpos"], r["motif"], r["pvalue"] = int(off[k[0]]) + k[1], motif[k], cache[t]
        r["pcov1"], r["ncov1"], r["pcov2"], r["ncov2"] = t
    p1, n1, p2, n2 = (rows[f].astype(np.int64) for f in ("pcov1", "ncov1", "pcov2", "ncov2"))
    rows["diff"] = 100.0 * p1 / (p1 + n1) - 100.0 * p2 / (p2 + n2)
    return rows


def expected_asm_regions(asm_rows, ctx, lo, hi):
    """-> (chains, R) of context ctx over the hm_asm_t rows inside [lo, hi), keep_edges as the GPU test asks"""
    import asm_regions_ref
    rows = asm_rows[(asm_rows["gpos"] >= lo) & (asm_rows["gpos"] < hi)]
    return asm_regions_ref.regions(rows, ctx, ASM_MAX_P, ASM_MAX_GAP, ASM_MIN_LOCI, keep_edges=True)
