"""One data set for `pileup_dist` on three, five and eight ranks (plain module, imported by test_dist_cases_cpu.py and
test_gpu_pileup_dist_worlds.py): a genome of four sequences, about a thousand short reads, a BED file and one option list, laid
out around the chunk boundaries that locus_ranges gives the three worlds.  Nothing is random beyond seeded generators.

    genome()            ctl (the unmethylated control of -B), chrA (the long one: it holds whole chunks of every world), chrS
                        (shorter than a world-8 chunk: one chunk holds all of it and parts of both neighbours), chrB;
                        n_loci = 120 019 is a multiple of neither 3, 5 nor 8, a world-8 chunk is longer than 3 HM_REGION_BLOCK
    reads()             coordinate-sorted AlignedRead records with HP 1 / 2 / none:
                        * ten around every chunk boundary of the three worlds, both strands, clips and gaps, one ending and one
                          starting on the boundary; the reference there holds a forward and a reverse CHH cytosine within three
                          bases on either side,
                        * a thin scatter everywhere,
                        * two stacks of 256 reads (128 per haplotype) on ctl and chrB, five world-8 chunks between them,
                        * the stretch Z of chrA, longer than a world-3 chunk: its reads list no CHG cytosine; untagged reads every
                          800 bases are methylated in CpG and CHH (one -D H segment), islands of 6 + 6 tagged reads that list CpG
                          only, methylated on HP 1 and not on HP 2, stand on every boundary in Z and at most 2500 bases apart (one
                          -G region under -g 3000)
    bed_rows()          the intervals of -R
    options(bed)        the option list of every run;  slab(world, n)  the --slab of a world
    ghost()             the input of the error test: a header sequence the FASTA lacks, one record on it in rank 1's slab

The conditions these are for are asserted, from the references, by test_dist_cases_cpu.py."""
import functools

import numpy as np

import pileup_cases as C
from hifimeth_amd.pileup import locus_ranges
from hifimeth_amd.synth import AlignedRead, revcomp

WORLDS = (3, 5, 8)
NAMES = ("ctl", "chrA", "chrS", "chrB")
LENGTHS = (31013, 64007, 9011, 15988)
CONTROL = "ctl"
REGION_BLOCK = 4096                # HM_REGION_BLOCK
MOTIF = "ATGCATGCAT"               # around a boundary b, from b - 5: G at b - 3 and b + 1 (ATG), C at b - 2 and b + 2 (CAT)
Z = (39400, 80700)                 # the stretch, in loci of the concatenated genome
MAX_GAP, MIN_LOCI = 3000, 4        # -g, -n
STACKS = ((0, 20000), (3, 8000))   # (sequence, position) of the two stacks
STACK_DEPTH, STACK_LEN = 256, 60
SMALL_SLAB = 7
FWD_CHH, REV_CHH = C._oracle().FWD_CHH, C._oracle().REV_CHH


def offsets():
    return np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)


N_LOCI = int(sum(LENGTHS))


def boundaries(world):
    """the first loci of the ranks 1 .. world - 1"""
    return [lo for lo, _hi in locus_ranges(N_LOCI, world)[1:]]


def all_boundaries():
    return sorted({b for w in WORLDS for b in boundaries(w)})


def locate(g):
    """a locus of the concatenated genome -> (sequence, position in it)"""
    off = offsets()
    sid = int(np.searchsorted(off, g, side="right") - 1)
    return sid, int(g - off[sid])


@functools.lru_cache(maxsize=None)
def genome():
    rng = np.random.default_rng(3301)
    cat = np.frombuffer(b"ACGT", np.uint8)[rng.choice(4, N_LOCI, p=[0.29, 0.21, 0.21, 0.29])].copy()
    off = offsets()
    for b in all_boundaries():
        assert all(abs(b - int(j)) > 700 for j in off), "a boundary next to a joint of two sequences"
        cat[b - 5:b + 5] = np.frombuffer(MOTIF.encode(), np.uint8)
    text = cat.tobytes().decode()
    return [(n, text[int(a):int(b)]) for n, a, b in zip(NAMES, off[:-1], off[1:])]


def _level(g, hp, rng):
    """the ML byte of a call at locus g of a read of haplotype hp (islands are made by _island)"""
    off = offsets()
    p = 0.95 if Z[0] <= g < Z[1] else 0.03 if g < off[1] else 0.1 if g < off[2] else 0.3
    if rng.random() < 0.08:
        return int(rng.integers(0, 256))                              # bytes on both sides of any threshold
    return int(rng.integers(200, 256)) if rng.random() < p else int(rng.integers(0, 56))


def _listed(fwd, mode):
    """-> [(base, MM head, keep)] of a read whose forward strand is fwd: "all" lists every C and G, "cpg" the C of CG only,
    "no_chg" the C of CG and of the forward CHH words and the G of the reverse CHH words (no call can make a CHG record)"""
    if mode == "all":
        return [("C", "C+m", None), ("G", "G-m", None)]
    cpg = lambda k, q: fwd[q + 1:q + 2] == "G"  # noqa: E731
    if mode == "cpg":
        return [("C", "C+m", cpg)]
    return [("C", "C+m", lambda k, q: cpg(k, q) or fwd[q:q + 3] in FWD_CHH), ("G", "G-m", lambda k, q: q >= 2 and fwd[q - 2:q + 1] in REV_CHH)]


def _read(name, flag, tid, pos, spec, hp, mode, rng, ml_of):
    g = genome()
    seq = C.build_seq(g[tid][1], pos, spec, rng)
    fwd = revcomp(seq) if flag & 16 else seq
    lead = spec[0][1] if spec[0][0] == "S" else 0
    base = int(offsets()[tid]) + pos - lead
    parts, ml = [], []
    for b, head, keep in _listed(fwd, mode):
        text, qs = C._positions_mm(fwd, b, head, keep)
        parts.append(text)
        ml += [ml_of(base + (len(seq) - 1 - q if flag & 16 else q), hp, rng) for q in qs]     # about the locus: gaps are short
    assert ml, name
    return AlignedRead(name, flag, tid, pos, 60, [(it[0], it[1]) for it in spec], seq, "".join(parts), np.array(ml, np.uint8), hp)


def _span(spec):
    return sum(it[1] for it in spec if it[0] in "M=XDN")


def _plain(name, k, tid, pos, spec, rng):
    """a read that is not an island's: in Z untagged and without CHG calls, elsewhere HP 1 / 2 / none and every C and G"""
    a = int(offsets()[tid]) + pos
    in_z = a < Z[1] and a + _span(spec) > Z[0]
    return _read(name, 16 if k % 2 else 0, tid, pos, spec, None if in_z else (1, 2, None)[k % 3], "no_chg" if in_z else "all", rng, _level)


def _shape(k, n):
    """the CIGAR of the k-th read of a group, n reference bases: plain, clipped at either end, with a deletion, with an insertion"""
    kind = k % 5
    if kind == 1:
        return [("S", 5), ("M", n)]
    if kind == 2:
        return [("M", n // 3), ("D", 3), ("M", n - n // 3 - 3)]
    if kind == 3:
        return [("M", n - 40), ("I", 2), ("M", 40), ("S", 8)]
    return [("M", n)]


WINDOW = ((590, 600), (450, 500), (300, 400), (180, 300), (90, 250), (40, 200), (10, 220), (2, 350), (0, 300), (300, 300))


def _island(name, k, g0, rng):
    """6 + 6 reads of one geometry and one strand (so that -I trims the same columns of all): CpG calls only, HP 1 methylated"""
    tid, pos = locate(g0)
    ml = lambda g, hp, _rng: (230 if hp == 1 else 10) + g % 20  # noqa: E731
    return [_read(f"{name}_{i}", 16 if k % 2 else 0, tid, pos, [("M", 200)], 1 + i % 2, "cpg", rng, ml) for i in range(12)]


def island_starts():
    """islands on every boundary in Z, one at either end of it, and more until no two are more than 2500 bases apart"""
    at = sorted({Z[0] + 100, Z[1] - 300} | {b - 100 for b in all_boundaries() if Z[0] + 200 < b < Z[1] - 300})
    out = [at[0]]
    for x in at[1:]:
        while x - out[-1] > 2500:
            out.append(out[-1] + 2400)
        out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def reads():
    rng = np.random.default_rng(3302)
    off, out = offsets(), []
    for b in all_boundaries():
        tid, at = locate(b)
        for k, (before, n) in enumerate(WINDOW):
            assert 0 <= at - before and at - before + n <= LENGTHS[tid]
            out.append(_plain(f"w{b}_{k}", k, tid, at - before, _shape(k, n), rng))
    k = 0
    for tid, L in enumerate(LENGTHS):                                 # the scatter: 300 bases every 1300
        for pos in range(150, L - 400, 1300):
            out.append(_plain(f"s{tid}_{pos}", k, tid, pos + int(rng.integers(0, 60)), _shape(k + 2, 300), rng))
            k += 1
    for k, g0 in enumerate(range(Z[0], Z[1] - 300, 800)):             # Z: methylated in CpG and CHH, rows at most 1000 apart
        tid, pos = locate(g0)
        out.append(_plain(f"z{g0}", k, tid, pos, [("M", 300)], rng))
    for k, g0 in enumerate(island_starts()):
        out += _island(f"i{g0}", k, g0, rng)
    for s, (tid, pos) in enumerate(STACKS):
        for i in range(STACK_DEPTH):
            out.append(_read(f"k{s}_{i}", 16 if (i >> 1) % 2 else 0, tid, pos, [("M", STACK_LEN)], 1 + i % 2, "all", rng, _level))
    out.sort(key=lambda r: (r.tid, r.pos))
    assert all(0 <= r.pos and r.pos + _span(r.cigar) <= LENGTHS[r.tid] for r in out) and int(off[-1]) == N_LOCI
    return tuple(out)


def hp_tags(rs):
    return [[("C", r.hp)] if r.hp else [] for r in rs]


def bed_rows():
    """[(sequence name, start, end, name, strand)], positions in the sequence"""
    r8 = locus_ranges(N_LOCI, 8)
    b3, b5 = boundaries(3), boundaries(5)
    rows = [("whole_chunk", r8[4][0] - 500, r8[4][1] + 300, "+"),                          # holds all of rank 4's chunk of eight
            ("whole_block", r8[5][0] + REGION_BLOCK - 10, r8[5][0] + 2 * REGION_BLOCK + 10, "-"),   # a block of rank 5's index, no boundary
            ("flank_up", r8[3][0] + 10, r8[3][0] + 200, "+"),                              # the upstream flank [b - 20, b + 10) crosses b
            ("flank_down", r8[6][0] - 200, r8[6][0] - 10, "-"),                            # the flank behind a reverse interval crosses b
            ("ends_on_8", r8[2][0] - 400, r8[2][0], "."), ("starts_on_8", r8[2][0], r8[2][0] + 350, "+"),
            ("ends_on_3", b3[1] - 333, b3[1], "-"), ("starts_on_3", b3[1], b3[1] + 77, "."),
            ("ends_on_5", b5[2] - 250, b5[2], "+"), ("starts_on_5", b5[2], b5[2] + 250, "-"),
            ("all_of_chrS", int(offsets()[2]), int(offsets()[3]), "+"),
            ("on_chrB", int(offsets()[3]) + 7000, int(offsets()[3]) + 9000, "."),          # ranks 0 .. 5 of eight do not touch chrB
            ("too_short", r8[1][0] - 1, r8[1][0] + 2, "+")]                                # fewer bases than bins: not in the metaplot
    out = []
    for name, a, b, strand in rows:
        sid, lo = locate(a)
        assert locate(b - 1)[0] == sid
        out.append((NAMES[sid], lo, lo + b - a, name, strand))
    return out


def write_bed(path):
    with open(path, "w") as f:
        f.write("".join("%s\t%d\t%d\t%s\t0\t%s\n" % r for r in bed_rows()))


def options(bed):
    return ["-H", "-A", "-a", "1", "-Q", "-G", "-g", str(MAX_GAP), "-n", str(MIN_LOCI), "-B", CONTROL, "-D", "-Y", "5", "-L", "200",
            "-P", "30", "-I", "3:2", "-R", bed, "-C", "2", "-J", "4:30:3", "-S", "3", "-O", "2"]


TRIM = (3, 2)                      # -I
LOCUS = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("motif", "<u4"), ("reserved", "<u4")])


@functools.lru_cache(maxsize=None)
def reference():
    """`pileup -H -I 3:2` over reads() by the CPU oracle's walk (oracle/pileup_oracle.py) with the entries at the read ends deleted
    first (readpos_ref): -> dict(thresholds, loci, hap: {1, 2: loci}, bed: {file tag: {context: text}}); loci are hm_locus_t-like
    rows, a haplotype's rows carry the combined motif"""
    import readpos_ref as RP
    P = C._oracle()
    g, off = genome(), offsets()
    bins = np.zeros((3, 256), np.int64)
    calls = []                                                        # (locus, ML byte, motif, haplotype) in BAM order
    for r in reads():
        rec = C.as_dict(r)
        fwd, _ = P.fwd_rev(rec["seq"], rec["flag"])
        for q, _s, ub, _code, prob in RP.trim_entries(RP.entries(rec), len(r.seq), *TRIM):
            c = P.mod_context(fwd, q) if ub in "CG" else -1
            if c >= 0:
                bins[c, prob] += 1
        calls += [(int(off[sid]) + soff, prob, motif, r.hp or 0) for motif, _p, _L, prob, sid, soff in RP.projected(rec, g, trim=TRIM)]
    thr = [P.resolve_threshold(bins[c])[0] for c in range(3)]
    cov = {0: {}, 1: {}, 2: {}}
    motif_of = {}
    for gpos, prob, motif, hp in calls:
        motif_of[gpos] = motif                                        # the last record of a locus decides
        for part in {0, hp}:
            cov[part].setdefault(gpos, [0, 0])[0 if prob >= thr[motif] else 1] += 1

    def rows(part):
        a = np.zeros(len(cov[part]), LOCUS)
        for i, gpos in enumerate(sorted(cov[part])):
            a[i] = (gpos, *cov[part][gpos], motif_of[gpos], 0)
        return a

    loci = {part: rows(part) for part in (0, 1, 2)}
    bed = {}
    for part, tag in ((0, ""), (1, "hap1."), (2, "hap2.")):
        bed[tag] = P.bed_text([(NAMES[locate(int(x["gpos"]))[0]], locate(int(x["gpos"]))[1], int(x["pcov"]), int(x["ncov"]), int(x["motif"]))
                               for x in loci[part]])
    return dict(thresholds=thr, loci=loci[0], hap={1: loci[1], 2: loci[2]}, bed=bed)


NAN_OPTIONS =["-H", "-e", "0.01,nan,0.02", "-D", "-u", "0.1:0.8,nan,0.02:0.2"]


def slab(world, n_records):
    """worlds 3 and 5: many slabs for every rank; world 8: five slabs, the ranks 5 .. 7 are dealt nothing"""
    return (n_records + 4) // 5 if world == 8 else SMALL_SLAB


def ghost():
    """-> (genome of the BAM header, reads, name): the header names `ghost` between ctl and chrA, the FASTA (genome()) does not hold
    it; record 10 is on it, which --slab 7 on three ranks deals to rank 1"""
    rs = reads()
    head = [r for r in rs if r.tid == 0 and r.name.startswith("s")][:10]
    tail = [r for r in rs if r.tid == 1 and r.name.startswith("s")][:15]
    rng = np.random.default_rng(3303)
    seq = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 500))
    g = [genome()[0], ("ghost", seq)] + list(genome()[1:])
    mm, ml = C.all_cg_mods(seq[100:300], rng)
    lost = AlignedRead("lost", 0, 1, 100, 60, [("M", 200)], seq[100:300], mm, ml, 1)
    import dataclasses
    out = head + [lost] + [dataclasses.replace(r, tid=r.tid + 1) for r in tail]
    assert (10 // SMALL_SLAB) % 3 == 1 and out[10] is lost
    return g, out, "ghost"
