"""`diff` on the device: hm_pileup_load_loci against its numpy restatement (diff_ref.Loader), every error and state rule, the command
against `pileup -H -A -Q -G` on the same counts, the Python path, two independent samples, and a reference past 2^32 bases.

Nothing here has a tolerance of its own: planes, rows and files are compared exactly.  The p-values of the hand-written samples are
compared with the exact Fisher test of test_gpu_pileup_asm.py under that file's bounds (1e-9 relative for totals <= 48 per table, 1e-5
for a p-value printed with six digits)."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import bigref as R
from diff_ref import HM_EDATA, HM_ESTATE, Loader, parse_cov_bed
from test_gpu_pileup_asm import CLI, CTX, _asm_files, _np_diff, _phased_reads, _rel_err, _run_cli, _write_bam, fisher_exact
from test_gpu_pileup_asm_q import _mirror
from test_gpu_pileup_asm_regions import _region_files

pytestmark = pytest.mark.gpu

LENGTHS = (3001, 2500, 1777)                                  # three contigs of a few kb
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)])
TOTAL = int(OFFSETS[-1])
EDGES = [int(x) for s in range(3) for x in (OFFSETS[s], OFFSETS[s + 1] - 1)]   # the first and the last base of each contig


def _genome(seed=3):
    rng = np.random.default_rng(seed)
    return [("ctg%d" % (s + 1), "".join(rng.choice(list("ACGT"), n))) for s, n in enumerate(LENGTHS)]


def _engine(planes=False, partitions=True, genome=None):
    """-> (engine, the seven tensors pcov, ncov, key, pcov1, ncov1, pcov2, ncov2 or None for planes of the engine's own)"""
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    if not planes:
        return MethylationPileup(genome or _genome(), partitions=partitions), None
    t = [torch.zeros(TOTAL, dtype=torch.int32, device="cuda") for _ in range(7)]
    return MethylationPileup(genome or _genome(), partitions=True, planes=t[:3], partition_planes=(t[3:5], t[5:7])), t


def _load(pu, part, rows):
    """hm_pileup_load_loci on (gpos, pcov, ncov, motif) without the wrapper's exception -> its return value"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    buf = np.zeros(len(rows[0]), LOCUS_DTYPE)
    buf["gpos"], buf["pcov"], buf["ncov"], buf["motif"] = rows
    return pu._L.hm_pileup_load_loci(pu._h, part, buf.ctypes.data_as(ctypes.c_void_p), len(buf))


def _sample_rows(n, seed):
    """n rows on distinct loci in shuffled order, the contig edges first among them, about one in eight without a count, and behind
    them n // 8 more rows without a count on loci the others use"""
    rng = np.random.default_rng(seed)
    others = rng.choice(np.setdiff1d(np.arange(TOTAL), EDGES), max(n - len(EDGES), 0), replace=False)
    g = np.array([EDGES[seed % 6]] if n == 1 else EDGES + others.tolist(), np.int64)
    p, nn = rng.integers(0, 40, n), rng.integers(0, 40, n)
    zero = rng.random(n) < 0.125
    p[zero & (np.arange(n) > 0)] = 0
    nn[zero & (np.arange(n) > 0)] = 0
    p[0] += 1                                                 # the single row of n = 1 carries a count
    extra = rng.choice(g, n // 8)
    g, p, nn = np.concatenate([g, extra]), np.concatenate([p, np.zeros(len(extra), np.int64)]), np.concatenate([nn, np.zeros(len(extra), np.int64)])
    m = rng.integers(0, 4, len(g))
    order = rng.permutation(len(g))
    return g[order], p[order], nn[order], m[order]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_loader_equals_the_restatement(n):
    """two calls per part, interleaved between the parts; into planes of the engine's own and into the caller's; the largest case
    also through slabs of 1000 rows"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    samples = {part: _sample_rows(n, 10 * n + part) for part in (1, 2)}
    ref = Loader(TOTAL)
    own, _none = _engine()
    mine, t = _engine(planes=True)
    if n == 4097:
        assert mine._L.hm_pileup_set_option(mine._h, b"load_slab", 1000.0) == 0
    try:
        for half in (0, 1):
            for part in (1, 2):
                rows = samples[part]
                cut = len(rows[0]) // 2
                piece = tuple(x[:cut] if half == 0 else x[cut:] for x in rows)
                want = ref.load(part, *piece)
                assert want == int((piece[1] + piece[2] > 0).sum())
                assert own.load_loci(part, *piece) == want and _load(mine, part, piece) == want
        assert n < 6 or all(e in samples[part][0] for e in EDGES for part in (1, 2))
        # the caller's planes, element for element; the engine hands the same pointers back
        ptr = [ctypes.c_void_p() for _ in range(7)]
        n_loci = ctypes.c_int64()
        assert mine._L.hm_pileup_planes(mine._h, ctypes.byref(ptr[0]), ctypes.byref(ptr[1]), ctypes.byref(ptr[2]), ctypes.byref(n_loci)) == 0
        for part in (1, 2):
            assert mine._L.hm_pileup_partition_planes(mine._h, part, ctypes.byref(ptr[2 * part + 1]), ctypes.byref(ptr[2 * part + 2])) == 0
        assert [p.value for p in ptr] == [x.data_ptr() for x in t] and n_loci.value == TOTAL
        for name, x in zip(("pcov", "ncov", "key", "pcov1", "ncov1", "pcov2", "ncov2"), t):
            assert (x.cpu().numpy().astype(np.int64) == ref.planes[name]).all(), name
        # the engine's own planes, through the fetch that lists every covered locus of a plane pair with its key
        for pu in (own, mine):
            for part in (0, 1, 2):
                got = pu.loci(partition=part)
                g, p, nn, m = ref.loci(part)
                want = np.zeros(len(g), LOCUS_DTYPE)
                want["gpos"], want["pcov"], want["ncov"], want["motif"] = g, p, nn, m
                assert got.tobytes() == want.tobytes(), part
        tested = ref.tested(1)
        rows = own.asm(min_cov=1)
        assert [(int(r["gpos"]), int(r["pcov1"]), int(r["ncov1"]), int(r["pcov2"]), int(r["ncov2"]), min(int(r["motif"]), 2)) for r in rows] == tested
        assert n < 63 or len(tested) >= 1
    finally:
        own.close()
        mine.close()


BAD = {"gpos -1": (([7, -1], [1, 1], [1, 1], [0, 0]), b"1 gpos outside"), "gpos = total": (([TOTAL, 3], [1, 1], [1, 1], [0, 0]), b"1 gpos outside"),
       "negative count": (([5, 6, 7], [1, 2, -1], [-3, 0, 1], [0, 0, 0]), b"2 negative count"), "motif 4": (([5], [1], [1], [4]), b"1 motif above 3"),
       "duplicate in a call": (([9, 5, 9, 9], [1, 1, 0, 1], [0, 1, 2, 0], [0, 0, 0, 0]), b"2 locus given twice"),
       "duplicate across calls": (([4], [0], [1], [1]), b"1 locus given twice")}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_rows_void_the_engine(what):
    from hifimeth_amd.caller import HifimethError
    rows, text = BAD[what]
    pu, _none = _engine()
    try:
        assert _load(pu, 1, ([4, 2000], [3, 1], [0, 1], [0, 2])) == 2 and _load(pu, 2, ([4], [1], [5], [0])) == 1
        ref = Loader(TOTAL)
        ref.load(1, [4, 2000], [3, 1], [0, 1], [0, 2])
        assert ref.load(1, *rows) == HM_EDATA
        assert _load(pu, 1, rows) == HM_EDATA
        err = pu._L.hm_pileup_last_error(pu._h)
        assert text in err and (b"%d bad rows" % sum(ref.bad.values())) in err, err
        good = ([100], [1], [1], [0])
        assert _load(pu, 1, good) == HM_ESTATE and _load(pu, 2, good) == HM_ESTATE
        f = pu._L
        assert f.hm_pileup_fetch_loci(pu._h, None, None, None, 0, 0, TOTAL, None, 0) == HM_ESTATE
        assert f.hm_pileup_fetch_asm(pu._h, None, None, None, None, None, 0, 0, TOTAL, 1, None, 0) == HM_ESTATE
        assert f.hm_pileup_fetch_asm_regions(pu._h, None, None, None, None, None, 0, 0, TOTAL, 1, 0, 0.01, 500, 3, 0, None, None, 0) == HM_ESTATE
        with pytest.raises(HifimethError):
            pu.load_loci(1, *good)
    finally:
        pu.close()


def _submit(pu, read):
    from hifimeth_amd.pileup import parse_mods
    mods = parse_mods(read.seq, read.flag, read.mm, read.ml)
    seq4 = np.ascontiguousarray(read.seq4, np.uint8)
    cig = np.ascontiguousarray(read.cigar_u32(), np.uint32)
    return pu._L.hm_pileup_submit_read(pu._h, 0, read.flag, read.tid, read.pos, read.mapq, len(read.seq), seq4.ctypes.data_as(ctypes.c_void_p),
                                       len(cig), cig.ctypes.data_as(ctypes.c_void_p), len(mods), mods.ctypes.data_as(ctypes.c_void_p))


def test_state_errors():
    from hifimeth_amd.synth import synth_alignments
    genome = _genome()
    read = next(r for r in synth_alignments(genome, 20, seed=4, median_len=600) if not r.flag & 4 and r.mm)
    good = ([100], [1], [1], [0])
    plain, _none = _engine(partitions=False, genome=genome)
    assert _load(plain, 1, good) == HM_ESTATE and b"partitions" in plain._L.hm_pileup_last_error(plain._h)
    plain.close()
    ran, _none = _engine(genome=genome)
    assert ran.add(read) == 1
    ran.flush()
    assert _load(ran, 1, good) == HM_ESTATE and b"records" in ran._L.hm_pileup_last_error(ran._h)
    ran.count([128, 128, 128])
    assert _load(ran, 2, good) == HM_ESTATE and len(ran.loci()) > 0           # the record path goes on as before
    ran.close()
    pu, _none = _engine(genome=genome)
    assert _load(pu, 3, good) == -1 and _load(pu, 0, good) == -1 and pu._L.hm_pileup_load_loci(pu._h, 1, None, 1) == -1   # HM_EINVAL
    assert pu._L.hm_pileup_load_loci(pu._h, 1, None, 0) == 0 and _submit(pu, read) == 1    # nothing loaded yet: records may still come
    pu.close()
    pu, _none = _engine(genome=genome)
    assert _load(pu, 1, good) == 1
    assert _submit(pu, read) == HM_ESTATE and b"loaded" in pu._L.hm_pileup_last_error(pu._h)
    pu.flush()
    pu.count([128, 128, 128])                                                 # nothing staged: neither changes the planes
    assert [tuple(int(x) for x in r) for r in pu.loci()[["gpos", "pcov", "ncov", "motif"]]] == [(100, 1, 1, 0)]
    pu.close()


# ---- the command against `pileup -H -A -Q -G` on the same counts ------------------------------------------------------------------------
ARGS = ["-Q", "-G", "-a", "2", "-n", "1"]


def _diff_cli(args, ok=True):
    r = subprocess.run([CLI, "diff", *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok and (ok or r.returncode == 1), r.stderr
    return r


def _diff_files(prefix):
    return ({c: open(f"{prefix}.diff.{c}.bed").read() for c in CTX}, {c: open(f"{prefix}.diff.regions.{c}.bed").read() for c in CTX},
            open(f"{prefix}.diff.summary.tsv").read())


@pytest.fixture(scope="module")
def round_trip(tmp_path_factory):
    from bamutil import write_fasta
    d = tmp_path_factory.mktemp("diff")
    genome, reads = _phased_reads()
    bam, fa, P, D, S = (str(d / x) for x in ("mod.bam", "ref.fa", "P", "D", "S"))
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    _run_cli(["-H", "-A", *ARGS, fa, bam, P])
    r = _diff_cli([*ARGS, fa, P + ".hap1", P + ".hap2", D])
    _diff_cli([*ARGS, "-t", "3", fa, P + ".hap2", P + ".hap1", S])
    return genome, fa, P, D, S, r.stderr


def test_diff_of_the_haplotype_files_is_the_haplotype_test(round_trip):
    _genome_, _fa, P, D, _S, stderr = round_trip
    rows, regions, summary = _diff_files(D)
    for c in CTX:                                             # the comparison cannot pass on empty files
        assert len(rows[c].splitlines()) >= 1 and len(regions[c].splitlines()) >= 1, c
        assert all(len(x.split("\t")) == 10 for x in rows[c].splitlines()) and all(len(x.split("\t")) == 11 for x in regions[c].splitlines())
    print({c: (len(rows[c].splitlines()), len(regions[c].splitlines())) for c in CTX})
    assert rows == _asm_files(P) and regions == _region_files(P) and summary == open(P + ".asm.summary.tsv").read()
    assert f"{D}.diff.*" in stderr and "Skip" not in stderr


def _negated(text):
    return text if text == "0" else text[1:] if text.startswith("-") else "-" + text


def test_swapped_samples_mirror_the_rows(round_trip):
    """diff ref P.hap2 P.hap1: every row and region mirrored -- the difference negated, the counts exchanged, the region signs flipped
    -- and p, q and the summary equal in every digit the files hold (the Fisher kernel sums the mirrored table in the other order,
    so beyond the printed digits its p is pinned to 2e-9 by test_gpu_pileup_asm.py, not to the bit)"""
    _genome_, _fa, _P, D, S, _e = round_trip
    (rows, regions, summary), (srows, sregions, ssummary) = _diff_files(D), _diff_files(S)
    assert summary == ssummary
    for c in CTX:
        for a, b in zip(rows[c].splitlines(), srows[c].splitlines()):
            a, b = a.split("\t"), b.split("\t")
            assert b[:3] == a[:3] and b[3] == _negated(a[3]) and b[4] == a[4] and b[9] == a[9]     # p and q: every digit the file holds
            assert b[5:9] == a[7:9] + a[5:7]
        assert len(rows[c].splitlines()) == len(srows[c].splitlines())
        for a, b in zip(regions[c].splitlines(), sregions[c].splitlines()):
            a, b = a.split("\t"), b.split("\t")
            assert b[:4] == a[:4] and {a[4], b[4]} == {"+", "-"} and b[5] == _negated(a[5]) and b[6] == a[6] and b[7:] == a[9:] + a[7:9]
        assert len(regions[c].splitlines()) == len(sregions[c].splitlines())
    assert any(x.split("\t")[4] == "+" for c in CTX for x in regions[c].splitlines())
    assert any(x.split("\t")[4] == "-" for c in CTX for x in regions[c].splitlines())


def test_python_path_gives_the_commands_rows(round_trip):
    from hifimeth_amd.pileup import MethylationPileup, asm_summary_tsv, read_cov_bed
    genome, _fa, P, D, _S, _e = round_trip
    pu = MethylationPileup(genome, partitions=True)
    try:
        names = [n for n, _ in genome]
        for part in (1, 2):
            for c in CTX:
                rows = read_cov_bed(f"{P}.hap{part}.{c}.cov.bed", names, pu.offsets)
                assert pu.load_loci(part, *rows) == len(rows[0]) > 0
        table, rq = _mirror(pu, 2)
        rows, regions, summary = _diff_files(D)
        assert pu.asm_bed(rq) == rows and asm_summary_tsv(table) == summary
        got = {c: "" for c in CTX}
        for s in range(len(genome)):                          # a region never crosses a sequence: fetched per sequence, as the command does
            for c in range(3):
                got[CTX[c]] += pu.asm_regions_bed(pu.asm_regions(c, int(pu.offsets[s]), int(pu.offsets[s + 1]), 2, 0.01, 500, 1)[0])[CTX[c]]
        assert got == regions
        # the pooled planes are the two samples added up: what `pileup` counted for the reads of HP 1 and HP 2
        pooled = pu.loci()
        parts = [pu.loci(partition=k) for k in (1, 2)]
        assert pooled["pcov"].sum() == sum(int(x["pcov"].sum()) for x in parts) and len(pooled) >= max(len(x) for x in parts)
    finally:
        pu.close()


# ---- two independent samples written by hand ----------------------------------------------------------------------------------------
def _bed(rows):
    return "".join("%s\t%d\t%d\t%g\t%d\t%d\n" % (n, k, k + 1, 100.0 * p / max(p + q, 1), p, q) for n, k, p, q in rows)


SAMPLE_A = {"CpG": [("ctg1", 0, 9, 1), ("ctg1", 40, 6, 0), ("ctg1", 41, 2, 9), ("ctg2", 10, 7, 3), ("ctg2", 700, 3, 3), ("ctg3", 1776, 12, 0)],
            "CHG": [("ctg1", 100, 1, 8), ("ctg2", 2499, 0, 5)], "CHH": [("ctg3", 5, 0, 20), ("ctg1", 3000, 4, 4)]}
SAMPLE_B = {"CpG": [("ctg1", 0, 1, 9), ("ctg1", 41, 8, 1), ("ctg2", 700, 3, 3), ("ctg3", 1776, 2, 11)],
            "CHG": [("ctg1", 100, 8, 1), ("ctg2", 10, 2, 8), ("ctg2", 2499, 5, 0)], "CHH": [("ctg3", 5, 2, 18), ("ctg1", 3000, 0, 1), ("ctg1", 2999, 6, 6)]}
# ctg1:40 and ctg1:2999 are covered by one sample only; ctg2:10 is a CpG locus in sample A and a CHG locus in sample B; ctg1:3000
# has one call in sample B, below -a 2


def test_independent_samples(tmp_path):
    from bamutil import write_fasta
    genome = _genome()
    names = [n for n, _ in genome]
    fa, A, B, out = (str(tmp_path / x) for x in ("ref.fa", "A", "B", "out"))
    write_fasta(fa, genome)
    ref = Loader(TOTAL)
    for part, (prefix, sample) in enumerate(((A, SAMPLE_A), (B, SAMPLE_B)), 1):
        for m, c in enumerate(CTX):
            path = f"{prefix}.{c}.cov.bed"
            if part == 2 and c == "CHG":                      # one of the six files is gzip under the plain name
                with open(path, "wb") as f:
                    f.write(gzip.compress(_bed(sample[c]).encode()))
            else:
                with open(path, "w") as f:
                    f.write(_bed(sample[c]))
            assert ref.load(part, *parse_cov_bed(path, names, LENGTHS, m)) == len(sample[c])
    _diff_cli(["-a", "2", fa, A, B, out])
    assert not os.path.exists(out + ".diff.summary.tsv") and not os.path.exists(out + ".diff.regions.CpG.bed")
    want = {c: [] for c in CTX}
    for g, p1, n1, p2, n2, ctx in ref.tested(2):
        s = int(np.searchsorted(OFFSETS, g, side="right")) - 1
        want[CTX[ctx]].append((names[s], g - int(OFFSETS[s]), p1, n1, p2, n2))
    assert {c: [r[:2] for r in want[c]] for c in CTX} == {"CpG": [("ctg1", 0), ("ctg1", 41), ("ctg2", 700), ("ctg3", 1776)],
                                                          "CHG": [("ctg1", 100), ("ctg2", 10), ("ctg2", 2499)], "CHH": [("ctg3", 5)]}
    for c in CTX:
        lines = open(f"{out}.diff.{c}.bed").read().splitlines()
        assert len(lines) == len(want[c])
        for line, (name, k, p1, n1, p2, n2) in zip(lines, want[c]):
            f = line.split("\t")
            assert len(f) == 9 and (f[0], int(f[1]), int(f[2]), [int(x) for x in f[5:]]) == (name, k, k + 1, [p1, n1, p2, n2])
            assert f[3] == "%g" % float(_np_diff(p1, n1, p2, n2))
            assert _rel_err(float(f[4]), fisher_exact(p1, n1, p2, n2)) <= 1e-5      # six printed digits
    # a context with one file missing is skipped and said so; without any pair the command fails
    os.remove(B + ".CHH.cov.bed")
    r = _diff_cli(["-a", "2", fa, A, B, out + "2"])
    assert "Skip context CHH" in r.stderr and B + ".CHH.cov.bed" in r.stderr
    assert open(out + "2.diff.CHH.bed").read() == "" and open(out + "2.diff.CpG.bed").read() == open(out + ".diff.CpG.bed").read()
    assert "no context" in _diff_cli([fa, A, str(tmp_path / "nothing"), out + "3"], ok=False).stderr
    # bad input: the file and the line; a locus twice in one sample
    with open(B + ".CpG.cov.bed", "a") as f:
        f.write("\nctg2\t2500\t2501\t50\t1\t1\n")
    r = _diff_cli([fa, A, B, out + "4"], ok=False)
    assert f"{B}.CpG.cov.bed:6: " in r.stderr and "ctg2" in r.stderr
    with open(B + ".CpG.cov.bed", "w") as f:
        f.write(_bed(SAMPLE_B["CpG"] + [("ctg1", 41, 1, 1)]))
    r = _diff_cli([fa, A, B, out + "5"], ok=False)
    assert f"{B}.CpG.cov.bed: " in r.stderr and "1 locus given twice" in r.stderr


# ---- a reference past 2^32 bases -----------------------------------------------------------------------------------------------------
def test_loci_around_two_to_the_32():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    total = R.HOST_LEN[R.B32]
    lengths = [R.B31, R.B31, total - R.B32]                   # 2^31 - 1 and 2^32 - 1 are the last bases of the first two contigs
    need = total * (1 + 4 * 7) + (1 << 30)
    free, _all = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip("the card has %.1f GB free, the case needs %.1f GB plus 8 GB" % (free / 1e9, need / 1e9))
    loci = [R.B31 - 1, R.B32 - 1, R.B32 + 5]
    counts = {1: ([9, 1, 30], [1, 9, 2]), 2: ([2, 8, 3], [8, 2, 40])}
    pu = MethylationPileup([("c%d" % k, n) for k, n in enumerate(lengths)], partitions=True, bases=np.full(total, ord("N"), np.uint8))
    try:
        assert pu.n_loci == total > R.B32
        assert pu.load_loci(2, loci[::-1], counts[2][0][::-1], counts[2][1][::-1], [2, 1, 0]) == 3
        assert pu.load_loci(1, loci, *counts[1], [0, 0, 2]) == 3
        rows = pu.asm(min_cov=5)
        assert rows["gpos"].tolist() == loci and rows["motif"].tolist() == [0, 1, 2]
        for k, r in enumerate(rows):
            t = (counts[1][0][k], counts[1][1][k], counts[2][0][k], counts[2][1][k])
            assert tuple(int(r[f]) for f in ("pcov1", "ncov1", "pcov2", "ncov2")) == t
            assert r["diff"] == _np_diff(*t) and _rel_err(r["pvalue"], fisher_exact(*t)) <= 1e-9     # totals <= 75: the bound of the small tables
        for lo, hi, want in ((0, R.B31, [loci[0]]), (R.B31, R.B32, [loci[1]]), (R.B32, total, [loci[2]]), (R.B31 - 1, R.B32 + 6, loci)):
            assert pu.asm(lo, hi, 5)["gpos"].tolist() == want
        assert pu.loci()["gpos"].tolist() == loci and pu.loci()["pcov"].tolist() == [11, 9, 33]
        assert _load(pu, 1, ([total], [1], [1], [0])) == HM_EDATA             # the bound is the 64-bit length
    finally:
        pu.close()
        torch.cuda.empty_cache()
