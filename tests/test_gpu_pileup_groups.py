"""`groupdiff` on the device: hm_pileup_group_sample / hm_pileup_load_sample_loci against their numpy restatement
(groups_ref.GroupLoader), exactly; every error and state rule; hm_pileup_fetch_groups' selection exactly and its D, phi and p against
mpmath at 50 digits; hm_group_qvalues against the restatement's BH; the command against the Python path; a reference past 2^32.

The bar of D, phi and p is 8 x E_ref, relative, where E_ref is the worst relative error of the float64 form of the statistic against
mpmath over the same loci (groups_ref.e_ref(), measured in test_pileup_groups_cpu.py: 8.2e-11 for D, 2.5e-14 for phi, 5.4e-11 for
p) and 8 the margin DESIGN.md section 4 uses for a GPU-against-reference error ratio.  Everything else is compared exactly."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import bigref as R
import groups_ref as G
from groups_ref import HM_EDATA, HM_EINVAL, HM_ESTATE, LENGTHS, OFFSETS, TOTAL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
CTX = ("CpG", "CHG", "CHH")
FIELDS = ("gpos", "motif", "m1", "pcov1", "ncov1", "m2", "pcov2", "ncov2")


def _genome(seed=3):
    rng = np.random.default_rng(seed)
    return [("ctg%d" % (s + 1), "".join(rng.choice(list("ACGT"), n))) for s, n in enumerate(LENGTHS)]


def _engine(planes=False, groups=True, min_cov=G.MIN_COV, genome=None, partitions=True):
    """-> (engine, the seven tensors pcov, ncov, key, pcov1, ncov1, pcov2, ncov2 or None for planes of the engine's own)"""
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    kw = dict(partitions=partitions, groups=groups, group_min_cov=min_cov) if groups else dict(partitions=partitions)
    if not planes:
        return MethylationPileup(genome or _genome(), **kw), None
    t = [torch.zeros(TOTAL, dtype=torch.int32, device="cuda") for _ in range(7)]
    return MethylationPileup(genome or _genome(), planes=t[:3], partition_planes=(t[3:5], t[5:7]), **kw), t


def _begin(pu, part):
    return pu._L.hm_pileup_group_sample(pu._h, part)


def _load(pu, rows):
    """hm_pileup_load_sample_loci on (gpos, pcov, ncov, motif) without the wrapper's exception -> its return value"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    buf = np.zeros(len(rows[0]), LOCUS_DTYPE)
    buf["gpos"], buf["pcov"], buf["ncov"], buf["motif"] = rows
    return pu._L.hm_pileup_load_sample_loci(pu._h, buf.ctypes.data_as(ctypes.c_void_p), len(buf))


def _fetch(pu, lo, hi, min_reps, out=None, cap=0):
    return pu._L.hm_pileup_fetch_groups(pu._h, lo, hi, min_reps, None if out is None else out.ctypes.data_as(ctypes.c_void_p), cap)


def _tuples(rows):
    return [tuple(int(r[f]) for f in FIELDS) for r in rows]


def _sample_rows(n, seed):
    """n rows on distinct loci in shuffled order, the contig ends first among them, coverage 0 .. 39 (one in eight without a count),
    and behind them n // 8 more rows without a count on loci the others use"""
    rng = np.random.default_rng(seed)
    others = rng.choice(np.setdiff1d(np.arange(TOTAL), G.ENDS), max(n - len(G.ENDS), 0), replace=False)
    g = np.array([G.ENDS[seed % 6]] if n == 1 else G.ENDS + others.tolist(), np.int64)
    cov = rng.integers(0, 40, n)
    cov[(rng.random(n) < 0.125) & (np.arange(n) > 0)] = 0
    cov[0] = max(cov[0], G.MIN_COV)                           # the single row of n = 1 counts
    p = rng.binomial(cov, rng.random(n))
    extra = rng.choice(g, n // 8)
    zeros = np.zeros(len(extra), np.int64)
    g, p, nn = np.concatenate([g, extra]), np.concatenate([p, zeros]), np.concatenate([cov - p, zeros])
    m = rng.integers(0, 4, len(g))
    order = rng.permutation(len(g))
    return g[order], p[order], nn[order], m[order]


@pytest.mark.parametrize("n,reps", [(1, (1, 1)), (63, (2, 2)), (64, (3, 3)), (65, (2, 3)), (4097, (3, 1))])
def test_loader_equals_the_restatement(n, reps):
    """each sample in two calls, the samples of the two groups taking turns; into planes of the engine's own and into the caller's; the
    largest case also through slabs of 1000 rows"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    ref = G.GroupLoader(TOTAL, G.MIN_COV)
    own, _none = _engine()
    mine, t = _engine(planes=True)
    if n == 4097:
        assert mine._L.hm_pileup_set_option(mine._h, b"load_slab", 1000.0) == 0
    try:
        for s in range(max(reps)):
            for part in (1, 2):
                if s >= reps[part - 1]:
                    continue
                rows = _sample_rows(n, 100 * n + 10 * s + part)
                assert ref.begin_sample(part) == s and own.begin_sample(part) == s and _begin(mine, part) == s
                cut = len(rows[0]) // 2
                for piece in (tuple(x[:cut] for x in rows), tuple(x[cut:] for x in rows)):
                    want = ref.load(*piece)
                    assert want == int((piece[1] + piece[2] >= G.MIN_COV).sum())
                    assert own.load_sample_loci(*piece) == want and _load(mine, piece) == want
        for name, x in zip(("pcov", "ncov", "key", "pcov1", "ncov1", "pcov2", "ncov2"), t):    # the caller's planes, element for element
            assert (x.cpu().numpy().astype(np.int64) == ref.planes[name]).all(), name
        for pu in (own, mine):
            for part in (1, 2):
                moment, samples = pu.group_planes(part)
                assert (moment == ref.moment[part]).all() and (samples == ref.samples[part]).all(), part
                lo, hi = int(OFFSETS[1]) - 3, int(OFFSETS[2]) + 5
                moment, samples = pu.group_planes(part, lo, hi)
                assert (moment == ref.moment[part][lo:hi]).all() and (samples == ref.samples[part][lo:hi]).all(), part
            for part in (0, 1, 2):                            # the engine's own planes, through the fetch that lists every covered locus
                got = pu.loci(partition=part)
                g, p, nn, m = ref.loci(part)
                want = np.zeros(len(g), LOCUS_DTYPE)
                want["gpos"], want["pcov"], want["ncov"], want["motif"] = g, p, nn, m
                assert got.tobytes() == want.tobytes(), part
            for r in (1, 2, 3):
                assert _tuples(pu.group_tests(min_reps=r)) == ref.tested(r), r
        assert n < 63 or len(ref.tested(1)) >= 1
        # the pooled Fisher test sees the group sums
        P = ref.planes
        both = np.flatnonzero((P["pcov1"] + P["ncov1"] >= 1) & (P["pcov2"] + P["ncov2"] >= 1))
        assert [(int(r["gpos"]), int(r["pcov1"]), int(r["ncov1"]), int(r["pcov2"]), int(r["ncov2"])) for r in own.asm(min_cov=1)] == \
            [(int(g), int(P["pcov1"][g]), int(P["ncov1"][g]), int(P["pcov2"][g]), int(P["ncov2"][g])) for g in both]
    finally:
        own.close()
        mine.close()


def test_a_locus_once_in_each_of_three_samples_is_no_duplicate():
    pu, _none = _engine()
    try:
        for part, k in ((1, 4), (1, 6), (1, 8), (2, 1), (2, 2)):
            assert _begin(pu, part) >= 0 and _load(pu, ([7, 9], [k, 0], [9 - k, 3], [0, 1])) == 1      # 9 is below the coverage
        assert _tuples(pu.group_tests(min_reps=2)) == [(7, 0, 3, 18, 9, 2, 3, 15)]
    finally:
        pu.close()


BAD = {"gpos -1": (([7, -1], [5, 5], [5, 5], [0, 0]), b"1 gpos outside"), "gpos = total": (([TOTAL, 3], [5, 5], [5, 5], [0, 0]), b"1 gpos outside"),
       "negative count": (([5, 6, 7], [9, 9, -1], [-3, 0, 9], [0, 0, 0]), b"2 negative count"),
       "a count of 2^20": (([5, 6], [1 << 20, (1 << 20) - 1], [0, 0], [0, 0]), b"1 count above 2^20 - 1"),
       "the sum reaches 2^20": (([5], [1 << 19], [1 << 19], [0]), b"1 count above 2^20 - 1"),
       "negative before large": (([5], [-1], [1 << 21], [7]), b"1 negative count"), "large before motif": (([5], [1 << 20], [0], [7]), b"1 count above"),
       "motif 4": (([5], [5], [5], [4]), b"1 motif above 3"),
       "twice in a call": (([9, 5, 9, 9], [5, 5, 0, 5], [0, 5, 0, 0], [0, 0, 0, 0]), b"1 locus given twice in one sample"),
       "twice across calls": (([4], [0], [9], [1]), b"1 locus given twice in one sample"),
       "twice, the first below the coverage": (([2000], [7], [7], [1]), b"1 locus given twice in one sample")}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_rows_void_the_engine(what):
    from hifimeth_amd.caller import HifimethError
    rows, text = BAD[what]
    first = ([4, 2000], [5, 1], [0, 1], [0, 2])
    pu, _none = _engine()
    ref = G.GroupLoader(TOTAL, G.MIN_COV)
    try:
        assert _begin(pu, 1) == 0 and ref.begin_sample(1) == 0
        assert _load(pu, first) == 1 and ref.load(*first) == 1
        assert ref.load(*rows) == HM_EDATA and _load(pu, rows) == HM_EDATA
        err = pu._L.hm_pileup_last_error(pu._h)
        assert text in err and (b"%d bad rows" % sum(ref.bad.values())) in err, err
        good = ([100], [5], [5], [0])
        assert _load(pu, good) == HM_ESTATE and _begin(pu, 2) == HM_ESTATE and _fetch(pu, 0, TOTAL, 1) == HM_ESTATE
        assert pu._L.hm_pileup_fetch_loci(pu._h, None, None, None, 0, 0, TOTAL, None, 0) == HM_ESTATE
        assert pu._L.hm_pileup_fetch_asm(pu._h, None, None, None, None, None, 0, 0, TOTAL, 1, None, 0) == HM_ESTATE
        with pytest.raises(HifimethError):
            pu.load_sample_loci(*good)
    finally:
        pu.close()


def test_state_errors():
    from hifimeth_amd.pileup import LOCUS_DTYPE
    from hifimeth_amd.synth import synth_alignments
    from test_gpu_pileup_diff import _submit
    genome = _genome()
    read = next(r for r in synth_alignments(genome, 20, seed=4, median_len=600) if not r.flag & 4 and r.mm)
    good = ([100], [5], [5], [0])
    buf = np.zeros(1, LOCUS_DTYPE)
    buf["gpos"], buf["pcov"], buf["ncov"] = 100, 5, 5
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    plain, _none = _engine(groups=False, genome=genome)       # without the option
    assert _begin(plain, 1) == HM_ESTATE and b"groups" in plain._L.hm_pileup_last_error(plain._h)
    assert _load(plain, good) == HM_ESTATE and _fetch(plain, 0, TOTAL, 2) == HM_ESTATE
    assert plain._L.hm_pileup_set_option(plain._h, b"groups", 1.0) == HM_ESTATE       # after hm_pileup_set_reference
    plain.close()
    from hifimeth_amd.caller import HifimethError
    with pytest.raises(HifimethError):                        # the option needs partitions
        _engine(partitions=False, genome=genome)
    ran, _none = _engine(genome=genome)                       # after records
    assert ran.add(read) == 1
    assert _begin(ran, 1) == HM_ESTATE and b"records" in ran._L.hm_pileup_last_error(ran._h)
    ran.close()
    pu, _none = _engine(genome=genome)                        # after hm_pileup_load_loci
    assert pu._L.hm_pileup_load_loci(pu._h, 1, ptr, 1) == 1
    assert _begin(pu, 1) == HM_ESTATE and b"hm_pileup_load_loci" in pu._L.hm_pileup_last_error(pu._h)
    pu.close()
    pu, _none = _engine(genome=genome)
    assert _load(pu, good) == HM_ESTATE and b"before hm_pileup_group_sample" in pu._L.hm_pileup_last_error(pu._h)
    assert _begin(pu, 0) == HM_EINVAL and _begin(pu, 3) == HM_EINVAL and pu._L.hm_pileup_load_sample_loci(pu._h, None, 1) == HM_EINVAL
    assert pu._L.hm_pileup_set_option(pu._h, b"group_min_cov", 0.0) == HM_EINVAL and pu._L.hm_pileup_set_option(pu._h, b"group_min_cov", 3.0) == 0
    assert _begin(pu, 2) == 0 and pu._L.hm_pileup_load_sample_loci(pu._h, None, 0) == 0
    assert pu._L.hm_pileup_set_option(pu._h, b"group_min_cov", 4.0) == HM_ESTATE      # a sample has been opened
    assert _load(pu, ([100, 101], [2, 1], [1, 1], [0, 0])) == 1                       # the minimum coverage is 3
    assert pu._L.hm_pileup_load_loci(pu._h, 1, ptr, 1) == HM_ESTATE and b"group" in pu._L.hm_pileup_last_error(pu._h)      # and the reverse
    assert _submit(pu, read) == HM_ESTATE and b"loaded" in pu._L.hm_pileup_last_error(pu._h)
    assert _fetch(pu, 0, TOTAL, 0) == HM_EINVAL and _fetch(pu, 0, TOTAL, 256) == HM_EINVAL and _fetch(pu, 5, 4, 1) == HM_EINVAL
    assert _fetch(pu, 0, TOTAL + 1, 1) == HM_EINVAL and _fetch(pu, -1, 4, 1) == HM_EINVAL and _fetch(pu, 9, 9, 1) == 0
    assert _fetch(pu, 0, TOTAL, 1) == 0                       # one sample in all: no degree of freedom
    pu.close()


def test_the_256th_sample_of_a_group():
    pu, _none = _engine(min_cov=1)
    try:
        assert [_begin(pu, 2) for _ in range(255)] == list(range(255))
        assert _begin(pu, 2) == HM_ESTATE and b"255" in pu._L.hm_pileup_last_error(pu._h)
        assert _begin(pu, 1) == 0 and _load(pu, ([3], [1], [0], [0])) == 1            # the other group goes on
    finally:
        pu.close()


# ---- the fetch: the random data set and the hand-made loci ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loaded():
    pu, _none = _engine()
    for (g, s), rows in sorted(G.dataset().items()):
        assert pu.begin_sample(g) == s
        pu.load_sample_loci(*rows)
    yield pu, G.dataset_loader()
    pu.close()


@pytest.mark.parametrize("min_reps", [1, 2, 3])
def test_selection_equals_the_restatement(loaded, min_reps):
    from hifimeth_amd.pileup import GROUP_DTYPE
    pu, ref = loaded
    rows = pu.group_tests(min_reps=min_reps)
    want = ref.tested(min_reps)
    assert _tuples(rows) == want and len(want) >= 50
    cuts = [0, 1, int(OFFSETS[1]) - 1, int(OFFSETS[1]), int(OFFSETS[1]) + 1, int(OFFSETS[2]), TOTAL - 1, TOTAL]
    for lo in cuts:
        for hi in cuts:
            if lo <= hi:
                part = pu.group_tests(lo, hi, min_reps)
                assert part.tobytes() == rows[(rows["gpos"] >= lo) & (rows["gpos"] < hi)].tobytes(), (lo, hi)
    out = np.full(len(rows), 0x55, np.uint8).view(np.uint8).repeat(GROUP_DTYPE.itemsize).view(GROUP_DTYPE)
    before = out.tobytes()
    assert _fetch(pu, 0, TOTAL, min_reps, out, len(rows) - 1) == len(rows) and out.tobytes() == before     # a cap one below: nothing written
    assert _fetch(pu, 0, TOTAL, min_reps, out, len(rows)) == len(rows) and out.tobytes() == rows.tobytes()


def _check_statistic(rows, refs_of, e_ref):
    """diff bit-equal, D, phi and p within 8 x E_ref of mpmath, p = 1 and the floor exact -> the worst E_gpu per quantity"""
    worst = {"D": 0.0, "phi": 0.0, "p": 0.0}
    for r in rows:
        sums, (mD, mphi, mp_) = refs_of(r)
        assert r["diff"] == G.np_diff(sums[0], sums[1], sums[4], sums[5]), r
        err = {"D": G.rel(r["D"], mD), "phi": G.rel(r["phi"], mphi)}
        if mD == 0:
            assert r["D"] == 0.0 and r["pvalue"] == 1.0, r
        elif mp_ < G.DBL_MIN:
            assert r["pvalue"] == G.DBL_MIN, r
        else:
            err["p"] = G.rel(r["pvalue"], mp_)
        for k, v in err.items():
            assert v <= 8 * e_ref[k], (k, v, e_ref[k], r)
            worst[k] = max(worst[k], v)
    return worst


def test_statistic_against_mpmath(loaded):
    pu, ref = loaded
    e_ref, refs = G.e_ref(), G.references()
    rows = pu.group_tests(min_reps=1)
    worst = _check_statistic(rows, lambda r: (ref.sums(int(r["gpos"])), refs["locus %d" % r["gpos"]][1]), e_ref)
    print("data set, %d loci: " % len(rows) + ", ".join("E_gpu(%s) = %.3g = %.3g E_ref" % (k, v, v / e_ref[k]) for k, v in worst.items()))
    assert (rows["pvalue"] == 1.0).sum() >= 1 and (rows["phi"] > 1.0).sum() >= 50 and (rows["phi"] == 1.0).sum() >= 50
    for r in (2, 3):                                          # a row does not depend on the selection it came with
        part = pu.group_tests(min_reps=r)
        assert part.tobytes() == rows[np.isin(rows["gpos"], part["gpos"])].tobytes()


def test_hand_made_loci_against_mpmath():
    """the loci of groups_ref.EDGE, one locus each, sample j of a group giving the j-th pair of every locus that has one"""
    names = list(G.EDGE)
    pu, _none = _engine(min_cov=1)
    try:
        for part in (1, 2):
            for j in range(max(len(G.EDGE[n][part - 1]) for n in names)):
                rows = [(k, *G.EDGE[n][part - 1][j]) for k, n in enumerate(names) if j < len(G.EDGE[n][part - 1])]
                assert _begin(pu, part) == j
                assert _load(pu, ([k for k, _p, _n in rows], [p for _k, p, _n in rows], [n - p for _k, p, n in rows], [0] * len(rows))) == len(rows)
        rows = pu.group_tests(min_reps=1)
        assert rows["gpos"].tolist() == list(range(len(names)))
        assert pu.group_tests(min_reps=2)["gpos"].tolist() == [k for k, n in enumerate(names) if G.EDGE[n][2] >= 2]
        cases, refs, e_ref = G.cases(), G.references(), G.e_ref()
        for r in rows:
            s = cases[names[r["gpos"]]]
            assert (int(r["pcov1"]), int(r["pcov1"]) + int(r["ncov1"]), int(r["m1"])) == (s[0], s[1], s[3]) and int(r["m2"]) == s[7]
            assert pu.group_planes(1, int(r["gpos"]), int(r["gpos"]) + 1)[0][0] == s[2]
        worst = _check_statistic(rows, lambda r: (cases[names[r["gpos"]]], refs[names[r["gpos"]]][1]), e_ref)
        print("hand-made, %d loci: " % len(rows) + ", ".join("E_gpu(%s) = %.3g = %.3g E_ref" % (k, v, v / e_ref[k]) for k, v in worst.items()))
        by = {n: rows[k] for k, n in enumerate(names)}
        assert by["p below DBL_MIN"]["pvalue"] == G.DBL_MIN and G.DBL_MIN < by["p near DBL_MIN"]["pvalue"] < 1e-306
        assert all(by[n]["pvalue"] == 1.0 and by[n]["D"] == 0.0 for n in ("D = 0", "D = 0 with spread", "both groups at 0"))
        assert by["D = 0 with spread"]["phi"] > 1.0 and by["D = 0"]["phi"] == 1.0
    finally:
        pu.close()


def test_qvalues_equal_the_restatements_bh(loaded):
    from hifimeth_amd.pileup import group_qvalues
    pu, _ref = loaded
    for r in (1, 2):
        rows = pu.group_tests(min_reps=r)
        q, m = group_qvalues(rows)
        want, wm = G.bh(rows["pvalue"], rows["motif"])
        assert q.tobytes() == want.tobytes() and m.tolist() == wm and min(wm) >= 10


# ---- the command ------------------------------------------------------------------------------------------------------------------
def _cli(args, ok=True):
    r = subprocess.run([CLI, "groupdiff", *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok and (ok or r.returncode == 1), r.stderr
    return r


def _files(prefix):
    return {c: open(f"{prefix}.groups.{c}.bed").read() for c in CTX}, open(f"{prefix}.groups.summary.tsv").read()


def _write_samples(d, names):
    """the data set as 3 + 3 prefixes of three cov.bed files each, rows in the order of the data set; one file gzip under the plain name"""
    prefixes = {1: [], 2: []}
    for (g, s), (gpos, p, n, motif) in sorted(G.dataset().items()):
        prefix = str(d / ("g%ds%d" % (g, s)))
        prefixes[g].append(prefix)
        sid = np.searchsorted(OFFSETS, gpos, side="right") - 1
        for c in range(3):
            sel = np.flatnonzero(np.minimum(motif, 2) == c)
            text = "".join("%s\t%d\t%d\t%g\t%d\t%d\n" % (names[sid[i]], gpos[i] - OFFSETS[sid[i]], gpos[i] - OFFSETS[sid[i]] + 1,
                                                        100.0 * p[i] / max(p[i] + n[i], 1), p[i], n[i]) for i in sel)
            with open(f"{prefix}.{CTX[c]}.cov.bed", "wb") as f:
                f.write(gzip.compress(text.encode()) if (g, s, c) == (2, 1, 1) else text.encode())
    return prefixes


@pytest.fixture(scope="module")
def command(tmp_path_factory):
    from bamutil import write_fasta
    d = tmp_path_factory.mktemp("groups")
    genome = _genome()
    fa = str(d / "ref.fa")
    write_fasta(fa, genome)
    prefixes = _write_samples(d, [n for n, _ in genome])
    A, B = ",".join(prefixes[1]), ",".join(prefixes[2])
    r = _cli([fa, A, B, str(d / "out")])
    _cli(["-t", "3", fa, B, A, str(d / "swapped")])
    return genome, fa, prefixes, str(d), r.stderr


def test_command_equals_the_python_path(command):
    from hifimeth_amd.pileup import MethylationPileup, group_qvalues, groups_summary_tsv, read_cov_bed
    genome, _fa, prefixes, d, stderr = command
    names = [n for n, _ in genome]
    pu = MethylationPileup(genome, partitions=True, groups=True, group_min_cov=5)
    try:
        for g in (1, 2):
            for s, prefix in enumerate(prefixes[g]):
                assert pu.begin_sample(g) == s
                for c in CTX:
                    pu.load_sample_loci(*read_cov_bed(f"{prefix}.{c}.cov.bed", names, pu.offsets))
        rows = pu.group_tests(min_reps=2)
        q, m = group_qvalues(rows)
        beds, summary = _files(d + "/out")
        assert pu.groups_bed(rows, q) == beds and groups_summary_tsv(rows, q, m) == summary
        assert all(len(beds[c].splitlines()) >= 10 and all(len(x.split("\t")) == 13 for x in beds[c].splitlines()) for c in CTX)
        assert [int(x.split("\t")[1]) for x in summary.splitlines()] == [len(beds[c].splitlines()) for c in CTX]
        assert sum(int(x.split("\t")[4]) for x in summary.splitlines()) == int((rows["phi"] > 1).sum()) >= 50
        assert f"{d}/out.groups.*" in stderr and "Skip" not in stderr and "min replicates per group 2" in stderr
    finally:
        pu.close()


def _negated(text):
    return text if text == "0" else text[1:] if text.startswith("-") else "-" + text


def test_swapped_groups_mirror_the_rows(command):
    _genome_, _fa, _prefixes, d, _e = command
    (beds, summary), (sbeds, ssummary) = _files(d + "/out"), _files(d + "/swapped")
    assert summary == ssummary
    for c in CTX:
        a_lines, b_lines = beds[c].splitlines(), sbeds[c].splitlines()
        assert len(a_lines) == len(b_lines)
        for a, b in zip(a_lines, b_lines):
            a, b = a.split("\t"), b.split("\t")
            assert b[:3] == a[:3] and b[3] == _negated(a[3]) and b[4:6] == a[4:6] and b[6:12] == a[9:12] + a[6:9] and b[12] == a[12]


def test_command_errors(command, tmp_path):
    genome, fa, prefixes, d, _e = command
    A, B = ",".join(prefixes[1]), ",".join(prefixes[2])
    out = str(tmp_path / "o")
    # -a and -r reach the engine
    _cli(["-a", "12", "-r", "3", fa, A, B, out])
    ref = G.GroupLoader(TOTAL, 12)
    for (g, s), rows in sorted(G.dataset().items()):
        ref.begin_sample(g)
        ref.load(rows[0], rows[1], rows[2], np.minimum(rows[3], 2))
    want = ref.tested(3)
    got = [(x.split("\t")[0], int(x.split("\t")[1])) for c in CTX for x in open(f"{out}.groups.{c}.bed").read().splitlines()]
    assert sorted(got) == sorted(("ctg%d" % (s + 1), g - int(OFFSETS[s])) for g, *_ in want for s in [int(np.searchsorted(OFFSETS, g, side="right")) - 1])
    assert 0 < len(want) < len(G.dataset_loader().tested(3))
    # one file missing: its context is skipped and the file named
    moved = prefixes[2][2] + ".CHG.cov.bed"
    os.rename(moved, moved + ".away")
    try:
        r = _cli([fa, A, B, out + "2"])
        assert "Skip context CHG" in r.stderr and moved in r.stderr
        assert open(out + "2.groups.CHG.bed").read() == "" and open(out + "2.groups.CpG.bed").read() == open(d + "/out.groups.CpG.bed").read()
    finally:
        os.rename(moved + ".away", moved)
    assert "no context" in _cli([fa, str(tmp_path / "x") + "," + str(tmp_path / "y"), B, out + "3"], ok=False).stderr
    # a group of one sample under the default -r
    r = _cli([fa, prefixes[1][0], B, out + "4"], ok=False)
    assert "group 1 has 1 samples, fewer than -r 2" in r.stderr
    _cli(["-r", "1", fa, prefixes[1][0], B, out + "4"])
    # a duplicate line: the file is named
    bad = str(tmp_path / "dup")
    for c in CTX:
        with open(f"{bad}.{c}.cov.bed", "w") as f:
            f.write("ctg1\t7\t8\t50\t5\t5\n" + ("ctg2\t9\t10\t50\t5\t5\nctg1\t7\t8\t0\t0\t9\n" if c == "CHG" else ""))
    r = _cli([fa, A, prefixes[2][0] + "," + bad, out + "5"], ok=False)
    assert f"{bad}.CHG.cov.bed: " in r.stderr and "1 locus given twice in one sample" in r.stderr      # ctg1:7 came in the sample's CpG file
    with open(f"{bad}.CpG.cov.bed", "w") as f:
        f.write("ctg1\t7\t8\t50\t1048576\t0\n")
    r = _cli([fa, A, prefixes[2][0] + "," + bad, out + "6"], ok=False)
    assert f"{bad}.CpG.cov.bed: " in r.stderr and "count above 2^20 - 1" in r.stderr


# ---- a reference past 2^32 bases -----------------------------------------------------------------------------------------------------
def test_groups_around_two_to_the_32():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    total = R.HOST_LEN[R.B32]
    lengths = [R.B31, R.B31, total - R.B32]                   # 2^31 - 1 and 2^32 - 1 are the last bases of the first two contigs
    need = total * (1 + 4 * 7 + 18) + total // 8 + (1 << 30)  # + the moment and sample-count planes and the seen bitmap
    free, _all = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip("the card has %.1f GB free, the case needs %.1f GB plus 8 GB" % (free / 1e9, need / 1e9))
    loci = [R.B31 - 1, R.B32 - 1, R.B32 + 5]
    samples = {1: [([9, 1, 30], [1, 9, 2]), ([7, 3, 20], [2, 9, 9])], 2: [([2, 8, 3], [8, 2, 40]), ([1, 9, 6], [9, 2, 30])]}
    pu = MethylationPileup([("c%d" % k, n) for k, n in enumerate(lengths)], partitions=True, groups=True,
                           bases=np.full(total, ord("N"), np.uint8))
    try:
        assert pu.n_loci == total > R.B32
        for part in (2, 1):
            for s, (p, n) in enumerate(samples[part]):
                assert pu.begin_sample(part) == s
                assert pu.load_sample_loci(loci[::-1], p[::-1], n[::-1], [2, 1, 0]) == 3
        rows = pu.group_tests(min_reps=2)
        assert rows["gpos"].tolist() == loci and rows["motif"].tolist() == [0, 1, 2] and rows["m1"].tolist() == rows["m2"].tolist() == [2, 2, 2]
        e_ref = G.e_ref()
        for k, r in enumerate(rows):
            s = G.sums_of(*([(p[k], p[k] + n[k]) for p, n in samples[part]] for part in (1, 2)))
            assert (int(r["pcov1"]), int(r["pcov1"] + r["ncov1"]), int(r["pcov2"]), int(r["pcov2"] + r["ncov2"])) == (s[0], s[1], s[4], s[5])
            assert pu.group_planes(1, loci[k], loci[k] + 1)[0][0] == s[2] and pu.group_planes(2, loci[k], loci[k] + 1)[1][0] == 2
            mD, mphi, mp_ = G.stat_mp(*s)
            assert r["diff"] == G.np_diff(s[0], s[1], s[4], s[5])
            assert G.rel(r["D"], mD) <= 8 * e_ref["D"] and G.rel(r["phi"], mphi) <= 8 * e_ref["phi"] and G.rel(r["pvalue"], mp_) <= 8 * e_ref["p"]
        for lo, hi, want in ((0, R.B31, [loci[0]]), (R.B31, R.B32, [loci[1]]), (R.B32, total, [loci[2]]), (R.B31 - 1, R.B32 + 6, loci)):
            assert pu.group_tests(lo, hi, 2)["gpos"].tolist() == want
        assert pu.loci()["gpos"].tolist() == loci
        assert _load(pu, ([total], [5], [5], [0])) == HM_EDATA                # the bound is the 64-bit length
    finally:
        pu.close()
        torch.cuda.empty_cache()
