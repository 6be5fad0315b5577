"""`groupdmr` on the device: hm_dmr_fetch_regions against the restatement of tests/group_regions_ref.py applied to the rows
hm_pileup_fetch_groups returns for the same range -- every field, the floats by their bits --, on counts laid out so that the
engine's own rows show every case, and on a random data set; the stitch of adjacent ranges; -F through Python; the command against
the Python path, its -L against `groupdiff`, its BED read by `regiondiff -R`.  Nothing here has a tolerance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import group_regions_ref as RR
from group_regions_ref import LENGTHS, MAX_GAP, MIN_COV, MIN_REPS, OFFSETS, TOTAL
from groups_ref import HM_EDATA, HM_EINVAL, HM_ESTATE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
CTX = ("CpG", "CHG", "CHH")


def _genome(seed=4):
    rng = np.random.default_rng(seed)
    return [("ctg%d" % (s + 1), "".join(rng.choice(list("ACGT"), n))) for s, n in enumerate(LENGTHS)]


def _loaded(samples):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(_genome(), partitions=True, groups=True, group_min_cov=MIN_COV)
    for (g, s), rows in sorted(samples.items()):
        assert pu.begin_sample(g) == s
        assert pu.load_sample_loci(*rows) == int((rows[1] + rows[2] >= MIN_COV).sum())
    return pu


@pytest.fixture(scope="module")
def crafted():
    """-> (engine, its hm_group_t rows over the whole reference): the reference every expected region is computed from, fetched once"""
    pu = _loaded(RR.layout_samples())
    rows = pu.group_tests(min_reps=MIN_REPS)
    rows.setflags(write=False)
    yield pu, rows
    pu.close()


@pytest.fixture(scope="module")
def random_set():
    pu = _loaded(RR.dataset())
    rows = pu.group_tests(min_reps=MIN_REPS)
    rows.setflags(write=False)
    yield pu, rows
    pu.close()


def _within(rows, lo, hi):
    return rows[(rows["gpos"] >= lo) & (rows["gpos"] < hi)]


def _same(pu, rows, ctx, lo, hi, max_p, min_diff, max_gap, min_loci, keep=False, min_reps=MIN_REPS):
    """one fetch equals the restatement on the rows of [lo, hi): regions byte for byte, R and the hits -> the regions"""
    got = pu.group_regions(ctx, lo, hi, min_reps, max_p, min_diff, max_gap, min_loci, keep)
    want = RR.regions(_within(rows, lo, hi), ctx, max_p, min_diff, max_gap, min_loci, keep)
    assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:], (ctx, lo, hi, max_p, min_diff, max_gap, min_loci, keep)
    return got[0]


def _chains(regions, base=0):
    return [(int(g["start"]) - base, int(g["end"]) - base, int(g["n_loci"]), int(g["sign"])) for g in regions]


def test_the_rows_are_those_of_fetch_groups(crafted):
    """the layout gives the rows it was made for: every kind tested or not as intended, the hits' p below 0.008"""
    _pu, rows = crafted
    kind = RR.layout()
    assert rows["gpos"].tolist() == [i for i, k in enumerate(kind) if k not in ".U"]
    by_kind = {k: rows[[kind[g] == k for g in rows["gpos"]]] for k in "PMNOABpq"}
    for k in "PMOpq":
        assert (by_kind[k]["pvalue"] < 0.008).all() and (np.sign(by_kind[k]["diff"]) == (-1 if k == "M" else 1)).all(), k
    assert (by_kind["N"]["pvalue"] == 1.0).all() and (by_kind["N"]["diff"] == 0.0).all()
    assert (by_kind["A"]["diff"] == 10.0).all() and (by_kind["A"]["pvalue"] > 0.01).all()
    assert (np.abs(by_kind["B"]["diff"] - 25.0 / 3.0) < 1e-9).all()
    assert (by_kind["p"]["m1"] == 2).all() and (by_kind["p"]["phi"] > 1).all() and (by_kind["q"]["phi"] > 1).all() and (by_kind["O"]["motif"] == 1).all()


def test_the_crafted_chains_of_sequence_one(crafted):
    """a single hit; a chain ended by a tested non-hit, by a sign flip; gaps of max_gap and max_gap + 1; a locus of another context
    and an untested one inside a chain; the chain with row 0 and the one with the last row"""
    pu, rows = crafted
    got = _same(pu, rows, 0, 0, 3000, 0.01, 0.0, MAX_GAP, 1)
    assert _chains(got) == RR.SEQ1_CHAINS
    assert [int(g["flags"]) for g in got] == [RR.FIRST] + [0] * 11 + [RR.LAST]
    assert (got["m1_min"] == 3).all() and (got["m2_min"] == 3).all() and (got["phi_max"] == 1.0).all() and (got["reserved"] == 0).all()
    assert got["pcov1"].tolist() == [20 * 3 * n if s > 0 else 0 for _s, _e, n, s in RR.SEQ1_CHAINS] and got["diff"][5] == -100.0
    for min_loci in (2, 3, 4):
        for keep in (False, True):
            kept = _same(pu, rows, 0, 0, 3000, 0.01, 0.0, MAX_GAP, min_loci, keep)
            assert _chains(kept) == [c for k, c in enumerate(RR.SEQ1_CHAINS) if c[2] >= min_loci or (keep and k in (0, 12))]
    assert _chains(_same(pu, rows, 0, 0, 3000, 0.01, 0.0, MAX_GAP + 1, 2))[4:6] == [(50, 62, 3, 1), (70, 76, 2, 1)]      # 55 .. 61 links now
    assert (85, 92, 2, 1) in _chains(_same(pu, rows, 0, 0, 3000, 0.01, 0.0, MAX_GAP + 1, 2))
    # the other context has its own rows: 72 and 88 are 16 apart
    assert _chains(_same(pu, rows, 1, 0, 3000, 0.01, 0.0, MAX_GAP, 1)) == [(72, 73, 1, 1), (88, 89, 1, 1)]
    assert _chains(_same(pu, rows, 1, 0, 3000, 0.01, 0.0, 16, 1)) == [(72, 89, 2, 1)]
    assert len(_same(pu, rows, 2, 0, TOTAL, 0.01, 0.0, MAX_GAP, 1)) == 0


def test_min_diff_just_under_and_just_at(crafted):
    pu, rows = crafted
    at = lambda regions: [c for c in _chains(regions) if 110 <= c[0] < 120]
    assert at(_same(pu, rows, 0, 0, 3000, 1.0, 0.0, MAX_GAP, 1)) == [(110, 113, 3, 1)]
    assert at(_same(pu, rows, 0, 0, 3000, 1.0, 10.0, MAX_GAP, 1)) == [(110, 111, 1, 1), (112, 113, 1, 1)]      # 111, at 8.33, breaks
    assert at(_same(pu, rows, 0, 0, 3000, 1.0, float(np.nextafter(10.0, 11.0)), MAX_GAP, 1)) == []
    assert at(_same(pu, rows, 0, 0, 3000, 1.0, 25.0 / 3.0 - 1e-9, MAX_GAP, 1)) == [(110, 113, 3, 1)]
    assert at(_same(pu, rows, 0, 0, 3000, 0.01, 0.0, MAX_GAP, 1)) == []                                    # their p is about 0.3
    assert len(_same(pu, rows, 0, 0, 3000, 1.0, 100.0, MAX_GAP, 1)) == 13                                   # every P and M chain is at 100


def test_the_sequence_boundary_and_the_long_chain(crafted):
    pu, rows = crafted
    whole = _same(pu, rows, 0, 0, TOTAL, 0.01, 0.0, MAX_GAP, 2)
    assert (2997, 3002, 5, 1) in _chains(whole)                # one chain over the whole reference ...
    one, two = _same(pu, rows, 0, 0, 3000, 0.01, 0.0, MAX_GAP, 2), _same(pu, rows, 0, 3000, TOTAL, 0.01, 0.0, MAX_GAP, 2)
    assert _chains(one)[-1] == (2997, 3000, 3, 1) and _chains(two, 3000)[0] == (0, 2, 2, 1)                  # ... two per sequence
    assert int(one[-1]["flags"]) == RR.LAST and int(two[0]["flags"]) == RR.FIRST and int(two[-1]["flags"]) == RR.LAST
    assert _chains(two, 3000) == [(0, 2, 2, 1), (RR.LONG_AT, RR.LONG_AT + RR.LONG_N, RR.LONG_N, 1), (1498, 1500, 2, 1)]
    long = whole[whole["n_loci"] == RR.LONG_N]
    assert len(long) == 1 and long[0]["m1_min"] == 2 and long[0]["m2_min"] == 3 and long[0]["phi_max"] > 1.0
    cpg_index = np.count_nonzero(rows["gpos"][RR.ctx_mask(rows, 0)] < 3000 + RR.LONG_AT)
    assert cpg_index < 4096 < cpg_index + RR.LONG_N - 1        # the chain's rows lie in two workgroups of the row selection
    for keep in (False, True):
        for min_loci in (1, 1000, 1001):
            _same(pu, rows, 0, 0, TOTAL, 0.01, 0.0, MAX_GAP, min_loci, keep)
            _same(pu, rows, 0, 3000, TOTAL, 0.01, 0.0, 1, min_loci, keep)


def test_other_fetches_in_between_change_nothing(crafted):
    """the fetch keeps its rows in a buffer of its own and shares the row staging with every other fetch: in any order, the same bytes"""
    pu, rows = crafted
    args = (0, 0, TOTAL, MIN_REPS, 0.01, 0.0, MAX_GAP, 2)
    first = pu.group_regions(*args)
    assert pu.group_tests(min_reps=MIN_REPS).tobytes() == rows.tobytes()
    other = pu.group_regions(1, 0, 3000, MIN_REPS, 1.0, 0.0, 50, 1)
    loci, tested = pu.loci(), pu.asm(min_cov=MIN_COV)
    again = pu.group_regions(*args)
    assert again[0].tobytes() == first[0].tobytes() and again[1:] == first[1:] and len(first[0]) > 5 and len(other[0]) == 1
    assert pu.group_tests(min_reps=MIN_REPS).tobytes() == rows.tobytes()
    assert pu.loci().tobytes() == loci.tobytes() and pu.asm(min_cov=MIN_COV).tobytes() == tested.tobytes() and len(tested) >= len(rows)


def _raw(pu, lo, hi, min_reps, ctx, max_p, min_diff, max_gap, min_loci, keep, out=None, cap=0, counts=True):
    R, H = ctypes.c_int64(-7), ctypes.c_int64(-7)
    n = pu._L.hm_dmr_fetch_regions(pu._h, lo, hi, min_reps, ctx, max_p, min_diff, max_gap, min_loci, keep,
                                            ctypes.byref(R) if counts else None, ctypes.byref(H) if counts else None,
                                            None if out is None else out.ctypes.data_as(ctypes.c_void_p), cap)
    return n, R.value, H.value


def test_cap_counts_and_empty_ranges(crafted):
    from hifimeth_amd.pileup import GROUP_REGION_DTYPE
    pu, rows = crafted
    want, R, hits = RR.regions(_within(rows, 0, 3000), 0, 0.01, 0.0, MAX_GAP, 1)
    args = (0, 3000, MIN_REPS, 0, 0.01, 0.0, MAX_GAP, 1, 0)
    assert _raw(pu, *args) == (13, R, hits) and _raw(pu, *args, counts=False)[0] == 13
    out = np.full(13, 0x55, np.uint8).repeat(96).view(GROUP_REGION_DTYPE)
    assert _raw(pu, *args, out=out, cap=12) == (13, R, hits) and (out.view(np.uint8) == 0x55).all()          # cap too small: nothing written
    assert _raw(pu, *args, out=out, cap=13) == (13, R, hits) and out.tobytes() == want.tobytes()
    assert _raw(pu, 500, 500, *args[2:]) == (0, 0, 0) and _raw(pu, TOTAL, TOTAL, *args[2:]) == (0, 0, 0)     # hi == lo
    assert _raw(pu, 2, 10, *args[2:]) == (0, 0, 0)            # a range without loci
    assert _raw(pu, 120, 2997, *args[2:]) == (0, 2877, 0)     # rows, no hit
    assert _raw(pu, 0, 3000, 3, *args[3:]) == (13, R, hits)   # min_reps 3: every row of sequence 1 has 3 + 3
    assert _raw(pu, 3000, TOTAL, 3, 0, 0.01, 0.0, MAX_GAP, 1, 0)[1] < _raw(pu, 3000, TOTAL, 2, 0, 0.01, 0.0, MAX_GAP, 1, 0)[1]   # the 'p' loci drop out


def test_errors(crafted):
    from hifimeth_amd.pileup import MethylationPileup
    pu, _rows = crafted
    ok = dict(lo=0, hi=TOTAL, min_reps=2, ctx=0, max_p=0.01, min_diff=0.0, max_gap=5, min_loci=1, keep=0)
    nan = float("nan")
    bad = [("min_reps", 0), ("min_reps", 256), ("ctx", -1), ("ctx", 3), ("max_p", 0.0), ("max_p", -0.5), ("max_p", 1.0000001), ("max_p", nan),
           ("min_diff", -1e-9), ("min_diff", 100.0000001), ("min_diff", nan), ("max_gap", 0), ("max_gap", -3), ("min_loci", 0), ("min_loci", -1),
           ("lo", -1), ("lo", TOTAL + 1), ("hi", TOTAL + 1), ("hi", -1)]
    for name, value in bad:
        assert _raw(pu, *{**ok, name: value}.values())[0] == HM_EINVAL, (name, value)
        assert b"hm_dmr_fetch_regions" in pu._L.hm_pileup_last_error(pu._h)
    assert _raw(pu, 10, 9, *list(ok.values())[2:])[0] == HM_EINVAL
    for name, value in (("max_p", 1.0), ("min_diff", 100.0), ("min_diff", 0.0), ("min_reps", 255), ("ctx", 2)):
        assert _raw(pu, *{**ok, name: value}.values())[0] >= 0, (name, value)
    assert pu._L.hm_dmr_fetch_regions(None, 0, 1, 2, 0, 0.01, 0.0, 5, 1, 0, None, None, None, 0) == HM_EINVAL
    plain = MethylationPileup(_genome(), partitions=True)     # an engine without "groups"
    try:
        assert _raw(plain, *ok.values())[0] == HM_ESTATE and b"groups" in plain._L.hm_pileup_last_error(plain._h)
    finally:
        plain.close()
    void = MethylationPileup(_genome(), partitions=True, groups=True)      # ... and one voided by a bad row
    try:
        from hifimeth_amd.pileup import LOCUS_DTYPE
        assert void.begin_sample(1) == 0
        row = np.zeros(1, LOCUS_DTYPE)
        row["gpos"], row["pcov"], row["ncov"] = TOTAL, 5, 5
        assert void._L.hm_pileup_load_sample_loci(void._h, row.ctypes.data_as(ctypes.c_void_p), 1) == HM_EDATA
        assert _raw(void, *ok.values())[0] == HM_ESTATE
    finally:
        void.close()


@pytest.mark.parametrize("max_p,min_diff,max_gap,min_loci", RR.THRESHOLDS)
def test_the_random_data_set(random_set, max_p, min_diff, max_gap, min_loci):
    pu, rows = random_set
    n = 0
    for ctx in (0, 1, 2):
        for keep in (False, True):
            for lo, hi in ((0, TOTAL), (0, 3000), (3000, TOTAL), (1234, 3777)):
                n += len(_same(pu, rows, ctx, lo, hi, max_p, min_diff, max_gap, min_loci, keep))
    assert n > 20
    if (max_p, min_diff, max_gap, min_loci) == RR.THRESHOLDS[0]:      # what the CPU suite asserts of the restated rows holds of the engine's
        kept = _same(pu, rows, 0, 0, TOTAL, max_p, min_diff, max_gap, min_loci)
        assert len(kept) >= 20 and (kept["sign"] > 0).sum() >= 5 and (kept["sign"] < 0).sum() >= 5
        assert (kept["phi_max"] > 1).any() and (kept["m1_min"] == 2).any()


def test_stitched_parts_equal_the_whole(random_set, crafted):
    from hifimeth_amd.pileup import stitch_group_regions
    for (pu, rows), lo, hi, cuts, (max_p, min_diff, max_gap, min_loci) in (
            (random_set, 0, 3000, (0, 1, 90, 1500, 1503, 2999, 3000), RR.THRESHOLDS[0]),
            (random_set, 3000, TOTAL, (3000, 3456, 4499), RR.THRESHOLDS[1]),
            (crafted, 3000, TOTAL, (3001, 3000 + RR.LONG_AT, 3000 + RR.LONG_AT + 1, 3777, 4096, TOTAL - 1), (0.01, 0.0, MAX_GAP, 3)),
            (crafted, 0, 3000, (1, 22, 23, 37, 53, 103, 2998), (0.01, 0.0, MAX_GAP, 2))):
        for keep in (False, True):
            whole = _same(pu, rows, 0, lo, hi, max_p, min_diff, max_gap, min_loci, keep)
            for m in cuts:
                parts = [pu.group_regions(0, a, b, MIN_REPS, max_p, min_diff, max_gap, min_loci, True)[:2] for a, b in ((lo, m), (m, hi))]
                got, R = stitch_group_regions(parts, max_gap, min_loci, keep_edges=keep)
                assert got.tobytes() == whole.tobytes() and R == np.count_nonzero(RR.ctx_mask(_within(rows, lo, hi), 0)), (lo, hi, m, keep)
            assert len(whole) > 0


def test_chaining_by_q_through_python(random_set):
    from hifimeth_amd.pileup import group_p_cutoff, group_qvalues
    pu, rows = random_set
    q, _m = group_qvalues(rows)
    n = 0
    for max_q in (0.05, 0.3, 1e-12):
        cut = group_p_cutoff(rows, q, max_q)
        assert cut.tobytes() == RR.p_cutoff(rows["pvalue"], q, rows["motif"], max_q).tobytes()
        for ctx in (0, 1, 2):
            for lo, hi in ((0, 3000), (3000, TOTAL)):
                sel = (rows["gpos"] >= lo) & (rows["gpos"] < hi)
                want = RR.regions(rows[sel], ctx, 1.0, 0.0, 30, 2, q=q[sel], max_q=max_q)
                if cut[ctx] == 0.0:                           # not fetched: 0 is no max_p
                    assert len(want[0]) == 0 and want[2] == 0 and max_q == 1e-12
                    continue
                got = pu.group_regions(ctx, lo, hi, MIN_REPS, float(cut[ctx]), 0.0, 30, 2)
                assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:]
                n += len(got[0])
    assert n > 20


# ---- the command ----------------------------------------------------------------------------------------------------------------------
def _cli(command, args, ok=True):
    r = subprocess.run([CLI, command, *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.fixture(scope="module")
def command(tmp_path_factory):
    from bamutil import write_fasta
    d = tmp_path_factory.mktemp("groupdmr")
    genome = _genome()
    names = [n for n, _ in genome]
    fa = str(d / "ref.fa")
    write_fasta(fa, genome)
    prefixes = {1: [], 2: []}
    for (g, s), (gpos, p, n, motif) in sorted(RR.dataset().items()):
        prefix = str(d / ("g%ds%d" % (g, s)))
        prefixes[g].append(prefix)
        sid = np.searchsorted(OFFSETS, gpos, side="right") - 1
        for c in range(3):
            with open(f"{prefix}.{CTX[c]}.cov.bed", "w") as f:
                f.write("".join("%s\t%d\t%d\t0\t%d\t%d\n" % (names[sid[i]], gpos[i] - OFFSETS[sid[i]], gpos[i] - OFFSETS[sid[i]] + 1, p[i], n[i])
                                for i in np.flatnonzero(np.minimum(motif, 2) == c)))
    A, B = ",".join(prefixes[1]), ",".join(prefixes[2])
    by_p = _cli("groupdmr", ["-s", "0.01", "-g", "30", "-n", "3", fa, A, B, str(d / "p")])
    _cli("groupdmr", ["-F", "0.3", "-m", "20", "-g", "30", "-n", "2", "-L", "-t", "3", fa, A, B, str(d / "q")])
    _cli("groupdiff", [fa, A, B, str(d / "loci")])
    return genome, fa, (A, B), str(d), by_p.stderr


def _python_path(pu, rows, cutoff, min_diff, max_gap, min_loci):
    """-> (the three BED texts, the summary) as the command writes them: per context, sequence by sequence"""
    from hifimeth_amd.pileup import GROUP_REGION_DTYPE, groupdmr_summary_tsv
    found, tested, hits = [], [0, 0, 0], [0, 0, 0]
    for ctx in (0, 1, 2):
        parts = [np.zeros(0, GROUP_REGION_DTYPE)]
        for s in range(2):
            if cutoff[ctx] > 0:
                got, R, H = pu.group_regions(ctx, int(OFFSETS[s]), int(OFFSETS[s + 1]), MIN_REPS, float(cutoff[ctx]), min_diff, max_gap, min_loci)
                parts.append(got)
                tested[ctx] += R
                hits[ctx] += H
        if not cutoff[ctx] > 0:
            tested[ctx] = int(np.count_nonzero(RR.ctx_mask(rows, ctx)))
        found.append(np.concatenate(parts))
    return pu.group_regions_bed(np.concatenate(found)), groupdmr_summary_tsv(tested, hits, [c if c > 0 else np.nan for c in cutoff], found)


def test_command_equals_the_python_path(command, random_set):
    from hifimeth_amd.pileup import group_p_cutoff, group_qvalues
    pu, rows = random_set
    _genome_, _fa, _ab, d, stderr = command
    beds, summary = _python_path(pu, rows, [0.01] * 3, 0.0, 30, 3)
    for c in CTX:
        assert open(f"{d}/p.groupdmr.{c}.bed").read() == beds[c], c
    assert open(f"{d}/p.groupdmr.summary.tsv").read() == summary
    lines = beds["CpG"].splitlines()
    assert len(lines) >= 20 and all(len(x.split("\t")) == 16 for x in lines)
    assert [x.split("\t")[3] for x in lines] == ["CpG_%d" % (k + 1) for k in range(len(lines))] and {x.split("\t")[5] for x in lines} == {"."}
    assert {x.split("\t")[6] for x in lines} == {"+", "-"} and {x.split("\t")[0] for x in lines} == {"ctg1", "ctg2"}
    assert not os.path.exists(f"{d}/p.groups.CpG.bed") and f"{d}/p.groupdmr.*" in stderr and "p <= 0.01" in stderr
    q, _m = group_qvalues(rows)
    cut = group_p_cutoff(rows, q, 0.3)
    beds, summary = _python_path(pu, rows, cut, 20.0, 30, 2)
    for c in CTX:
        assert open(f"{d}/q.groupdmr.{c}.bed").read() == beds[c], c
    assert open(f"{d}/q.groupdmr.summary.tsv").read() == summary and len(beds["CpG"].splitlines()) >= 10
    assert [x.split("\t")[3] for x in summary.splitlines()] == ["%.6g" % c for c in cut]


def test_loci_output_equals_groupdiff(command):
    _genome_, _fa, _ab, d, _e = command
    for name in [f"groups.{c}.bed" for c in CTX] + ["groups.summary.tsv"]:
        assert open(f"{d}/q.{name}", "rb").read() == open(f"{d}/loci.{name}", "rb").read() != b"", name


def test_a_cutoff_of_zero_and_the_regions_as_intervals(command, tmp_path):
    _genome_, fa, (A, B), d, _e = command
    out = str(tmp_path / "none")
    _cli("groupdmr", ["-F", "1e-12", fa, A, B, out])          # no locus has such a q: no context is fetched
    assert all(open(f"{out}.groupdmr.{c}.bed").read() == "" for c in CTX)
    rows = [x.split("\t") for x in open(f"{out}.groupdmr.summary.tsv").read().splitlines()]
    assert [r[0] for r in rows] == list(CTX) and all(int(r[1]) > 50 and r[2:] == ["0", "nan", "0", "0", "0", "0"] for r in rows)
    # the BED is input to regiondiff -R: name from column 4, no strand
    _cli("regiondiff", ["-R", f"{d}/p.groupdmr.CpG.bed", fa, A, B, str(tmp_path / "rd")])
    table = [x.split("\t") for x in open(str(tmp_path / "rd") + ".regiondiff.CpG.tsv").read().splitlines()[1:]]
    bed = [x.split("\t") for x in open(f"{d}/p.groupdmr.CpG.bed").read().splitlines()]
    assert [r[:5] for r in table] == [b[:4] + ["."] for b in bed] and len(table) >= 20
    assert sum(r[14] != "nan" for r in table) >= 10           # intervals the samples can be tested on
