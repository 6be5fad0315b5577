"""A second hm_pileup_set_reference on one engine (tests/retarget_cases.py has the inputs, the depths and the in-bounds rule).

The contract of include/hifimeth_hip.h: after the call returns HM_OK the engine is a newly created one with the same options and
caller planes on the new reference.  Every case runs job A on an engine to a stated depth, re-targets it and runs job B; a freshly
created engine runs job B only.  Every comparison is exact -- rows and planes byte for byte, p-values as bits: the device tests are
functions of the counts alone.  Job B's answers are also held to the restatements (pileup_oracle, bedmethyl_ref, patterns_ref,
linkage_ref, readpos_ref, diff_ref.Loader, groups_ref.GroupLoader, samples_ref.SampleLoader), so that two engines wrong alike do
not pass.

On the library before the contract was implemented 52 of 64 cases failed (the negative-length case was not run
there: that library leaves its sequence offsets half written): every record case -- records
resident at depth b, job A's histogram bins at c and d, job A's staged reads at a --, the caller-plane case, `diff` (1500 of job B's
rows `given twice`), `groupdiff` (the engine's own partition planes kept job A's counts), groups + diff and the three flag cases."""
import ctypes

import numpy as np
import pytest

import retarget_cases as R
import sequence_cases as S
from sequence_cases import HM_EINVAL, HM_ESTATE

pytestmark = pytest.mark.gpu
_CACHE = {}
HM_EDATA = -4
VOID = "a load of this engine met bad rows (hm_pileup_load_loci): its planes mean nothing"
STAGED = "hm_pileup_load_loci on an engine that has staged records: counts come from records or from loads, not both"
LOADED = "hm_pileup_submit_read on an engine whose counts were loaded (hm_pileup_load_loci, hm_pileup_group_sample, hm_sample_open)"
ONE_SOURCE = "hm_pileup_group_sample on an engine that staged records or used hm_pileup_load_loci / hm_sample_open: counts come from one source"


def _new(genome, **options):
    from hifimeth_amd.pileup import MethylationPileup
    return MethylationPileup(genome, **options)


def _err(pu):
    return pu._L.hm_pileup_last_error(pu._h).decode()


def _answers(pu, family):
    return {name: S.evaluate(fn, pu) for name, fn in R.readers(family)}


def _fresh(family, target):
    """name -> (bytes, result) of the family's readers on an engine of its own that ran job B of `target` and nothing else"""
    key = ("fresh", family, target)
    if key not in _CACHE:
        g, reads = R.job(target)
        pu = _new(g, **R.FAMILIES[family][0])
        thrs = R.run_job(pu, reads)
        _CACHE[key] = (_answers(pu, family), thrs, pu.names, pu.offsets.tolist(), pu.bed(pu.loci()))
        pu.close()
    return _CACHE[key]


# ---- jobs on records -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,depth,target", R.RECORD_CASES, ids=["%s-%s-%s" % c for c in R.RECORD_CASES])
def test_job_b_after_job_a_equals_job_b_alone(family, depth, target):
    assert R.rule_holds(depth, target)
    want, want_thrs, names, offsets, bed = _fresh(family, target)
    g_a, reads_a = R.job("A")
    g_b, reads_b = R.job(target)
    pu = _new(g_a, **R.FAMILIES[family][0])
    try:
        R.run_to(pu, depth, reads_a, [fn for _n, fn in R.readers(family)])
        pu.set_reference(g_b)
        assert _err(pu) == "" and pu.num_records() == 0 and pu.num_pattern_records() == 0
        assert not pu.histograms().any(), "the histograms of job A outlive the call"
        thrs = R.run_job(pu, reads_b)
        print(family, depth, target, thrs, want_thrs)
        assert thrs == want_thrs, "the thresholds resolved from the histograms"
        assert pu.resolve_thresholds(pu.histograms()) == pu.resolve_thresholds(want["histograms"][1][0])
        got = _answers(pu, family)
        for name in want:
            assert want[name][1] is not None, (name, want[name][0])
            assert got[name][0] == want[name][0], name
        assert pu.names == names and pu.offsets.tolist() == offsets and pu.bed(pu.loci()) == bed
    finally:
        pu.close()


@pytest.mark.parametrize("family,target", [("all", t) for t in R.TARGETS] + [("plain", "same"), ("filtered", "same"), ("patterns", "same"),
                                                                              ("bedmethyl", "same"), ("linkage", "same")])
def test_job_b_alone_equals_the_restatements(family, target):
    """the other side of every comparison above, held once to the restatements"""
    options = R.FAMILIES[family][0]
    ref = R.restated(target, trim="trim" in options, filtered=family == "filtered")
    fresh, thrs, _names, _offsets, _bed = _fresh(family, target)
    assert thrs == ref["thresholds"]
    checked = 0
    for name, (_bytes, result) in fresh.items():
        if name in ref:
            got = R.as_tuples(name, result)
            assert (got == ref[name]).all() if name == "histograms" else got == ref[name], name
            checked += 1
    assert checked >= {"all": 9, "plain": 2, "filtered": 2}.get(family, 3)


def test_options_that_must_precede_the_reference_still_answer_estate():
    g, reads = R.job("A")
    pu = _new(g, min_mapq=R.FILTER["min_mapq"])
    try:
        R.run_to(pu, "c", reads)
        pu.set_reference(R.reference("changed"))
        for key in (b"partitions", b"groups", b"samples", b"patterns"):
            assert pu._L.hm_pileup_set_option(pu._h, key, 2.0) == HM_ESTATE, key
            assert _err(pu) == key.decode() + " must be set before hm_pileup_set_reference" + (" / hm_pileup_use_planes" if key == b"partitions" else "")
        assert pu._L.hm_pileup_set_option(pu._h, b"min_mapq", 0.0) == 0                  # the ones of any time still work
    finally:
        pu.close()


@pytest.mark.parametrize("how", ["n_seqs = 0", "negative length", "NULL bases"])
def test_a_failed_second_call_leaves_the_engine_as_it_was(how):
    """at depth b: the records and the pattern windows of job A are resident; the count and the fetches that follow give job A's
    result, which is that of an engine that was never called a second time"""
    family = "all"
    g, reads = R.job("A")
    key = ("depth b then counted", family)
    if key not in _CACHE:
        pu = _new(g, **R.FAMILIES[family][0])
        R.run_to(pu, "b", reads)
        pu.count([100, 128, 150])
        _CACHE[key] = {n: b for n, (b, _r) in _answers(pu, family).items()}
        pu.close()
    pu = _new(g, **R.FAMILIES[family][0])
    try:
        R.run_to(pu, "b", reads)
        n_recs = pu.num_records()
        lengths = pu.lengths.copy()
        bases = np.frombuffer("".join(s for _n, s in g).encode(), np.uint8)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        if how == "n_seqs = 0":
            args, text = (0, vp(lengths), vp(bases)), "hm_pileup_set_reference: bad argument"
        elif how == "NULL bases":
            args, text = (3, vp(lengths), None), "hm_pileup_set_reference: bad argument"
        else:
            lengths[1] = -1
            args, text = (3, vp(lengths), vp(bases)), "negative sequence length"
        assert pu._L.hm_pileup_set_reference(pu._h, *args) == HM_EINVAL and _err(pu) == text
        assert pu.num_records() == n_recs > 1000 and pu.n_loci == sum(len(s) for _n, s in g)
        n_loci = ctypes.c_int64(0)
        assert pu._L.hm_pileup_planes(pu._h, None, None, None, ctypes.byref(n_loci)) == 0 and n_loci.value == pu.n_loci
        pu.count([100, 128, 150])
        for name, (got, _r) in _answers(pu, family).items():
            assert got == _CACHE[key][name], name
    finally:
        pu.close()


def test_caller_planes_stay_registered_and_are_the_callers_to_zero():
    import torch
    g_a, reads_a = R.job("A")
    g_b, reads_b = R.job("same")
    n = sum(len(s) for _n, s in g_a)
    t = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(7)]
    pu = _new(g_a, partitions=True, planes=t[:3], partition_planes=(t[3:5], t[5:7]))
    want, want_thrs, *_ = _fresh("partitions", "same")
    try:
        R.run_to(pu, "d", reads_a)
        held = [x.clone() for x in t]
        rows_a = pu.loci().tobytes()
        pu.set_reference(g_b)
        assert all(torch.equal(x, y) for x, y in zip(t, held)) and all(x.any() for x in t[:2] + t[3:]), "the call touched the caller's planes"
        assert pu.loci().tobytes() == rows_a                                           # they still hold job A's counts
        for x in t:
            x.zero_()
        torch.cuda.synchronize()
        assert R.run_job(pu, reads_b) == want_thrs
        got = _answers(pu, "partitions")
        for name in want:
            assert got[name][0] == want[name][0], name
    finally:
        pu.close()


# ---- jobs on loaded rows ---------------------------------------------------------------------------------------------------------------
def _diff_job(pu, job):
    return [pu.load_loci(part, *R.load_rows(job, part - 1)) for part in (1, 2)]


def _diff_answers(pu):
    return S.blob((pu.loci(), pu.loci(partition=1), pu.loci(partition=2), pu.asm(min_cov=2)))


def _rows_of(ref_loci):
    from hifimeth_amd.pileup import LOCUS_DTYPE
    g, p, n, m = ref_loci
    want = np.zeros(len(g), LOCUS_DTYPE)
    want["gpos"], want["pcov"], want["ncov"], want["motif"] = g, p, n, m
    return want.tobytes()


def _fresh_diff():
    if "diff" not in _CACHE:
        pu = _new(R.load_genome(), partitions=True)
        returns = _diff_job(pu, "B")
        ref, ref_returns = R.diff_restated("B")
        assert returns == ref_returns
        for part in (0, 1, 2):
            assert pu.loci(partition=part).tobytes() == _rows_of(ref.loci(part)), part
        _CACHE["diff"] = returns, _diff_answers(pu)
        pu.close()
    return _CACHE["diff"]


@pytest.mark.parametrize("replanes", [False, True], ids=["", "partition planes registered again"])
def test_diff_loader_forgets_the_loci_of_job_a(replanes):
    """job A into both parts, then job B, half of whose loci job A gave to the same part: none is `given twice`; then duplicates
    inside job B: exactly k - 1 of k, in the engine's words"""
    import torch
    from hifimeth_amd.pileup import HifimethError
    want_returns, want = _fresh_diff()
    g = R.load_genome()
    t = [torch.zeros(R.TOTAL, dtype=torch.int32, device="cuda") for _ in range(4)] if replanes else None
    pu = _new(g, partitions=True, partition_planes=(t[:2], t[2:]) if replanes else None)
    try:
        assert min(_diff_job(pu, "A")) > 0
        pu.set_reference(g)
        if replanes:
            for x in t:
                x.zero_()
            torch.cuda.synchronize()
            for part in (1, 2):
                assert pu._L.hm_pileup_use_partition_planes(pu._h, part, *(ctypes.c_void_p(x.data_ptr()) for x in t[2 * part - 2:2 * part])) == 0
        assert _diff_job(pu, "B") == want_returns, _err(pu)
        assert _err(pu) == "" and _diff_answers(pu) == want
        pu.set_reference(g)                                                            # and once more: duplicates inside job B
        if replanes:
            for x in t:
                x.zero_()
            torch.cuda.synchronize()
        assert pu.load_loci(1, *R.load_rows("B", 0)) == want_returns[0]
        with pytest.raises(HifimethError):
            pu.load_loci(2, *R.duplicated(R.load_rows("B", 1), 3))
        assert _err(pu) == "hm_pileup_load_loci: 10 bad rows: 10 locus given twice for one part"
    finally:
        pu.close()


def _group_job(pu, job):
    indices, returns = [], []
    for k, g in enumerate(R.GROUP_SAMPLES[job]):
        indices.append(pu.begin_sample(g))
        returns.append(pu.load_sample_loci(*R.load_rows(job, k)))
    return indices, returns


def _group_answers(pu):
    return S.blob((pu.loci(), pu.loci(partition=1), pu.loci(partition=2), *pu.group_planes(1), *pu.group_planes(2), pu.group_tests(min_reps=1),
                   pu.group_tests(min_reps=2)))


GROUP_OPTIONS = dict(partitions=True, groups=True, group_min_cov=R.LOAD_MIN_COV)


def _fresh_groups():
    if "groups" not in _CACHE:
        import test_gpu_pileup_groups as TG
        pu = _new(R.load_genome(), **GROUP_OPTIONS)
        indices, returns = _group_job(pu, "B")
        ref, ref_indices, ref_returns = R.groups_restated("B")
        assert indices == ref_indices == [0, 0, 1, 1] and returns == ref_returns
        for part in (0, 1, 2):
            assert pu.loci(partition=part).tobytes() == _rows_of(ref.loci(part)), part
        for grp in (1, 2):
            moment, samples = pu.group_planes(grp)
            assert (moment == ref.moment[grp]).all() and (samples == ref.samples[grp]).all()
        for reps in (1, 2):
            assert TG._tuples(pu.group_tests(min_reps=reps)) == ref.tested(reps)
        _CACHE["groups"] = indices, returns, _group_answers(pu)
        pu.close()
    return _CACHE["groups"]


def test_groupdiff_restarts_its_samples():
    indices, returns, want = _fresh_groups()
    g = R.load_genome()
    pu = _new(g, **GROUP_OPTIONS)
    try:
        assert _group_job(pu, "A")[0] == [0, 1, 0, 1]
        pu.group_tests(min_reps=1)
        pu.set_reference(g)
        assert not pu.group_planes(1)[1].any() and not pu.group_planes(2)[0].any() and len(pu.loci()) == 0
        assert _group_job(pu, "B") == (indices, returns), _err(pu)
        assert _group_answers(pu) == want
    finally:
        pu.close()


def test_a_group_sample_after_a_diff_load_sees_no_locus_as_seen():
    """option groups on, a `diff` load grows the seen bitmap to two; the engine is re-targeted, a group sample is opened and loaded"""
    indices, returns, want = _fresh_groups()
    g = R.load_genome()
    pu = _new(g, **GROUP_OPTIONS)
    try:
        assert min(_diff_job(pu, "B")) > 0
        assert pu._L.hm_pileup_group_sample(pu._h, 1) == HM_ESTATE and _err(pu) == ONE_SOURCE
        pu.set_reference(g)
        assert _group_job(pu, "B") == (indices, returns), _err(pu)
        assert _group_answers(pu) == want
    finally:
        pu.close()


def _sample_job(pu, job):
    out = []
    for k in range(R.SAMPLES_OPENED[job]):
        assert pu.open_sample() == k
        out.append(pu.load_sample(*R.load_rows(job, k)))
    return out


def _sample_answers(pu):
    start, end = R.load_intervals()
    return S.blob((pu.loci(), *(pu.sample_plane(s) for s in range(R.SAMPLES_OPTION)), pu.sample_sums(), pu.sample_sums(complete=True),
                   *(pu.sample_intervals(start, end, c) for c in range(3))))


def test_samplecorr_and_regiondiff_count_the_samples_opened_since():
    import intervals_ref as I
    from hifimeth_amd.pileup import SAMPLE_PAIR_DTYPE
    g = R.load_genome()
    options = dict(samples=R.SAMPLES_OPTION, sample_min_cov=R.LOAD_MIN_COV)
    fresh = _new(g, **options)
    pu = _new(g, **options)
    try:
        ref, ref_returns = R.samples_restated("B")
        assert _sample_job(fresh, "B") == ref_returns
        want = _sample_answers(fresh)
        for s in range(R.SAMPLES_OPTION):
            assert (fresh.sample_plane(s) == ref.level[s]).all(), s
        sums = fresh.sample_sums()
        assert [tuple(int(e[f]) for f in SAMPLE_PAIR_DTYPE.names if f != "reserved") for e in sums] == ref.sums() and len(sums) == 9
        start, end = R.load_intervals()
        for c in range(3):
            iv = fresh.sample_intervals(start, end, c)
            assert iv.shape == (len(start), 2, 2) and (iv == I.interval_sums(ref, start, end, c)).all()
        assert len(_sample_job(pu, "A")) == 3
        pu.sample_sums()
        pu.sample_intervals(start, end, 0)
        pu.set_reference(g)
        assert len(pu.sample_sums()) == 0 and not pu.sample_plane(2).any()
        assert _sample_job(pu, "B") == ref_returns, _err(pu)
        assert _sample_answers(pu) == want
    finally:
        fresh.close()
        pu.close()


# ---- the three flags of "counts come from one source" -----------------------------------------------------------------------------------
def _submit(pu, read):
    from hifimeth_amd.pileup import parse_mods
    mods = parse_mods(read.seq, read.flag, read.mm, read.ml)
    seq4, cig = np.ascontiguousarray(read.seq4, np.uint8), np.ascontiguousarray(read.cigar_u32(), np.uint32)
    return pu._L.hm_pileup_submit_read(pu._h, 0, read.flag, read.tid, read.pos, read.mapq, len(read.seq), seq4.ctypes.data_as(ctypes.c_void_p),
                                       len(cig), cig.ctypes.data_as(ctypes.c_void_p), len(mods), mods.ctypes.data_as(ctypes.c_void_p))


def _load_code(pu, part, rows):
    from hifimeth_amd.pileup import LOCUS_DTYPE
    a = np.zeros(len(rows[0]), LOCUS_DTYPE)
    a["gpos"], a["pcov"], a["ncov"], a["motif"] = rows
    return pu._L.hm_pileup_load_loci(pu._h, part, a.ctypes.data_as(ctypes.c_void_p), len(a))


def test_an_engine_that_staged_a_record_loads_after_the_call():
    want_returns, want = _fresh_diff()
    g, reads = R.job("A")
    some = ([10], [3], [1], [0])
    pu = _new(g, partitions=True)
    try:
        assert _submit(pu, reads[0]) == 1
        assert _load_code(pu, 1, some) == HM_ESTATE and _err(pu) == STAGED           # without the call the refusal holds
        pu.flush()
        pu.count([128, 128, 128])
        assert _load_code(pu, 1, some) == HM_ESTATE and _err(pu) == STAGED
        pu.set_reference(R.load_genome())
        assert _diff_job(pu, "B") == want_returns, _err(pu)
        assert _diff_answers(pu) == want
    finally:
        pu.close()


def test_an_engine_that_loaded_takes_records_and_group_samples_after_the_call():
    g_b, reads_b = R.job("same")
    want, want_thrs, *_ = _fresh("partitions", "same")
    pu = _new(R.load_genome(), **GROUP_OPTIONS)
    try:
        assert min(_diff_job(pu, "A")) > 0
        assert _submit(pu, reads_b[0]) == HM_ESTATE and _err(pu) == LOADED           # without the call the refusals hold
        assert pu._L.hm_pileup_group_sample(pu._h, 2) == HM_ESTATE and _err(pu) == ONE_SOURCE
        pu.set_reference(R.load_genome())
        assert pu.begin_sample(2) == 0 and pu.load_sample_loci(*R.load_rows("B", 0)) == R.groups_restated("B")[2][0]
        pu.set_reference(g_b)
        assert R.run_job(pu, reads_b) == want_thrs
        got = _answers(pu, "partitions")
        for name in want:
            assert got[name][0] == want[name][0], name
    finally:
        pu.close()


def test_an_engine_voided_by_a_bad_row_is_whole_after_the_call():
    want_returns, want = _fresh_diff()
    g = R.load_genome()
    pu = _new(g, partitions=True)
    try:
        assert _load_code(pu, 1, R.load_rows("A", 0)) > 0
        assert _load_code(pu, 2, ([5, R.TOTAL], [1, 1], [1, 1], [0, 0])) == HM_EDATA
        assert _err(pu) == "hm_pileup_load_loci: 1 bad rows: 1 gpos outside the reference"
        assert _load_code(pu, 2, ([7], [1], [1], [0])) == HM_ESTATE and _err(pu) == "hm_pileup_load_loci: " + VOID   # without the call
        assert pu._L.hm_pileup_fetch_loci(pu._h, None, None, None, 0, 0, R.TOTAL, None, 0) == HM_ESTATE and _err(pu) == VOID
        pu.set_reference(g)
        assert _err(pu) == ""
        assert _diff_job(pu, "B") == want_returns, _err(pu)
        assert _diff_answers(pu) == want
    finally:
        pu.close()
