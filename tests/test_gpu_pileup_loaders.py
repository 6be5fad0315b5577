"""The three loaders of `diff`, `groupdiff` and `samplecorr` held to each other: they share one kernel and one host loop, and the files
of the three commands each look at one loader only.  The same rows go through hm_pileup_load_loci, hm_pileup_load_sample_loci and
hm_sample_load and must leave the same combined planes and the same count; every loader's counters are checked against known
multiplicities placed in chosen wavefronts; the 2^20 limit must hold for the two loaders that have it and not for `diff`.

Everything is compared exactly: the planes byte for byte, the messages as the literals the engine has written since each loader was
added.  The restatements are the existing ones (diff_ref.Loader, groups_ref.GroupLoader, samples_ref.SampleLoader).

The reference has three contigs of 9877 bases together: the 2 * 4096 + 70 rows sit on distinct loci, so it cannot be shorter than
that."""
import functools

import numpy as np
import pytest

from diff_ref import Loader
from groups_ref import GroupLoader
from samples_ref import BELOW, SampleLoader
from test_gpu_pileup_diff import _load as _load_part
from test_gpu_pileup_groups import _begin, _load as _load_group
from test_gpu_pileup_samples import _open, _load as _load_sample

pytestmark = pytest.mark.gpu

HM_EDATA, HM_ESTATE = -4, -5
LENGTHS = (4099, 3001, 2777)
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)])
TOTAL = int(OFFSETS[-1])
ENDS = [int(x) for s in range(3) for x in (OFFSETS[s], OFFSETS[s + 1] - 1)]
N_ROWS = 2 * 4096 + 70                                        # 33 workgroups of 256 threads, the last wavefront holds 6 rows
WAVE, GROUP = 64, 256                                         # row i of a launch is thread i: wavefront i // 64 of workgroup i // 256
LIMIT = 1 << 20
VOID = b": a load of this engine met bad rows (hm_pileup_load_loci): its planes mean nothing"
LOADERS = ("diff", "groupdiff", "samplecorr")
WHO = {"diff": b"hm_pileup_load_loci", "groupdiff": b"hm_pileup_load_sample_loci", "samplecorr": b"hm_sample_load"}


@functools.lru_cache(maxsize=None)
def _rows():
    """N_ROWS rows on distinct loci in shuffled order, the contig ends among them: coverage 1 .. 12, one row in sixteen without a
    count, motif 0 .. 3"""
    rng = np.random.default_rng(20)
    g = np.concatenate([ENDS, rng.choice(np.setdiff1d(np.arange(TOTAL), ENDS), N_ROWS - len(ENDS), replace=False)]).astype(np.int64)
    cov = rng.integers(1, 13, N_ROWS)
    cov[rng.random(N_ROWS) < 0.0625] = 0
    p = rng.binomial(cov, rng.random(N_ROWS))
    m = rng.integers(0, 4, N_ROWS)
    order = rng.permutation(N_ROWS)
    out = tuple(x[order] for x in (g, p, cov - p, m))
    for x in out:
        x.setflags(write=False)
    return out


def _genome():
    rng = np.random.default_rng(3)
    return [("ctg%d" % (s + 1), "".join(rng.choice(list("ACGT"), n))) for s, n in enumerate(LENGTHS)]


def _engine(loader, planes=False, slab=None):
    """an engine of the loader's command with minimum coverage 1 and its sample open -> (engine, load(rows) -> the call's return
    value, the caller's plane tensors pcov, ncov, key, ... or None)"""
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    t = [torch.zeros(TOTAL, dtype=torch.int32, device="cuda") for _ in range(3 if loader == "samplecorr" else 7)] if planes else None
    kw = {} if t is None else dict(planes=t[:3]) if loader == "samplecorr" else dict(planes=t[:3], partition_planes=(t[3:5], t[5:7]))
    if loader == "diff":
        pu = MethylationPileup(_genome(), partitions=True, **kw)
        call = lambda pu, rows: _load_part(pu, 1, rows)
    elif loader == "groupdiff":
        pu = MethylationPileup(_genome(), partitions=True, groups=True, group_min_cov=1, **kw)
        assert _begin(pu, 1) == 0
        call = _load_group
    else:
        pu = MethylationPileup(_genome(), samples=2, sample_min_cov=1, **kw)
        assert _open(pu) == 0
        call = _load_sample
    if slab is not None:
        assert pu._L.hm_pileup_set_option(pu._h, b"load_slab", float(slab)) == 0
    return pu, functools.partial(call, pu), t


def _restatement(loader):
    """the loader's restatement in the state of _engine's engine -> (it, load(rows))"""
    if loader == "diff":
        ref = Loader(TOTAL)
        return ref, lambda rows: ref.load(1, *rows)
    ref = GroupLoader(TOTAL, 1) if loader == "groupdiff" else SampleLoader(TOTAL, 2, 1)
    assert (ref.begin_sample(1) if loader == "groupdiff" else ref.open()) == 0
    return ref, lambda rows: ref.load(*rows)


@functools.lru_cache(maxsize=None)
def _loaded_restatements():
    """the three restatements after _rows(), and what each returned: built once, only read afterwards"""
    out = {}
    for loader in LOADERS:
        ref, load = _restatement(loader)
        out[loader] = (ref, load(_rows()))
    return out


def _err(pu):
    return pu._L.hm_pileup_last_error(pu._h)


# ---- 1. the same rows through the three loaders ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", [None, 64, N_ROWS], ids=["default slab", "slabs of 64", "one slab of n"])
def test_same_rows_three_loaders(slab):
    """slabs of 64: 130 launches of one wavefront each, the last of 6 rows; a slab of n rows: one launch, as with the default"""
    rows = _rows()
    want = int((rows[1] + rows[2] > 0).sum())
    assert N_ROWS % WAVE and N_ROWS > GROUP and 0 < want < N_ROWS and len(np.unique(rows[0])) == N_ROWS
    refs = _loaded_restatements()
    engines = {loader: _engine(loader, planes=True, slab=slab) for loader in LOADERS}
    try:
        got = {loader: load(rows) for loader, (_pu, load, _t) in engines.items()}
        print(got, {loader: r for loader, (_ref, r) in refs.items()})
        assert got == dict.fromkeys(LOADERS, want) and all(r == want for _ref, r in refs.values())
        planes = {loader: [x.cpu().numpy() for x in t] for loader, (_pu, _load, t) in engines.items()}
        for k, name in enumerate(("pcov", "ncov", "key")):
            assert planes["diff"][k].tobytes() == planes["groupdiff"][k].tobytes() == planes["samplecorr"][k].tobytes(), name
            for loader in LOADERS:
                assert (planes[loader][k].astype(np.int64) == refs[loader][0].planes[name]).all(), (loader, name)
        assert planes["diff"][0].any() and planes["diff"][1].any() and planes["diff"][2].any()
        # what each loader keeps beside the combined planes
        for loader in ("diff", "groupdiff"):
            for k, name in enumerate(("pcov1", "ncov1", "pcov2", "ncov2"), 3):
                assert (planes[loader][k].astype(np.int64) == refs[loader][0].planes[name]).all(), (loader, name)
            assert planes[loader][3].tobytes() == planes[loader][0].tobytes() and not planes[loader][5].any()
        moment, samples = engines["groupdiff"][0].group_planes(1)
        assert (moment == refs["groupdiff"][0].moment[1]).all() and (samples == refs["groupdiff"][0].samples[1]).all()
        assert int(samples.sum()) == want and not engines["groupdiff"][0].group_planes(2)[1].any()
        level = engines["samplecorr"][0].sample_plane(0)
        assert (level == refs["samplecorr"][0].level[0]).all() and int((level != 0).sum()) == want and not (level == BELOW).any()
        assert not engines["samplecorr"][0].sample_plane(1).any()
    finally:
        for pu, _load, _t in engines.values():
            pu.close()


# ---- 2. the counters -----------------------------------------------------------------------------------------------------------------
# rows of each kind and where they stand in the call: gpos 2, negative 3, above the limit 5 (not for `diff`), motif 7, twice 11
KIND_ROWS = {"gpos": 2, "negative": 3, "big": 5, "motif": 7, "twice": 11}
MESSAGE = {
    "diff": b"hm_pileup_load_loci: 23 bad rows: 2 gpos outside the reference, 3 negative count, 7 motif above 3, 11 locus given twice for one part",
    "groupdiff": b"hm_pileup_load_sample_loci: 28 bad rows: 2 gpos outside the reference, 3 negative count, 5 count above 2^20 - 1, 7 motif above 3, "
                 b"11 locus given twice in one sample",
    "samplecorr": b"hm_sample_load: 28 bad rows: 2 gpos outside the reference, 3 negative count, 5 count above 2^20 - 1, 7 motif above 3, "
                  b"11 locus given twice in one sample",
}


def _call_with_bad_rows(loader):
    """_rows() with the bad rows of KIND_ROWS put in between -> (rows, {kind: indices in the call}).  A bad row also fails every later
    check: the first failure names it.  The k rows of a kind stand in k different workgroups; the last motif row and the last
    duplicate stand at the end of the call, in its partial wavefront.  A duplicate and the row it repeats carry the same one
    of the two counts: `diff` knows a duplicate by the old values of its two adds, so of two rows of one locus that run at the same
    time in two wavefronts both see the other if both carry both counts, and neither need if one is (0, n) and the other (p, 0); with
    one common count exactly one does, as in the restatement."""
    g, p, n, m = (x.copy() for x in _rows())
    kinds = [k for k in KIND_ROWS if not (k == "big" and loader == "diff")]
    total = N_ROWS + sum(KIND_ROWS[k] for k in kinds)
    only_p, only_n = np.flatnonzero((p > 0) & (n == 0)), np.flatnonzero((p == 0) & (n > 0))
    where, bad = {}, {}
    for a, kind in enumerate(kinds):
        count = KIND_ROWS[kind]
        where[kind] = [3 + 70 * a + (2 * GROUP + WAVE + 1) * j for j in range(count)]
        if kind in ("motif", "twice"):
            where[kind][-1] = total - (2 if kind == "motif" else 1)
        again = np.concatenate([g[only_p[20 * np.arange(6)]], g[only_n[20 * np.arange(5)]]])[:count]
        bad[kind] = {"gpos": ([-1, TOTAL][:count], [-1] * count, [1] * count, [9] * count),
                     "negative": ([5] * count, [-1, 1, -7][:count], [1, -2, -7][:count], [4] * count),
                     "big": ([6] * count, [LIMIT, 0, LIMIT - 1, 2 ** 31 - 1, 1 << 19][:count], [0, LIMIT, 1, 2 ** 31 - 1, 1 << 19][:count], [4] * count),
                     "motif": ([7] * count, [1] * count, [1] * count, [4, 5, 6, 7, 255, 2 ** 31, 2 ** 32 - 1][:count]),
                     "twice": (again, [1, 2, 3, 1, 2, 3, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1, 2, 3, 1, 2], [0] * count)}[kind]
    at = np.concatenate([where[k] for k in kinds])
    assert len(np.unique(at)) == len(at) and at.max() == total - 1
    out = [np.zeros(total, np.int64) for _ in range(4)]
    rest = np.setdiff1d(np.arange(total), at)
    for x, base in zip(out, (g, p, n, m)):
        x[rest] = base
    for kind in kinds:
        for x, v in zip(out, bad[kind]):
            x[where[kind]] = v
    return tuple(out), where


@pytest.mark.parametrize("loader", LOADERS)
def test_counters(loader):
    rows, where = _call_with_bad_rows(loader)
    total = len(rows[0])
    assert total % WAVE                                       # the launch ends in a partial wavefront
    for kind, at in where.items():
        assert len(at) == KIND_ROWS[kind] and len({i // WAVE for i in at}) >= 2 and len({i // GROUP for i in at}) == len(at), kind
    assert all(where[k][-1] >= total // WAVE * WAVE for k in ("motif", "twice"))
    ref, ref_load = _restatement(loader)
    assert ref_load(rows) == HM_EDATA
    print(loader, ref.bad)
    assert list(ref.bad.values()) == [KIND_ROWS[k] for k in where]
    pu, load, _none = _engine(loader)
    try:
        assert load(rows) == HM_EDATA
        print(_err(pu))
        assert _err(pu) == MESSAGE[loader]
        good = ([100], [1], [1], [0])
        assert load(good) == HM_ESTATE and _err(pu) == WHO[loader] + VOID
    finally:
        pu.close()


# ---- 3. the limit of 2^20 ------------------------------------------------------------------------------------------------------------
UNDER = ([10], [LIMIT - 1], [0], [0])                            # the largest count a sample may hold
OVER = ([20, 30, 40, 50], [1 << 19, 0, LIMIT - 1, 2 ** 31 - 1], [1 << 19, LIMIT, 1, 2 ** 31 - 1], [0, 1, 2, 3])    # the last sums to 2^32 - 2


@pytest.mark.parametrize("loader", LOADERS)
def test_count_limit(loader):
    pu, load, _none = _engine(loader)
    ref, ref_load = _restatement(loader)
    try:
        assert load(UNDER) == ref_load(UNDER) == 1
        if loader == "diff":
            from hifimeth_amd.pileup import LOCUS_DTYPE
            assert load(OVER) == ref_load(OVER) == 4
            g, p, n, m = ref.loci(1)
            want = np.zeros(len(g), LOCUS_DTYPE)
            want["gpos"], want["pcov"], want["ncov"], want["motif"] = g, p, n, m
            assert want["gpos"].tolist() == [10, 20, 30, 40, 50] and want["pcov"].tolist()[-1] == 2 ** 31 - 1
            assert pu.loci(partition=1).tobytes() == want.tobytes() == pu.loci().tobytes()
        else:
            assert ref_load(OVER) == HM_EDATA and load(OVER) == HM_EDATA
            assert _err(pu) == WHO[loader] + b": 4 bad rows: 4 count above 2^20 - 1"
            assert load(UNDER) == HM_ESTATE and _err(pu) == WHO[loader] + VOID
    finally:
        pu.close()
