"""`samplecorr` on the device, through the C ABI via the Python binding, against samples_ref.py: the level planes element for element,
every uint64 of hm_sample_fetch_sums exactly (both modes, ranges aligned to nothing, additivity, 2 .. 64 samples), the
accumulators at 2^47, a reference past 2^32, every error and state rule, hm_sample_corr against Python integers, and the command
against the Python path byte for byte.

The one floating-point bar, 1e-12 absolute on r, is derived: num, va and vb are exact integers on both sides, and what remains is
three conversions, two square roots, a product and a quotient in double on a value of magnitude <= 1, a few 1e-16."""
import ctypes
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

import bigref as R
import samples_ref as S
from samples_ref import HM_EDATA, HM_EINVAL, HM_ESTATE, LENGTHS, OFFSETS, TOTAL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
FIELDS = ("i", "j", "ctx", "n", "si", "sj", "sii", "sjj", "sij")


def _genome(seed=3):
    rng = np.random.default_rng(seed)
    return [("ctg%d" % (s + 1), "".join(rng.choice(list("ACGT"), n))) for s, n in enumerate(LENGTHS)]


def _engine(n=3, min_cov=S.MIN_COV, genome=None, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    return MethylationPileup(genome or _genome(), samples=n, sample_min_cov=min_cov, **kw)


def _tile():
    from hifimeth_amd.pileup import sample_geometry
    tile, most = sample_geometry()
    assert most == S.MAX_SAMPLES and tile >= 1
    return tile


def _open(pu):
    return pu._L.hm_sample_open(pu._h)


def _load(pu, rows):
    """hm_sample_load on (gpos, pcov, ncov, motif) without the wrapper's exception -> its return value"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    buf = np.zeros(len(rows[0]), LOCUS_DTYPE)
    buf["gpos"], buf["pcov"], buf["ncov"], buf["motif"] = rows
    return pu._L.hm_sample_load(pu._h, buf.ctypes.data_as(ctypes.c_void_p), len(buf))


def _sums(pu, lo, hi, complete, out=None):
    from hifimeth_amd.pileup import SAMPLE_PAIR_DTYPE
    out = np.zeros(3 * 2080, SAMPLE_PAIR_DTYPE) if out is None else out
    return pu._L.hm_sample_fetch_sums(pu._h, lo, hi, complete, out.ctypes.data_as(ctypes.c_void_p))


def _tuples(entries):
    assert not entries["reserved"].any()
    return [tuple(int(e[f]) for f in FIELDS) for e in entries]


def _err(pu):
    return pu._L.hm_pileup_last_error(pu._h)


# ---- 1. the planes ----------------------------------------------------------------------------------------------------------------------
def test_planes_equal_the_restatement_in_any_order_and_slab():
    """three samples on the three-sequence reference, loci at position 0, at the last base and on both sides of every sequence
    boundary; rows in file (ascending) order, shuffled, and shuffled through slabs of 7 rows"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    data = S.dataset(3, _tile())
    ref = S.loaded(3, _tile())
    for rows in data:
        assert set(S.ENDS) <= set(rows[0].tolist())
    g, p, n, m = ref.loci()
    want = np.zeros(len(g), LOCUS_DTYPE)
    want["gpos"], want["pcov"], want["ncov"], want["motif"] = g, p, n, m
    seen = []
    for how in ("file order", "shuffled", "slab of 7"):
        pu = _engine(3)
        try:
            if how == "slab of 7":
                assert pu._L.hm_pileup_set_option(pu._h, b"load_slab", 7.0) == 0
            for s, rows in enumerate(data):
                if how == "file order":
                    order = np.argsort(rows[0])
                    rows = tuple(x[order] for x in rows)
                assert pu.open_sample() == s
                cut = len(rows[0]) // 3
                assert pu.load_sample(*(x[:cut] for x in rows)) + pu.load_sample(*(x[cut:] for x in rows)) == len(rows[0])
            planes = [pu.sample_plane(s) for s in range(3)]
            for s in range(3):
                assert planes[s].dtype == np.uint16 and (planes[s] == ref.level[s]).all(), (how, s)
                lo, hi = int(OFFSETS[1]) - 3, int(OFFSETS[2]) + 5
                assert (pu.sample_plane(s, lo, hi) == ref.level[s, lo:hi]).all()
            assert any((x == S.BELOW).any() for x in planes) and len(pu.sample_plane(1, 9, 9)) == 0
            loci = pu.loci()
            assert loci.tobytes() == want.tobytes(), how
            seen.append((b"".join(x.tobytes() for x in planes), loci.tobytes()))
        finally:
            pu.close()
    assert seen[0] == seen[1] == seen[2]


# ---- 2. the sums ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[2, 3, 17, 23, 64])
def loaded(request):
    """N = 17 passes a multiple of 16, 23 is the first N with more than 256 pairs, 64 is the cap: 2080 pairs per context"""
    n = request.param
    pu = _engine(n)
    for s, rows in enumerate(S.dataset(n, _tile())):
        assert pu.open_sample() == s
        assert pu.load_sample(*rows) == len(rows[0])
    yield n, pu, S.loaded(n, _tile())
    pu.close()


@pytest.mark.parametrize("complete", [False, True])
def test_sums_equal_the_restatement(loaded, complete):
    n, pu, ref = loaded
    tile = _tile()
    full = pu.sample_sums(complete=complete)
    want = ref.sums(complete=complete)
    assert len(full) == 3 * n * (n + 1) // 2 and _tuples(full) == want
    # loci in all three contexts and coverage on both sides of the minimum: every pair of every context has loci
    assert min(e[3] for e in want) >= 20 and (ref.level == S.BELOW).any()
    for lo, hi in ((tile - 1, tile + 1), (tile, 7 * tile), (7 * tile - 1, 7 * tile + 2), (1237, TOTAL - 3), (0, 1), (TOTAL - 1, TOTAL), (333, 333)):
        assert _tuples(pu.sample_sums(lo, hi, complete)) == ref.sums(lo, hi, complete), (lo, hi)
    assert all(e[3:] == (0,) * 6 for e in _tuples(pu.sample_sums(333, 333, complete)))
    lo, hi = 1237, TOTAL - 3                                  # additivity: a split on a tile boundary, one inside a tile, one on a sequence boundary
    total = np.array([e[3:] for e in _tuples(pu.sample_sums(lo, hi, complete))], object)
    for m in (7 * tile, 7 * tile + 101, int(OFFSETS[2])):
        a, b = (np.array([e[3:] for e in _tuples(pu.sample_sums(x, y, complete))], object) for x, y in ((lo, m), (m, hi)))
        assert (a + b == total).all(), m


def test_complete_differs_from_pairwise(loaded):
    n, pu, ref = loaded
    g = S.ALL_BUT_ONE                                         # all but the last sample count there
    c = min(int(ref.planes["key"][g]) & 3, 2)
    pairwise, complete = (_tuples(pu.sample_sums(g, g + 1, k)) for k in (False, True))
    assert [e[3] for e in pairwise if e[2] == c] == [1 if j < n - 1 else 0 for i in range(n) for j in range(i, n)]
    assert all(e[3] == 0 for e in complete)
    assert _tuples(pu.sample_sums(complete=True)) != _tuples(pu.sample_sums(complete=False))


@pytest.mark.parametrize("n,opened", [(3, 2), (23, 17), (5, 0)])
def test_a_fetch_after_m_of_n_samples_gives_the_m_table(n, opened):
    pu = _engine(n)
    try:
        for rows in S.dataset(n, _tile())[:opened]:
            pu.open_sample()
            pu.load_sample(*rows)
        ref = S.loaded(n, _tile(), opened=opened)
        for complete in (False, True):
            got = pu.sample_sums(complete=complete)
            assert len(got) == 3 * opened * (opened + 1) // 2 and _tuples(got) == ref.sums(complete=complete)
        assert not pu.sample_plane(n - 1).any()
    finally:
        pu.close()


def test_fetches_in_any_order_repeated_and_interleaved():
    """what tests/sequence_cases.py asks of every reader of the engine, for the sample readers on a samples-fed engine: each fetch
    on an engine of its own that is asked nothing else, then all of them on one engine in two shuffled orders with repeats, the
    other fetches over the combined planes between them; every answer byte for byte the same"""
    n, tile = 5, _tile()
    cut = (int(OFFSETS[1]) - 200, int(OFFSETS[1]) + 300)
    readers = {"sums": lambda pu: pu.sample_sums(), "sums complete": lambda pu: pu.sample_sums(complete=True),
               "sums cut": lambda pu: pu.sample_sums(*cut), "sums cut complete": lambda pu: pu.sample_sums(*cut, complete=True),
               "sums inside a tile": lambda pu: pu.sample_sums(7 * tile + 3, 7 * tile + 90), "plane": lambda pu: pu.sample_plane(n - 1),
               "plane cut": lambda pu: pu.sample_plane(0, *cut), "loci": lambda pu: pu.loci(), "loci cut": lambda pu: pu.loci(*cut)}

    def fed():
        pu = _engine(n)
        for rows in S.dataset(n, tile):
            pu.open_sample()
            pu.load_sample(*rows)
        return pu
    fresh = {}
    for name, fn in readers.items():
        pu = fed()
        try:
            fresh[name] = fn(pu).tobytes()
        finally:
            pu.close()
    assert len(set(fresh.values())) == len(fresh)
    pu = fed()
    try:
        for seed in (1, 2):
            rng = np.random.default_rng(seed)
            for name in rng.permutation(list(readers) * 3):
                assert readers[name](pu).tobytes() == fresh[name], (seed, name)
    finally:
        pu.close()


# ---- 3. magnitude -----------------------------------------------------------------------------------------------------------------------
def test_accumulators_are_64_bit_end_to_end():
    """2^17 loci with k = n in both samples: u = 32768 everywhere, sii = 2^17 x 2^30 = 2^47"""
    from hifimeth_amd.pileup import MethylationPileup
    count = 1 << 17
    total = count + 5
    pu = MethylationPileup([("c", total)], samples=2, bases=np.full(total, ord("C"), np.uint8))
    try:
        g = np.arange(count) + 3
        for s in range(2):
            assert pu.open_sample() == s and pu.load_sample(g, np.full(count, 7 + s), np.zeros(count, np.int64), 0) == count
        e = _tuples(pu.sample_sums())
        assert e[:3] == [(i, j, 0, count, count << 15, count << 15, 1 << 47, 1 << 47, 1 << 47) for i, j in ((0, 0), (0, 1), (1, 1))]
        assert all(x[3:] == (0,) * 6 for x in e[3:])
        assert (pu.sample_plane(1, 3, 3 + count) == 32769).all() and not pu.sample_plane(1, 0, 3).any()
    finally:
        pu.close()


# ---- 4. a reference past 2^32 bases --------------------------------------------------------------------------------------------------
def test_samples_around_two_to_the_32():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    total = R.HOST_LEN[R.B32]
    lengths = [R.B31, R.B31, total - R.B32]                   # 2^31 - 1 and 2^32 - 1 are the last bases of the first two contigs
    need = total * (1 + 4 * 3 + 2 * 2) + (1 << 30)            # the bases, the three combined planes, two level planes
    free, _all = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip("the card has %.1f GB free, the case needs %.1f GB plus 8 GB" % (free / 1e9, need / 1e9))
    loci = [5, R.B31 - 1, R.B31, R.B32 - 1, R.B32, R.B32 + 5]
    counts = [([9, 1, 30, 4, 0, 12], [1, 9, 2, 6, 8, 0]), ([7, 3, 20, 1, 5, 2], [2, 9, 9, 2, 5, 9])]      # (pcov, ncov) per sample: the fourth locus is below 5 in sample 1
    pu = MethylationPileup([("c%d" % k, n) for k, n in enumerate(lengths)], samples=2, bases=np.full(total, ord("N"), np.uint8))
    try:
        assert pu.n_loci == total > R.B32
        for s, (p, n) in enumerate(counts):
            assert pu.open_sample() == s and pu.load_sample(loci[::-1], p[::-1], n[::-1], 0) == 6
        stored = [[S.level(p, p + n) + 1 if p + n >= 5 else S.BELOW for p, n in zip(*c)] for c in counts]
        for s in range(2):
            for k, g in enumerate(loci):
                lo = max(g - 2, 0)
                want = np.zeros(min(g + 3, total) - lo, np.uint16)
                for kk, gg in enumerate(loci):
                    if lo <= gg < lo + len(want):
                        want[gg - lo] = stored[s][kk]
                assert (pu.sample_plane(s, lo, lo + len(want)) == want).all(), (s, g)

        def sums(lo, hi):
            inside = [(v, w) for g, v, w in zip(loci, *stored) if lo <= g < hi]
            own = [[x[s] - 1 for x in inside if x[s] != S.BELOW] for s in (0, 1)]
            both = [(v - 1, w - 1) for v, w in inside if v != S.BELOW and w != S.BELOW]
            return [(0, 0, 0, len(own[0]), sum(own[0]), sum(own[0]), *(sum(a * a for a in own[0]),) * 3),
                    (0, 1, 0, len(both), sum(a for a, _ in both), sum(b for _, b in both), sum(a * a for a, _ in both), sum(b * b for _, b in both),
                     sum(a * b for a, b in both)),
                    (1, 1, 0, len(own[1]), sum(own[1]), sum(own[1]), *(sum(b * b for b in own[1]),) * 3)]
        for lo, hi in ((0, total), (0, R.B31), (R.B31, R.B32), (R.B32, total), (R.B31 - 1, R.B32 + 1), (R.B32 - 1, R.B32)):
            assert _tuples(pu.sample_sums(lo, hi))[:3] == sums(lo, hi), (lo, hi)
        assert sums(0, total)[1][3] == 5 and sums(0, total)[0][3] == 6
        assert [e[3] for e in _tuples(pu.sample_sums(complete=True))[:3]] == [5, 5, 5]
        assert pu.loci()["gpos"].tolist() == loci
        assert _load(pu, ([total], [5], [5], [0])) == HM_EDATA                # the bound is the 64-bit length
    finally:
        pu.close()
        torch.cuda.empty_cache()


# ---- 5. errors and state ------------------------------------------------------------------------------------------------------------------
BAD = {"gpos -1": (([7, -1], [5, 5], [5, 5], [0, 0]), b"1 gpos outside"), "gpos = total": (([TOTAL, 3], [5, 5], [5, 5], [0, 0]), b"1 gpos outside"),
       "negative count": (([5, 6, 7], [9, 9, -1], [-3, 0, 9], [0, 0, 0]), b"2 negative count"),
       "a count of 2^20": (([5, 6], [1 << 20, (1 << 20) - 1], [0, 0], [0, 0]), b"1 count above 2^20 - 1"),
       "the sum reaches 2^20": (([5], [1 << 19], [1 << 19], [0]), b"1 count above 2^20 - 1"),
       "negative before large": (([5], [-1], [1 << 21], [7]), b"1 negative count"), "large before motif": (([5], [1 << 20], [0], [7]), b"1 count above"),
       "motif 4": (([5], [5], [5], [4]), b"1 motif above 3"),
       "two rows of one locus in one slab": (([9, 5, 9, 9], [5, 5, 0, 5], [0, 5, 0, 0], [0, 0, 0, 0]), b"1 locus given twice in one sample"),
       "duplicate of a counting row": (([4], [0], [9], [1]), b"1 locus given twice in one sample"),
       "duplicate of a row below the coverage": (([2000], [7], [7], [1]), b"1 locus given twice in one sample")}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_rows_void_the_engine(what):
    from hifimeth_amd.caller import HifimethError
    rows, text = BAD[what]
    first = ([4, 2000], [5, 1], [0, 1], [0, 2])               # 2000 has two calls: seen, below the coverage
    pu = _engine(3)
    ref = S.SampleLoader(TOTAL, 3)
    try:
        assert _open(pu) == 0 and ref.open() == 0
        assert _load(pu, first) == 2 and ref.load(*first) == 2
        assert ref.load(*rows) == HM_EDATA and _load(pu, rows) == HM_EDATA
        err = _err(pu)
        assert text in err and (b"%d bad rows" % sum(ref.bad.values())) in err, err
        good = ([100], [5], [5], [0])
        assert _load(pu, good) == HM_ESTATE and _open(pu) == HM_ESTATE and _sums(pu, 0, TOTAL, 0) == HM_ESTATE
        assert pu._L.hm_sample_plane(pu._h, 0, 0, 4, np.zeros(4, np.uint16).ctypes.data_as(ctypes.c_void_p)) == HM_ESTATE
        assert pu._L.hm_pileup_fetch_loci(pu._h, None, None, None, 0, 0, TOTAL, None, 0) == HM_ESTATE
        with pytest.raises(HifimethError):
            pu.load_sample(*good)
    finally:
        pu.close()


def test_two_rows_of_one_locus_in_one_slab_give_one_value_and_one_duplicate():
    """in either order: the stored value is that of one of the two rows, the other is the duplicate"""
    for order in ((0, 1), (1, 0)):
        pu = _engine(2)
        try:
            rows = tuple(np.array(x)[list(order)] for x in ([77, 77], [9, 1], [1, 1], [0, 0]))     # 9 / 10 counts, 1 / 2 is below the coverage
            assert _open(pu) == 0 and _load(pu, rows) == HM_EDATA and b"1 bad rows: 1 locus given twice" in _err(pu)
        finally:
            pu.close()
        pu = _engine(2)
        try:
            assert _open(pu) == 0 and _load(pu, ([77], [9], [1], [0])) == 1 and int(pu.sample_plane(0, 77, 78)[0]) == S.level(9, 10) + 1
            assert int(pu.sample_plane(0, 76, 77)[0]) == 0 and _load(pu, ([76], [1], [1], [0])) == 1      # the neighbour in the same 32-bit word
            assert pu.sample_plane(0, 76, 78).tolist() == [S.BELOW, S.level(9, 10) + 1]
        finally:
            pu.close()


def test_state_errors():
    from hifimeth_amd.caller import HifimethError
    from hifimeth_amd.pileup import LOCUS_DTYPE, MethylationPileup
    from hifimeth_amd.synth import synth_alignments
    from test_gpu_pileup_diff import _submit
    genome = _genome()
    read = next(r for r in synth_alignments(genome, 20, seed=4, median_len=600) if not r.flag & 4 and r.mm)
    good = ([100], [5], [5], [0])
    buf = np.zeros(1, LOCUS_DTYPE)
    buf["gpos"], buf["pcov"], buf["ncov"] = 100, 5, 5
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    plain = MethylationPileup(genome)                         # without the option
    assert _open(plain) == HM_ESTATE and b"samples" in _err(plain)
    assert _load(plain, good) == HM_ESTATE and _sums(plain, 0, TOTAL, 0) == HM_ESTATE
    assert plain._L.hm_pileup_set_option(plain._h, b"samples", 3.0) == HM_ESTATE      # after hm_pileup_set_reference
    plain.close()
    for bad in (1, 65, 2.5, -1):
        with pytest.raises(HifimethError):
            _engine(bad, genome=genome)
    ran = _engine(3, genome=genome)                           # after records
    assert ran.add(read) == 1
    assert _open(ran) == HM_ESTATE and b"records" in _err(ran)
    ran.close()
    pu = _engine(3, genome=genome, partitions=True)           # after hm_pileup_load_loci
    assert pu._L.hm_pileup_load_loci(pu._h, 1, ptr, 1) == 1
    assert _open(pu) == HM_ESTATE and b"hm_pileup_load_loci" in _err(pu)
    pu.close()
    pu = _engine(3, genome=genome, partitions=True, groups=True)      # after hm_pileup_group_sample
    assert pu._L.hm_pileup_group_sample(pu._h, 1) == 0
    assert _open(pu) == HM_ESTATE and b"hm_pileup_group_sample" in _err(pu)
    pu.close()
    pu = _engine(2, genome=genome, partitions=True, groups=True)
    assert _load(pu, good) == HM_ESTATE and b"before hm_sample_open" in _err(pu)
    assert pu._L.hm_sample_load(pu._h, None, 1) == HM_EINVAL and pu._L.hm_sample_load(pu._h, ptr, -1) == HM_EINVAL
    assert pu._L.hm_pileup_set_option(pu._h, b"sample_min_cov", 0.0) == HM_EINVAL and pu._L.hm_pileup_set_option(pu._h, b"sample_min_cov", float(1 << 20)) == HM_EINVAL
    assert pu._L.hm_pileup_set_option(pu._h, b"sample_min_cov", 3.0) == 0
    assert _sums(pu, 0, TOTAL, 0) == 0                        # no sample yet: no entry
    assert _open(pu) == 0 and pu._L.hm_sample_load(pu._h, None, 0) == 0
    assert pu._L.hm_pileup_set_option(pu._h, b"sample_min_cov", 4.0) == HM_ESTATE     # a sample has been opened
    assert _load(pu, ([100, 101], [2, 1], [1, 1], [0, 0])) == 2 and pu.sample_plane(0, 100, 102).tolist() == [S.level(2, 3) + 1, S.BELOW]     # the minimum coverage is 3
    assert pu._L.hm_pileup_load_loci(pu._h, 1, ptr, 1) == HM_ESTATE and b"sample" in _err(pu)       # and the reverse
    assert pu._L.hm_pileup_group_sample(pu._h, 1) == HM_ESTATE and b"hm_sample_open" in _err(pu)
    assert _submit(pu, read) == HM_ESTATE and b"loaded" in _err(pu)
    assert _sums(pu, 0, TOTAL, 2) == HM_EINVAL and _sums(pu, 0, TOTAL, -1) == HM_EINVAL and _sums(pu, 5, 4, 0) == HM_EINVAL
    assert _sums(pu, 0, TOTAL + 1, 0) == HM_EINVAL and _sums(pu, -1, 4, 1) == HM_EINVAL and _sums(pu, 9, 9, 1) == 3
    out = np.zeros(4, np.uint16).ctypes.data_as(ctypes.c_void_p)
    plane = pu._L.hm_sample_plane
    assert plane(pu._h, 2, 0, 4, out) == HM_EINVAL and plane(pu._h, -1, 0, 4, out) == HM_EINVAL and plane(pu._h, 0, 3, 2, out) == HM_EINVAL
    assert plane(pu._h, 0, TOTAL - 3, TOTAL + 1, out) == HM_EINVAL and plane(pu._h, 1, 0, 4, out) == 0
    assert _open(pu) == 1 and _open(pu) == HM_ESTATE and b"all 2 samples" in _err(pu)      # sample N + 1
    assert _load(pu, ([100], [5], [5], [0])) == 1             # the same locus in the next sample is the point of the exercise
    pu.close()


# ---- 6. r ---------------------------------------------------------------------------------------------------------------------------------
def test_r_and_means_against_python_integers(loaded):
    from hifimeth_amd.pileup import sample_corr
    n, pu, ref = loaded
    worst = 0.0
    for complete in (False, True):
        entries = pu.sample_sums(complete=complete)
        r, mi, mj = sample_corr(entries)
        for k, e in enumerate(ref.sums(complete=complete)):
            wr, wi, wj = S.corr(e)
            assert math.isnan(wr) == math.isnan(r[k]) and (math.isnan(wr) or abs(r[k] - wr) <= 1e-12), (e, r[k], wr)
            assert mi[k] == wi and mj[k] == wj
            worst = max(worst, 0.0 if math.isnan(wr) else abs(r[k] - wr))
        assert np.isfinite(r).all() and (np.abs(r[entries["i"] != entries["j"]]) < 0.999).all()
    print("N = %d: worst |r - reference| = %.3g" % (n, worst))


def test_nan_cases_and_null_outputs():
    from hifimeth_amd.pileup import SAMPLE_PAIR_DTYPE, sample_corr
    e = np.zeros(4, SAMPLE_PAIR_DTYPE)
    e[1] = (0, 1, 0, 0, 1, 7, 9, 49, 81, 63)                  # n = 1
    e[2] = (0, 1, 0, 0, 3, 15, 6, 75, 14, 30)                 # u_i = 5, 5, 5: no variance; u_j = 1, 2, 3
    e[3] = (0, 1, 0, 0, 3, 6, 6, 14, 14, 10)                  # 1, 2, 3 against 3, 2, 1
    r, mi, mj = sample_corr(e)
    assert np.isnan(r[:3]).all() and abs(r[3] + 1.0) <= 4 * 2.0 ** -53
    assert math.isnan(mi[0]) and mi[1] == 100.0 * 7 / 32768 and mj[2] == 100.0 * 6 / (3 * 32768.0)
    from hifimeth_amd._lib import lib
    L = lib()
    only_r = np.zeros(4)
    assert L.hm_sample_corr(e.ctypes.data_as(ctypes.c_void_p), 4, only_r.ctypes.data_as(ctypes.c_void_p), None, None) == 0 and only_r[3] == r[3]
    assert L.hm_sample_corr(None, 1, None, None, None) == HM_EINVAL and L.hm_sample_corr(None, 0, None, None, None) == 0


def test_samples_in_reverse_order_give_the_transposed_table():
    n, tile = 5, _tile()
    data = S.dataset(n, tile)
    pu = _engine(n)
    try:
        for rows in data[::-1]:
            pu.open_sample()
            pu.load_sample(*rows)
        got = {(e[2], e[0], e[1]): e[3:] for e in _tuples(pu.sample_sums())}
        for i, j, c, cnt, si, sj, sii, sjj, sij in S.loaded(n, tile).sums():
            assert got[(c, n - 1 - j, n - 1 - i)] == (cnt, sj, si, sjj, sii, sij)
    finally:
        pu.close()


# ---- 7. the command -----------------------------------------------------------------------------------------------------------------------
def _cli(args, ok=True):
    r = subprocess.run([CLI, "samplecorr", *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok and (ok or r.returncode == 1), r.stderr
    return r


def _files(prefix, contexts=S.CTX):
    return ({c: open(f"{prefix}.samplecorr.{c}.tsv").read() for c in contexts}, {c: open(f"{prefix}.samplecorr.{c}.matrix.tsv").read() for c in contexts},
            open(f"{prefix}.samplecorr.samples.tsv").read())


@pytest.fixture(scope="module")
def command(tmp_path_factory):
    """four samples as three cov.bed files each, rows in the order of the data set; the files of two samples gzip"""
    from bamutil import write_fasta
    d = tmp_path_factory.mktemp("samplecorr")
    genome = _genome()
    names = [n for n, _ in genome]
    fa = str(d / "ref.fa")
    write_fasta(fa, genome)
    prefixes = []
    for s, (gpos, p, n, motif) in enumerate(S.dataset(4, _tile())):
        prefixes.append(str(d / ("s%d" % s)))
        sid = np.searchsorted(OFFSETS, gpos, side="right") - 1
        for c in range(3):
            sel = np.flatnonzero(np.minimum(motif, 2) == c)
            text = "".join("%s\t%d\t%d\t%g\t%d\t%d\n" % (names[sid[i]], gpos[i] - OFFSETS[sid[i]], gpos[i] - OFFSETS[sid[i]] + 1,
                                                        100.0 * p[i] / max(p[i] + n[i], 1), p[i], n[i]) for i in sel)
            with open(prefixes[-1] + "." + S.CTX[c] + ".cov.bed" + (".gz" if s in (1, 3) else ""), "wb") as f:
                f.write(gzip.compress(text.encode()) if s in (1, 3) else text.encode())
    return genome, fa, prefixes, str(d)


@pytest.mark.parametrize("args,min_cov,complete", [((), 5, False), (("-k", "-a", "3"), 3, True)])
def test_command_equals_the_python_path(command, args, min_cov, complete):
    from hifimeth_amd.pileup import MethylationPileup, read_cov_bed, samplecorr_matrix_tsv, samplecorr_samples_tsv, samplecorr_tsv
    genome, fa, prefixes, d = command
    out = d + "/out" + "".join(args)
    r = _cli([*args, "-t", "3", fa, ",".join(prefixes), out])
    assert f"{out}.samplecorr.*" in r.stderr and "Skip" not in r.stderr and "min sample coverage %d" % min_cov in r.stderr
    names = [n for n, _ in genome]
    pu = MethylationPileup(genome, samples=4, sample_min_cov=min_cov)
    ref = S.SampleLoader(TOTAL, 4, min_cov)
    try:
        for s, prefix in enumerate(prefixes):
            assert pu.open_sample() == s == ref.open()
            for k, c in enumerate(S.CTX):
                rows = read_cov_bed(f"{prefix}.{c}.cov.bed" + (".gz" if s in (1, 3) else ""), names, pu.offsets, motif=k)
                assert pu.load_sample(*rows) == ref.load(*rows)
        entries, own = pu.sample_sums(complete=complete), pu.sample_sums()
        pairs, matrices, samples = _files(out)
        for k, c in enumerate(S.CTX):
            assert samplecorr_tsv(prefixes, entries, k) == pairs[c] == S.samplecorr_tsv(prefixes, ref.sums(complete=complete), k)
            assert samplecorr_matrix_tsv(prefixes, entries, k) == matrices[c] == S.samplecorr_matrix_tsv(prefixes, ref.sums(complete=complete), k)
            assert len(pairs[c].splitlines()) == 7 and len(matrices[c].splitlines()) == 5 and "nan" not in pairs[c]
        assert samplecorr_samples_tsv(prefixes, own) == samples == S.samplecorr_samples_tsv(prefixes, ref.sums())
        assert len(samples.splitlines()) == 13
    finally:
        pu.close()


def test_command_skips_a_context_and_names_a_bad_line(command, tmp_path):
    genome, fa, prefixes, d = command
    moved = prefixes[2] + ".CHH.cov.bed"
    os.rename(moved, moved + ".away")
    try:
        out = str(tmp_path / "o")
        r = _cli([fa, ",".join(prefixes), out])
        assert "Skip context CHH" in r.stderr and moved in r.stderr
        assert not os.path.exists(out + ".samplecorr.CHH.tsv") and not os.path.exists(out + ".samplecorr.CHH.matrix.tsv")
        pairs, matrices, samples = _files(out, S.CTX[:2])
        assert len(samples.splitlines()) == 9 and "CHH" not in samples and all(len(pairs[c].splitlines()) == 7 for c in S.CTX[:2])
        assert samples.splitlines()[0] == "ctx\tsample\tn\tmean" and [x.split("\t")[1] for x in samples.splitlines()[1:5]] == prefixes
    finally:
        os.rename(moved + ".away", moved)
    assert "no context" in _cli([fa, str(tmp_path / "x") + "," + str(tmp_path / "y"), str(tmp_path / "o3")], ok=False).stderr
    bad = str(tmp_path / "bad")
    for k, c in enumerate(S.CTX):                            # a locus of its own per file: 7, 17, 27
        with open(f"{bad}.{c}.cov.bed", "w") as f:
            f.write("ctg1\t%d\t%d\t50\t5\t5\n" % (7 + 10 * k, 8 + 10 * k) + ("ctg2\t9\t10\t50\t5\t5\nctg2\t11\t12\t50\tfive\t5\n" if c == "CHG" else ""))
    r = _cli([fa, prefixes[0] + "," + bad, str(tmp_path / "o4")], ok=False)
    assert f"{bad}.CHG.cov.bed:3: " in r.stderr
    with open(f"{bad}.CHG.cov.bed", "w") as f:                # a duplicate across the sample's files: the file is named
        f.write("ctg1\t7\t8\t0\t0\t9\n")
    r = _cli([fa, prefixes[0] + "," + bad, str(tmp_path / "o5")], ok=False)
    assert f"{bad}.CHG.cov.bed: " in r.stderr and "1 locus given twice in one sample" in r.stderr
