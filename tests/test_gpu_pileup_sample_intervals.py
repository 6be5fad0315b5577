"""`regiondiff` on the device, through the C ABI via the Python binding, against intervals_ref.py: every uint64 of
hm_sample_fetch_intervals exactly -- both modes, every context, every class of interval the query tells apart, ranges aligned to
nothing, additivity, 2 .. 64 samples opened or not, more blocks than one partition of the scan, a reference past 2^32 --, the
engine's other fetches in between, every error and state rule, hm_sample_interval_test against mpmath, hm_sample_qvalues against
the restatement's BH, and the command against the Python path byte for byte.

The one floating-point bar, 8 x E_ref on t, df and p, is the margin of DESIGN.md section 4 over the float64 restatement's own
worst error against mpmath (E_ref, measured by test_pileup_sample_intervals_cpu.py over the same cases).
Measured: the library's worst error is 1.00 E_ref for t, 1.00 E_ref for df and 0.96 E_ref for p."""
import ctypes
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

import bigref as R
import intervals_ref as I
import samples_ref as S
from samples_ref import HM_EDATA, HM_EINVAL, HM_ESTATE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


def _geometry():
    from hifimeth_amd.pileup import region_geometry
    block, scan = region_geometry()
    assert block >= 256 and scan >= 2
    return block, scan


def _genome(seed=3):
    rng = np.random.default_rng(seed)
    return [("ctg%d" % (s + 1), "".join(rng.choice(list("ACGT"), n))) for s, n in enumerate(I.lengths(_geometry()[0]))]


def _engine(n, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    return MethylationPileup(_genome(), samples=n, **kw)


def _load(pu, n, opened):
    for s, rows in enumerate(I.dataset(n, _geometry()[0])[:opened]):
        assert pu.open_sample() == s and pu.load_sample(*rows) == len(rows[0])
    return pu


def _fetch(pu, lo, hi, ctx, complete, start, end, out=None, n=None):
    """hm_sample_fetch_intervals without the wrapper's exception -> its return value"""
    a, b = (np.ascontiguousarray(x, np.int64) for x in (start, end))
    out = np.zeros((len(a), S.MAX_SAMPLES, 2), np.uint64) if out is None else out
    ptr = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return pu._L.hm_sample_fetch_intervals(pu._h, lo, hi, ctx, complete, ptr(a) if len(a) else ptr(a), ptr(b), len(a) if n is None else n, ptr(out))


def _err(pu):
    return pu._L.hm_pileup_last_error(pu._h)


# ---- 1. the sums ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(2, 2), (3, 3), (17, 17), (64, 64), (3, 2), (64, 17)], ids=lambda p: "N%d-M%d" % p)
def loaded(request):
    """N planes, M of them opened: an unopened plane is all zero and takes no part, also not in complete mode.  M = 2 has 32 parts
    per sample, 3 has 16, 17 has 2, 64 one"""
    n, m = request.param
    pu = _load(_engine(n), n, m)
    yield m, pu, I.loaded(n, _geometry()[0], m)
    pu.close()


def test_sums_equal_the_restatement(loaded):
    """every class of interval, per context and mode, over the whole reference and over a range aligned to nothing"""
    m, pu, ref = loaded
    block, _ = _geometry()
    assert ref.total == 3 * block + 777 and ref.opened == m
    stored = set(np.unique(ref.level[:m]).tolist())
    assert {0, S.BELOW, 1, 32769} <= stored
    for lo, hi in ((0, ref.total), (37, ref.total - 41)):
        for ctx in range(3):
            classes = I.interval_classes(ref, ctx, block, lo, hi)
            start, end = [c[1] for c in classes], [c[2] for c in classes]
            both = []
            for complete in (False, True):
                got = pu.sample_intervals(start, end, ctx, lo, hi, complete)
                want = I.interval_sums(ref, start, end, ctx, lo, hi, complete)
                assert got.shape == want.shape == (len(classes), m, 2) and got.dtype == np.uint64
                for k, (name, _a, _b) in enumerate(classes):
                    assert (got[k] == want[k]).all(), (name, lo, hi, ctx, complete, got[k].tolist(), want[k].tolist())
                by = {c[0]: got[k] for k, c in enumerate(classes)}
                assert not by["empty"].any() and not by["wholly below"].any() and not by["wholly above"].any() and not by["far outside"].any()
                assert (by["one base on a counting locus"][:, 0] == 1).all()
                assert (by["one whole block"][:, 0] > 100).all() and (by["duplicate"] == by["inside one block"]).all()
                assert (by["past both"] == by["the whole range"]).all() and (by["the whole reference"] == by["the whole range"]).all()
                both.append(got)
            assert (both[0] != both[1]).any() and (both[1] <= both[0]).all()      # the modes differ on these data
            assert (both[1][:, :, 0] == both[1][:, :1, 0]).all()                  # complete: every sample counts at the same loci


def test_one_interval_and_more_than_a_grid_stride():
    """70 000 intervals are more than the 65 536 wavefronts of the largest grid; their order does not matter"""
    block, _ = _geometry()
    pu = _load(_engine(3), 3, 3)
    ref = I.loaded(3, block, 3)
    try:
        rng = np.random.default_rng(9)
        start = rng.integers(-50, ref.total, 70000)
        end = start + np.where(rng.random(70000) < 0.02, rng.integers(0, 3 * block, 70000), rng.integers(0, 400, 70000))
        for ctx, complete in ((0, False), (2, True)):
            got = pu.sample_intervals(start, end, ctx, complete=complete)
            assert (got == I.interval_sums(ref, start, end, ctx, complete=complete)).all() and got[65536:].any()
            back = pu.sample_intervals(start[::-1], end[::-1], ctx, complete=complete)
            assert (back[::-1] == got).all()
            one = pu.sample_intervals(start[69999:], end[69999:], ctx, complete=complete)
            assert one.shape == (1, 3, 2) and (one[0] == got[69999]).all()
    finally:
        pu.close()


def test_the_sums_over_two_halves_add_up(loaded):
    """at a split inside a block and at a block edge, for a range aligned to nothing"""
    m, pu, ref = loaded
    block, _ = _geometry()
    lo, hi = 37, ref.total - 41
    classes = I.interval_classes(ref, 0, block, lo, hi)
    start, end = [c[1] for c in classes], [c[2] for c in classes]
    for ctx, complete in ((0, False), (1, True), (2, False)):
        whole = pu.sample_intervals(start, end, ctx, lo, hi, complete)
        for mid in (lo + block + 1000, lo + 2 * block, 2 * block, lo, hi):
            parts = pu.sample_intervals(start, end, ctx, lo, mid, complete) + pu.sample_intervals(start, end, ctx, mid, hi, complete)
            assert (parts == whole).all(), (ctx, complete, mid)


# ---- 2. scale -----------------------------------------------------------------------------------------------------------------------------
def test_more_blocks_than_one_partition_of_the_scan():
    from hifimeth_amd.pileup import MethylationPileup
    block, scan = _geometry()
    total = (scan + 1) * block + 5                              # scan + 2 blocks, the last of 5 bases
    rng = np.random.default_rng(21)
    pu = MethylationPileup([("c", total)], samples=2, bases=np.full(total, ord("C"), np.uint8))
    ref = S.SampleLoader(total, 2)
    try:
        for s in range(2):
            g = np.unique(np.concatenate([rng.choice(total, 30000, replace=False), [0, total - 1, scan * block - 1, scan * block]]))
            cov = rng.integers(3, 30, len(g))
            p = rng.binomial(cov, 0.5)
            motif = rng.integers(0, 3, len(g))
            assert pu.open_sample() == s == ref.open() and pu.load_sample(g, p, cov - p, motif) == len(g) == ref.load(g, p, cov - p, motif)
        e = scan * block
        start = np.concatenate([[0, 0, e - 1, e - block - 3, 5, block * (scan // 2) + 1, e, total - 5], rng.integers(0, total, 300)])
        end = np.concatenate([[total, e, e + 1, e + block + 3, total - 1, e + 9, total, total], rng.integers(0, total, 300)])
        end = np.maximum(start, end)
        for ctx in range(3):
            for lo, hi, complete in ((0, total, False), (777, total - 3, True)):
                got = pu.sample_intervals(start, end, ctx, lo, hi, complete)
                assert (got == I.interval_sums(ref, start, end, ctx, lo, hi, complete)).all(), (ctx, lo, hi, complete)
        assert pu.sample_intervals([0], [total], 0)[0, :, 0].min() > 5000
    finally:
        pu.close()


def test_intervals_around_two_to_the_32():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    total = R.HOST_LEN[R.B32]
    lengths = [R.B31, R.B31, total - R.B32]
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

        def want(start, end, lo, hi, complete):
            out = []
            for a, b in zip(start, end):
                a, b = min(max(a, lo), hi), min(max(b, lo), hi)
                row = []
                for s in range(2):
                    u = [stored[s][k] - 1 for k, g in enumerate(loci) if a <= g < b and stored[s][k] != S.BELOW
                         and (not complete or stored[1 - s][k] != S.BELOW)]
                    row.append([len(u), sum(u)])
                out.append(row)
            return out
        start = [0, 0, R.B31 - 1, R.B31, R.B32 - 1, R.B32, R.B32 - 5000, 6, R.B31 + 1, total - 10, R.B32 + 5]
        end = [total, R.B32, R.B31, R.B32, R.B32 + 1, total, R.B32 + 5000, R.B31 - 1, R.B32 - 1, total, R.B32 + 6]
        for lo, hi in ((0, total), (R.B31, total), (3, R.B32), (R.B32 - 1, R.B32 + 1)):
            for complete in (False, True):
                assert pu.sample_intervals(start, end, 0, lo, hi, complete).tolist() == want(start, end, lo, hi, complete), (lo, hi, complete)
        assert want(start, end, 0, total, False)[0] == [[6, sum(v - 1 for v in stored[0])], [5, sum(v - 1 for v in stored[1] if v != S.BELOW)]]
        assert not pu.sample_intervals(start, end, 1).any()
    finally:
        pu.close()
        torch.cuda.empty_cache()


# ---- 3. one engine, many fetches ----------------------------------------------------------------------------------------------------------
def test_other_fetches_in_between_change_nothing():
    block, _ = _geometry()
    ref = I.loaded(3, block, 3)
    classes = I.interval_classes(ref, 0, block, 0, ref.total)
    start, end = np.array([c[1] for c in classes]), np.array([c[2] for c in classes])
    fresh = _load(_engine(3), 3, 3)
    want = {(c, k): fresh.sample_intervals(start, end, c, complete=k).tobytes() for c in range(3) for k in (False, True)}
    fresh.close()
    pu = _load(_engine(3), 3, 3)
    try:
        a, b = np.clip(start, 0, ref.total), np.clip(end, 0, ref.total)
        others = [pu.sample_sums().tobytes(), pu.regions(a, b).tobytes(), pu.loci().tobytes()]
        for rounds in range(2):
            for (c, k), x in want.items():
                assert pu.sample_intervals(start, end, c, complete=k).tobytes() == x
                assert pu.sample_sums().tobytes() == others[0]
                assert pu.sample_intervals(start, end, c, complete=k).tobytes() == x
                assert pu.regions(a, b).tobytes() == others[1]
                assert pu.sample_intervals(start[::-1], end[::-1], c, complete=k)[::-1].tobytes() == x
                assert pu.loci().tobytes() == others[2]
        assert pu.sample_intervals(start, end, 0).tobytes() == want[(0, False)]
    finally:
        pu.close()


@pytest.mark.parametrize("m", [2, 3])
def test_interval_fetches_share_their_buffers(m):
    """regions, metaplot and sample_intervals keep their index, intervals and sums in ONE set of device buffers, those of
    whichever ran last.  In rotation on one engine, with all the interval classes and then one interval (the buffers grow, then
    serve a smaller call), every answer equals -- exactly -- that of an engine whose first interval fetch it is."""
    block, _ = _geometry()
    ref = I.loaded(3, block, 3)
    assert ref.total == 3 * block + 777                          # three blocks and a remainder
    classes = I.interval_classes(ref, 0, block, 0, ref.total)
    start, end = np.array([c[1] for c in classes]), np.array([c[2] for c in classes])
    one = [c[0] for c in classes].index("the whole range")
    picks = (slice(None), slice(one, one + 1))                   # all the classes, then one interval: the smaller call after the larger
    meta = dict(bins=4, flank=8, flank_bins=2)

    def calls(pick):
        s, e = start[pick], end[pick]
        a, b = np.clip(s, 0, ref.total), np.clip(e, 0, ref.total)
        z, t = np.zeros_like(a), np.full_like(a, ref.total)
        return (("sample_intervals CpG", lambda pu: pu.sample_intervals(s, e, 0).tobytes()),
                ("regions", lambda pu: pu.regions(a, b).tobytes()),
                ("sample_intervals CHG complete", lambda pu: pu.sample_intervals(s, e, 1, complete=True).tobytes()),
                ("metaplot", lambda pu: (lambda rows, used: rows.tobytes() + bytes([used]))(*pu.metaplot(a, b, z, t, **meta))))

    want = {}
    for k, pick in enumerate(picks):
        for name, call in calls(pick):
            fresh = _load(_engine(3), 3, m)
            want[k, name] = call(fresh)
            fresh.close()
            assert any(want[k, name]), (k, name)
    assert want[0, "regions"] != want[1, "regions"] and want[0, "metaplot"] != want[1, "metaplot"]
    pu = _load(_engine(3), 3, m)
    try:
        others = [pu.sample_sums().tobytes(), pu.loci().tobytes()]
        for rounds in range(2):
            for k, pick in enumerate(picks):
                for name, call in calls(pick):
                    assert call(pu) == want[k, name], (rounds, k, name)
                    assert call(pu) == want[k, name], (rounds, k, name, "again")
                assert [pu.sample_sums().tobytes(), pu.loci().tobytes()] == others
        for name, call in calls(picks[0])[::-1]:                 # ... and each large call straight after the small one of another kind
            assert calls(picks[1])[0][1](pu) == want[1, "sample_intervals CpG"]
            assert call(pu) == want[0, name], name
    finally:
        pu.close()


# ---- 4. errors and states -----------------------------------------------------------------------------------------------------------------
def test_errors_and_states():
    from hifimeth_amd.pileup import MethylationPileup
    block, _ = _geometry()
    total = 3 * block + 777
    genome = _genome()
    plain = MethylationPileup(genome)                         # without the option
    assert _fetch(plain, 0, total, 0, 0, [1], [2]) == HM_ESTATE and b"samples" in _err(plain)
    plain.close()
    pu = _engine(3)
    ref = I.loaded(3, block, 2)
    try:
        assert _fetch(pu, 0, total, 0, 0, [1], [2]) == 0      # no sample yet: no entry
        _load(pu, 3, 2)
        start, end = [0, 5, 9000], [total, 300, 9001]
        good = lambda: (pu.sample_intervals(start, end, 1) == I.interval_sums(ref, start, end, 1)).all()  # noqa: E731
        assert good()
        for args, text in (((0, total, 3, 0, start, end), b"ctx"), ((0, total, -1, 0, start, end), b"ctx"), ((0, total, 0, 2, start, end), b"complete"),
                           ((0, total, 0, -1, start, end), b"complete"), ((-1, total, 0, 0, start, end), b"bad range"), ((9, 8, 0, 0, start, end), b"bad range"),
                           ((0, total + 1, 0, 0, start, end), b"bad range"), ((0, total, 0, 0, [0, 7, 3], [5, 6, 4]), b"interval 1 has start > end")):
            assert _fetch(pu, *args) == HM_EINVAL and text in _err(pu), args
            assert good()                                     # after an error the next good call is right
        out = np.zeros((3, 64, 2), np.uint64)
        a = np.array(start, np.int64)
        null = lambda s, e, o, n: pu._L.hm_sample_fetch_intervals(pu._h, 0, total, 0, 0, s, e, n, o)  # noqa: E731
        pa, po = a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
        assert null(None, pa, po, 3) == HM_EINVAL and null(pa, None, po, 3) == HM_EINVAL and null(pa, pa, None, 3) == HM_EINVAL
        assert null(pa, pa, po, -1) == HM_EINVAL and null(None, None, None, 0) == 0 and good()
        assert pu._L.hm_sample_fetch_intervals(None, 0, total, 0, 0, pa, pa, 3, po) == HM_EINVAL
        out[:] = 7
        assert _fetch(pu, 9, 9, 0, 0, start, end, out) == 6 and not out.reshape(-1)[:12].any() and (out.reshape(-1)[12:] == 7).all()     # hi == lo: zeros
        assert _fetch(pu, 0, total, 2, 1, start, end, out) == 6 and (out.reshape(-1)[:12].reshape(3, 2, 2) == I.interval_sums(ref, start, end, 2, complete=True)).all()
        assert pu.open_sample() == 2                          # a third sample, empty: M = 3
        assert _fetch(pu, 0, total, 0, 0, start, end, out) == 9 and not pu.sample_intervals(start, end, 0, complete=True).any()
        from hifimeth_amd.pileup import LOCUS_DTYPE
        bad = np.zeros(1, LOCUS_DTYPE)
        bad["gpos"], bad["pcov"], bad["ncov"] = total, 5, 5
        assert pu._L.hm_sample_load(pu._h, bad.ctypes.data_as(ctypes.c_void_p), 1) == HM_EDATA
        assert _fetch(pu, 0, total, 0, 0, start, end, out) == HM_ESTATE and b"bad rows" in _err(pu)      # a voided engine
    finally:
        pu.close()


# ---- 5. the test and the q-values -----------------------------------------------------------------------------------------------------------
def test_the_statistic_against_mpmath_and_bh_against_the_restatement():
    from hifimeth_amd.pileup import sample_interval_test, sample_qvalues
    e_ref = I.e_ref()
    worst = {"t": 0.0, "df": 0.0, "p": 0.0}
    pvalues = []
    for pairs, group in I.cases():
        got = sample_interval_test(np.array([pairs], np.uint64), group)[0]
        want = I.welch(pairs, group)
        assert (int(got["m1"]), int(got["m2"]), int(got["n1"]), int(got["n2"])) == want[:4]
        for k, w in zip(("mean1", "mean2"), want[4:6]):
            assert got[k] == w or (got[k] != got[k] and w != w)      # the same operations in the same order
        mp = I.welch_mp(pairs, group)
        if mp is None:                                        # untested, or no spread at all: the same NaN, 0, 1 or infinity
            for k, w in zip(("t", "df", "pvalue"), want[6:]):
                assert got[k] == w or (got[k] != got[k] and w != w), (pairs, k)
        else:
            for k, f, w in zip(("t", "df", "p"), ("t", "df", "pvalue"), mp):
                worst[k] = max(worst[k], I.relerr(float(got[f]), w))
        pvalues.append(float(got["pvalue"]))
    print("worst relative error against mpmath: " + ", ".join("%s %.3g (%.2f E_ref)" % (k, worst[k], worst[k] / e_ref[k]) for k in worst))
    for k in worst:
        assert worst[k] <= 8 * e_ref[k], (k, worst[k], e_ref[k])
    q = sample_qvalues(np.array(pvalues))
    want = I.bh(pvalues)
    assert all(a == b or (a != a and b != b) for a, b in zip(q.tolist(), want)) and np.isnan(q).sum() == sum(1 for p in pvalues if p != p) > 0
    # other thresholds, in one call over all the hand-made cases of six samples
    six = [k for k, v in I.HAND.items() if len(v[0]) == 6 and v[1] == I.GROUPS6]
    got = sample_interval_test(np.array([I.HAND[k][0] for k in six], np.uint64), I.GROUPS6, min_loci=5, min_reps=3)
    for k, r in zip(six, got):
        want = I.welch(I.HAND[k][0], I.GROUPS6, 5, 3)
        assert (int(r["m1"]), int(r["m2"])) == want[:2] and (r["pvalue"] != r["pvalue"]) == (want[8] != want[8]), k
        assert want[8] != want[8] or abs(r["pvalue"] - want[8]) <= 1e-12 * want[8]
    L = __import__("hifimeth_amd._lib", fromlist=["lib"]).lib()
    s = np.zeros((1, 6, 2), np.uint64)
    g = np.array(I.GROUPS6, np.uint8)
    out = np.zeros(64, np.uint8)
    call = lambda n, m, grp, ml, mr: L.hm_sample_interval_test(s.ctypes.data_as(ctypes.c_void_p), n, m, grp, ml, mr, out.ctypes.data_as(ctypes.c_void_p))  # noqa: E731
    pg = g.ctypes.data_as(ctypes.c_void_p)
    assert call(1, 6, pg, 3, 2) == 0 and call(-1, 6, pg, 3, 2) == HM_EINVAL and call(1, 0, pg, 3, 2) == HM_EINVAL and call(1, 65, pg, 3, 2) == HM_EINVAL
    assert call(1, 6, None, 3, 2) == HM_EINVAL and call(1, 6, pg, 0, 2) == HM_EINVAL and call(1, 6, pg, 3, 1) == HM_EINVAL and call(1, 6, pg, 3, 65) == HM_EINVAL
    assert call(1, 6, np.array([1, 1, 1, 2, 2, 3], np.uint8).ctypes.data_as(ctypes.c_void_p), 3, 2) == HM_EINVAL
    from hifimeth_amd.caller import HifimethError
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(HifimethError):
            sample_qvalues(np.array([0.5, bad]))
    assert sample_qvalues(np.array([])).size == 0


# ---- 6. the command -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def command(tmp_path_factory):
    """six samples as three cov.bed files each, the files of two samples gzip; the intervals: tiles of 300 bases of every sequence,
    a promoter-like set with names and strands, one interval without a locus, in no order, plain and gzip"""
    from bamutil import write_fasta
    block, _ = _geometry()
    d = tmp_path_factory.mktemp("regiondiff")
    genome = _genome()
    names = [n for n, _ in genome]
    offsets = np.concatenate([[0], np.cumsum(I.lengths(block))]).astype(np.int64)
    fa = str(d / "ref.fa")
    write_fasta(fa, genome)
    prefixes = []
    for s, (gpos, p, n, motif) in enumerate(I.dataset(6, block)):
        prefixes.append(str(d / ("s%d" % s)))
        sid = np.searchsorted(offsets, gpos, side="right") - 1
        for c in range(3):
            sel = np.flatnonzero(np.minimum(motif, 2) == c)
            text = "".join("%s\t%d\t%d\t%g\t%d\t%d\n" % (names[sid[i]], gpos[i] - offsets[sid[i]], gpos[i] - offsets[sid[i]] + 1,
                                                        100.0 * p[i] / max(p[i] + n[i], 1), p[i], n[i]) for i in sel)
            with open(prefixes[-1] + "." + S.CTX[c] + ".cov.bed" + (".gz" if s in (1, 4) else ""), "wb") as f:
                f.write(gzip.compress(text.encode()) if s in (1, 4) else text.encode())
    lines = ["# tiles and promoters", "track name=x"]
    for k, n in enumerate(I.lengths(block)):
        lines += ["%s\t%d\t%d" % (names[k], a, min(a + 300, n)) for a in range(0, n, 300)][::-1]
    lines += ["ctg2\t100\t2100\tgeneA\t0\t+", "ctg2\t100\t2100\tgeneA_again\t0\t-", "ctg1\t0\t%d\twhole\t0\t." % I.lengths(block)[0], "",
              "ctg3\t17\t18\tone_base", "ctg1\t%d\t%d\tover_an_edge" % (block - 3, block + 3)]
    bed = str(d / "iv.bed")
    with open(bed, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(bed + ".gz", "wb") as f:
        f.write(gzip.compress(("\n".join(lines) + "\n").encode()))
    return genome, fa, prefixes, bed, str(d)


def _run(args, ok=True):
    r = subprocess.run([CLI, "regiondiff", *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok and (ok or r.returncode == 1), r.stderr
    return r


@pytest.mark.parametrize("args,gz,min_cov,complete,min_loci,min_reps", [((), False, 5, False, 3, 2), (("-k", "-a", "3", "-l", "6", "-r", "3"), True, 3, True, 6, 3)])
def test_command_equals_the_python_path(command, args, gz, min_cov, complete, min_loci, min_reps):
    from hifimeth_amd.pileup import (MethylationPileup, parse_regions_bed, read_cov_bed, regiondiff_summary_tsv, regiondiff_tsv, sample_interval_test,
                                     sample_qvalues)
    genome, fa, prefixes, bed, d = command
    block, _ = _geometry()
    out = d + "/out" + "".join(args)
    r = _run(["-R", bed + (".gz" if gz else ""), *args, "-t", "3", fa, ",".join(prefixes[:3]), ",".join(prefixes[3:]), out])
    assert f"{out}.regiondiff.*" in r.stderr and "Skip" not in r.stderr and "min sample coverage %d" % min_cov in r.stderr
    names = [n for n, _ in genome]
    regions = parse_regions_bed(bed, names, I.lengths(block))
    pu = MethylationPileup(genome, samples=6, sample_min_cov=min_cov)
    ref = S.SampleLoader(sum(I.lengths(block)), 6, min_cov)
    try:
        for s, prefix in enumerate(prefixes):
            assert pu.open_sample() == s == ref.open()
            for k, c in enumerate(S.CTX):
                rows = read_cov_bed(f"{prefix}.{c}.cov.bed" + (".gz" if s in (1, 4) else ""), names, pu.offsets, motif=k)
                assert pu.load_sample(*rows) == ref.load(*rows)
        xy = regions.coords(pu.offsets)
        tests, q = {}, {}
        for k, c in enumerate(S.CTX):
            sums = pu.sample_intervals(xy["start"], xy["end"], k, complete=complete)
            assert (sums == I.interval_sums(ref, xy["start"], xy["end"], k, complete=complete)).all()
            tests[k] = sample_interval_test(sums, I.GROUPS6, min_loci, min_reps)
            q[k] = sample_qvalues(tests[k]["pvalue"])
            text = open(f"{out}.regiondiff.{c}.tsv").read()
            assert text == regiondiff_tsv(regions, names, tests[k], q[k])
            rows = [x.split("\t") for x in text.splitlines()]
            want = [I.welch(row.tolist(), I.GROUPS6, min_loci, min_reps) for row in sums]
            assert len(rows) == len(regions) + 1 == len(want) + 1 and rows[-1][:5] == ["ctg1", str(block - 3), str(block + 3), "over_an_edge", "."]
            assert [x[5:9] for x in rows[1:]] == [[str(v) for v in w[:4]] for w in want]
            assert [x[14] == "nan" for x in rows[1:]] == [w[8] != w[8] for w in want]
            near = lambda a, b: (a != a and b != b) or a == b or abs(a - b) <= 1e-5 * abs(b)  # noqa: E731  (six printed digits: 5e-6 of rounding)
            assert all(near(float(x[14]), w[8]) and near(float(x[9]), w[4]) for x, w in zip(rows[1:], want))
            geneA = next(x for x in rows if x[3] == "geneA")
            again = next(x for x in rows if x[3] == "geneA_again")
            assert geneA[4] == "+" and again[4] == "-" and geneA[5:] == again[5:]
        assert open(f"{out}.regiondiff.summary.tsv").read() == regiondiff_summary_tsv(tests, q)
        if not complete:
            assert any(np.isnan(tests[k]["t"]).any() for k in tests) and any((q[k] <= 0.05).any() for k in q)
    finally:
        pu.close()


def test_command_skips_a_context_and_checks_its_lists(command, tmp_path):
    genome, fa, prefixes, bed, d = command
    moved = prefixes[2] + ".CHH.cov.bed"
    os.rename(moved, moved + ".away")
    try:
        out = str(tmp_path / "o")
        r = _run(["-R", bed, fa, ",".join(prefixes[:3]), ",".join(prefixes[3:]), out])
        assert "Skip context CHH" in r.stderr and moved in r.stderr and not os.path.exists(out + ".regiondiff.CHH.tsv")
        summary = open(out + ".regiondiff.summary.tsv").read().splitlines()
        assert len(summary) == 3 and "CHH" not in "".join(summary) and os.path.exists(out + ".regiondiff.CHG.tsv")
    finally:
        os.rename(moved + ".away", moved)
    bad = str(tmp_path / "bad.bed")
    with open(bad, "w") as f:
        f.write("ctg1\t5\t50\nctg9\t5\t50\n")
    r = _run(["-R", bad, fa, ",".join(prefixes[:3]), ",".join(prefixes[3:]), str(tmp_path / "o2")], ok=False)
    assert "bad.bed:2: unknown sequence ctg9" in r.stderr
    r = _run(["-R", str(tmp_path / "none.bed"), fa, ",".join(prefixes[:3]), ",".join(prefixes[3:]), str(tmp_path / "o3")], ok=False)
    assert "cannot open" in r.stderr and "none.bed" in r.stderr
