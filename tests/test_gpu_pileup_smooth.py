"""`smooth` on the GPU: hm_smooth_fetch against tests/smooth_ref.py, as structs byte for byte -- everything is integers, so
there is no tolerance.  Rows go in through hm_pileup_load_loci.  The reference is the running-sum formulation;
tests/test_pileup_smooth_cpu.py holds it against the window-by-window one on the same data."""
import ctypes
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

import bigref
import smooth_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL, HM_ESTATE = -1, -5


def _engine(offsets, rows, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    lengths = np.diff(np.asarray(offsets, np.int64)).tolist()
    pu = MethylationPileup([("s%d" % (k + 1), n) for k, n in enumerate(lengths)], partitions=True, bases=np.full(int(offsets[-1]), ord("N"), np.uint8), **kw)
    if rows is not None:
        assert pu.load_loci(1, rows["gpos"], rows["pcov"], rows["ncov"], rows["motif"]) == len(rows)
    return pu


@functools.lru_cache(maxsize=None)
def _boundary():
    """-> (engine with the boundary set in part 1, rows, offsets); read-only"""
    rows, off = S.boundary_rows()
    return _engine(off, rows), rows, off


@functools.lru_cache(maxsize=None)
def _want(ctx, h, min_cov=1, min_loci=1):
    _pu, rows, off = _boundary()
    want = S.smooth_prefix(rows, off, ctx, h, min_cov, min_loci)
    want.setflags(write=False)
    return want


def _raw(pu, part, ctx, lo, hi, h, min_cov, min_loci, out=None, cap=0):
    ptr = out.ctypes.data_as(ctypes.c_void_p) if out is not None else None
    return pu._L.hm_smooth_fetch(pu._h, part, ctx, lo, hi, h, min_cov, min_loci, ptr, cap)


def _same(got, want, what):
    assert got.dtype == want.dtype == S.SMOOTH_DTYPE and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        k = int(np.flatnonzero(got != want)[0])
        raise AssertionError((what, k, got[k], want[k]))


# ---- 1: boundaries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", S.HALF_WIDTHS)
def test_every_window_cut_at_its_sequence(h):
    pu, rows, off = _boundary()
    for ctx in (0, 1, 2):
        got = pu.fetch_smooth(ctx, half_width=h, partition=1)
        want = _want(ctx, h)
        _same(got, want, (ctx, h))
        assert len(got) == len(S.counting(rows, ctx, 1)[0]) > 5000
        if h == 1:                                            # the locus itself
            assert (got["loci"] == 1).all() and (got["wp"] == got["pcov"]).all() and (got["wn"] == got["ncov"]).all()
        short = got[got["gpos"] < off[3]]                     # the sequences of 1, 2 and 5 bases: no neighbour leaks in
        assert (len(short) >= 1 or ctx == 1) and (short["loci"] <= 3).all()
        if h >= 4096:                                         # the sequence of 3 000 bases is shorter than the window: all of it, and no more
            mid = got[(got["gpos"] >= off[3]) & (got["gpos"] < off[4])]
            assert (mid["loci"] == len(mid)).all()


# ---- 2: min_cov and min_loci -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_cov", [1, 3])
def test_min_cov_and_min_loci(min_cov):
    pu, rows, off = _boundary()
    for ctx, h in ((0, 7), (0, 500), (2, 7), (1, 16384)):
        every = pu.fetch_smooth(ctx, half_width=h, min_cov=min_cov, partition=1)
        _same(every, _want(ctx, h, min_cov, 1), (ctx, h, min_cov))
        assert (every["pcov"] + every["ncov"] >= min_cov).all()
        for min_loci in (2, 5):
            got = pu.fetch_smooth(ctx, half_width=h, min_cov=min_cov, min_loci=min_loci, partition=1)
            _same(got, _want(ctx, h, min_cov, min_loci), (ctx, h, min_cov, min_loci))
            assert got.tobytes() == every[every["loci"] >= min_loci].tobytes()       # min_loci only drops rows
            assert 0 < len(got) <= len(every)
    assert len(_want(0, 500, 3)) < len(_want(0, 500, 1)) and _want(0, 500, 3)["loci"].sum() < _want(0, 500, 1)["loci"].sum()


# ---- 3: sub-range fetches --------------------------------------------------------------------------------------------------------
def _cuts(rows, total):
    from hifimeth_amd.pileup import region_geometry
    B = region_geometry()[0]
    pos = S.counting(rows, 0, 1)[0]
    g = int(pos[np.searchsorted(pos, 40000)])                 # a locus deep inside the long sequence
    pts = {0, total, 3008, 3007}
    pts |= {B * k + d for k in (1, 5, 17) for d in (-1, 0, 1)} | {256 * k + d for k in (3, 130) for d in (-1, 1)}
    pts |= {32768 + d for d in (-1, 0, 1)} | {g - 3, g, g + 1, g + 400}
    return sorted(p for p in pts if 0 <= p <= total)


@pytest.mark.parametrize("h", [500, 16384])
def test_a_sub_range_is_the_slice_of_the_whole(h):
    pu, rows, off = _boundary()
    total = int(off[-1])
    whole = _want(0, h, 1, 2)
    cuts = _cuts(rows, total)
    assert len(cuts) >= 20
    for i, lo in enumerate(cuts):
        for hi in cuts[i + 1:: 3] + [cuts[-1]]:
            got = pu.fetch_smooth(0, lo, hi, half_width=h, min_loci=2, partition=1)
            want = whole[(whole["gpos"] >= lo) & (whole["gpos"] < hi)]
            _same(got, want, (h, lo, hi))
    for lo, hi in ((4095, 4500), (32767, 33300), (40000, 40900)):   # the planes outside [lo, hi) were read: the loci inside alone give less
        got = pu.fetch_smooth(0, lo, hi, half_width=h, partition=1)
        alone = S.smooth_prefix(rows[(rows["gpos"] >= lo) & (rows["gpos"] < hi)], off, 0, h, 1, 1, lo, hi)
        assert len(got) == len(alone) > 0 and (alone["loci"] < got["loci"]).all() and (alone["wp"] <= got["wp"]).all()
    # cap smaller than the count: the count, and `out` untouched
    n = len(whole)
    buf = np.frombuffer(bytearray(b"\x5a" * (n * 40)), np.uint8)
    assert _raw(pu, 1, 0, 0, total, h, 1, 2, buf, n - 1) == n and (buf == 0x5A).all()
    assert _raw(pu, 1, 0, 0, total, h, 1, 2, None, n) == n
    assert _raw(pu, 1, 0, 0, total, h, 1, 2, buf, n) == n and buf.tobytes() == whole.tobytes()
    assert _raw(pu, 1, 0, 77, 77, h, 1, 1) == 0


# ---- 4: exactness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True])
def test_the_largest_sums_come_out_exact(mirror):
    rows, off = S.exact_rows(mirror)
    pu = _engine(off, rows)
    try:
        got = pu.fetch_smooth(0, half_width=16384, partition=1)
        _same(got, S.smooth_prefix(rows, off, 0, 16384), mirror)
        big, none = ("wn", "wp") if mirror else ("wp", "wn")
        assert int(got[big][20000]) == (2 ** 31 - 1) * 16384 ** 2 > 2 ** 58 and (got[none] == 0).all() and int(got["loci"][20000]) == 32767
        part = pu.fetch_smooth(0, 30000, 36000, half_width=16384)       # a range whose running sums start elsewhere; the combined planes
        assert part.tobytes() == got[30000:36000].tobytes()
    finally:
        pu.close()


# ---- 5: a reference past 2^32 bases ----------------------------------------------------------------------------------------------
def test_around_two_to_the_31_and_32():
    import torch
    B31, B32 = bigref.B31, bigref.B32
    total = bigref.HOST_LEN[B32]
    off = np.array([0, B31, B32, total], np.int64)            # 2^31 - 1 and 2^32 - 1 are the last bases of the first two sequences
    need = total * (1 + 4 * 7) + (1 << 30)                    # as test_gpu_pileup_diff.py::test_loci_around_two_to_the_32
    free, _all = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip("the card has %.1f GB free, the case needs %.1f GB plus 8 GB" % (free / 1e9, need / 1e9))
    rng = np.random.default_rng(23)
    zones = [(B31 - 20000, B31 + 20000), (B32 - 20000, B32 + 20000), (total - 20000, total)]
    gpos = np.unique(np.concatenate([rng.integers(a, b, 1500) for a, b in zones] + [[B31 - 1, B31, B32 - 1, B32, total - 1]]))
    rows = S.locus_rows(gpos, rng.integers(0, 40, len(gpos)), rng.integers(1, 40, len(gpos)), rng.integers(0, 2, len(gpos)) * 2)
    pu = _engine(off, rows)
    try:
        assert pu.n_loci == total > B32 and 4000 < len(rows)
        for ctx in (0, 2):
            for h in (500, 16384):
                for lo, hi in zones + [(B31 - 5000, B31 + 1), (B32 - 1, B32 + 4097)]:
                    got = pu.fetch_smooth(ctx, lo, hi, half_width=h, partition=1)
                    _same(got, S.smooth_prefix(rows, off, ctx, h, lo=lo, hi=hi), (ctx, h, lo, hi))
                    assert len(got) > 50 and got["gpos"].min() >= lo and got["loci"].max() > (10 if h == 500 else 200)
        last = pu.fetch_smooth(int(rows["motif"][-1]), total - 1, total, half_width=16384, partition=1)
        assert last["gpos"].tolist() == [total - 1] and int(last["loci"][0]) > 200
        assert _raw(pu, 1, 0, 0, total + 1, 500, 1, 1) == HM_EINVAL
    finally:
        pu.close()
        torch.cuda.empty_cache()


# ---- 6: state --------------------------------------------------------------------------------------------------------------------
def test_state_and_errors():
    from hifimeth_amd.pileup import MethylationPileup
    pu, rows, off = _boundary()
    total = int(off[-1])
    before = pu.loci().tobytes(), pu.loci(partition=1).tobytes(), pu.asm(min_cov=1).tobytes()
    one = pu.fetch_smooth(2, half_width=500, partition=1)
    assert one.tobytes() == pu.fetch_smooth(2, half_width=500, partition=0).tobytes()        # only part 1 was loaded
    assert len(pu.fetch_smooth(2, half_width=500, partition=2)) == 0
    assert before == (pu.loci().tobytes(), pu.loci(partition=1).tobytes(), pu.asm(min_cov=1).tobytes())
    assert pu.fetch_smooth(2, half_width=500, partition=1).tobytes() == one.tobytes()
    good = dict(part=1, ctx=0, lo=0, hi=total, h=500, min_cov=1, min_loci=1)
    for bad in (dict(ctx=3), dict(ctx=-1), dict(part=3), dict(part=-1), dict(h=0), dict(h=16385), dict(min_cov=0), dict(min_loci=0),
                dict(lo=-1), dict(lo=5, hi=4), dict(hi=total + 1)):
        assert _raw(pu, **{**good, **bad}) == HM_EINVAL, bad
        assert pu._L.hm_pileup_last_error(pu._h).startswith(b"hm_smooth_fetch")
    assert _raw(pu, **good) == len(_want(0, 500))
    plain = MethylationPileup([("s1", 100)], bases=np.full(100, ord("N"), np.uint8))     # no partitions: part 0 answers, 1 and 2 do not
    void = _engine([0, 100], None)
    try:
        assert _raw(plain, **{**good, "hi": 100, "part": 0}) == 0
        assert _raw(plain, **{**good, "hi": 100}) == HM_ESTATE and _raw(plain, **{**good, "hi": 100, "part": 2}) == HM_ESTATE
        assert _raw(void, **{**good, "hi": 100}) == 0
        dup = np.zeros(2, S.LOCUS_DTYPE)
        dup["gpos"], dup["pcov"] = 7, 1
        assert void._L.hm_pileup_load_loci(void._h, 1, dup.ctypes.data_as(ctypes.c_void_p), 2) < 0    # a locus twice: the planes are void
        assert void._L.hm_pileup_fetch_loci(void._h, None, None, None, 0, 0, 100, None, 0) == HM_ESTATE
        for part in (0, 1, 2):
            assert _raw(void, **{**good, "hi": 100, "part": part}) == HM_ESTATE
    finally:
        plain.close()
        void.close()


# ---- 7: the command --------------------------------------------------------------------------------------------------------------
def test_the_command_writes_what_the_reference_writes(tmp_path):
    from bamutil import write_fasta
    rows, off = S.boundary_rows()
    names = ["s%d" % (k + 1) for k in range(len(off) - 1)]
    fa, A, out, ref = (str(tmp_path / x) for x in ("ref.fa", "A", "out", "ref"))
    write_fasta(fa, [(n, "ACGT"[k % 4] * int(off[k + 1] - off[k])) for k, n in enumerate(names)])
    for ctx in (0, 1):                                        # CpG plain, CHG gzip, CHH missing
        text = "".join("%s\t%d\t%d\t%g\t%d\t%d\n" % (names[s], g - off[s], g - off[s] + 1, 100.0 * p / (p + n), p, n)
                       for g, p, n, s in ((int(r["gpos"]), int(r["pcov"]), int(r["ncov"]), int(np.searchsorted(off, r["gpos"], side="right")) - 1)
                                          for r in rows[rows["motif"] == ctx]))
        if ctx == 0:
            with open(A + ".CpG.cov.bed", "w") as f:
                f.write(text)
        else:
            with open(A + ".CHG.cov.bed.gz", "wb") as f:
                f.write(gzip.compress(text.encode()))
    loaded = rows[rows["motif"] < 2]
    for k, (args, kw) in enumerate(((["-W", "700", "-a", "2", "-i", "3"], dict(h=700, min_cov=2, min_loci=3)), ([], dict(h=500)),
                                    (["-W", "16384", "-t", "3"], dict(h=16384)))):
        r = subprocess.run([CLI, "smooth", *args, fa, A, out + str(k)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout == "" and "Skip context CHH" in r.stderr, r.stderr[-2000:]
        paths = S.write_outputs(ref + str(k), {0: loaded, 1: loaded}, names, off, **kw)
        assert [os.path.basename(p) for p in paths] == ["ref%d.smooth.CpG.bed" % k, "ref%d.smooth.CHG.bed" % k, "ref%d.smooth.summary.tsv" % k]
        for p in paths:
            got = open(p.replace(ref + str(k), out + str(k)), "rb").read()
            assert got == open(p, "rb").read() and len(got) > 0, p
        assert not os.path.exists("%s%d.smooth.CHH.bed" % (out, k))
    assert open(out + "0.smooth.summary.tsv").read().count("\n") == 2 and len(open(out + "0.smooth.CpG.bed").readline().split("\t")) == 8
