"""Benjamini-Hochberg q-values of the haplotype test (`pileup -H -A -Q`): the histogram of the tested loci per (context, pcov1, ncov1,
pcov2, ncov2) with its list of loci beyond 63 reads per haplotype, the p of every tuple that occurs, rows written with their q by
lookup, the CLI and the distributed driver.

Nothing here has a tolerance.  Bins and the big list must equal the numpy restatement below exactly; a row must be the row of
hm_pileup_fetch_asm byte for byte; a bin's pvalue must be the bits of a row's with the same counts (both come out of asm_test_kernel);
and qvalue must be the bits of numpy BH (asm_q_ref.bh_numpy, the header's definition) over the device's own pvalue column."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from asm_q_ref import ASM_BINS, ASM_T, bh_numpy, bin_index
from conftest import ROOT
from test_gpu_pileup_asm import CTX, _asm_files, _cov_files, _dist_env, _engine, _phased_reads, _run_cli, _write_bam

pytestmark = pytest.mark.gpu

N_LOCI = 3 * 4096 + 7
EDGES = (0, 4095, 4096, 8191, 8192, N_LOCI - 1)            # first / last index of a block and of the range
NEGATIVE = (17, 4097, 9000)


def _crafted():
    """-> pcov1, ncov1, pcov2, ncov2, key (int32 [N_LOCI])"""
    rng = np.random.default_rng(2024)
    t = np.zeros((4, N_LOCI), np.int64)
    motif = rng.integers(0, 3, N_LOCI)
    # background: a third of the loci, totals 0 .. 12 per haplotype from few distinct tuples (ties, weights > 1, totals below min_cov 5)
    bg = rng.choice(N_LOCI, N_LOCI // 3, replace=False)
    tot = rng.integers(0, 13, (2, len(bg)))
    k = (rng.random((2, len(bg))) * (tot + 1)).astype(np.int64)
    t[0, bg], t[1, bg], t[2, bg], t[3, bg] = k[0], tot[0] - k[0], k[1], tot[1] - k[1]
    # the dense / big edge on either haplotype alone and on both, at the block and range edges and elsewhere
    edge = [(a, b) for a in (62, 63, 64, 65) for b in (7, 62, 63, 64, 65)] + [(7, b) for b in (62, 63, 64, 65)]
    spots = list(EDGES) + rng.choice(np.setdiff1d(np.arange(N_LOCI), EDGES), 3 * len(edge) - len(EDGES), replace=False).tolist()
    for j, i in enumerate(spots):
        a, b = edge[j % len(edge)]
        ka, kb = int(rng.integers(0, a + 1)), int(rng.integers(0, b + 1))
        t[:, i] = (ka, a - ka, kb, b - kb)
    # identical haplotypes (p = q = 1), small and big
    same = rng.choice(np.setdiff1d(np.arange(N_LOCI), spots), 40, replace=False)
    t[:, same[:30]] = np.array([3, 4, 3, 4])[:, None]
    t[:, same[30:]] = np.array([50, 30, 50, 30])[:, None]
    for i in NEGATIVE:                                        # no counts: skipped, whatever the other counters say
        t[:, i] = (-1, 70, 9, 9) if i != 4097 else (6, 6, 6, -2)
    key = (rng.integers(0, 1 << 20, N_LOCI) << 2) | motif
    key[spots[::4]] |= 3                                      # low bits 3: counted as CHH, like the BED writers do
    key[bg[:50]] |= 3
    return tuple(x.astype(np.int32) for x in t) + (key.astype(np.int32),)


def ref_tested(host, min_cov):
    p1, n1, p2, n2 = (x.astype(np.int64) for x in host[:4])
    ok = (p1 >= 0) & (n1 >= 0) & (p2 >= 0) & (n2 >= 0) & (p1 + n1 >= min_cov) & (p2 + n2 >= min_cov)
    return ok, ok & (p1 + n1 < ASM_T) & (p2 + n2 < ASM_T)


def ref_histogram(host, lo, hi, min_cov):
    """-> (non-empty bins as {bin: count}, indices of the big loci) of planes[lo, hi)"""
    ok, dense = ref_tested(host, min_cov)
    inside = np.zeros(N_LOCI, bool)
    inside[lo:hi] = True
    d = np.nonzero(dense & inside)[0]
    p1, n1, p2, n2 = (x.astype(np.int64) for x in host[:4])
    b = bin_index(np.minimum(host[4][d] & 3, 2).astype(np.int64), p1[d], n1[d], p2[d], n2[d])
    u, c = np.unique(b, return_counts=True)
    return dict(zip(u.tolist(), c.tolist())), np.nonzero(ok & ~dense & inside)[0]


def _nonzero(bins):
    i = np.nonzero(bins)[0]
    return dict(zip(i.tolist(), bins[i].tolist()))


@pytest.fixture(scope="module")
def crafted():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    host = _crafted()
    pu = MethylationPileup([("c", "ACGT" * 50)])             # caller-owned planes: the reference plays no part
    dev = [torch.from_numpy(x.copy()).cuda() for x in host]
    yield pu, host, dev
    pu.close()


@pytest.fixture(scope="module")
def solved(crafted):
    """min_cov -> (bins, big, AsmTable, plain rows, rows with q) over the whole crafted range, computed once"""
    from hifimeth_amd.pileup import asm_qvalues
    pu, _host, dev = crafted
    out = {}
    for min_cov in (1, 5):
        bins, big = pu.asm_histogram(0, N_LOCI, min_cov, planes=dev)
        table = asm_qvalues(pu.asm_bin_pvalues(bins), big)
        out[min_cov] = (bins, big, table, pu.asm(0, N_LOCI, min_cov, planes=dev), pu.asm(0, N_LOCI, min_cov, planes=dev, table=table))
    return out


def test_crafted_planes_hold_the_cases():
    host = _crafted()
    p1, n1, p2, n2 = (x.astype(np.int64) for x in host[:4])
    for min_cov in (1, 5):
        ok, dense = ref_tested(host, min_cov)
        assert ok[list(EDGES)].all() and not ok[list(NEGATIVE)].any()
        t1, t2 = (p1 + n1)[ok], (p2 + n2)[ok]
        for a in (62, 63, 64, 65):                            # either haplotype alone, and both
            assert ((t1 == a) & (t2 < 62)).any() and ((t2 == a) & (t1 < 62)).any()
            assert all(((t1 == a) & (t2 == b)).any() for b in (62, 63, 64, 65))
        assert dense[list(EDGES)].any() and (~dense[list(EDGES)]).any()
        assert ((host[4] & 3) == 3)[ok & dense].any() and ((host[4] & 3) == 3)[ok & ~dense].any()
        same = ok & (p1 == p2) & (n1 == n2)
        assert (same & dense).sum() >= 30 and (same & ~dense).sum() >= 10
        assert (ok & ~dense).sum() >= 40 and dense.sum() > 1000
    assert ref_tested(host, 1)[0].sum() > ref_tested(host, 5)[0].sum() + 500


def test_histogram_and_big_list(crafted, solved):
    pu, host, dev = crafted
    for min_cov in (1, 5):
        bins, big, _table, rows, _rq = solved[min_cov]
        want_bins, want_big = ref_histogram(host, 0, N_LOCI, min_cov)
        assert _nonzero(bins) == want_bins
        ok, dense = ref_tested(host, min_cov)
        assert (big["gpos"] == want_big).all() and len(big) == len(want_big)
        assert (big == rows[np.isin(rows["gpos"], want_big)]).all()          # as hm_pileup_fetch_asm's rows: diff and pvalue filled
        assert int(bins.sum()) + len(big) == ok.sum() == len(rows)
    # ranges inside and across blocks, an empty one; bins given are added to
    bins = np.zeros(ASM_BINS, np.uint64)
    total, bigs = {}, []
    for lo, hi in ((0, 1), (1, 4097), (4097, 4097), (4097, N_LOCI - 1), (N_LOCI - 1, N_LOCI)):
        want_bins, want_big = ref_histogram(host, lo, hi, 1)
        for b, c in want_bins.items():
            total[b] = total.get(b, 0) + c
        back, big = pu.asm_histogram(lo, hi, 1, planes=dev, bins=bins)
        assert back is bins and (big["gpos"] == want_big).all() and len(big) == len(want_big)
        assert _nonzero(bins) == total
        bigs.append(big)
    assert _nonzero(bins) == _nonzero(solved[1][0]) and (np.concatenate(bigs) == solved[1][1]).all()


def test_rows_equal_fetch_asm_and_q_is_bh_of_the_device_p(solved):
    from hifimeth_amd.pileup import ASM_DTYPE, ASMQ_DTYPE
    for min_cov in (1, 5):
        _bins, big, table, rows, rq = solved[min_cov]
        assert rq.dtype == ASMQ_DTYPE and len(rq) == len(rows) > 1000
        assert np.ascontiguousarray(rq[list(ASM_DTYPE.names)]).astype(ASM_DTYPE).tobytes() == rows.tobytes()      # (a)
        assert not np.isnan(rq["qvalue"]).any()
        ctx = np.minimum(rq["motif"], 2)
        for c in range(3):                                                                                        # (b)
            sel = ctx == c
            assert sel.sum() == table.m[c] > 100
            want = bh_numpy(rq["pvalue"][sel])
            assert (rq["qvalue"][sel].view(np.uint64) == want.view(np.uint64)).all()
        same = (rq["pcov1"] == rq["pcov2"]) & (rq["ncov1"] == rq["ncov2"])
        assert same.sum() >= 40 and (rq["pvalue"][same] == 1.0).all() and (rq["qvalue"][same] == 1.0).all()
        assert (rq["qvalue"] >= rq["pvalue"]).all() and (rq["qvalue"] < 0.05).any()


def test_bin_pvalues_are_the_rows_pvalues(solved):
    for min_cov in (1, 5):
        bins, _big, table, rows, _rq = solved[min_cov]
        tab = table.tab
        assert (np.diff(tab["bin"].astype(np.int64)) > 0).all() and (tab["reserved"] == 0).all()
        assert _nonzero(bins) == dict(zip(tab["bin"].tolist(), tab["count"].tolist()))
        dense = (rows["pcov1"].astype(np.int64) + rows["ncov1"] < ASM_T) & (rows["pcov2"].astype(np.int64) + rows["ncov2"] < ASM_T)
        r = rows[dense]
        b = bin_index(np.minimum(r["motif"], 2).astype(np.int64), *(r[f].astype(np.int64) for f in ("pcov1", "ncov1", "pcov2", "ncov2")))
        assert set(b.tolist()) == set(tab["bin"].tolist())
        j = np.searchsorted(tab["bin"], b)
        assert (tab["pvalue"][j].view(np.uint64) == r["pvalue"].view(np.uint64)).all()                            # (c)
    assert len(solved[1][2].tab) > len(solved[5][2].tab) > 200


def _moved(rows, shift):
    out = rows.copy()
    out["gpos"] += shift
    return out


def test_histogram_of_two_halves_with_plane_base(crafted, solved):
    """`shift` is what locus 0 of the crafted planes is called.  Beyond 0 it puts the second half's first locus (mid = 6001) on
    2^31 and on 2^32: the rows' gpos = plane_base + i and the binary search by gpos in the job's big list then run over loci on
    both sides of the boundary."""
    from hifimeth_amd.pileup import AsmTable
    pu, _host, dev = crafted
    for shift in (0, (1 << 31) - 6001, (1 << 32) - 6001):
        table = solved[5][2]
        table = AsmTable(table.tab, _moved(table.big, shift), table.big_q, table.m)     # the job-wide list, where the job's loci are
        B = shift + 6001
        assert shift == 0 or ((table.big["gpos"] < B).sum() > 10 and (table.big["gpos"] >= B).sum() > 10)
        for mid in (4096, 6001):                                                                                  # (d)
            bins, big_lo = pu.asm_histogram(0, mid, 5, planes=dev, plane_base=shift)
            chunk = [t[mid:] for t in dev]                    # a rank's chunk: element 0 is locus `mid`
            _b, big_hi = pu.asm_histogram(0, N_LOCI - mid, 5, planes=chunk, plane_base=shift + mid, bins=bins)
            assert (bins == solved[5][0]).all()
            assert len(big_lo) and len(big_hi) and (np.concatenate([big_lo, big_hi]) == _moved(solved[5][1], shift)).all()
            rq = pu.asm(0, N_LOCI - mid, 5, planes=chunk, plane_base=shift + mid, table=table)
            want = _moved(solved[5][4], shift)
            assert (rq == want[want["gpos"] >= shift + mid]).all() and not np.isnan(rq["qvalue"]).any()
            whole = pu.asm(0, N_LOCI, 5, planes=dev, plane_base=shift, table=table)
            assert whole.tobytes() == want.tobytes()


def test_cap_rule(crafted, solved):
    from hifimeth_amd.pileup import ASM_BIN_DTYPE, ASM_DTYPE
    pu, _host, dev = crafted
    L, ptrs = pu._L, [ctypes.c_void_p(t.data_ptr()) for t in dev]
    bins0, big0, table, _rows, rq0 = solved[5]
    n_big, n_tab = len(big0), len(table.tab)
    bins = np.full(ASM_BINS, 3, np.uint64)
    big = np.zeros(n_big, ASM_DTYPE)
    big["gpos"] = -7
    pb, pg = bins.ctypes.data_as(ctypes.c_void_p), big.ctypes.data_as(ctypes.c_void_p)
    hist = lambda big_ptr, cap: L.hm_pileup_asm_histogram(pu._h, *ptrs, 0, 0, N_LOCI, 5, pb, big_ptr, cap)   # noqa: E731
    assert hist(pg, n_big - 1) == n_big and hist(None, 0) == n_big and hist(None, n_big) == n_big                 # (e)
    assert (bins == 3).all() and (big["gpos"] == -7).all() and (big["pvalue"] == 0).all()
    assert hist(pg, n_big) == n_big and (big == big0).all() and (bins - 3 == bins0).all()
    assert L.hm_pileup_asm_histogram(pu._h, *ptrs, 0, 77, 77, 5, pb, None, 0) == 0 and (bins - 3 == bins0).all()
    tab = np.zeros(n_tab, ASM_BIN_DTYPE)
    tab["bin"] = 12345
    pt, pb0 = tab.ctypes.data_as(ctypes.c_void_p), bins0.ctypes.data_as(ctypes.c_void_p)
    assert L.hm_pileup_asm_bin_pvalues(pu._h, pb0, pt, n_tab - 1) == n_tab and (tab["bin"] == 12345).all() and (tab["count"] == 0).all()
    assert L.hm_pileup_asm_bin_pvalues(pu._h, pb0, None, 0) == n_tab
    assert L.hm_pileup_asm_bin_pvalues(pu._h, pb0, pt, n_tab) == n_tab
    assert np.isnan(tab["qvalue"]).all() and (tab[["bin", "count", "pvalue"]] == table.tab[["bin", "count", "pvalue"]]).all()
    out = np.zeros(len(rq0), rq0.dtype)
    out["gpos"] = -7
    args = (table.tab.ctypes.data_as(ctypes.c_void_p), n_tab, big0.ctypes.data_as(ctypes.c_void_p),
            table.big_q.ctypes.data_as(ctypes.c_void_p), n_big, out.ctypes.data_as(ctypes.c_void_p))
    assert L.hm_pileup_fetch_asm_q(pu._h, *ptrs, 0, 0, N_LOCI, 5, *args, len(rq0) - 1) == len(rq0) and (out["gpos"] == -7).all()
    assert L.hm_pileup_fetch_asm_q(pu._h, *ptrs, 0, 0, N_LOCI, 5, *args, len(rq0)) == len(rq0) and (out == rq0).all()


def test_missing_entries_give_nan_not_a_wrong_q(crafted, solved):
    from hifimeth_amd.pileup import AsmTable
    pu, _host, dev = crafted
    _bins, big, table, _rows, rq5 = solved[5]
    # (f) a big locus absent from the list: that row NaN, every other row as before
    for drop in (0, len(big) // 2, len(big) - 1):
        keep = np.arange(len(big)) != drop
        got = pu.asm(0, N_LOCI, 5, planes=dev, table=AsmTable(table.tab, big[keep].copy(), table.big_q[keep].copy(), table.m))
        at = got["gpos"] == big["gpos"][drop]
        assert at.sum() == 1 and np.isnan(got["qvalue"][at]).all() and (got[~at] == rq5[~at]).all()
    # no big list at all, no table at all
    got = pu.asm(0, N_LOCI, 5, planes=dev, table=AsmTable(table.tab, big[:0].copy(), table.big_q[:0].copy(), table.m))
    is_big = np.isin(got["gpos"], big["gpos"])
    assert np.isnan(got["qvalue"][is_big]).all() and (got[~is_big] == rq5[~is_big]).all()
    got = pu.asm(0, N_LOCI, 5, planes=dev, table=AsmTable(table.tab[:0].copy(), big, table.big_q, table.m))
    assert np.isnan(got["qvalue"][~is_big]).all() and (got[is_big] == rq5[is_big]).all()
    # a table solved for min_cov 5 under a fetch with min_cov 1: a tuple the table does not hold gets NaN, never another tuple's q
    got = pu.asm(0, N_LOCI, 1, planes=dev, table=table)
    low = np.minimum(got["pcov1"] + got["ncov1"], got["pcov2"] + got["ncov2"]) < 5
    assert low.sum() > 500 and np.isnan(got["qvalue"][low]).all()
    assert (got[~low] == rq5).all()


def test_abi_errors(crafted):
    from hifimeth_amd.pileup import MethylationPileup
    pu, _host, dev = crafted
    L, ptrs, none = pu._L, [ctypes.c_void_p(t.data_ptr()) for t in dev], [None] * 5
    bins = np.zeros(ASM_BINS, np.uint64)
    pb = bins.ctypes.data_as(ctypes.c_void_p)
    h, f = L.hm_pileup_asm_histogram, L.hm_pileup_fetch_asm_q
    assert h(pu._h, *none, 0, 0, 100, 5, pb, None, 0) == -5 and b"partitions" in L.hm_pileup_last_error(pu._h)  # HM_ESTATE
    assert f(pu._h, *none, 0, 0, 100, 5, None, 0, None, None, 0, None, 0) == -5
    for k in range(5):
        mix = list(ptrs)
        mix[k] = None
        assert h(pu._h, *mix, 0, 0, 100, 5, pb, None, 0) == -1 and f(pu._h, *mix, 0, 0, 100, 5, None, 0, None, None, 0, None, 0) == -1
    assert h(pu._h, *ptrs, 0, 0, 100, 0, pb, None, 0) == -1 and h(pu._h, *ptrs, 0, 9, 8, 5, pb, None, 0) == -1
    assert h(pu._h, *ptrs, 0, 0, 100, 5, None, None, 0) == -1 and h(None, *ptrs, 0, 0, 100, 5, pb, None, 0) == -1
    assert f(pu._h, *ptrs, 0, 0, 100, 5, None, 3, None, None, 0, None, 0) == -1          # entries announced, no table
    assert not bins.any()
    # a non-empty bin no tested locus can fall in: a haplotype total of 0
    for bad in (0, bin_index(1, 0, 0, 3, 3), bin_index(2, 3, 3, 0, 0)):
        bins[bad] = 1
        assert L.hm_pileup_asm_bin_pvalues(pu._h, pb, None, 0) == -1
        bins[bad] = 0
    assert L.hm_pileup_asm_bin_pvalues(pu._h, pb, None, 0) == 0 and L.hm_pileup_asm_bin_pvalues(pu._h, None, None, 0) == -1
    bins[bin_index(2, 63, 0, 0, 63)] = 5                      # the last dense tuple needs no planes and no reference
    bare = MethylationPileup.__new__(MethylationPileup)
    bare._L, bare._h = L, ctypes.c_void_p()
    assert L.hm_pileup_create(ctypes.byref(bare._h), 0) == 0
    tab = bare.asm_bin_pvalues(bins)
    bare.close()
    assert len(tab) == 1 and tab["count"][0] == 5 and tab["bin"][0] == bin_index(2, 63, 0, 0, 63) and 0 < tab["pvalue"][0] < 1e-30


# ---- through reads: the engine's own planes, the CLI, the distributed driver --------------------------------------------------------
class _Ptr:
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p.value


def _mirror(pu, min_cov):
    from hifimeth_amd.pileup import asm_qvalues
    bins, big = pu.asm_histogram(min_cov=min_cov)
    table = asm_qvalues(pu.asm_bin_pvalues(bins), big)
    return table, pu.asm(min_cov=min_cov, table=table)


def test_own_planes_through_reads():
    from hifimeth_amd.pileup import ASM_DTYPE
    genome, reads = _phased_reads()
    pu = _engine(genome, reads, partitions=True)
    table, rq = _mirror(pu, 3)                                                                                    # (g)
    rows = pu.asm(min_cov=3)
    assert len(rows) >= 200 and np.ascontiguousarray(rq[list(ASM_DTYPE.names)]).astype(ASM_DTYPE).tobytes() == rows.tobytes()
    ctx = np.minimum(rq["motif"], 2)
    for c in range(3):
        assert (ctx == c).sum() == table.m[c] > 0
        assert (rq["qvalue"][ctx == c].view(np.uint64) == bh_numpy(rq["pvalue"][ctx == c]).view(np.uint64)).all()
    assert (rq["qvalue"] <= 0.05).sum() >= 10 and (rq["qvalue"] == 1.0).any()
    # the same planes handed over as the caller's, whole and per sequence with a plane_base: the same rows
    ptr = [ctypes.c_void_p() for _ in range(5)]
    for part in (1, 2):
        pu._check(pu._L.hm_pileup_partition_planes(pu._h, part, ctypes.byref(ptr[2 * part - 2]), ctypes.byref(ptr[2 * part - 1])))
    pu._check(pu._L.hm_pileup_planes(pu._h, None, None, ctypes.byref(ptr[4]), None))
    assert (pu.asm(min_cov=3, planes=[_Ptr(p) for p in ptr], table=table) == rq).all()
    per_seq = []
    for s in range(len(genome)):
        o, n = int(pu.offsets[s]), int(pu.lengths[s])
        chunk = [_Ptr(ctypes.c_void_p(p.value + 4 * o)) for p in ptr]
        per_seq.append(pu.asm(0, n, 3, planes=chunk, plane_base=o, table=table))
    assert (np.concatenate(per_seq) == rq).all()
    pu.close()


def test_cli_asm_q(tmp_path):
    from bamutil import write_fasta
    from hifimeth_amd.pileup import asm_summary_tsv
    genome, reads = _phased_reads()
    bam, fa, prefix = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "out")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    _run_cli(["-H", "-A", "-a", "3", fa, bam, prefix + "0"])
    r1 = _run_cli(["-H", "-A", "-a", "3", "-Q", fa, bam, prefix + "1"])
    assert "asm.summary.tsv" in r1.stderr
    assert _cov_files(prefix + "0") == _cov_files(prefix + "1")
    assert not os.path.exists(prefix + "0.asm.summary.tsv")
    plain, with_q = _asm_files(prefix + "0"), _asm_files(prefix + "1")
    pu = _engine(genome, reads, partitions=True)
    table, rq = _mirror(pu, 3)
    mirror = pu.asm_bed(rq)
    pu.close()
    for c in CTX:
        lines = with_q[c].splitlines()
        assert lines and all(len(x.split("\t")) == 10 for x in lines)
        assert [x.rsplit("\t", 1)[0] for x in lines] == plain[c].splitlines()                  # columns 1-9: the files without -Q
        assert with_q[c] == mirror[c]                                                           # column 10: the mirror's %.6g
    assert open(prefix + "1.asm.summary.tsv").read() == asm_summary_tsv(table)
    assert [int(x.split("\t")[1]) for x in open(prefix + "1.asm.summary.tsv")] == [len(with_q[c].splitlines()) for c in CTX]


def test_pileup_dist_asm_q(tmp_path):
    """python -m hifimeth_amd.pileup_dist -H -A -Q on two gloo ranks sharing the card: the rank parts, concatenated in rank order,
    and the summary are the CLI's files byte for byte; the ranks' border lies inside chr2 with tested loci on both sides"""
    from bamutil import write_fasta
    genome, reads = _phased_reads()
    bam, fa = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    _run_cli(["-H", "-A", "-a", "3", "-Q", fa, bam, str(tmp_path / "cli")])
    want = (_cov_files(str(tmp_path / "cli")), _asm_files(str(tmp_path / "cli")), open(str(tmp_path / "cli.asm.summary.tsv")).read())
    border = (sum(len(s) for _, s in genome) + 1) // 2 - len(genome[0][1])
    chr2 = [int(line.split("\t")[1]) for c in CTX for line in want[1][c].splitlines() if line.startswith(genome[1][0] + "\t")]
    assert min(chr2) < border <= max(chr2) and all(len(line.split("\t")) == 10 for c in CTX for line in want[1][c].splitlines())
    prefix = str(tmp_path / "gloo")
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", "-H", "-A", "-a", "3", "-Q", "--slab", "7", "--backend", "gloo"]
    procs = [subprocess.Popen([*mod, fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29587"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert (_cov_files(prefix), _asm_files(prefix), open(prefix + ".asm.summary.tsv").read()) == want
