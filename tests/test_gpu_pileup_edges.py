"""GPU parity of the pileup kernels on the inputs hifimeth_amd.synth never makes (tests/pileup_cases.py): edge CIGARs,
reads on the first and last base of a chromosome, crowds of tiny alignments, MM/ML in other callers' dialects, identities
that hit -f exactly, covered-loci ranges beyond 1024 blocks, and malformed records.  Bit-exact against
oracle/pileup_oracle.py with the `_check` discipline of tests/test_gpu_pileup.py (histograms, projected records as a multiset,
thresholds, loci, BED text); the oracle itself is pinned on these inputs by tests/test_pileup_edges_cpu.py.

Not covered: references above 2^32 bases (the 8 high bits of gpos in a device record) need more than 50 GB of planes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pileup_cases as C
from conftest import ROOT
from test_gpu_pileup_hp import _expect, _write_bam      # the haplotype expectation and the HP-tagged BAM writer, shared

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
CTX = ("CpG", "CHG", "CHH")
HM_EDATA = -4
_CACHE = {}


@pytest.fixture(scope="module")
def P():
    from oracle import pileup_oracle
    return pileup_oracle


def _reads(name):
    if name not in _CACHE:
        _CACHE[name] = C.everything() if name == "all" else C.CLASSES[name]()
    return _CACHE[name]


def _want(P, name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = P.pileup([C.as_dict(r) for r in _reads(name)], C.genome(), **kw)
    return _CACHE[key]


def _run(genome, reads, batch=None, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(genome, **kw)
    for i, r in enumerate(reads):
        pu.add(r)
        if batch and (i + 1) % batch == 0:
            pu.flush()                    # records accumulate in HBM across runs
    pu.flush()
    return pu


def _rows(loci):
    return [(int(l["gpos"]), int(l["pcov"]), int(l["ncov"]), int(l["motif"])) for l in loci]


def _check(pu, want, thresholds=None):
    off = pu.offsets
    bins = pu.histograms()
    assert (bins == want["bins"]).all()
    g, p, m, _o = pu.records()
    exp = sorted((int(off[sid] + soff), prob, motif) for sid, soff, prob, motif in want["records"])
    assert sorted(zip(g.tolist(), p.tolist(), m.tolist())) == exp
    thr = pu.resolve_thresholds(bins) if thresholds is None else thresholds
    assert thr == want["thresholds"]
    pu.count(thr)
    assert pu.num_records() == 0
    loci = pu.loci()
    assert _rows(loci) == [(int(off[sid] + soff), pc, nc, mo) for sid, soff, pc, nc, mo in want["loci"]]
    assert pu.bed(loci) == want["bed"]
    return loci


CLASS_NAMES = [*C.CLASSES, "all"]


@pytest.mark.parametrize("batch", [1, 7, None], ids=["flush1", "flush7", "flush_end"])
@pytest.mark.parametrize("name", CLASS_NAMES)
def test_edge_classes_match_oracle(P, name, batch):
    """each class alone and all of them in one engine; a flush after every read, after every 7 reads, and once at the end:
    batch cuts must not matter"""
    reads = _reads(name)
    want = _want(P, name)
    assert want["records"] and want["bins"].sum() > 0
    pu = _run(C.genome(), reads, batch=batch)
    _check(pu, want)
    pu.close()


@pytest.mark.parametrize("batch", [1, 7, None], ids=["flush1", "flush7", "flush_end"])
@pytest.mark.parametrize("name", CLASS_NAMES)
def test_edge_classes_partitions(P, name, batch):
    """partitions=True with HP 1 / 2 / none dealt round-robin: combined output unchanged, each haplotype's planes equal the
    oracle's counts over that haplotype's records"""
    import dataclasses
    genome = C.genome()
    reads = [dataclasses.replace(r, hp=(1, 2, None)[i % 3]) for i, r in enumerate(_reads(name))]
    parts = [r.hp or 0 for r in reads]
    key = ("hp", name)
    if key not in _CACHE:
        _CACHE[key] = _expect(P, genome, reads, parts)
    comb, want = _CACHE[key]
    assert comb["loci"] == _want(P, name)["loci"]
    pu = _run(genome, reads, batch=batch, partitions=True)
    _check(pu, comb)
    off = pu.offsets
    assert sum(len(want[p][0]) for p in (1, 2)) > 0
    for part in (1, 2):
        got = pu.loci(partition=part)
        assert _rows(got) == [(int(off[sid] + soff), p, n, m) for sid, soff, p, n, m in want[part][0]]
        assert pu.bed(got) == want[part][1]
    pu.close()


def test_identity_ties_and_filters(P):
    """-f at values some reads hit exactly (39/40 = 97.5, 197/200 = 98.5): the tie reads are kept, as the oracle keeps them,
    and dropped at the next double above; tiny alignments put several reads into one wavefront of the identity kernel"""
    genome = C.genome()
    name = "ties+crowd"
    _CACHE[name] = sorted(_reads("identity_ties") + _reads("tiny_crowd"), key=lambda r: (r.tid, r.pos))
    reads = _CACHE[name]
    base = _want(P, name)
    ups = [float(np.nextafter(x, 200.0)) for x in C.TIE_VALUES]
    for kw in (dict(min_pi=C.TIE_VALUES[0]), dict(min_pi=ups[0]), dict(min_pi=C.TIE_VALUES[1]), dict(min_pi=ups[1]), dict(min_mapq=30),
               dict(min_mapq=20, min_pi=C.TIE_VALUES[0]), dict(min_pi=100.0), dict(min_pi=1e-300)):
        want = _want(P, name, **kw)
        assert (want["bins"] == base["bins"]).all()
        assert len(want["records"]) <= len(base["records"])
        for batch in (None, 5):
            pu = _run(genome, reads, batch=batch, **kw)
            _check(pu, want)
            pu.close()
    for x, up in zip(C.TIE_VALUES, ups):                      # the tie reads make the difference between x and the next double
        assert len(_want(P, name, min_pi=x)["records"]) > len(_want(P, name, min_pi=up)["records"])
    assert len(_want(P, name, min_mapq=30)["records"]) < len(base["records"])
    # the ties alone, one engine per read: a batch of one read is one wavefront's worth of columns or less
    for r in _reads("identity_ties"):
        for x in C.TIE_VALUES:
            want = P.pileup([C.as_dict(r)], genome, min_pi=x)
            pu = _run(genome, [r], min_pi=x)
            _check(pu, want)
            pu.close()


def test_cli_edge_set(P, tmp_path):
    """the whole set through `hifimeth-hip pileup` and `-H` from a BAM: every *.cov.bed byte-identical to the oracle's text"""
    from bamutil import write_fasta
    genome = C.genome()
    reads = _reads("all")
    hps = [(1, 2, 0, 3)[i % 4] for i in range(len(reads))]
    parts = [h if h in (1, 2) else 0 for h in hps]
    bam, fa, prefix = str(tmp_path / "edges.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "out")
    _write_bam(bam, genome, reads, [[("i", h)] if h else [] for h in hps])
    write_fasta(fa, genome)
    for tag, args, kw in (("a", ["-t", "4", "-b", "25"], {}), ("q", ["-q", "20", "-f", "97.5"], dict(min_mapq=20, min_pi=97.5)),
                          ("b", ["-b", "1"], {})):
        r = subprocess.run([CLI, "pileup", *args, fa, bam, prefix + tag], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        rh = subprocess.run([CLI, "pileup", *args, "-H", fa, bam, prefix + tag + "h"], capture_output=True, text=True, timeout=300)
        assert rh.returncode == 0, rh.stderr
        comb, want = _expect(P, genome, reads, parts, **kw)
        assert sum(len(want[p][0]) for p in (1, 2)) > 100
        for c in CTX:
            assert open(f"{prefix}{tag}.{c}.cov.bed").read() == comb["bed"][c], (tag, c)
            assert open(f"{prefix}{tag}h.{c}.cov.bed").read() == comb["bed"][c], (tag, c)
            for part in (1, 2):
                assert open(f"{prefix}{tag}h.hap{part}.{c}.cov.bed").read() == want[part][1][c], (tag, part, c)


# ---- covered loci of big ranges against NumPy ------------------------------------------------------------------------
BLK = 4096


def _loci_expect(pc, nc, key, lo, hi, base):
    i = np.nonzero(pc[lo:hi] | nc[lo:hi])[0] + lo
    return (base + i).astype(np.int64), pc[i], nc[i], (key[i] & 3).astype(np.uint32)


def _assert_loci(got, exp):
    gpos, pc, nc, mo = exp
    assert len(got) == len(gpos)
    assert (got["gpos"] == gpos).all() and (got["pcov"] == pc).all() and (got["ncov"] == nc).all() and (got["motif"] == mo).all()
    assert (got["reserved"] == 0).all()


def test_loci_ranges_beyond_1024_blocks():
    """loci_count / loci_scan / loci_write on caller-owned planes, no reads: ranges of 1024 blocks -1 / 0 / +1 locus (the scan's
    per-thread share goes from 1 to 2 blocks), ~6 M loci, a range that starts off a block boundary, empty, fully covered, and
    one covered locus at each end.  Expected rows = np.nonzero(pcov | ncov) with the planes' values and key & 3."""
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    n = 6_300_000
    rng = np.random.default_rng(301)
    pc = np.zeros(n, np.int32)
    nc = np.zeros(n, np.int32)
    hit = rng.random(n) < 0.01
    kind = rng.integers(0, 3, n)
    pc[hit & (kind != 1)] = rng.integers(1, 1000, int((hit & (kind != 1)).sum()))
    nc[hit & (kind != 0)] = rng.integers(1, 1000, int((hit & (kind != 0)).sum()))
    pc[5 * BLK:6 * BLK] = 7                                        # one block fully covered, its neighbours sparse
    nc[1023 * BLK - 3:1024 * BLK + 3] = 2                          # dense across the 1024-block mark
    pc[2047 * BLK - 1:2048 * BLK + 1] = 1
    key = rng.integers(0, 2 ** 31 - 1, n).astype(np.int32)
    planes = [torch.from_numpy(a).cuda() for a in (pc, nc, key)]
    pu = MethylationPileup([("c", "ACGT" * 8)])
    M = BLK * 1024
    cases = [(0, M - 1, 0), (0, M, 17), (0, M + 1, 0), (0, 6_000_001, 5_000_000_000), (1_234_567, 1_234_567 + M + 5, 10 ** 9 + 7),
             (BLK - 1, n - 1, 0), (0, n, 0), (n - 1, n, 3), (4 * BLK + 1, 4 * BLK + 2, 0), (100, 100, 0)]
    for lo, hi, base in cases:
        assert 0 <= lo <= hi <= n                                  # the engine trusts the caller's range: stay inside the planes
        exp = _loci_expect(pc, nc, key, lo, hi, base)
        # the engine reads plane[lo:hi] of the planes it is given and reports plane_base + index
        got = pu.loci(lo, hi, planes=planes, plane_base=base)
        _assert_loci(got, exp)
        assert hi - lo < 2 or len(got) > 0
    # a slice handed over as its own plane (what a rank does after the reduce-scatter): range starts at 0 of the slice
    sl = [t[777:777 + M + 1] for t in planes]
    _assert_loci(pu.loci(0, M + 1, planes=sl, plane_base=777), _loci_expect(pc, nc, key, 777, 777 + M + 1, 0))
    del planes, sl
    torch.cuda.empty_cache()

    m = M + 1
    zero = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(3)]
    assert len(pu.loci(0, m, planes=zero)) == 0                    # all empty
    zero[0][0] = 3
    zero[1][m - 1] = 4
    zero[2][m - 1] = 2
    got = pu.loci(0, m, planes=zero, plane_base=9)                 # one covered locus at each end only
    assert _rows(got) == [(9, 3, 0, 0), (9 + m - 1, 0, 4, 2)]
    assert _rows(pu.loci(1, m, planes=zero)) == [(m - 1, 0, 4, 2)]
    assert _rows(pu.loci(0, m - 1, planes=zero)) == [(0, 3, 0, 0)]
    zero[0].fill_(1)                                               # all covered
    zero[1].zero_()
    zero[2].copy_(torch.arange(m, dtype=torch.int32, device="cuda"))
    got = pu.loci(0, m, planes=zero, plane_base=1)
    assert len(got) == m and (got["gpos"] == np.arange(1, m + 1)).all() and (got["pcov"] == 1).all()
    assert (got["ncov"] == 0).all() and (got["motif"] == (np.arange(m) & 3)).all()
    del zero, got
    torch.cuda.empty_cache()
    pu.close()


# ---- the shared count / scan / write skeleton: loci, asm, site histogram and sites rows on one set of crafted planes --------------
SK_N = 3 * BLK + 5
SK_NEG = {"pcov1": 5000, "ncov1": 5001, "pcov2": 5002, "ncov2": 5003}     # the locus whose counter in that plane is negative
SK_BIG = (6000, 7000)                                                    # pcov + ncov >= 256
SK_EDGES = (0, 63, 64, 255, 256, BLK - 1, BLK, 2 * BLK - 1, 2 * BLK, SK_N - 1)
SK_RANGES = ((0, SK_N), (1, SK_N - 1), (BLK - 1, BLK + 1), (BLK + 1, BLK + 1))
SK_SLICE = 100                                                           # planes handed over from this locus on, plane_base = it
# what locus 0 of the crafted planes is called: 0, or a rank's base that puts the rows' gpos across B = 2^31 / 2^32 -- the two big
# loci on either side of B (the binary search in the job-wide big list then runs over entries that differ in bit 31 / 32), or a
# block boundary of the planes on B
SK_BASES = [0] + [B - x for B in (1 << 31, 1 << 32) for x in (SK_BIG[0] + 1, BLK)]


def _skeleton_planes():
    """-> dict of int32 planes.  Block 0 is fully selected (with it locus 0 and both sides of the lane boundary 63 / 64, of the
    256-thread iteration boundary 255 / 256 and, with locus 4096, of the block boundary); block 1 holds the sparse loci, the
    negative counters and the big loci; of block 2 only its first locus is selected, and the last locus of the planes is.  Every
    aligned block of (0, n) therefore holds a selected locus (0, 4096, 8192 and the last one must be selected), so the block with
    no selected locus is the third block of the range (1, n - 1), [8193, 12289)."""
    i = np.arange(SK_N)
    rng = np.random.default_rng(302)
    h = {k: np.zeros(SK_N, np.int64) for k in ("pcov1", "ncov1", "pcov2", "ncov2")}
    full = i < BLK
    h["pcov1"][full], h["ncov1"][full] = 1 + i[full] % 5, 2 + i[full] % 3            # each haplotype's sum >= 3
    h["pcov2"][full], h["ncov2"][full] = 3 + i[full] % 2, i[full] % 7
    sparse = BLK + 1 + rng.choice(BLK - 2, 700, replace=False)                       # inside block 1, its two ends left alone
    for k in h:                                                                      # 0 .. 4 per counter: some loci fail min_cov 1 or 3
        h[k][sparse] = rng.integers(0, 5, len(sparse))
    for e in (BLK, 2 * BLK - 1, 2 * BLK, SK_N - 1):
        h["pcov1"][e], h["ncov1"][e], h["pcov2"][e], h["ncov2"][e] = 4, 1, 2, 3
    for k, at in SK_NEG.items():
        for j in h:
            h[j][at] = 0 if j[0] == k[0] else 6                                      # the other haplotype's same counter is 0: the sum is negative too
        h[k][at] = -2
    h["pcov1"][SK_BIG[0]], h["ncov1"][SK_BIG[0]], h["pcov2"][SK_BIG[0]], h["ncov2"][SK_BIG[0]] = 200, 100, 50, 30
    h["pcov1"][SK_BIG[1]], h["ncov1"][SK_BIG[1]], h["pcov2"][SK_BIG[1]], h["ncov2"][SK_BIG[1]] = 0, 128, 128, 0
    h["pcov"], h["ncov"] = h["pcov1"] + h["pcov2"], h["ncov1"] + h["ncov2"]
    h["key"] = (rng.integers(0, 1 << 20, SK_N) << 2) | (i & 3)
    return {k: v.astype(np.int32) for k, v in h.items()}


def _sk_loci(h):
    return (h["pcov"] | h["ncov"]) != 0                                              # a negative counter counts as covered


def _sk_asm(h, min_cov):
    p1, n1, p2, n2 = (h[k].astype(np.int64) for k in ("pcov1", "ncov1", "pcov2", "ncov2"))
    return ((p1 | n1 | p2 | n2) >= 0) & (p1 + n1 >= min_cov) & (p2 + n2 >= min_cov)


def _sk_counted(h):
    return (h["pcov"] | h["ncov"]) > 0


def _sk_sites(h, ctx_mask):
    return _sk_counted(h) & (((ctx_mask >> np.minimum(h["key"] & 3, 2)) & 1) != 0)


def _sk_histogram(h, lo, hi):
    """-> (bins [3, 256, 256], selection of the big loci) of planes[lo, hi)"""
    big = _sk_counted(h) & (h["pcov"].astype(np.int64) + h["ncov"] >= 256)
    at = np.nonzero((_sk_counted(h) & ~big)[lo:hi])[0] + lo
    bins = np.zeros((3, 256, 256), np.uint64)
    np.add.at(bins, (np.minimum(h["key"][at] & 3, 2), h["pcov"][at].astype(np.int64) + h["ncov"][at], h["pcov"][at]), 1)
    return bins, big


def test_skeleton_planes_hold_the_cases():
    h = _skeleton_planes()
    assert len(h["key"]) == SK_N == 3 * 4096 + 5
    assert (h["pcov"] == h["pcov1"] + h["pcov2"]).all() and (h["ncov"] == h["ncov1"] + h["ncov2"]).all()
    every = _sk_loci(h) & _sk_asm(h, 3) & _sk_sites(h, 7)
    assert (every & _sk_sites(h, 5))[list(SK_EDGES)].all()      # 0, 63 | 64, 255 | 256, 4095 | 4096, 8191 | 8192, the last locus
    assert every[:BLK].all()                                    # one block fully selected ...
    for sel in (_sk_loci(h), _sk_asm(h, 1), _sk_sites(h, 7)):   # ... and one with none, in the ranges whose third block is [8193, 12289)
        assert not sel[2 * BLK + 1:3 * BLK + 1].any()
        assert 0 < sel[BLK:2 * BLK].sum() < BLK
    assert (1, SK_N - 1) in SK_RANGES and 1 + 3 * BLK < SK_N - 1                     # [1 + 2 * 4096, 1 + 3 * 4096) is a whole block of it
    for k, at in SK_NEG.items():                                # in loci, not in sites, not in asm
        assert h[k][at] < 0 and sum(h[j][at] < 0 for j in ("pcov1", "ncov1", "pcov2", "ncov2")) == 1
        assert _sk_loci(h)[at] and not _sk_counted(h)[at] and not _sk_asm(h, 1)[at]
    assert (h["pcov"][list(SK_NEG.values())] < 0).sum() == 2 and (h["ncov"][list(SK_NEG.values())] < 0).sum() == 2
    tot = h["pcov"].astype(np.int64) + h["ncov"]
    assert (tot[list(SK_BIG)] >= 256).all() and (_sk_counted(h) & (tot >= 256)).sum() == len(SK_BIG)
    assert {0, 1, 2, 3} == set((h["key"] & 3)[_sk_loci(h)].tolist()) and ((h["key"] & 3) == 3)[_sk_counted(h)].sum() > 1000
    assert _sk_asm(h, 1).sum() > _sk_asm(h, 3).sum() > BLK and _sk_loci(h).sum() > _sk_asm(h, 1).sum()
    assert _sk_sites(h, 7).sum() > _sk_sites(h, 5).sum() > 0


@pytest.mark.parametrize("base", SK_BASES, ids=["base0", "big_loci_at_2^31", "block_at_2^31", "big_loci_at_2^32", "block_at_2^32"])
def test_one_skeleton_behind_loci_asm_and_sites(base):
    """With `base` the planes' first locus is called `base` instead of 0 (every plane_base below is counted from it): the rows'
    gpos = plane_base + i and the lookups by gpos in the big list then cross 2^31 / 2^32.
    pu.loci, pu.asm (min_cov 1 and 3), pu.site_histogram and pu.sites (ctx_mask 7 and 5) over the crafted planes against NumPy,
    field for field, with the three predicates written out above (_sk_loci, _sk_asm, _sk_sites; big loci: _sk_histogram): the
    whole planes, (1, n - 1), two loci across a block boundary, an empty range, and sliced planes with a plane_base.  p and q of a sites row are the table's entries bit for bit; asm's diff is numpy's bit for bit and its pvalue is
    within the bounds test_gpu_pileup_asm.py derives (1e-9 relative for row sums <= 24, 1e-6 above).  Through the raw ABI each of
    the three fetches, given cap = n - 1, returns n and leaves `out` as it was."""
    import torch
    from hifimeth_amd.pileup import ASM_DTYPE, LOCUS_DTYPE, SITE_DTYPE, MethylationPileup, sites_table
    from test_gpu_pileup_asm import _np_diff, _rel_err, fisher_exact
    h = _skeleton_planes()
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in h.items()}
    pu = MethylationPileup([("c", "ACGT" * 8)])
    i64 = {k: v.astype(np.int64) for k, v in h.items()}
    motif3, motif2 = i64["key"] & 3, np.minimum(i64["key"] & 3, 2)
    fisher = {}

    def planes(names, start=0):
        return [dev[k][start:] for k in names]

    def check_common(rows, sel, lo, hi, fields, motif):
        at = np.nonzero(sel[lo:hi])[0] + lo
        assert len(rows) == len(at) and rows["gpos"].dtype == np.int64 and (rows["gpos"] == base + at).all(), (lo, hi)
        assert (rows["reserved"] == 0).all(), (lo, hi)
        for f in fields:
            assert (rows[f] == h[f][at]).all(), (f, lo, hi)
        assert (rows["motif"] == motif[at]).all(), (lo, hi)
        return at

    def check_asm(rows, at):
        want = _np_diff(*(i64[k][at] for k in ("pcov1", "ncov1", "pcov2", "ncov2")))
        assert (rows["diff"].view(np.uint64) == want.view(np.uint64)).all()
        distinct = np.unique(np.stack([i64[k][at] for k in ("pcov1", "ncov1", "pcov2", "ncov2")] + [rows["pvalue"].view(np.int64)], axis=1), axis=0)
        for *t, bits in distinct.tolist():                               # every distinct (table, value) once
            t = tuple(t)
            if t not in fisher:
                fisher[t] = fisher_exact(*t)
            pvalue = float(np.array(bits, np.int64).view(np.float64))
            assert _rel_err(pvalue, fisher[t]) <= (1e-9 if max(t[0] + t[1], t[2] + t[3]) <= 24 else 1e-6), t

    # one histogram and one table per ctx_mask for the whole planes: a range's rows look their p and q up in it
    bins, big = pu.site_histogram(0, SK_N, planes=planes(("pcov", "ncov", "key")), plane_base=base)
    assert [int(g) for g in big["gpos"]] == [base + g for g in SK_BIG]
    if base:
        B = base + SK_BIG[0] + 1 if base & (BLK - 1) else base + BLK
        assert B in (1 << 31, 1 << 32) and base < B < base + SK_N and (big["gpos"][0] < B <= big["gpos"][1]) == bool(base & (BLK - 1))
    tables = {7: sites_table([0.02, 0.05, 0.013], bins, big), 5: sites_table([0.02, float("nan"), 0.013], bins, big)}
    assert {m: t.ctx_mask for m, t in tables.items()} == {7: 7, 5: 5}
    big_at = {int(g) - base: k for k, g in enumerate(big["gpos"])}

    def check_sites(rows, at, table):
        tot = i64["pcov"][at] + i64["ncov"][at]
        small = tot < 256
        for name, tab, bigtab in (("pvalue", table.ptab, table.big_p), ("qvalue", table.qtab, table.big_q)):
            want = np.empty(len(at))
            want[small] = tab[motif2[at][small], tot[small], i64["pcov"][at][small]]
            want[~small] = bigtab[[big_at[int(g)] for g in at[~small]]]
            assert (rows[name].view(np.uint64) == want.view(np.uint64)).all(), name
            assert not np.isnan(rows[name]).any()

    seen = dict(loci=0, asm=0, sites=0, big=0)
    for lo, hi, start in [(lo, hi, 0) for lo, hi in SK_RANGES] + [(5, SK_N - SK_SLICE, SK_SLICE)]:
        a, b = start + lo, start + hi                                # the same range in the coordinates of the whole planes
        assert 0 <= a <= b <= SK_N                                   # the engine trusts the caller's range: stay inside the planes
        kw = dict(plane_base=base + start)
        rows = pu.loci(lo, hi, planes=planes(("pcov", "ncov", "key"), start), **kw)
        seen["loci"] += len(check_common(rows, _sk_loci(h), a, b, ("pcov", "ncov"), motif3))
        for min_cov in (1, 3):
            rows = pu.asm(lo, hi, min_cov=min_cov, planes=planes(("pcov1", "ncov1", "pcov2", "ncov2", "key"), start), **kw)
            at = check_common(rows, _sk_asm(h, min_cov), a, b, ("pcov1", "ncov1", "pcov2", "ncov2"), motif3)
            check_asm(rows, at)
            seen["asm"] += len(at)
        got_bins, got_big = pu.site_histogram(lo, hi, planes=planes(("pcov", "ncov", "key"), start), **kw)
        want_bins, big_sel = _sk_histogram(h, a, b)
        assert (got_bins == want_bins).all(), (lo, hi)
        seen["big"] += len(check_common(got_big, big_sel, a, b, ("pcov", "ncov"), motif2))
        for mask, table in tables.items():
            rows = pu.sites(table, lo, hi, planes=planes(("pcov", "ncov", "key"), start), **kw)
            at = check_common(rows, _sk_sites(h, mask), a, b, ("pcov", "ncov"), motif2)
            check_sites(rows, at, table)
            seen["sites"] += len(at)
    assert min(seen.values()) > 0
    # the point of the negative counters: such a locus is a row of loci and of nothing else
    neg = sorted(SK_NEG.values())
    lo, hi = neg[0] - 1, neg[-1] + 2
    assert set(neg) <= set(pu.loci(lo, hi, planes=planes(("pcov", "ncov", "key")))["gpos"].tolist())
    assert not set(neg) & set(pu.asm(lo, hi, min_cov=1, planes=planes(("pcov1", "ncov1", "pcov2", "ncov2", "key")))["gpos"].tolist())
    assert not set(neg) & set(pu.sites(tables[7], lo, hi, planes=planes(("pcov", "ncov", "key")))["gpos"].tolist())

    # cap one below the count, raw ABI: the count comes back and the sentinel-filled rows stay as they were
    vp = ctypes.c_void_p
    ptr3 = [vp(dev[k].data_ptr()) for k in ("pcov", "ncov", "key")]
    ptr5 = [vp(dev[k].data_ptr()) for k in ("pcov1", "ncov1", "pcov2", "ncov2", "key")]
    t7 = tables[7]
    tab_args = (*(x.ctypes.data_as(vp) for x in (t7.ptab, t7.qtab, t7.big, t7.big_p, t7.big_q)), len(t7.big))
    for dtype, n, call in (
            (LOCUS_DTYPE, int(_sk_loci(h).sum()), lambda out, cap: pu._L.hm_pileup_fetch_loci(pu._h, *ptr3, 0, 0, SK_N, out, cap)),
            (ASM_DTYPE, int(_sk_asm(h, 1).sum()), lambda out, cap: pu._L.hm_pileup_fetch_asm(pu._h, *ptr5, 0, 0, SK_N, 1, out, cap)),
            (SITE_DTYPE, int(_sk_sites(h, 7).sum()), lambda out, cap: pu._L.hm_pileup_fetch_sites(pu._h, *ptr3, 0, 0, SK_N, 7, *tab_args, out, cap))):
        out = np.frombuffer(b"\xa5" * (dtype.itemsize * n), dtype).copy()
        assert n > BLK and call(out.ctypes.data_as(vp), n - 1) == n
        assert out.tobytes() == b"\xa5" * (dtype.itemsize * n), dtype
        assert call(None, 0) == n
    pu.close()


# ---- submit-time errors ---------------------------------------------------------------------------------------------
def _submit(pu, read, mods=None):
    """hm_pileup_submit_read as MethylationPileup.add calls it, returning (code, message) instead of raising"""
    from hifimeth_amd.pileup import parse_mods
    if mods is None:
        mods = parse_mods(read.seq, read.flag, read.mm, read.ml)
    seq4 = np.ascontiguousarray(read.seq4, np.uint8)
    cig = np.ascontiguousarray(read.cigar_u32(), np.uint32)
    order = pu._order
    pu._order += 1
    rc = pu._L.hm_pileup_submit_read(pu._h, order, read.flag, read.tid, read.pos, read.mapq, len(read.seq),
                                     seq4.ctypes.data_as(ctypes.c_void_p), len(cig), cig.ctypes.data_as(ctypes.c_void_p), len(mods),
                                     mods.ctypes.data_as(ctypes.c_void_p))
    return rc, pu._L.hm_pileup_last_error(pu._h).decode()


def test_submit_errors_leave_the_batch_unchanged(P):
    from hifimeth_amd import HifimethError
    from hifimeth_amd.pileup import MethylationPileup, parse_mods
    genome = C.genome()
    good = [r for r in _reads("all") if r.name in ("zoo_all_ops_f", "zoo_tick1_r", "bnd_whole1_r")]
    good.sort(key=lambda r: r.name, reverse=True)                  # the whole-chromosome read last
    assert len(good) == 3
    bad = C.bad_records()
    assert {n.split("_")[1][:6] for n, _r, _m in bad} == {"nibble", "cigar", "past"} and len(bad) == 12
    pu = MethylationPileup(genome)
    assert pu.add(good[0]) == 1
    kept = [good[0]]
    for i, (name, read, msg) in enumerate(bad):
        rc, err = _submit(pu, read)
        assert rc == HM_EDATA and msg in err, (name, rc, err)
        with pytest.raises(HifimethError, match=msg):           # and through the Python mirror
            pu.add(read)
        if i == 4:                                                  # a good read between refusals joins the same batch
            assert pu.add(good[1]) == 1
            kept.append(good[1])
    # a modification offset outside the read, behind valid entries of the same read (they must not stay staged)
    src = good[2]
    mods = parse_mods(src.seq, src.flag, src.mm, src.ml)
    for qoff in (src.l_qseq, -1, 2 ** 31 - 1):
        m = mods.copy()
        m["qoff"][len(m) // 2] = qoff
        rc, err = _submit(pu, src, m)
        assert rc == HM_EDATA and "modification offset outside the read" in err, (qoff, rc, err)
    assert pu.add(good[2]) == 1
    kept.append(good[2])
    pu.flush()
    want = P.pileup([C.as_dict(r) for r in kept], genome)
    assert len(want["records"]) > 50
    _check(pu, want)
    # the engine is usable afterwards: a second round on the same handle adds to the planes
    for r in kept:
        assert pu.add(r) == 1
    pu.flush()
    assert pu.num_records() == len(want["records"])
    pu.count(want["thresholds"])
    twice = pu.loci()
    assert _rows(twice) == [(int(pu.offsets[s] + o), 2 * p, 2 * n, m) for s, o, p, n, m in want["loci"]]
    pu.close()
