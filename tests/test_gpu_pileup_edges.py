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
