"""`pileup -R` / `pileup -J` on the GPU: hm_pileup_fetch_regions and hm_pileup_fetch_metaplot against the numpy restatement
(tests/regions_ref.py) at the block and scan-partition boundaries of the two-level index, on chunks, on counters that need 64 bits,
on real records, and through the four front ends.  Every integer is compared by equality."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import pileup_cases as C
import regions_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL, HM_ESTATE = -1, -5
THR = (128, 100, 60)
_CACHE = {}


def _geometry():
    from hifimeth_amd.pileup import region_geometry
    return region_geometry()


def _pu():
    """one engine for every query over planes handed in as tensors"""
    if "pu" not in _CACHE:
        from hifimeth_amd.pileup import MethylationPileup
        _CACHE["pu"] = MethylationPileup(C.genome())
    return _CACHE["pu"]


def _synthetic(n, seed, covered=0.5, top=6):
    """host planes of n loci: about `covered` of them with counts below `top`, random contexts under random order bits"""
    rng = np.random.default_rng(seed)
    on = rng.random(n) < covered
    pc = np.where(on, rng.integers(0, top, n), 0).astype(np.int32)
    nc = np.where(on, rng.integers(0, top, n), 0).astype(np.int32)
    ky = ((rng.integers(0, 1 << 20, n) << 2) | rng.integers(0, 3, n)).astype(np.int32)
    return pc, nc, ky


def _dev(planes):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes)


def _block_planes():
    if "block" not in _CACHE:
        B, _ = _geometry()
        host = _synthetic(3 * B + 5, 11)
        _CACHE["block"] = (host, _dev(host), R.Running(*host))
    return _CACHE["block"]


def _got(sums):
    return np.stack([sums[k] for k in R.QUANTITIES], axis=-1).astype(np.int64)


def _points():
    B, _ = _geometry()
    return [0, 1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B, 3 * B + 4, 3 * B + 5]


def _pairs(points):
    return np.array([(a, b) for a in points for b in points if a < b], np.int64).T


def test_block_boundaries():
    host, dev, run = _block_planes()
    start, end = _pairs(_points())
    want = R.region_sums(run, start, end)
    assert (want[:, :, 0].sum(axis=1) == 0).any() and (want[:, :, 0] > 0).all(axis=1).any()
    got = _got(_pu().regions(start, end, planes=dev, hi=len(host[0])))
    assert got.shape == want.shape and (got == want).all()


def test_non_zero_base_and_unaligned_lo():
    host, dev, _ = _block_planes()
    B, _ = _geometry()
    base, lo, hi = 1000003, B // 2 + 7, len(host[0]) - 3
    assert lo % B
    run = R.Running(*host, base=base)
    start, end = _pairs(_points()) + base
    want = R.region_sums(run, start, end, lo=base + lo, hi=base + hi)
    got = _got(_pu().regions(start, end, lo=lo, hi=hi, planes=dev, plane_base=base))
    assert (got == want).all() and want.any()
    far = _got(_pu().regions([0, base + hi], [base + lo, base + hi + 50], lo=lo, hi=hi, planes=dev, plane_base=base))
    assert not far.any()                                                          # wholly outside the range: clamped to nothing


def test_chunks_add_up():
    host, dev, run = _block_planes()
    B, _ = _geometry()
    n = len(host[0])
    start, end = _pairs(_points())
    whole = R.region_sums(run, start, end)
    for cut in (1, B - 1, B, B + 1, 2 * B, 3 * B + 4):
        left = _got(_pu().regions(start, end, lo=0, hi=cut, planes=dev))
        right = _got(_pu().regions(start, end, lo=0, hi=n - cut, planes=tuple(t[cut:] for t in dev), plane_base=cut))
        assert (left + right == whole).all(), cut
        assert (left == R.region_sums(run, start, end, lo=0, hi=cut)).all(), cut
        assert (_got(_pu().regions(start, end, lo=cut, hi=n, planes=dev)) == right).all(), cut


def test_64_bit_arithmetic():
    big = 2 ** 31 - 1
    pc = np.array([0, big, big, big, 1, 0, big, 0], np.int32)
    nc = np.array([0, big, big, big, 0, 0, 0, 0], np.int32)
    ky = np.array([0, 0, 0, 0, 1, 0, 2, 0], np.int32)
    got = _got(_pu().regions([0, 1, 6], [8, 4, 7], planes=_dev((pc, nc, ky)), hi=8))
    assert got[0].tolist() == [[3, 3 * big, 3 * big, 1500000], [1, 1, 0, 1000000], [1, big, 0, 1000000]] and 3 * big > 2 ** 32
    assert got[1].tolist() == [[3, 3 * big, 3 * big, 1500000], [0] * 4, [0] * 4]
    assert (got == R.region_sums(R.Running(pc, nc, ky), [0, 1, 6], [8, 4, 7])).all()
    deep = _got(_pu().regions([0], [8], min_cov=2 * big, planes=_dev((pc, nc, ky)), hi=8))           # cov = 2^32 - 2 does not wrap
    assert deep[0].tolist() == [[3, 3 * big, 3 * big, 1500000], [0] * 4, [0] * 4]


@pytest.mark.parametrize("min_cov", [1, 2, 100])
def test_min_coverage(min_cov):
    host, dev, _ = _block_planes()
    start, end = _pairs(_points()[::2])
    want = R.region_sums(R.Running(*host, min_cov=min_cov), start, end)
    assert want.any() == (min_cov < 100)
    assert (_got(_pu().regions(start, end, min_cov=min_cov, planes=dev, hi=len(host[0]))) == want).all()


def test_no_interval_and_many_intervals():
    host, dev, run = _block_planes()
    n = len(host[0])
    assert _pu().regions([], [], planes=dev, hi=n).shape == (0, 3)
    start = (np.arange(70000, dtype=np.int64) * 7) % n                            # more wavefronts than one grid dimension of 65 535
    got = _got(_pu().regions(start, start + 1, planes=dev, hi=n))
    pc, nc, ky = (np.asarray(p, np.int64) for p in host)
    on = (pc + nc)[start] >= 1
    assert (got[:, :, 0].sum(axis=1) == on).all() and (got[np.arange(70000), ky[start] & 3, 1] == np.where(on, pc[start], 0)).all()
    assert (got[:999] == R.region_sums(run, start[:999], start[:999] + 1)).all()


def test_scan_of_several_partitions():
    """more blocks than one workgroup of the scan takes: the carries between its partitions"""
    B, part = _geometry()
    n = (part + 1) * B + 5                                                        # one block and a few loci into the second partition
    host = _synthetic(n, 5, covered=0.125)
    rng = np.random.default_rng(6)
    edges = [0, 1, (part - 1) * B, part * B - 1, part * B, part * B + 1, (part + 1) * B - 1, (part + 1) * B, n - 1, n]
    start, end = _pairs(edges)
    a, b = np.sort(rng.integers(0, n + 1, (2, 300)), axis=0)
    start, end = np.concatenate([start, a]), np.concatenate([end, b])
    want = R.region_sums(R.Running(*host), start, end)
    assert (_got(_pu().regions(start, end, planes=_dev(host), hi=n)) == want).all() and want[:, :, 0].sum(axis=1).max() > n // 16


# ---- metaplot --------------------------------------------------------------------------------------------------------------------------
def _meta_case():
    """planes of two sequences back to back; intervals on all strands, of bins - 1, bins and bins + 1 bases, at position 0 of the
    second sequence (its upstream flank is empty: the first sequence ends in covered loci that must not be read) and at both ends"""
    B, _ = _geometry()
    n1 = B + 37
    n = 3 * B + 5
    bins, flank, fb = 5, 12, 3
    iv = [(10, 10 + bins - 1, 0, "+"), (20, 20 + bins, 0, "+"), (30, 30 + bins + 1, 0, "-"), (B - 3, B + 9, 0, "."), (n1 - 8, n1, 0, "-"),
          (0, 7, 0, "+"), (n1, n1 + 9, 1, "+"), (n1, n1 + 6, 1, "-"), (n - 11, n, 1, "."), (n1 + B - 2, n1 + B + B // 2 + 3, 1, "-"), (n - 5, n, 1, "+")]
    off = [0, n1, n]
    start, end = (np.array([x[k] for x in iv], np.int64) for k in (0, 1))
    s0, s1 = (np.array([off[x[2] + k] for x in iv], np.int64) for k in (0, 1))
    return n, (start, end, s0, s1, "".join(x[3] for x in iv).encode()), (bins, flank, fb)


def _meta_table(rows, nb):
    assert rows["motif"].tolist() == [c for c in range(3) for _ in range(nb)] and rows["bin"].tolist() == list(range(nb)) * 3
    return np.stack([rows[k] for k in ("n_regions",) + R.QUANTITIES], axis=-1).astype(np.int64).reshape(3, nb, 5)


def test_metaplot_geometry():
    host, dev, run = _block_planes()
    n, (start, end, s0, s1, strand), (bins, flank, fb) = _meta_case()
    assert n == len(host[0]) and (host[0][s0[6] - flank:s0[6]].any() or host[1][s0[6] - flank:s0[6]].any())
    want, used = R.metaplot(run, start, end, s0, s1, strand.decode(), bins, flank, fb)
    assert used == len(start) - 1 and (want[:, :fb, 0] < used).all() and want[:, :, 1:].any(axis=(0, 2)).all()
    rows, n_used = _pu().metaplot(start, end, s0, s1, strand, bins, flank, fb, planes=dev, hi=n)
    assert n_used == used and (_meta_table(rows, bins + 2 * fb) == want).all()
    only = [6]                                                                    # the interval at position 0 of the second sequence
    rows, n_used = _pu().metaplot(start[only], end[only], s0[only], s1[only], b"+", bins, flank, fb, planes=dev, hi=n)
    tab = _meta_table(rows, bins + 2 * fb)
    assert n_used == 1 and not tab[:, :fb].any() and (tab == R.metaplot(run, start[only], end[only], s0[only], s1[only], "+", bins, flank, fb)[0]).all()
    body, n_used = _pu().metaplot(start, end, s0, s1, None, bins, planes=dev, hi=n)      # body only, no strand: all forward
    assert (_meta_table(body, bins) == R.metaplot(run, start, end, s0, s1, "+" * len(start), bins)[0]).all()


def test_metaplot_chunks_add_up():
    host, dev, run = _block_planes()
    B, _ = _geometry()
    n, (start, end, s0, s1, strand), (bins, flank, fb) = _meta_case()
    nb = bins + 2 * fb
    whole = R.metaplot(run, start, end, s0, s1, strand.decode(), bins, flank, fb)[0]
    for cut in (1, B - 1, B + 40, 2 * B, 3 * B + 4):
        left = _meta_table(_pu().metaplot(start, end, s0, s1, strand, bins, flank, fb, lo=0, hi=cut, planes=dev)[0], nb)
        right = _meta_table(_pu().metaplot(start, end, s0, s1, strand, bins, flank, fb, lo=0, hi=n - cut, planes=tuple(t[cut:] for t in dev),
                                           plane_base=cut)[0], nb)
        assert (left[:, :, 0] == whole[:, :, 0]).all() and (right[:, :, 0] == whole[:, :, 0]).all(), cut    # n_regions: no chunk's business
        assert (left[:, :, 1:] + right[:, :, 1:] == whole[:, :, 1:]).all(), cut
        assert (left == R.metaplot(run, start, end, s0, s1, strand.decode(), bins, flank, fb, lo=0, hi=cut)[0]).all(), cut


# ---- planes next to 2^31 and 2^32 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", [2 ** 31, 2 ** 32], ids=["2^31", "2^32"])
def test_planes_next_to_a_32_bit_boundary(boundary):
    """the four blocks of _block_planes with a plane_base that puts the boundary inside the second block, off the block grid:
    interval edges, plane_base and the metaplot's sequence clamp are coordinates beyond 2^31 / 2^32, and the expectation of the
    same intervals with their coordinates through 32 bits is another one.  The smallest shape at which a 32-bit coordinate in
    region_query_kernel / metaplot_kernel shows, on any card; the index of a reference of that size (2^20 blocks, 1024 scan
    workgroups) runs in test_gpu_pileup_bigref.py.  `pileup -S` cannot be reached this way: it refuses a plane_base + hi beyond
    the engine's reference, so its only run at such coordinates is the one in test_gpu_pileup_bigref.py."""
    from bigref import wrap32
    host, dev, _ = _block_planes()
    blk, _ = _geometry()
    n = len(host[0])
    base = boundary - (blk + 5)
    assert blk < boundary - base < 2 * blk and (boundary - base) % blk
    run = R.Running(*host, base=base)
    start, end = _pairs(_points()) + base
    more = np.array([(boundary - 1, boundary + 1), (boundary, boundary + 7), (boundary - 7, boundary), (base, base + n)], np.int64).T
    start, end = np.concatenate([start, more[0]]), np.concatenate([end, more[1]])
    want = R.region_sums(run, start, end)
    assert (R.region_sums(run, [base, boundary], [boundary, base + n])[:, :, 0] > 0).all()        # counted loci on both sides of it
    assert want[-4:-1, :, 0].sum(axis=1).all()                                                    # ... and in the three intervals on it
    got = _got(_pu().regions(start, end, planes=dev, plane_base=base, hi=n))
    assert got.shape == want.shape and (got == want).all()
    casts = (True,) if boundary < 2 ** 32 else (True, False)
    for signed in casts:
        assert (R.region_sums(run, wrap32(start, signed), wrap32(end, signed)) != want).any()
    # the metaplot of a sequence that begins three bases below the boundary: the upstream flank of the first interval is clamped there
    bins, flank, fb = 5, 12, 3
    S0, S1 = boundary - 3, base + n
    iv = [(boundary, boundary + 40, "+"), (boundary + 10, boundary + 31, "-"), (S0, boundary + 5, "."), (S1 - 25, S1, "+"),
          (boundary + blk - 9, boundary + blk + 9, "-"), (boundary + 3, boundary + 3 + bins - 1, "+")]
    a, b = (np.array([x[k] for x in iv], np.int64) for k in (0, 1))
    s0, s1 = np.full(len(iv), S0, np.int64), np.full(len(iv), S1, np.int64)
    strand = "".join(x[2] for x in iv)
    tab, used = R.metaplot(run, a, b, s0, s1, strand, bins, flank, fb)
    assert used == len(iv) - 1 and (tab[:, 0, 0] < used).all() and tab[:, :, 1].sum(axis=0).all()
    rows, n_used = _pu().metaplot(a, b, s0, s1, strand.encode(), bins, flank, fb, planes=dev, plane_base=base, hi=n)
    assert n_used == used and (_meta_table(rows, bins + 2 * fb) == tab).all()
    for signed in casts:
        assert (R.metaplot(run, *(wrap32(x, signed) for x in (a, b, s0, s1)), strand, bins, flank, fb)[0] != tab).any()


# ---- real records ----------------------------------------------------------------------------------------------------------------------
def _tagged_reads():
    if "reads" not in _CACHE:
        _CACHE["reads"] = [dataclasses.replace(r, hp=(None, 1, 2)[i % 3]) for i, r in enumerate(C.everything())]
    return _CACHE["reads"]


def _real_intervals(genome):
    """on every sequence: the whole of it, its first and its last base, a few inside; the last ends at the last base of the last"""
    rows = []
    for k, (name, seq) in enumerate(genome):
        n = len(seq)
        rows += [(name, 0, n, f"whole{k}", "+"), (name, 0, 1, ".", "."), (name, 290, 380, f"cluster{k}", "-"), (name, 295, 305, ".", "."),
                 (name, n - 40, n - 1, f"tail{k}", "+"), (name, n - 1, n, f"last{k}", "-")]
    return rows


def _as_regions(rows, genome):
    from hifimeth_amd.pileup import Regions
    sid = {n: i for i, (n, _) in enumerate(genome)}
    return Regions([sid[r[0]] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])


def test_real_records_under_haplotypes():
    from hifimeth_amd.pileup import MethylationPileup, metaplot_tsv, regions_tsv
    genome, reads = C.genome(), _tagged_reads()
    pu = MethylationPileup(genome, partitions=True)
    for r in reads:
        pu.add(r)
    pu.flush()
    pu.count(list(THR))
    rows = _real_intervals(genome)
    reg = _as_regions(rows, genome)
    xy = reg.coords(pu.offsets)
    assert xy["end"][-1] == pu.n_loci
    for part in (0, 1, 2):
        loci = pu.loci(partition=part)
        assert len(loci) > 50
        for min_cov in (1, 2):
            run = R.Running(*R.planes_from_loci(loci, pu.n_loci), min_cov=min_cov)
            want = R.region_sums(run, xy["start"], xy["end"])
            sums = pu.regions(xy["start"], xy["end"], min_cov, partition=part)
            assert (_got(sums) == want).all() and (want[:, :, 0].sum(axis=0) > 0).all()
            assert regions_tsv(reg, pu.names, sums) == R.regions_text(rows, want)
            tab, used = R.metaplot(run, xy["start"], xy["end"], xy["seq_start"], xy["seq_end"], xy["strand"].decode(), 4, 30, 3)
            got, n_used = pu.metaplot(**xy, bins=4, flank=30, flank_bins=3, min_cov=min_cov, partition=part)
            assert n_used == used == len(rows) - 6 and (_meta_table(got, 10) == tab).all()
            assert metaplot_tsv(got, n_used, len(rows) - n_used, 4, 3) == R.metaplot_text(tab, used, len(rows) - used, 4, 3)
    pu.close()


# ---- the ABI's refusals ----------------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.caller import HifimethError
    L = lib()
    one = np.array([0, 5], np.int64)
    out = np.zeros(64, np.int64)
    args = (one[:1].ctypes.data_as(ctypes.c_void_p), one[1:].ctypes.data_as(ctypes.c_void_p), 1, out.ctypes.data_as(ctypes.c_void_p))
    h = ctypes.c_void_p()
    assert L.hm_pileup_create(ctypes.byref(h), 0) == 0
    assert L.hm_pileup_fetch_regions(h, None, None, None, 0, 0, 10, 1, *args) == HM_ESTATE      # no reference, no planes, no count
    assert b"no planes" in L.hm_pileup_last_error(h)
    used = ctypes.c_int64(-1)
    assert L.hm_pileup_fetch_metaplot(h, None, None, None, 0, 0, 10, 1, *args[:2], *args[:2], None, 1, 2, 0, 0, args[3], ctypes.byref(used)) == HM_ESTATE
    L.hm_pileup_destroy(h)
    host, dev, _ = _block_planes()
    pu, n = _pu(), len(host[0])
    for bad in (dict(start=[5], end=[4]), dict(start=[0], end=[4], min_cov=0), dict(start=[0], end=[4], lo=5, hi=4), dict(start=[0], end=[4], lo=-1)):
        with pytest.raises(HifimethError):
            pu.regions(**{"planes": dev, "hi": n, **bad})
    s, e, s0, s1 = [10], [30], [0], [n]
    for bad in (dict(bins=0), dict(bins=1001), dict(bins=4, flank=10, flank_bins=3), dict(bins=4, flank=0, flank_bins=2), dict(bins=4, flank=8, flank_bins=0),
                dict(bins=4, flank=-4, flank_bins=2), dict(bins=4, min_cov=0)):
        with pytest.raises(HifimethError):
            pu.metaplot(s, e, s0, s1, b"+", **{"planes": dev, "hi": n, **bad})
    with pytest.raises(HifimethError):
        pu.metaplot([30], [10], s0, s1, b"+", 4, planes=dev, hi=n)                # start > end
    with pytest.raises(HifimethError):
        pu.metaplot([10], [30], [12], s1, b"+", 4, planes=dev, hi=n)              # not within its sequence
    assert _got(pu.regions([0], [n], planes=dev, hi=n))[0, :, 0].sum() > 0        # the engine still answers


# ---- the four front ends ---------------------------------------------------------------------------------------------------------------
OPTS = ["-C", "2", "-J", "4:30:3"]


def _cli(args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    return r.returncode, r.stderr


def _files(prefix):
    d, b = os.path.dirname(prefix), os.path.basename(prefix) + "."
    return {n[len(b):]: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.startswith(b)}


def _ours(files):
    return {k: v for k, v in files.items() if "regions." in k.replace("asm.regions.", "") or "metaplot." in k}


def _dist_env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HM_FORCE_COLLECTIVES"):
        env.pop(k, None)
    env.update(kw)
    return env


@pytest.fixture(scope="module")
def on_disk(tmp_path_factory):
    from bamutil import write_fasta
    from test_gpu_pileup_hp import _write_bam
    d = tmp_path_factory.mktemp("regions")
    reads = _tagged_reads()
    bam, fa, bed = str(d / "in.bam"), str(d / "ref.fa"), str(d / "iv.bed")
    _write_bam(bam, C.genome(), reads, [[("C", r.hp)] if r.hp else [] for r in reads])
    write_fasta(fa, C.genome())
    with open(bed, "w") as f:
        f.write("track name=test\n# comment\n\n" + "".join("%s\t%d\t%d\t%s\t0\t%s\n" % r for r in _real_intervals(C.genome())))
    rc, err = _cli(["pileup", "-H", "-R", bed, *OPTS, "-b", "20", fa, bam, str(d / "t")])
    assert rc == 0, err[-2000:]
    return reads, bam, fa, bed, d


def test_cli_equals_python_and_the_restatement(on_disk):
    from hifimeth_amd.pileup import MethylationPileup, metaplot_tsv, parse_regions_bed, regions_tsv
    reads, bam, fa, bed, d = on_disk
    genome = C.genome()
    pu = MethylationPileup(genome, partitions=True)
    for r in reads:
        pu.add(r)
    pu.flush()
    pu.count(pu.resolve_thresholds(pu.histograms()))
    reg = parse_regions_bed(bed, pu.names, pu.lengths)
    assert len(reg) == len(_real_intervals(genome))
    xy = reg.coords(pu.offsets)
    got = _ours(_files(str(d / "t")))
    assert len(got) == 18
    for part, tag in enumerate(("", "hap1.", "hap2.")):
        sums = pu.regions(xy["start"], xy["end"], 2, partition=part)
        rows, used = pu.metaplot(**xy, bins=4, flank=30, flank_bins=3, min_cov=2, partition=part)
        run = R.Running(*R.planes_from_loci(pu.loci(partition=part), pu.n_loci), min_cov=2)
        tab, _ = R.metaplot(run, xy["start"], xy["end"], xy["seq_start"], xy["seq_end"], xy["strand"].decode(), 4, 30, 3)
        for ctx, text in regions_tsv(reg, pu.names, sums).items():
            assert got[f"{tag}regions.{ctx}.tsv"].decode() == text == R.regions_text(_real_intervals(genome), R.region_sums(run, xy["start"], xy["end"]))[ctx]
        for ctx, text in metaplot_tsv(rows, used, len(reg) - used, 4, 3).items():
            assert got[f"{tag}metaplot.{ctx}.tsv"].decode() == text == R.metaplot_text(tab, used, len(reg) - used, 4, 3)[ctx]
    assert got["regions.CpG.tsv"] != got["hap1.regions.CpG.tsv"] and b"nan" in got["regions.CHG.tsv"]
    pu.close()


def test_every_other_file_is_what_it_was(on_disk):
    _reads, bam, fa, bed, d = on_disk
    many = ["-H", "-A", "-a", "1", "-B", "chr2", "-D", "-E", "2", "-M", "-L", "50", "-P", "30", "-b", "20"]
    rc, err = _cli(["pileup", *many, fa, bam, str(d / "m")])
    assert rc == 0, err[-2000:]
    rc, err = _cli(["pileup", *many, "-R", bed, *OPTS, fa, bam, str(d / "mr")])
    assert rc == 0, err[-2000:]
    a, b = _files(str(d / "m")), _files(str(d / "mr"))
    assert not _ours(a) and len(a) > 20 and set(b) == set(a) | set(_ours(b)) and all(b[n] == a[n] for n in a)
    assert _ours(b) == _ours(_files(str(d / "t")))
    rc, err = _cli(["pileup", "-R", bed, fa, bam, str(d / "r")])                  # -R alone: no haplotype files, no metaplot
    assert rc == 0, err[-2000:]
    assert sorted(_ours(_files(str(d / "r")))) == ["regions.CHG.tsv", "regions.CHH.tsv", "regions.CpG.tsv"]


def test_pileup_dist_world_of_one_equals_the_cli(on_disk):
    _reads, bam, fa, bed, d = on_disk
    prefix = str(d / "one")
    r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", "-H", "-R", bed, *OPTS, fa, bam, prefix], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=_dist_env())
    assert r.returncode == 0, r.stderr[-2000:]
    assert _ours(_files(prefix)) == _ours(_files(str(d / "t"))) and _files(prefix)["CpG.cov.bed"] == _files(str(d / "t"))["CpG.cov.bed"]


def test_pileup_dist_two_ranks_equal_the_cli(on_disk):
    """two gloo ranks sharing the card: each queries its half of the planes, the integer columns add up to the CLI's files"""
    _reads, bam, fa, bed, d = on_disk
    prefix = str(d / "gloo")
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", "-H", "-R", bed, *OPTS, "--slab", "7", "--backend", "gloo"]
    procs = [subprocess.Popen([*mod, fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29617"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert _ours(_files(prefix)) == _ours(_files(str(d / "t"))) and _files(prefix)["CpG.cov.bed"] == _files(str(d / "t"))["CpG.cov.bed"]
