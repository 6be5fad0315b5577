"""Allele-specific regions (`pileup -H -A -G`) on the device: hm_pileup_fetch_asm_regions over caller-owned crafted planes, range
splits stitched on the host, the CLI and the distributed driver.

Nothing here has a tolerance.  The expectation is asm_regions_ref.regions (the header's definition in numpy) applied to the
device's own hm_pileup_fetch_asm rows of the same range, and the comparison is byte for byte.  That the crafted planes hold the
planted cases is checked on the CPU from the planes alone, with exact Fisher p-values (test_gpu_pileup_asm.fisher_exact)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from asm_regions_ref import FIRST, LAST, ctx_rows, regions
from conftest import ROOT
from test_gpu_pileup_asm import CTX, _asm_files, _cov_files, _dist_env, _engine, _np_diff, _phased_reads, _run_cli, _write_bam, fisher_exact

pytestmark = pytest.mark.gpu

N_LOCI = 5 * 4096 + 7
MIN_COV = 5
UP, DOWN = (12, 0, 0, 12), (0, 12, 12, 0)                    # hits under every max_p used here: p = 7.4e-7
EDGE_UP = (9, 1, 3, 7)                                        # p = 0.0198: max_p of set "edge" is the device's p of this tuple
OVER_UP = (9, 1, 4, 6)                                        # p = 0.057: the next larger p among the planted tuples
MILD, FLAT = (7, 5, 5, 7), (6, 6, 6, 6)                       # no hits below max_p 1: p = 0.68 with diff > 0; diff == 0 with p = 1
LONG = (9000, 12000)                                          # one chain of about 3000 rows
# name -> (max_p or None = the device's p of EDGE_UP, max_gap, min_loci)
SETS = {"edge": (None, 7, 3), "all": (1.0, 7, 3), "wide": (0.01, 500, 1)}


def _crafted():
    """-> pcov1, ncov1, pcov2, ncov2, key (int32 [N_LOCI]).  Every locus is a tested CpG row that is no hit (MILD, every fifth FLAT)
    unless something is planted on it."""
    t = np.zeros((4, N_LOCI), np.int64)
    t[:] = np.array(MILD)[:, None]
    t[:, ::5] = np.array(FLAT)[:, None]
    motif = np.zeros(N_LOCI, np.int64)

    def put(lo, hi, tup, m=None):
        t[:, lo:hi] = np.array(tup)[:, None]
        if m is not None:
            motif[lo:hi] = m

    put(0, 5, (0, 0, 0, 0))                                   # row index = locus index - 5 at the start
    put(5, 7, DOWN)                                           # a chain of two at r_0
    put(60, 80, UP)                                           # rows 63 | 64
    put(250, 270, DOWN)                                       # rows 255 | 256
    put(4090, 4100, UP)                                       # loci 4095 | 4096 ...
    put(4100, 4180, DOWN)                                     # ... a sign flip inside a run of hits, and rows 4095 | 4096
    put(8185, 8200, UP)                                       # loci 8191 | 8192
    put(*LONG, UP)
    put(9500, 9501, DOWN, 1)                                  # a tested hit of another context inside it: does not break
    put(9600, 9601, (0, 0, 0, 0))                             # not covered
    put(9700, 9701, (-1, 70, 9, 9))                           # a negative counter: not tested
    put(9800, 9801, (4, 0, 0, 12))                            # below min_cov on one haplotype
    put(13000, 13016, (0, 0, 0, 0))                           # gaps: 13000 -7- 13007 -8- 13015
    for i in (13000, 13007, 13015):
        put(i, i + 1, UP)
    put(13100, 13103, UP)                                     # n_loci == min_loci
    put(13200, 13202, UP)                                     # n_loci == min_loci - 1
    put(13300, 13306, UP)
    put(13302, 13303, FLAT)                                   # diff == 0 inside a run of hits
    put(13400, 13403, DOWN)
    put(13401, 13402, MILD)                                   # a non-hit of the context between two hits: breaks
    put(13500, 13506, UP)
    put(13502, 13503, EDGE_UP)                                # p == max_p: links
    put(13600, 13606, UP)
    put(13602, 13603, OVER_UP)                                # p just above: breaks
    put(14000, 14010, DOWN, 2)                                # a CHH chain, every other key with low bits 3
    motif[14001:14010:2] = 3
    put(14100, 14110, UP)
    put(14104, 14105, (6, 6, 6, -2))                          # negative counter between two hits
    motif[15000:19000:37] = 1                                 # CHG rows 37 apart: chains of one unless max_gap allows more
    t[:, 15000:19000:37] = np.array(DOWN)[:, None]
    t[:, 15000 + 37 * 50] = MILD
    put(N_LOCI - 2, N_LOCI, UP)                               # a chain of two at r_{R-1}
    key = (np.arange(N_LOCI, dtype=np.int64) % 100003) << 2 | motif
    return tuple(x.astype(np.int32) for x in t) + (key.astype(np.int32),)


def _host_rows(host):
    """the hm_asm_t rows the planes must give, pvalue = the exact Fisher p rounded to fp64 (the device's differs in the last bits)"""
    from hifimeth_amd.pileup import ASM_DTYPE
    p1, n1, p2, n2 = (x.astype(np.int64) for x in host[:4])
    ok = np.nonzero((p1 >= 0) & (n1 >= 0) & (p2 >= 0) & (n2 >= 0) & (p1 + n1 >= MIN_COV) & (p2 + n2 >= MIN_COV))[0]
    rows = np.zeros(len(ok), ASM_DTYPE)
    rows["gpos"], rows["motif"] = ok, host[4][ok] & 3
    rows["pcov1"], rows["ncov1"], rows["pcov2"], rows["ncov2"] = p1[ok], n1[ok], p2[ok], n2[ok]
    rows["diff"] = _np_diff(p1[ok], n1[ok], p2[ok], n2[ok])
    cache = {}
    for r in rows:
        k = (int(r["pcov1"]), int(r["ncov1"]), int(r["pcov2"]), int(r["ncov2"]))
        if k not in cache:
            cache[k] = float(fisher_exact(*k))
        r["pvalue"] = cache[k]
    return rows, cache


def _brief(regs):
    return [tuple(int(g[f]) for f in ("start", "end", "n_loci", "sign", "flags", "pcov1", "ncov1", "pcov2", "ncov2")) for g in regs]


def _moved(regs, shift):
    out = regs.copy()
    out["start"] += shift
    out["end"] += shift
    return out


def test_crafted_planes_hold_the_cases():
    rows, p = _host_rows(_crafted())
    assert p[UP] == p[DOWN] < 1e-5 < 0.01 < p[EDGE_UP] < p[OVER_UP] < 0.1 < p[MILD] < p[FLAT] == 1.0
    r0 = ctx_rows(rows, 0)
    assert len(r0) > 2 * 4096 + 4096 and len(ctx_rows(rows, 1)) > 100 and len(ctx_rows(rows, 2)) == 10
    assert (ctx_rows(rows, 2)["motif"] == 3).sum() == 5
    row_of = {int(g): i for i, g in enumerate(r0["gpos"])}
    edge, _ = regions(rows, 0, p[EDGE_UP], 7, 3, keep_edges=True)
    by_start = {int(g["start"]): g for g in edge}

    def crosses_rows(a):                                      # a chain that holds rows a and a + 1
        return any(row_of[int(g["start"])] <= a and a + 1 <= row_of[int(g["end"]) - 1] for g in edge)

    def crosses_loci(a):
        return any(g["start"] <= a and a + 1 < g["end"] for g in edge)

    assert all(crosses_rows(a) for a in (63, 255, 4095)) and all(crosses_loci(a) for a in (4095, 8191))
    assert row_of[64 + 5] == 64 and row_of[4096] != 4096      # row and locus boundaries are different places
    g = by_start[LONG[0]]
    assert g["end"] == LONG[1] and g["n_loci"] == LONG[1] - LONG[0] - 4 and g["sign"] == 1   # another context, uncovered, negative, low: none breaks
    assert _brief([by_start[4090], by_start[4100]]) == [(4090, 4100, 10, 1, 0, 120, 0, 0, 120), (4100, 4180, 80, -1, 0, 0, 960, 960, 0)]
    gaps = [b[:3] for b in _brief(regions(rows, 0, p[EDGE_UP], 7, 1)[0]) if 13000 <= b[0] < 13100]
    assert gaps == [(13000, 13008, 2), (13015, 13016, 1)]                     # a gap of max_gap links, max_gap + 1 does not
    assert by_start[13100]["n_loci"] == 3 and 13200 not in by_start           # n_loci == min_loci stays, min_loci - 1 goes
    assert by_start[13500]["n_loci"] == 6 and by_start[13500]["pmin"] == p[UP]            # p == max_p links
    assert [k for k in by_start if 13600 <= k < 13700] == [13603]                         # p above max_p breaks: 2 + 3, only the 3 stays
    assert [k for k in by_start if 13400 <= k < 13500] == []                              # a non-hit of the context breaks: 1 + 1
    assert [k for k in by_start if 13300 <= k < 13400] == [13303]                         # diff == 0 breaks: 2 + 3
    assert by_start[14100]["n_loci"] == 9 and by_start[14100]["end"] == 14110             # a negative counter does not break
    assert by_start[5]["flags"] == FIRST and by_start[5]["n_loci"] == 2 and by_start[N_LOCI - 2]["flags"] == LAST
    assert 5 not in {int(g["start"]) for g in regions(rows, 0, p[EDGE_UP], 7, 3)[0]}
    chh, R = regions(rows, 2, p[EDGE_UP], 7, 3)
    assert R == 10 and _brief(chh) == [(14000, 14010, 10, -1, FIRST | LAST, 0, 120, 120, 0)]
    # under max_p = 1 a row is a hit unless diff == 0: the background becomes chains of four MILD rows between FLAT ones
    every, _ = regions(rows, 0, 1.0, 7, 3)
    assert sum(int(g["n_loci"]) == 4 and int(g["pcov1"]) == 28 for g in every) > 2000
    # CHG: hits 37 apart are chains of one under max_gap 7 and one chain per side of the non-hit under max_gap 500
    assert len(regions(rows, 1, 0.01, 7, 1)[0]) > 100
    assert [int(g["n_loci"]) for g in regions(rows, 1, 0.01, 500, 1)[0]] == [1, 50, 58]


@pytest.fixture(scope="module")
def crafted():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    host = _crafted()
    pu = MethylationPileup([("c", "ACGT" * 50)])             # caller-owned planes: the reference plays no part
    dev = [torch.from_numpy(x.copy()).cuda() for x in host]
    rows = pu.asm(0, N_LOCI, MIN_COV, planes=dev)
    edge_p = {float(r["pvalue"]) for r in rows if tuple(int(r[f]) for f in ("pcov1", "ncov1", "pcov2", "ncov2")) == EDGE_UP}
    assert len(edge_p) == 1                                   # one tuple, one p: its exact bits become max_p
    params = {k: (edge_p.copy().pop() if p is None else p, gap, n) for k, (p, gap, n) in SETS.items()}
    yield pu, host, dev, rows, params
    pu.close()


@pytest.mark.parametrize("name", list(SETS))
def test_regions_equal_the_reference_on_the_device_rows(crafted, name):
    from hifimeth_amd.pileup import ASM_REGION_DTYPE
    pu, host, dev, rows, params = crafted
    max_p, max_gap, min_loci = params[name]
    host_rows, _ = _host_rows(host)
    assert (rows[["gpos", "pcov1", "ncov1", "pcov2", "ncov2", "motif"]] == host_rows[["gpos", "pcov1", "ncov1", "pcov2", "ncov2", "motif"]]).all()
    seen = 0
    for ctx in range(3):
        for keep in (False, True):
            want, R = regions(rows, ctx, max_p, max_gap, min_loci, keep)
            got, n_ctx = pu.asm_regions(ctx, 0, N_LOCI, MIN_COV, max_p, max_gap, min_loci, planes=dev, keep_edges=keep)
            assert got.dtype == ASM_REGION_DTYPE and n_ctx == R
            assert len(got) == len(want) and got.tobytes() == want.tobytes(), (name, ctx, keep)
            # the structure is also what the planes predict with exact p-values (only pmin's last bits may differ)
            host_p = max_p if name != "edge" else float(fisher_exact(*EDGE_UP))
            assert _brief(got) == _brief(regions(host_rows, ctx, host_p, max_gap, min_loci, keep)[0])
            seen += len(got)
    assert seen > {"edge": 20, "all": 4000, "wide": 30}[name]
    if name == "edge":
        edge = pu.asm_regions(0, 0, N_LOCI, MIN_COV, max_p, max_gap, min_loci, planes=dev, keep_edges=True)[0]
        plain = pu.asm_regions(0, 0, N_LOCI, MIN_COV, max_p, max_gap, min_loci, planes=dev)[0]
        assert len(edge) == len(plain) + 2 and edge[0]["flags"] == FIRST and edge[-1]["flags"] == LAST
        assert edge[1:-1].tobytes() == plain.tobytes() and (plain["flags"] == 0).all()
        below = pu.asm_regions(0, 0, N_LOCI, MIN_COV, np.nextafter(max_p, 0.0), max_gap, min_loci, planes=dev)[0]
        assert 13500 in plain["start"] and 13500 not in below["start"] and 13503 in below["start"]
        shift = (1 << 31) - 10000                             # plane_base: 2^31 falls inside the long chain
        moved = pu.asm_regions(0, 0, N_LOCI, MIN_COV, max_p, max_gap, min_loci, planes=dev, plane_base=shift)[0]
        assert moved.tobytes() == _moved(plain, shift).tobytes() and ((moved["start"] < 1 << 31) & (moved["end"] > 1 << 31)).sum() == 1


SPLITS = {"inside one chain, three parts of it": (9400, 10500), "in a gap between two linked hits": (13003, 13600),
          "on block edges": (4096, 8192), "a middle part without rows": (13001, 13007), "a part without loci": (13300, 13300),
          "between a chain and its breaker": (13302, 13303)}


@pytest.mark.parametrize("where", list(SPLITS))
def test_range_splits_stitch_to_the_whole(crafted, where):
    """three adjacent fetches with keep_edges, each over a chunk whose element 0 is its first locus, under a plane_base that puts
    2^31 inside the long chain"""
    from hifimeth_amd.pileup import stitch_asm_regions
    pu, _host, dev, _rows, params = crafted
    a, b = SPLITS[where]
    shift = (1 << 31) - 10000
    for name in ("edge", "wide"):
        max_p, max_gap, min_loci = params[name]
        for ctx in (0, 1):
            whole = {keep: pu.asm_regions(ctx, 0, N_LOCI, MIN_COV, max_p, max_gap, min_loci, planes=dev, keep_edges=keep) for keep in (False, True)}
            parts = []
            for lo, hi in ((0, a), (a, b), (b, N_LOCI)):
                chunk = [t[lo:] for t in dev]
                parts.append(pu.asm_regions(ctx, 0, hi - lo, MIN_COV, max_p, max_gap, min_loci, planes=chunk, plane_base=shift + lo, keep_edges=True))
            if where == "a middle part without rows":
                assert parts[1][1] == 0 and len(parts[1][0]) == 0
            for keep in (False, True):
                got, R = stitch_asm_regions(parts, max_gap, min_loci, keep_edges=keep)
                assert R == whole[keep][1] and got.tobytes() == _moved(whole[keep][0], shift).tobytes(), (where, name, ctx, keep)


def test_cap_empty_range_and_abi_errors(crafted):
    from hifimeth_amd.pileup import ASM_REGION_DTYPE, MethylationPileup
    pu, _host, dev, _rows, params = crafted
    max_p, max_gap, min_loci = params["edge"]
    L, ptrs, none = pu._L, [ctypes.c_void_p(t.data_ptr()) for t in dev], [None] * 5
    f = L.hm_pileup_fetch_asm_regions
    want, R = pu.asm_regions(0, 0, N_LOCI, MIN_COV, max_p, max_gap, min_loci, planes=dev)
    n = len(want)
    out = np.zeros(n, ASM_REGION_DTYPE)
    out["start"] = -7
    po, rows_seen = out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(-1)
    ok = (0, max_p, max_gap, min_loci, 0)
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, MIN_COV, *ok, ctypes.byref(rows_seen), po, n - 1) == n and rows_seen.value == R
    assert (out["start"] == -7).all() and (out["n_loci"] == 0).all()                    # cap too small: nothing is written
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, MIN_COV, *ok, None, None, 0) == n
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, MIN_COV, *ok, None, po, n) == n and out.tobytes() == want.tobytes()
    rows_seen.value = -1
    assert f(pu._h, *ptrs, 0, 77, 77, MIN_COV, *ok, ctypes.byref(rows_seen), po, n) == 0 and rows_seen.value == 0   # hi == lo
    assert out.tobytes() == want.tobytes()
    assert f(pu._h, *ptrs, 0, 0, 5, MIN_COV, *ok, ctypes.byref(rows_seen), po, n) == 0 and rows_seen.value == 0      # no tested locus
    bad = [(-1, max_p, 7, 3, 0), (3, max_p, 7, 3, 0), (0, 0.0, 7, 3, 0), (0, -0.5, 7, 3, 0), (0, np.nextafter(1.0, 2.0), 7, 3, 0),
           (0, float("nan"), 7, 3, 0), (0, max_p, 0, 3, 0), (0, max_p, -5, 3, 0), (0, max_p, 7, 0, 0), (0, max_p, 7, -1, 0)]
    for args in bad:
        assert f(pu._h, *ptrs, 0, 0, N_LOCI, MIN_COV, *args, None, None, 0) == -1, args
        assert b"hm_pileup_fetch_asm_regions" in L.hm_pileup_last_error(pu._h)
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, MIN_COV, 0, 1.0, 1, 1, 1, None, None, 0) > 0   # the bounds themselves are allowed
    # what hm_pileup_fetch_asm refuses
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, 0, *ok, None, None, 0) == -1 and f(pu._h, *ptrs, 0, 9, 8, MIN_COV, *ok, None, None, 0) == -1
    assert f(pu._h, *ptrs, 0, -1, 8, MIN_COV, *ok, None, None, 0) == -1 and f(None, *ptrs, 0, 0, 8, MIN_COV, *ok, None, None, 0) == -1
    for k in range(5):
        mix = list(ptrs)
        mix[k] = None
        assert f(pu._h, *mix, 0, 0, 100, MIN_COV, *ok, None, None, 0) == -1
    assert f(pu._h, *none, 0, 0, 100, MIN_COV, *ok, None, None, 0) == -5 and b"partitions" in L.hm_pileup_last_error(pu._h)   # HM_ESTATE
    hp = MethylationPileup([("c", "ACGT" * 50)], partitions=True)
    assert hp.asm_regions(0)[1] == 0 and len(hp.asm_regions(2, keep_edges=True)[0]) == 0    # own planes, nothing counted yet
    assert f(hp._h, *none, 0, 0, 201, MIN_COV, *ok, None, None, 0) == -1                   # own planes end with the reference
    hp.close()


# ---- through reads: the engine's own planes, the CLI, the distributed driver --------------------------------------------------------
E2E = dict(min_cov=3, max_p=0.05, max_gap=100, min_loci=2)
E2E_ARGS = ["-H", "-A", "-a", "3", "-G", "-s", "0.05", "-g", "100", "-n", "2"]


def _region_files(prefix):
    return {c: open(f"{prefix}.asm.regions.{c}.bed").read() for c in CTX}


def _mirror_text(pu, genome):
    """-> ({context: text}, regions of each sign) per sequence, as the CLI writes; each fetch equals the reference on pu.asm's rows"""
    text, signs = {c: "" for c in CTX}, {1: 0, -1: 0}
    for s in range(len(genome)):
        lo, hi = int(pu.offsets[s]), int(pu.offsets[s + 1])
        rows = pu.asm(lo, hi, E2E["min_cov"])
        for c in range(3):
            got, R = pu.asm_regions(c, lo, hi, **E2E)
            want, Rw = regions(rows, c, E2E["max_p"], E2E["max_gap"], E2E["min_loci"])
            assert R == Rw and got.tobytes() == want.tobytes()
            text[CTX[c]] += pu.asm_regions_bed(got)[CTX[c]]
            for g in got:
                signs[int(g["sign"])] += 1
    return text, signs


def test_cli_regions(tmp_path):
    from bamutil import write_fasta
    genome, reads = _phased_reads()
    bam, fa, prefix = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "out")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    _run_cli(["-H", "-A", "-a", "3", fa, bam, prefix + "0"])
    r1 = _run_cli([*E2E_ARGS, fa, bam, prefix + "1"])
    assert f"{prefix}1.asm.regions.*" in r1.stderr
    pu = _engine(genome, reads, partitions=True)
    text, signs = _mirror_text(pu, genome)
    pu.close()
    print("regions per sign:", signs, {c: len(t.splitlines()) for c, t in text.items()})
    assert signs[1] >= 2 and signs[-1] >= 2                   # an empty expectation cannot pass
    assert _region_files(prefix + "1") == text
    assert all(len(line.split("\t")) == 11 and line.split("\t")[4] in "+-" for t in text.values() for line in t.splitlines())
    # every other file of the run is the run's without -G, and that run writes no region file
    assert _cov_files(prefix + "0") == _cov_files(prefix + "1") and _asm_files(prefix + "0") == _asm_files(prefix + "1")
    assert sorted(os.listdir(tmp_path)) == sorted(
        ["mod.bam", "ref.fa"] + [f"out{k}.{t}{c}.cov.bed" for k in "01" for t in ("", "hap1.", "hap2.") for c in CTX]
        + [f"out{k}.asm.{c}.bed" for k in "01" for c in CTX] + [f"out1.asm.regions.{c}.bed" for c in CTX])


def test_pileup_dist_regions(tmp_path):
    """python -m hifimeth_amd.pileup_dist -H -A -G on two gloo ranks sharing the card: the region files are the CLI's byte for byte;
    the ranks' border lies inside chr2"""
    from bamutil import write_fasta
    genome, reads = _phased_reads()
    bam, fa = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    _run_cli([*E2E_ARGS, fa, bam, str(tmp_path / "cli")])
    want = (_cov_files(str(tmp_path / "cli")), _asm_files(str(tmp_path / "cli")), _region_files(str(tmp_path / "cli")))
    assert sum(len(t.splitlines()) for t in want[2].values()) >= 4
    border = (sum(len(s) for _, s in genome) + 1) // 2 - len(genome[0][1])
    assert 0 < border < len(genome[1][1])
    prefix = str(tmp_path / "gloo")
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", *E2E_ARGS, "--slab", "7", "--backend", "gloo"]
    procs = [subprocess.Popen([*mod, fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29589"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert (_cov_files(prefix), _asm_files(prefix), _region_files(prefix)) == want
