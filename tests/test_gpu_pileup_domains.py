"""Methylation domains (`pileup -D`) on the device: hm_pileup_fetch_domains over caller-owned crafted planes, and the CLI.

Nothing here has a tolerance.  The expectation is domains_ref.domains (the header's definition as textbook Viterbi in Python ints)
applied to the device's own hm_pileup_fetch_loci rows of the same range, and the comparison is byte for byte, floats as bits.  That
the crafted planes hold the planted cases is checked on the CPU from the planes alone."""
import ctypes
import os

import numpy as np
import pytest

from domains_ref import AFTER_BREAK, BEFORE_BREAK, ctx_rows, domains, emissions, switch_costs
from test_gpu_pileup_asm import CTX, _phased_reads, _run_cli, _write_bam

pytestmark = pytest.mark.gpu

N_LOCI = 5 * 4096 + 7
WG = 1024                                                     # rows per row-scan workgroup (SCAN_ROWS)
BIG = (1 << 20) + 5
# name -> (A, B, S, max_gap).  "tie": e = 4 (pcov - ncov), so the planted ties are exact; "scores": domain_scores(0.1, 0.8, 8)
SETS = {"tie": (4, -4, 8, 7), "scores": (136278, -98571, 524288, 1000), "free": (4, -4, 0, 7), "bounds": (1 << 24, -(1 << 24), 1 << 24, 1)}
HIGH, LOW, FLAT, NONE = (3, 0), (0, 3), (1, 1), (0, 0)


def _crafted():
    """-> pcov, ncov, key (int32 [N_LOCI]).  Every locus is a CpG row with e = 0 under "tie" (FLAT) unless something is planted."""
    t = np.zeros((2, N_LOCI), np.int64)
    t[:] = np.array(FLAT)[:, None]
    motif = np.zeros(N_LOCI, np.int64)

    def put(lo, hi, tup, m=None):
        t[:, lo:hi] = np.array(tup)[:, None]
        if m is not None:
            motif[lo:hi] = m

    put(0, 5, NONE)                                           # row index = locus index - 5 up to the first gap
    put(5, 6, HIGH)                                           # r_0
    put(WG - 20 + 5, WG + 5, HIGH)                            # a state change between rows WG - 1 | WG ...
    put(WG + 5, WG + 45, LOW)
    put(2 * WG + 5, 2 * WG + 13, NONE)                        # ... and a break between rows 2 WG - 1 | 2 WG (8 loci without a row)
    put(2 * WG + 13, 2 * WG + 20, HIGH)
    put(4080, 4096, HIGH)                                     # a state change between loci 4095 | 4096
    put(4096, 4120, LOW)
    put(8180, 8192, LOW)                                      # a break between locus 8191 and the next row
    put(8192, 8200, NONE)
    put(8200, 8210, HIGH)
    t[0, 9000:13000:2], t[1, 9000:13000:2] = 2, 1             # 4000 rows of e = +4, -4, ... under S = 8: no clamp acts and every
    t[0, 9001:13000:2], t[1, 9001:13000:2] = 1, 2             # back-pointer is the identity, across more than three workgroups
    put(8560, 8600, LOW)
    put(8600, 8700, HIGH)                                     # one high segment with, inside it ...
    put(8620, 8621, LOW, 1)                                   # ... a locus of another context
    put(8640, 8641, NONE)                                     # ... an uncovered locus
    put(8660, 8661, (-1, 70))                                 # ... a negative counter
    put(8680, 8681, (BIG, 0))                                 # ... a counter above 2^20
    put(8750, 8751, (0, 2 * BIG))
    # ties, each behind a break (d restarts at e):  d == S, then low rows;  d == -S, then high rows;  d == 0 at a break
    put(13000, 13110, NONE)
    put(13008, 13009, (2, 0))                                 # d = 8 == S
    put(13009, 13012, LOW)
    put(13030, 13031, (0, 2))                                 # d = -8 == -S
    put(13031, 13034, HIGH)
    put(13050, 13051, FLAT)                                   # d = 0, and the next row is beyond max_gap
    put(13060, 13062, HIGH)
    put(13080, 13081, HIGH)                                   # gaps: 13080 -7- 13087 -8- 13095
    put(13087, 13088, HIGH)
    put(13095, 13096, HIGH)
    put(14000, 14010, HIGH, 2)                                # CHH rows, every other key with low bits 3
    motif[14001:14010:2] = 3
    motif[15000:16000:37] = 1                                 # CHG rows 37 apart
    t[:, 15000:16000:37] = np.array(LOW)[:, None]
    rng = np.random.default_rng(99)                           # and noise: counts 0 .. 3, a quarter of the loci uncovered
    t[:, 16000:20000] = rng.integers(0, 4, (2, 4000)) * (rng.random(4000) > 0.25)
    put(N_LOCI - 12, N_LOCI - 2, NONE)
    put(N_LOCI - 2, N_LOCI, FLAT)                             # d == 0 at the end
    key = (np.arange(N_LOCI, dtype=np.int64) % 100003) << 2 | motif
    return t[0].astype(np.int32), t[1].astype(np.int32), key.astype(np.int32)


def _host_loci(host, lo=0, hi=N_LOCI, base=0):
    """the hm_locus_t rows hm_pileup_fetch_loci must give for the planes"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    p, n, key = (x[lo:hi] for x in host)
    on = np.nonzero((p | n) != 0)[0]
    rows = np.zeros(len(on), LOCUS_DTYPE)
    rows["gpos"], rows["pcov"], rows["ncov"], rows["motif"] = on + lo + base, p[on], n[on], key[on] & 3
    return rows


def _d(rows, A, B, S, max_gap):
    """-> (d_t, S_t) per row: delta_t(1) - delta_t(0) by its recurrence, to locate the planted ties"""
    e, cost = emissions(rows["pcov"], rows["ncov"], A, B), switch_costs(rows["gpos"], S, max_gap)
    d, x = [], 0
    for t in range(len(e)):
        x = min(max(x, -cost[t]), cost[t]) + e[t]
        d.append(x)
    return d, cost


def _brief(segs):
    return [tuple(int(g[f]) for f in ("start", "end", "n_loci", "state", "flags")) for g in segs]


def test_crafted_planes_hold_the_cases():
    host = _crafted()
    loci = _host_loci(host)
    A, B, S, max_gap = SETS["tie"]
    r0 = ctx_rows(loci, 0)
    assert len(r0) > 3 * WG + 4096 * 3 and len(ctx_rows(loci, 1)) == 29 and len(ctx_rows(loci, 2)) == 10
    assert (ctx_rows(loci, 2)["motif"] == 3).sum() == 5 and (host[0] < 0).sum() == 1 and host[0].max() > 1 << 20 and host[1].max() > 1 << 21
    row_of = {int(g): i for i, g in enumerate(r0["gpos"])}
    segs, R = domains(loci, 0, A, B, S, max_gap)
    by_start = {int(g["start"]): g for g in segs}
    d, cost = _d(r0, A, B, S, max_gap)
    # a change of state and a break on a row-scan workgroup boundary, and on a 4096-locus boundary
    assert row_of[WG + 5] == WG and by_start[WG + 5]["state"] == 0 and by_start[WG + 5]["flags"] == BEFORE_BREAK
    assert any(g["end"] == WG + 5 and g["state"] == 1 for g in segs)
    assert row_of[2 * WG + 13] == 2 * WG and by_start[2 * WG + 13]["flags"] & AFTER_BREAK and cost[2 * WG] == 0
    assert by_start[4096]["state"] == 0 and any(g["end"] == 4096 and g["state"] == 1 for g in segs)
    assert by_start[8200]["flags"] & AFTER_BREAK and any(g["end"] == 8192 and g["flags"] & BEFORE_BREAK for g in segs)
    # the long run: neither clamp acts and every back-pointer is the identity, over more than a whole workgroup on either side
    a, b = row_of[9000], row_of[12999]
    assert b - a > 3 * WG and all(abs(d[t - 1]) <= cost[t] == S for t in range(a + 1, b + 1))
    assert sum(1 for g in segs if g["start"] <= 9000 and g["end"] >= 13000) == 1
    # the high segment is not cut by another context's locus, an uncovered locus, a negative counter or a counter above 2^20
    g = by_start[8600]
    assert g["end"] == 8700 and g["n_loci"] == 97 and g["state"] == 1 and g["pcov"] == 3 * 96 + BIG
    # ties
    assert d[row_of[13008]] == S == cost[row_of[13009]] and by_start[13008]["state"] == 0 and by_start[13008]["n_loci"] == 4
    assert d[row_of[13030]] == -S and by_start[13030]["state"] == 1 and by_start[13030]["n_loci"] == 4
    assert d[row_of[13050]] == 0 and cost[row_of[13060]] == 0 and _brief([by_start[13050]]) == [(13050, 13051, 1, 1, AFTER_BREAK | BEFORE_BREAK)]
    assert d[-1] == 0 and _brief(segs[-1:]) == [(N_LOCI - 2, N_LOCI, 2, 0, AFTER_BREAK | BEFORE_BREAK)]
    # a gap of max_gap links, max_gap + 1 breaks
    assert _brief([by_start[13080], by_start[13095]]) == [(13080, 13088, 2, 1, AFTER_BREAK | BEFORE_BREAK), (13095, 13096, 1, 1, AFTER_BREAK | BEFORE_BREAK)]
    chh, R2 = domains(loci, 2, A, B, S, max_gap)
    assert R2 == 10 and _brief(chh) == [(14000, 14010, 10, 1, AFTER_BREAK | BEFORE_BREAK)]
    assert len(domains(loci, 1, A, B, S, max_gap)[0]) == 29 and len(domains(loci, 1, *SETS["scores"])[0]) == 2
    assert len(segs) > 200 and {int(s) for s in segs["state"]} == {0, 1}


@pytest.fixture(scope="module")
def crafted():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    host = _crafted()
    pu = MethylationPileup([("c", "ACGT" * 50)])             # caller-owned planes: the reference plays no part
    dev = [torch.from_numpy(x.copy()).cuda() for x in host]
    loci = pu.loci(0, N_LOCI, planes=dev)
    assert loci.tobytes() == _host_loci(host).tobytes()
    yield pu, host, dev, loci
    pu.close()


def _partitions(got, n_ctx, host, lo, hi, ctx):
    p, n, key = (x[lo:hi].astype(np.int64) for x in host)
    row = (p >= 0) & (n >= 0) & (p + n > 0) & (np.minimum(key & 3, 2) == ctx)
    assert int(got["n_loci"].sum()) == n_ctx == int(row.sum())
    assert int(got["pcov"].sum()) == int(p[row].sum()) and int(got["ncov"].sum()) == int(n[row].sum())
    assert (got["start"][1:] >= got["end"][:-1]).all() and (got["motif"] == ctx).all()


@pytest.mark.parametrize("name", list(SETS))
def test_domains_equal_the_reference_on_the_device_rows(crafted, name):
    from hifimeth_amd.pileup import DOMAIN_DTYPE
    pu, host, dev, loci = crafted
    rule = SETS[name]
    seen = 0
    for ctx in range(3):
        want, R = domains(loci, ctx, *rule)
        got, n_ctx = pu.domains(ctx, 0, N_LOCI, *rule, planes=dev)
        assert got.dtype == DOMAIN_DTYPE and n_ctx == R
        assert len(got) == len(want) and got.tobytes() == want.tobytes(), (name, ctx)
        _partitions(got, n_ctx, host, 0, N_LOCI, ctx)
        seen += len(got)
    print(name, "segments:", seen)
    assert seen > {"tie": 200, "scores": 20, "free": 3000, "bounds": 1000}[name]


RANGES = {"mid-segment, rows from one workgroup into the next": (8650, 8650 + 3000), "inside the long run": (9500, 12001),
          "on block edges": (4096, 8192), "one row": (5, 6), "no row": (0, 5), "two rows across a break": (13050, 13061)}


@pytest.mark.parametrize("where", list(RANGES))
def test_sub_ranges_and_plane_base(crafted, where):
    """[lo, hi) in plane coordinates, then the same loci as a chunk whose element 0 is locus plane_base, just below 2^31 and 2^32"""
    pu, host, dev, _loci = crafted
    lo, hi = RANGES[where]
    for name in ("tie", "scores"):
        rule = SETS[name]
        for ctx in (0, 1):
            rows = pu.loci(lo, hi, planes=dev)
            want, R = domains(rows, ctx, *rule)
            got, n_ctx = pu.domains(ctx, lo, hi, *rule, planes=dev)
            assert n_ctx == R and got.tobytes() == want.tobytes(), (where, name, ctx)
            _partitions(got, n_ctx, host, lo, hi, ctx)
            if where == "one row" and ctx == 0:
                assert R == 1 and len(got) == 1 and got[0]["flags"] == AFTER_BREAK | BEFORE_BREAK and got[0]["n_loci"] == 1
            if where == "no row":
                assert R == 0 and len(got) == 0
            for shift in ((1 << 31) - lo - 1000, (1 << 32) - lo - 1000):
                chunk = [t[lo:] for t in dev]
                moved, n2 = pu.domains(ctx, 0, hi - lo, *rule, planes=chunk, plane_base=shift + lo)
                w2, R2 = domains(pu.loci(0, hi - lo, planes=chunk, plane_base=shift + lo), ctx, *rule)
                assert n2 == R2 == R and moved.tobytes() == w2.tobytes()
                back = moved.copy()
                back["start"] -= shift
                back["end"] -= shift
                assert back.tobytes() == got.tobytes()
    if where == "mid-segment, rows from one workgroup into the next":
        whole = pu.domains(0, 0, N_LOCI, *SETS["tie"], planes=dev)[0]
        part = pu.domains(0, lo, hi, *SETS["tie"], planes=dev)[0]
        assert part[0]["start"] == lo and part[0]["end"] == 8700 and part[0]["state"] == 1 and lo not in whole["start"]


def test_cap_empty_range_and_abi_errors(crafted):
    from hifimeth_amd.pileup import DOMAIN_DTYPE, MethylationPileup
    pu, _host, dev, _loci = crafted
    A, B, S, max_gap = SETS["tie"]
    L, ptrs, none = pu._L, [ctypes.c_void_p(t.data_ptr()) for t in dev], [None] * 3
    f = L.hm_pileup_fetch_domains
    want, R = pu.domains(0, 0, N_LOCI, A, B, S, max_gap, planes=dev)
    n = len(want)
    out = np.zeros(n, DOMAIN_DTYPE)
    out["start"] = -7
    po, rows_seen = out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(-1)
    ok = (0, A, B, S, max_gap)
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, *ok, ctypes.byref(rows_seen), po, n - 1) == n and rows_seen.value == R
    assert (out["start"] == -7).all() and (out["n_loci"] == 0).all()                    # cap too small: nothing is written
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, *ok, None, None, 0) == n
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, *ok, None, po, n) == n and out.tobytes() == want.tobytes()
    rows_seen.value = -1
    assert f(pu._h, *ptrs, 0, 77, 77, *ok, ctypes.byref(rows_seen), po, n) == 0 and rows_seen.value == 0          # hi == lo
    assert out.tobytes() == want.tobytes()
    W = 1 << 24
    bad = [(-1, A, B, S, 7), (3, A, B, S, 7), (0, 0, B, S, 7), (0, -4, B, S, 7), (0, W + 1, B, S, 7), (0, A, 0, S, 7), (0, A, 4, S, 7),
           (0, A, -W - 1, S, 7), (0, A, B, -1, 7), (0, A, B, W + 1, 7), (0, A, B, S, 0), (0, A, B, S, -3)]
    for args in bad:
        assert f(pu._h, *ptrs, 0, 0, N_LOCI, *args, None, None, 0) == -1, args
        assert b"hm_pileup_fetch_domains" in L.hm_pileup_last_error(pu._h)
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, 0, 1, -1, 0, 1, None, None, 0) > 0              # the bounds themselves are allowed
    assert f(pu._h, *ptrs, 0, 9, 8, *ok, None, None, 0) == -1 and f(pu._h, *ptrs, 0, -1, 8, *ok, None, None, 0) == -1
    assert f(None, *ptrs, 0, 0, 8, *ok, None, None, 0) == -1
    own = MethylationPileup([("c", "ACGT" * 50)])
    rows, R0 = own.domains(0)                                 # own planes, nothing counted yet; the default weights
    assert R0 == 0 and len(rows) == 0 and own.domains(2, A=A, B=B, S=S, max_gap=max_gap)[1] == 0
    assert f(own._h, *none, 0, 0, 201, *ok, None, None, 0) < 0                           # own planes end with the reference
    own.close()


# ---- through reads: the engine's own planes and the CLI ------------------------------------------------------------------------------
def _parse_cov(prefix, genome):
    """-> hm_locus_t-like rows per (sequence index, context) from <prefix>.<ctx>.cov.bed, gpos in the concatenated reference"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    names = [n for n, _ in genome]
    start = dict(zip(names, np.concatenate([[0], np.cumsum([len(s) for _, s in genome])])))
    rows = {(s, c): [] for s in range(len(genome)) for c in range(3)}
    for c, cn in enumerate(CTX):
        for line in open(f"{prefix}.{cn}.cov.bed"):
            chrom, a, _b, _f, p, n = line.split("\t")
            rows[names.index(chrom), c].append((int(start[chrom]) + int(a), int(p), int(n), c, 0))
    return {k: np.array(v, LOCUS_DTYPE) if v else np.zeros(0, LOCUS_DTYPE) for k, v in rows.items()}


def test_cli_domains(tmp_path):
    from bamutil import write_fasta
    from hifimeth_amd.pileup import domain_scores, domains_bed
    genome, reads = _phased_reads()
    bam, fa, prefix = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "out")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    levels, penalty, max_gap = ((0.2, 0.8), None, (0.1, 0.6)), 1.5, 40
    args = ["-D", "-u", "0.2:0.8,nan,0.1:0.6", "-x", "1.5", "-j", "40"]
    _run_cli([fa, bam, prefix + "0"])
    r1 = _run_cli([*args, fa, bam, prefix + "1"])
    _run_cli(["-H", *args, fa, bam, prefix + "2"])
    assert f"{prefix}1.domains.*" in r1.stderr
    cov = _parse_cov(prefix + "1", genome)
    offsets = np.concatenate([[0], np.cumsum([len(s) for _, s in genome])])
    text, states = {c: "" for c in CTX}, set()
    for s in range(len(genome)):
        for c in range(3):
            if levels[c] is None:
                continue
            segs, _R = domains(cov[s, c], c, *domain_scores(*levels[c], penalty), max_gap)
            text[CTX[c]] += domains_bed(segs, [n for n, _ in genome], offsets)[CTX[c]]
            states |= {(c, int(z)) for z in segs["state"]}
    got = {c: open(f"{prefix}1.domains.{c}.bed").read() for c in CTX}
    print("segments:", {c: len(t.splitlines()) for c, t in got.items()})
    assert states >= {(0, 0), (0, 1), (2, 0)} and text["CHG"] == ""                    # an empty expectation cannot pass
    assert got == text and got == {c: open(f"{prefix}2.domains.{c}.bed").read() for c in CTX}
    assert all(len(line.split("\t")) == 9 and line.split("\t")[4] in "LH" for t in got.values() for line in t.splitlines())
    # every other file of the run is the run's without -D, and that run writes no domain file
    for c in CTX:
        assert open(f"{prefix}0.{c}.cov.bed").read() == open(f"{prefix}1.{c}.cov.bed").read() == open(f"{prefix}2.{c}.cov.bed").read()
    assert sorted(os.listdir(tmp_path)) == sorted(
        ["mod.bam", "ref.fa"] + [f"out{k}.{c}.cov.bed" for k in "012" for c in CTX] + [f"out{k}.domains.{c}.bed" for k in "12" for c in CTX]
        + [f"out2.hap{h}.{c}.cov.bed" for h in "12" for c in CTX])
