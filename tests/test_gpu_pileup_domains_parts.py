"""Methylation domains from pieces on the device: hm_pileup_fetch_domains_part chained by chain_domain_parts and joined by
stitch_domains over caller-owned crafted planes, against ONE hm_pileup_fetch_domains over the whole -- the raw 64-byte rows must be
equal, floats as bits, flags included -- and `pileup_dist -D` against `pileup -D`.  Nothing here has a tolerance."""
import ctypes
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest

from test_gpu_pileup_asm import CTX, ROOT, _dist_env, _run_cli, _write_bam

pytestmark = pytest.mark.gpu

WG = 1024                                                     # rows per row-scan workgroup (SCAN_ROWS)
TIE = (4, -4, 8, 7)                                           # (A, B, S, max_gap); e = 4 (pcov - ncov)
SCORES = (136278, -98571, 524288, 1000)                       # domain_scores(0.1, 0.8, 8)
HIGH, LOW, NONE = (3, 0), (0, 3), (0, 0)


@pytest.fixture(scope="module")
def pu():
    from hifimeth_amd.pileup import MethylationPileup
    p = MethylationPileup([("c", "ACGT" * 50)])              # caller-owned planes: the reference plays no part
    yield p
    p.close()


def _dev(host):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in host]


def _raw(rows):
    return np.ascontiguousarray(rows).view(np.uint8).reshape(-1, 64)


def _chain(pu, dev, edges, ctx, rule, base=0):
    """the loci [edges[0], edges[-1]) of the planes cut at edges[1:-1] -> (stitched, per-piece segments)"""
    from hifimeth_amd.pileup import chain_domain_parts, stitch_domains
    pieces = [partial(pu.domains_part, ctx, a, b, planes=dev, plane_base=base) for a, b in zip(edges, edges[1:])]
    parts = chain_domain_parts(pieces, *rule)
    return stitch_domains(parts, rule[0], rule[1]), parts


def _same(pu, dev, cuts, ctx, rule, whole, n):
    got, parts = _chain(pu, dev, [0, *cuts, n], ctx, rule)
    assert np.array_equal(_raw(got), _raw(whole)), (cuts, ctx, rule)
    return parts


def _mixed(n, seed):
    """n loci: stretches of high and of low rows with noise, a quarter uncovered, the three contexts interleaved at random"""
    rng = np.random.default_rng(seed)
    run = np.repeat(rng.integers(0, 2, n), rng.integers(2, 9, n))[:n]
    p = np.where(run, rng.integers(1, 4, n), rng.integers(0, 2, n))
    u = np.where(run, rng.integers(0, 2, n), rng.integers(1, 4, n))
    off = rng.random(n) < 0.25
    p[off], u[off] = 0, 0
    motif = rng.integers(0, 4, n)                             # 3: CHH too (min(key & 3, 2))
    key = (np.arange(n) % 1009) << 2 | motif
    return p, u, key


def test_thirty_rows_every_cut(pu):
    """about 30 rows per context among 120 loci: cut before every locus into two pieces, and at a sample of pairs into three"""
    n = 120
    host = _mixed(n, 21)
    dev = _dev(host)
    rng = np.random.default_rng(22)
    pairs = [tuple(sorted(int(x) for x in rng.integers(0, n + 1, 2))) for _ in range(10)] + [(0, 0), (n, n), (40, 40), (0, n)]
    for ctx in range(3):
        for rule in (TIE, SCORES):
            whole, R = pu.domains(ctx, 0, n, *rule, planes=dev)
            assert 20 <= R <= 60 and (rule is SCORES or len(whole) >= 4)
            for cut in range(n + 1):
                _same(pu, dev, [cut], ctx, rule, whole, n)
            for a, b in pairs:
                _same(pu, dev, [a, b], ctx, rule, whole, n)
    assert {int(z) for z in pu.domains(0, 0, n, *TIE, planes=dev)[0]["state"]} == {0, 1}


def _three_workgroups():
    """3 * WG + 5 CpG rows, row k at locus 3 k + 1 between a CHG row and an uncovered locus; stretches of 40 high / 25 low rows, a
    state change on rows WG - 1 | WG, and two breaks (max_gap 7: five loci of the pattern without their CpG row)"""
    R = 3 * WG + 5
    n = 3 * (R + 10)
    p, u, key = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    cpg = np.arange(1, n, 3)
    p[cpg - 1], u[cpg - 1], key[cpg - 1] = 1, 2, 1            # CHG rows; loci 3 k + 2 stay uncovered
    cpg = np.delete(cpg, np.r_[700:705, 2 * WG + 2:2 * WG + 7])   # ten candidates less: R rows
    high = (np.arange(R) + 16) % 65 < 40                      # row WG - 1 is low, row WG high
    p[cpg], u[cpg] = np.where(high, 3, 0), np.where(high, 0, 3)
    key = key | (np.arange(n) % 997) << 2
    return (p, u, key), R


def test_pieces_and_whole_span_several_scan_workgroups(pu):
    host, R = _three_workgroups()
    n = len(host[0])
    dev = _dev(host)
    rows = pu.loci(0, n, planes=dev)
    gpos = rows["gpos"][(rows["motif"] == 0)]
    assert len(gpos) == R == 3 * WG + 5 and gpos[WG] != WG    # locus index and row index differ
    cuts = [int(gpos[k]) for k in (1023, 1024, 1025, 2048, 3076)]   # the piece right of a cut starts with that row
    for rule in (TIE, SCORES):
        whole, Rw = pu.domains(0, 0, n, *rule, planes=dev)
        assert Rw == R
        for c in cuts:
            _same(pu, dev, [c], 0, rule, whole, n)
        parts = _same(pu, dev, cuts, 0, rule, whole, n)
        assert [int(p["n_loci"].sum()) for p in parts] == [1023, 1, 1, 1023, 1028, 1]
    whole = pu.domains(0, 0, n, *TIE, planes=dev)[0]
    assert len(whole) > 90 and (whole["flags"] != 0).sum() == 6 and int(gpos[WG]) in whole["start"]
    whole1, R1 = pu.domains(1, 0, n, *TIE, planes=dev)        # the other context of the same planes, cut at the same loci
    assert R1 == R + 10
    _same(pu, dev, cuts, 1, TIE, whole1, n)


def test_one_high_domain_in_sixteen_pieces(pu):
    R = 2 * WG + 52
    host = (np.full(R, 3), np.zeros(R, np.int64), np.arange(R) << 2)
    dev = _dev(host)
    whole, Rw = pu.domains(0, 0, R, *TIE, planes=dev)
    assert Rw == R > 2048 and len(whole) == 1
    edges = [R * k // 16 for k in range(17)]
    got, parts = _chain(pu, dev, edges, 0, TIE)
    assert all(len(p) == 1 for p in parts) and len(got) == 1
    assert (int(got[0]["pcov"]), int(got[0]["ncov"]), int(got[0]["n_loci"]), int(got[0]["state"]), int(got[0]["flags"])) == (3 * R, 0, R, 1, 3)
    assert np.array_equal(_raw(got), _raw(whole))


def test_cuts_in_and_next_to_a_break(pu):
    from hifimeth_amd.pileup import DOMAIN_AFTER_BREAK, DOMAIN_BEFORE_BREAK
    n = 60
    p, u = np.zeros(n, np.int64), np.zeros(n, np.int64)
    p[10:20], p[40:50] = 3, 3                                 # high rows 10 .. 19, nothing for 20 loci (max_gap 7), high rows 40 .. 49
    u[5:10], u[50:55] = 3, 3
    dev = _dev((p, u, np.arange(n) << 2))
    whole, R = pu.domains(0, 0, n, *TIE, planes=dev)
    assert R == 30 and [(int(g["start"]), int(g["end"]), int(g["state"]), int(g["flags"])) for g in whole] == \
        [(5, 10, 0, DOMAIN_AFTER_BREAK), (10, 20, 1, DOMAIN_BEFORE_BREAK), (40, 50, 1, DOMAIN_AFTER_BREAK), (50, 55, 0, DOMAIN_BEFORE_BREAK)]
    for cut in (30, 19, 20, 21, 39, 40, 41):                  # inside the break; one locus before it, on it and after it, at either end
        parts = _same(pu, dev, [cut], 0, TIE, whole, n)
        if 20 <= cut <= 40:                                   # the break lies on the cut: both edge segments say so
            assert int(parts[0][-1]["flags"]) & DOMAIN_BEFORE_BREAK and int(parts[1][0]["flags"]) & DOMAIN_AFTER_BREAK
        else:
            assert not int(parts[0][-1]["flags"]) & DOMAIN_BEFORE_BREAK and not int(parts[1][0]["flags"]) & DOMAIN_AFTER_BREAK
    _same(pu, dev, [25, 35], 0, TIE, whole, n)                # a piece without rows inside the break
    _same(pu, dev, [19, 41], 0, TIE, whole, n)


@pytest.mark.parametrize("edge", [1 << 31, 1 << 32])
def test_separate_buffers_with_a_boundary_on_a_power_of_two(pu, edge):
    """three pieces, each a buffer of its own whose element 0 is the piece's first locus; the middle one starts at `edge`"""
    from hifimeth_amd.pileup import chain_domain_parts, stitch_domains
    n = 120
    host = _mixed(n, 33)
    whole_dev = _dev(host)
    for ctx in (0, 2):
        at0 = pu.domains(ctx, 0, n, *TIE, planes=whole_dev)[0]
        g = at0[np.argmax(at0["n_loci"])]                     # the boundary goes inside the segment with the most rows
        a = (int(g["start"]) + int(g["end"])) // 2
        b, base = min(a + 35, n - 5), edge - a
        assert g["n_loci"] >= 3 and g["start"] < a < g["end"] - 1 and 0 < a < b
        whole, R = pu.domains(ctx, 0, n, *TIE, planes=whole_dev, plane_base=base)
        assert R >= 15 and any(w["start"] < edge < w["end"] - 1 for w in whole)
        pieces = [partial(pu.domains_part, ctx, 0, hi - lo, planes=_dev([x[lo:hi] for x in host]), plane_base=base + lo)
                  for lo, hi in ((0, a), (a, b), (b, n))]
        got = stitch_domains(chain_domain_parts(pieces, *TIE), TIE[0], TIE[1])
        assert np.array_equal(_raw(got), _raw(whole))


def test_pieces_without_a_row_of_the_context(pu):
    from hifimeth_amd.pileup import DOMAIN_PASS_SUMMARY
    n = 90
    p, u, key = _mixed(n, 44)
    key[30:60] &= ~3                                          # nothing but CpG loci in the middle third
    p[28], u[28], key[28] = 3, 0, 29 << 2 | 1                 # CHG rows right at its edges, 33 loci apart: under SCORES they link
    p[61], u[61], key[61] = 3, 0, 62 << 2 | 1
    dev = _dev((p, u, key))
    assert pu.domains_part(1, 30, 60, DOMAIN_PASS_SUMMARY, None, *TIE, planes=dev) == {"n_rows": 0}
    assert pu.domains_part(0, 30, 60, DOMAIN_PASS_SUMMARY, None, *TIE, planes=dev)["n_rows"] > 10
    for rule in (TIE, SCORES):
        whole, R = pu.domains(1, 0, n, *rule, planes=dev)
        assert R >= 8
        for cuts in ([30, 60], [30, 40, 50, 60], [10, 30, 60, 80], [29, 30, 60, 61]):
            _same(pu, dev, cuts, 1, rule, whole, n)
    assert any(g["start"] <= 28 and g["end"] >= 62 for g in pu.domains(1, 0, n, *SCORES, planes=dev)[0])   # a segment across the empty pieces


def test_argument_errors_leave_the_engine_usable(pu):
    from hifimeth_amd.caller import HifimethError
    from hifimeth_amd.pileup import DOMAIN_PASS_CODES, DOMAIN_PASS_SEGMENTS
    n = 120
    dev = _dev(_mixed(n, 21))
    whole = pu.domains(0, 0, n, *TIE, planes=dev)[0]
    ok = {"has_prev": 1, "prev_gpos": 999, "prev_d": 1 << 46}
    for bad in ({**ok, "prev_d": (1 << 46) + 1}, {**ok, "prev_d": -(1 << 46) - 1}, {**ok, "prev_gpos": 1040}, {**ok, "prev_gpos": 1041},
                {**ok, "prev_gpos": -1}):
        for pass_ in (DOMAIN_PASS_CODES, DOMAIN_PASS_SEGMENTS):
            with pytest.raises(HifimethError, match="hm_pileup_fetch_domains_part"):
                pu.domains_part(0, 40, n, pass_, bad, *TIE, planes=dev, plane_base=1000)
        rc = pu._L.hm_pileup_fetch_domains_part(pu._h, *[ctypes.c_void_p(t.data_ptr()) for t in dev], 1000, 40, n, 0, *TIE, DOMAIN_PASS_CODES,
                                                ctypes.byref(_part(bad)), None, 0)
        assert rc == -1                                       # HM_EINVAL
        _same(pu, dev, [40], 0, TIE, whole, n)                # the following valid calls are correct
    for good in (ok, {**ok, "prev_d": -(1 << 46)}, {**ok, "prev_gpos": 1039}):
        assert pu.domains_part(0, 40, n, DOMAIN_PASS_CODES, good, *TIE, planes=dev, plane_base=1000)["n_rows"] > 0
    with pytest.raises(HifimethError):
        pu.domains_part(0, 40, n, DOMAIN_PASS_SEGMENTS, {"has_next": 1, "next_gpos": n + 5, "last_state": 2}, *TIE, planes=dev)
    with pytest.raises(HifimethError):
        pu.domains_part(0, 40, n, DOMAIN_PASS_SEGMENTS, {"has_next": 1, "next_gpos": n - 1, "last_state": 1}, *TIE, planes=dev)
    with pytest.raises(HifimethError):
        pu.domains_part(0, 40, n, 3, None, *TIE, planes=dev)
    _same(pu, dev, [40], 0, TIE, whole, n)


def _part(fields):
    from hifimeth_amd.pileup import _DomainPart
    return _DomainPart(**fields)


# ---- the distributed driver against the CLI ------------------------------------------------------------------------------------------
LEVELS = "0.2:0.8,0.1:0.6,0.1:0.6"
J = 150


def _two_sequences(case):
    """-> (genome, reads): two sequences, the first the longer one, so that the middle of the concatenated planes -- the border of
    two ranks -- lies in it; "domain": the reads are methylated in the 1000 bases around the border and unmethylated elsewhere on
    that sequence; "gap": no read touches the 600 bases around it"""
    import dataclasses
    from hifimeth_amd.pileup import parse_mods
    from hifimeth_amd.synth import synth_alignments, synth_genome
    g3 = synth_genome(n_chr=3, length=4000, seed=77)
    genome = [g3[2], g3[0]]                                   # 6400 and 4000 bases
    border = (sum(len(s) for _, s in genome) + 1) // 2
    assert border + 1000 < len(genome[0][1])
    rng = np.random.default_rng(78)
    out = []
    for r in synth_alignments(genome, 220, seed=79, median_len=1000):
        ml = r.ml
        span = sum(n for op, n in r.cigar if op in "M=XDN")
        if r.tid == 0 and not r.flag & 4:
            if case == "gap" and r.pos < border + 300 and r.pos + span > border - 300:
                continue
            if ml is not None:
                q = parse_mods(r.seq, r.flag, r.mm, ml)["qoff"].astype(np.int64)
                g = r.pos + (r.l_qseq - 1 - q if r.flag & 16 else q)      # about the reference position (indels are rare)
                ml = np.where(np.abs(g - border) < 500, 225 + (q % 30), 5 + (q % 30)).astype(np.uint8)
        out.append(dataclasses.replace(r, ml=ml, hp=[1, 2, None][int(rng.integers(0, 3))]))
    return genome, out, border


def _dist(args, fa, bam, prefix, port):
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "--slab", "7", "--backend", "gloo"]
    procs = [subprocess.Popen([*mod, fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]


def _files(prefix, domains):
    names = [f"{t}{c}.cov.bed" for t in ("", "hap1.", "hap2.") for c in CTX] + [f"asm.{c}.bed" for c in CTX]
    return {n: open(f"{prefix}.{n}").read() for n in (([f"domains.{c}.bed" for c in CTX]) if domains else names)}


@pytest.mark.parametrize("case", ["domain", "gap", "nan"])
def test_pileup_dist_domains(tmp_path, case):
    """python -m hifimeth_amd.pileup_dist -H -A -D on two gloo ranks sharing the card: the three domain files are `pileup -D`'s byte
    for byte and the twelve other files are those of the run without -D.  The ranks' border lies inside a high CpG domain of the
    first sequence ("domain", and "nan" with CHG not segmented, also run as a world of one) or inside a gap wider than -j ("gap")."""
    from bamutil import write_fasta
    genome, reads, border = _two_sequences("gap" if case == "gap" else "domain")
    bam, fa, cli, prefix = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "cli"), str(tmp_path / "gloo")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    args = ["-D", "-u", "0.2:0.8,nan,0.1:0.6" if case == "nan" else LEVELS, "-x", "1.5", "-j", str(J)]
    _run_cli([*args, fa, bam, cli])
    want = _files(cli, True)
    rows = [line.split("\t") for line in want["domains.CpG.bed"].splitlines()]
    first = [(int(f[1]), int(f[2]), f[4]) for f in rows if f[0] == genome[0][0]]
    assert any(f[0] == genome[1][0] for f in rows) and all(want[f"domains.{c}.bed"] or (case == "nan" and c == "CHG") for c in CTX)
    if case == "gap":
        loci = [int(line.split("\t")[1]) for line in open(f"{cli}.CpG.cov.bed") if line.split("\t")[0] == genome[0][0]]
        assert max(x for x in loci if x < border) + J < border < min(x for x in loci if x >= border) - J
        assert all(b <= border or a >= border for a, b, _z in first)
    else:
        assert any(a < border - J and b > border + J and z == "H" for a, b, z in first), first
    _dist(["-H", "-A", *args], fa, bam, prefix, 29591)
    assert _files(prefix, True) == want
    if case == "nan":                                         # a world of one: the same code with the exchanges skipped
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "--slab", "7", fa, bam, prefix + "1"], capture_output=True,
                           text=True, env=_dist_env(), cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert _files(prefix + "1", True) == want
    else:
        _dist(["-H", "-A"], fa, bam, prefix + "0", 29592)
        assert _files(prefix + "0", False) == _files(prefix, False)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("gloo0.domains")]
