"""Allele-specific methylation (`pileup -H -A`): loci where each haplotype has at least `min_cov` counted calls, the difference of
the two methylation percentages and the two-sided Fisher exact test of [[p1, n1], [p2, n2]] (R's rule), computed on the device.

The reference for `pvalue` is exact integer arithmetic (`fisher_exact` below): weights w(x) = C(r1, x) C(r2, c1 - x), a table is
included iff w(x) * 10^7 <= w(observed) * (10^7 + 1), p = sum / C(n, c1) as a Fraction.  Tolerances are derived, not measured:
* tables with row sums <= 24: log n! <= 141 (n <= 48), nine table terms per probability, fp64 ulp there 3e-14 -> about 3e-13
  expected; the bound is 1e-9 relative, three orders above that for the device's exp;
* cells up to 1e4 / totals up to 8e4: log n! ~ 8e5, ulp 1.2e-10, nine terms -> about 1e-9 per probability; the bound is 1e-6.
`diff` must be bit-equal to numpy's 100.0 * p1 / (p1 + n1) - 100.0 * p2 / (p2 + n2)."""
import ctypes
import dataclasses
import math
import os
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
CTX = ("CpG", "CHG", "CHH")
DBL_MIN = 2.2250738585072014e-308
HM_EINVAL, HM_ESTATE = -1, -5


# ---- the exact reference ----------------------------------------------------------------------------------------------------
def fisher_weights(p1, n1, p2, n2):
    """-> (xlo, [w(x) for x in xlo..xhi], C(n, c1)): integer weights of all tables with the margins of [[p1, n1], [p2, n2]].
    w(x+1) = w(x) (r1 - x)(c1 - x) / ((x + 1)(r2 - c1 + x + 1)) exactly (both sides are products of binomials), which keeps the
    large tables cheap; the end points, the observed table and the total are checked against math.comb."""
    r1, r2, c1 = p1 + n1, p2 + n2, p1 + p2
    xlo, xhi = max(0, c1 - r2), min(r1, c1)
    w = [math.comb(r1, xlo) * math.comb(r2, c1 - xlo)]
    for x in range(xlo, xhi):
        num = w[-1] * (r1 - x) * (c1 - x)
        den = (x + 1) * (r2 - c1 + x + 1)
        assert num % den == 0
        w.append(num // den)
    total = math.comb(r1 + r2, c1)
    assert w[-1] == math.comb(r1, xhi) * math.comb(r2, c1 - xhi) and w[p1 - xlo] == math.comb(r1, p1) * math.comb(r2, p2)
    assert sum(w) == total                                    # Vandermonde
    return xlo, w, total


def fisher_exact(p1, n1, p2, n2, band_check=False):
    """two-sided Fisher exact p of [[p1, n1], [p2, n2]] as a Fraction, R's rule.  band_check: assert (in integers) that no weight
    other than an exact tie lies within 1e-6 relative of the band edge w(obs) (1 + 1e-7), so that rounding on the device
    cannot change which tables are summed."""
    xlo, w, total = fisher_weights(p1, n1, p2, n2)
    obs = w[p1 - xlo]
    edge7 = obs * (10 ** 7 + 1)                               # edge * 10^7
    if band_check:
        for v in w:
            assert v == obs or abs(v * 10 ** 7 - edge7) * 10 ** 6 > edge7, (p1, n1, p2, n2)
    return Fraction(sum(v for v in w if v * 10 ** 7 <= edge7), total)


def _rel_err(got, want: Fraction):
    return float(abs(Fraction(float(got)) - want) / want)


def _np_diff(p1, n1, p2, n2):
    p1, n1, p2, n2 = (np.asarray(x, np.int64) for x in (p1, n1, p2, n2))
    return 100.0 * p1 / (p1 + n1) - 100.0 * p2 / (p2 + n2)


# ---- planes filled by hand ----------------------------------------------------------------------------------------------------
def _all_tables(max_row=24):
    t = [(a, r1 - a, c, r2 - c) for r1 in range(1, max_row + 1) for a in range(r1 + 1)
         for r2 in range(1, max_row + 1) for c in range(r2 + 1)]
    return np.array(t, np.int32)


def _planes(tables, gap=0):
    """four int32 planes + key (motif cycling 0 / 1 / 2 under an order in the upper bits) on the GPU; `gap` zero loci between rows"""
    import torch
    n = len(tables) * (gap + 1)
    host = np.zeros((4, n), np.int32)
    host[:, ::gap + 1] = tables.T
    key = ((np.arange(n, dtype=np.int64) % 1000) << 2 | (np.arange(n) % 3)).astype(np.int32)
    return [torch.from_numpy(host[k].copy()).cuda() for k in range(4)] + [torch.from_numpy(key).cuda()]


@pytest.fixture(scope="module")
def engine():
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup([("c", "ACGT" * 50)])
    yield pu
    pu.close()


@pytest.fixture(scope="module")
def every_table(engine):
    tables = _all_tables()
    assert len(tables) == 324 * 324
    planes = _planes(tables)
    rows = engine.asm(0, len(tables), min_cov=1, planes=planes)
    return tables, planes, rows


def test_every_table_through_caller_planes(every_table):
    tables, _planes_, rows = every_table
    assert len(rows) == len(tables)
    assert (rows["gpos"] == np.arange(len(tables))).all()
    for k, f in enumerate(("pcov1", "ncov1", "pcov2", "ncov2")):
        assert (rows[f] == tables[:, k]).all()
    assert (rows["motif"] == np.arange(len(tables)) % 3).all() and (rows["reserved"] == 0).all()
    want_diff = _np_diff(*tables.T)
    assert (rows["diff"].view(np.uint64) == want_diff.view(np.uint64)).all()
    assert ((rows["pvalue"] >= DBL_MIN) & (rows["pvalue"] <= 1.0)).all()
    cache, worst = {}, 0.0
    for t, got in zip(tables.tolist(), rows["pvalue"]):
        key = tuple(t)
        if key not in cache:
            cache[key] = fisher_exact(*t)
        worst = max(worst, _rel_err(got, cache[key]))
    print(f"worst relative error of pvalue over {len(tables)} tables: {worst:.3e}")
    assert worst <= 1e-9
    # a function of the four counts alone: the mirrored table (haplotypes swapped) has the same p and the opposite diff
    index = {tuple(t): i for i, t in enumerate(tables.tolist())}
    swap = np.array([index[(c, d, a, b)] for a, b, c, d in tables.tolist()])
    assert (rows["diff"][swap] == -rows["diff"]).all()
    assert np.allclose(rows["pvalue"][swap], rows["pvalue"], rtol=2e-9, atol=0)      # both within 1e-9 of the same exact value


def test_min_cov_ranges_and_cap(engine, every_table):
    from hifimeth_amd.pileup import ASM_DTYPE
    tables, planes, rows = every_table
    r1, r2 = tables[:, 0] + tables[:, 1], tables[:, 2] + tables[:, 3]
    for min_cov in (5, 25):
        sel = np.nonzero((r1 >= min_cov) & (r2 >= min_cov))[0]
        got = engine.asm(0, len(tables), min_cov=min_cov, planes=planes)
        assert len(got) == len(sel) and (got == rows[sel]).all()
    assert len(engine.asm(0, len(tables), min_cov=25, planes=planes)) == 0
    for lo, hi in ((0, 1), (4095, 4097), (1000, 50001), (len(tables) - 3, len(tables)), (77, 77)):
        got = engine.asm(lo, hi, min_cov=1, planes=planes)
        assert (got == rows[lo:hi]).all() and len(got) == hi - lo
    # a rank's chunk: planes that start at locus `base` of the job-wide range
    base, lo, hi = 20000, 123, 9000
    chunk = [t[base:] for t in planes]
    got = engine.asm(lo, hi, min_cov=5, planes=chunk, plane_base=base)
    sel = np.nonzero((r1 >= 5) & (r2 >= 5))[0]
    sel = sel[(sel >= base + lo) & (sel < base + hi)]
    assert len(sel) > 100 and (got == rows[sel]).all() and (got["gpos"] == sel).all()
    # cap below the count: the count comes back, nothing is written
    L, ptrs = engine._L, [ctypes.c_void_p(t.data_ptr()) for t in planes]
    out = np.zeros(10, ASM_DTYPE)
    out["gpos"] = -7
    assert L.hm_pileup_fetch_asm(engine._h, *ptrs, 0, 0, 100, 1, out.ctypes.data_as(ctypes.c_void_p), 10) == 100
    assert (out["gpos"] == -7).all() and (out["pvalue"] == 0).all()
    assert L.hm_pileup_fetch_asm(engine._h, *ptrs, 0, 0, 100, 1, None, 0) == 100
    assert L.hm_pileup_fetch_asm(engine._h, *ptrs, 0, 0, 10, 1, out.ctypes.data_as(ctypes.c_void_p), 10) == 10
    assert (out == rows[:10]).all()


BIG = [(10000, 10000, 9800, 10000), (10000, 3, 9990, 17), (5000, 5000, 5000, 5000), (2000, 0, 0, 2000), (1234, 8766, 1300, 8700),
       (9000, 1000, 8900, 1100), (0, 10000, 7, 9993), (3000, 7000, 3000, 7000), (100, 200, 150, 150),
       # totals beyond the 65 536-entry table (lgamma in the kernel); the smallest margin stays small, so the exact sum is short
       (40000, 30, 20, 40000), (70000, 30, 20, 5), (40000, 3, 40000, 40)]


def test_large_counts(engine):
    tables = np.array(BIG, np.int32)
    assert tables[:9].max() == 10000 and (tables[:9].sum(1) <= 40000).all() and (tables[9:].sum(1) > 65536).all()
    planes = _planes(tables, gap=3)
    rows = engine.asm(0, 4 * len(tables), min_cov=1, planes=planes)
    assert (rows["gpos"] == 4 * np.arange(len(tables))).all()
    assert (rows["diff"].view(np.uint64) == _np_diff(*tables.T).view(np.uint64)).all()
    for t, got in zip(BIG, rows["pvalue"]):
        want = fisher_exact(*t, band_check=True)
        if want < Fraction(DBL_MIN):
            print(t, "exact p below the smallest normal double, reported", got)
            assert got == DBL_MIN
            continue
        err = _rel_err(got, want)
        print(t, f"p = {float(want):.6e}, device {got:.6e}, relative error {err:.3e}")
        assert err <= 1e-6, t
    assert fisher_exact(2000, 0, 0, 2000) < Fraction(1, 10 ** 1200) and rows["pvalue"][3] == DBL_MIN
    for i in (2, 7):                                          # identical haplotypes: every table is included
        assert fisher_exact(*BIG[i]) == 1 and rows["pvalue"][i] == 1.0 and rows["diff"][i] == 0.0


# ---- through reads --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def P():
    from oracle import pileup_oracle
    return pileup_oracle


def _as_dict(r):
    return dict(flag=r.flag, tid=r.tid, pos=r.pos, mapq=r.mapq, cigar=r.cigar, seq=r.seq, mm=r.mm, ml=r.ml)


def _phased_reads(n=300, seed=141, median_len=1200, length=4000):
    """synth_alignments reads, hp drawn from {1, 2} (a few None / 3), extra secondary / supplementary flags; inside every third
    600 bp reference interval the ML bytes depend on the haplotype (HP 1 high and HP 2 low, or the reverse)"""
    from hifimeth_amd.pileup import parse_mods
    from hifimeth_amd.synth import synth_alignments, synth_genome
    genome = synth_genome(n_chr=3, length=length, seed=seed)
    reads = synth_alignments(genome, n, seed=seed + 1, median_len=median_len)
    rng = np.random.default_rng(seed + 2)
    out = []
    for r in reads:
        hp = [1, 2, 1, 2, 1, 2, 1, 2, None, 3][int(rng.integers(0, 10))]
        flag = r.flag
        if not flag & 4 and rng.random() < 0.05:
            flag |= 0x100 if rng.random() < 0.5 else 0x800
        ml = r.ml
        if ml is not None and hp in (1, 2) and not flag & 4:
            q = parse_mods(r.seq, flag, r.mm, ml)["qoff"].astype(np.int64)
            g = r.pos + (r.l_qseq - 1 - q if flag & 16 else q)            # about the reference position (indels are rare)
            kind = (g // 600 + r.tid) % 3                                  # 0: as synthesised, 1: HP 1 high, 2: HP 2 high
            high = ((kind == 1) & (hp == 1)) | ((kind == 2) & (hp == 2))
            ml = np.where(kind == 0, ml, np.where(high, 225 + (q % 30), 5 + (q % 30))).astype(np.uint8)
        out.append(dataclasses.replace(r, hp=hp, flag=flag, ml=ml))
    return genome, out


def _expect(P, genome, reads, parts, min_cov, min_mapq=0, min_pi=0.0):
    """-> (combined oracle result, {part: {(sid, soff): [pcov, ncov]}}, tested rows [(sid, soff, p1, n1, p2, n2, motif)])"""
    recs = [_as_dict(r) for r in reads]
    comb = P.pileup(recs, genome, min_mapq=min_mapq, min_pi=min_pi)
    thr = comb["thresholds"]
    motif = {(sid, soff): m for sid, soff, _p, _n, m in comb["loci"]}
    cov = {1: {}, 2: {}}
    for rec, hp in zip(recs, parts):
        if hp not in (1, 2):
            continue
        for sid, soff, prob, m in P.read_contribution(rec, genome, min_mapq, min_pi)[1]:
            e = cov[hp].setdefault((sid, soff), [0, 0])
            e[0 if prob >= thr[m] else 1] += 1
    rows = []
    for k in sorted(set(cov[1]) & set(cov[2])):
        (p1, n1), (p2, n2) = cov[1][k], cov[2][k]
        if p1 + n1 >= min_cov and p2 + n2 >= min_cov:
            rows.append((k[0], k[1], p1, n1, p2, n2, motif[k]))
    return comb, cov, rows


def _engine(genome, reads, batch=64, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(genome, **kw)
    for i, r in enumerate(reads):
        pu.add(r)
        if (i + 1) % batch == 0:
            pu.flush()
    pu.flush()
    pu.count(pu.resolve_thresholds(pu.histograms()))
    return pu


def _check_rows(pu, got, want, tol):
    assert len(got) == len(want)
    assert [(int(r["gpos"]), int(r["pcov1"]), int(r["ncov1"]), int(r["pcov2"]), int(r["ncov2"]), int(r["motif"])) for r in got] == \
           [(int(pu.offsets[sid] + soff), p1, n1, p2, n2, m) for sid, soff, p1, n1, p2, n2, m in want]
    w = np.array([r[2:6] for r in want], np.int64)
    assert (got["diff"].view(np.uint64) == _np_diff(*w.T).view(np.uint64)).all()
    exact = [fisher_exact(*r[2:6]) for r in want]
    worst = max(_rel_err(g, e) for g, e in zip(got["pvalue"], exact))
    print(f"{len(want)} tested loci, worst relative error of pvalue {worst:.3e}")
    assert worst <= tol
    return exact


def test_through_reads_python_api(P):
    genome, reads = _phased_reads()
    parts = [r.hp if r.hp in (1, 2) else 0 for r in reads]
    assert {r.hp for r in reads} == {None, 1, 2, 3}
    _comb, _cov, want = _expect(P, genome, reads, parts, min_cov=5)
    pu = _engine(genome, reads, partitions=True)
    got = pu.asm()                                            # min_cov defaults to 5
    exact = _check_rows(pu, got, want, 1e-9)                  # the bound of the small tables: totals <= 75 keep log n! < 256,
    assert max(sum(r[2:6]) for r in want) <= 75               # the same fp64 ulp (2.8e-14) as n <= 48 there
    assert len(want) >= 200
    assert (got["diff"] > 0).any() and (got["diff"] < 0).any()
    assert sum(e < Fraction(1, 100) for e in exact) >= 20 and sum(e > Fraction(1, 2) for e in exact) >= 20
    assert len({int(m) for m in got["motif"]}) == 3
    per_seq = [pu.asm(int(pu.offsets[s]), int(pu.offsets[s + 1])) for s in range(len(genome))]
    assert all(len(x) for x in per_seq) and (np.concatenate(per_seq) == got).all()
    # a tested locus is a locus of both hap files and of the combined output
    for part in (1, 2):
        hl = pu.loci(partition=part)
        j = np.searchsorted(hl["gpos"], got["gpos"])
        assert (hl["gpos"][j] == got["gpos"]).all()
        assert (hl["pcov"][j] == got[f"pcov{part}"]).all() and (hl["ncov"][j] == got[f"ncov{part}"]).all()
    _c, _v, want3 = _expect(P, genome, reads, parts, min_cov=3)
    got3 = pu.asm(min_cov=3)
    assert len(want3) > len(want)
    _check_rows(pu, got3, want3, 1e-9)
    pu.close()


# ---- CLI and the distributed driver -------------------------------------------------------------------------------------------
_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}


def _write_bam(path, genome, reads):
    """bamutil.aligned_to_bam with the read's hp as an HP:i field behind MM / ML / MN"""
    from bamutil import aux_B, aux_i, aux_Z, write_bgzf
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{len(s)}\n" for n, s in genome)
    parts = [b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(genome))]
    for n, s in genome:
        nm = n.encode() + b"\0"
        parts.append(struct.pack("<I", len(nm)) + nm + struct.pack("<I", len(s)))
    for r in reads:
        aux = aux_Z("RG", "rg0")
        if r.mm is not None:
            aux += aux_Z("MM", r.mm) + aux_B("ML", np.asarray(r.ml, np.uint8)) + aux_i("MN", r.l_qseq)
        if r.hp is not None:
            aux += b"HPi" + struct.pack("<i", r.hp)
        qn = r.name.encode() + b"\0"
        cig = r.cigar_u32()
        core = struct.pack("<iiBBHHHiiii", r.tid, r.pos, len(qn), r.mapq, 4680, len(cig), r.flag, r.l_qseq, -1, -1, 0)
        body = core + qn + cig.astype("<u4").tobytes() + bytes(r.seq4) + b"\xff" * r.l_qseq + aux
        parts.append(struct.pack("<I", len(body)) + body)
    write_bgzf(path, b"".join(parts))


def _cov_files(prefix):
    return {t + c: open(f"{prefix}.{t}{c}.cov.bed").read() for t in ("", "hap1.", "hap2.") for c in CTX}


def _asm_files(prefix):
    return {c: open(f"{prefix}.asm.{c}.bed").read() for c in CTX}


def _run_cli(args, ok=True):
    r = subprocess.run([CLI, "pileup", *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def test_cli_asm(P, tmp_path):
    from bamutil import write_fasta
    genome, reads = _phased_reads()
    parts = [r.hp if r.hp in (1, 2) else 0 for r in reads]
    bam, fa, prefix = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "out")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    r0 = _run_cli(["-H", fa, bam, prefix + "0"])
    r1 = _run_cli(["-H", "-A", "-a", "3", fa, bam, prefix + "1"])
    assert _cov_files(prefix + "0") == _cov_files(prefix + "1")
    assert not os.path.exists(prefix + "0.asm.CpG.bed")
    assert f"asm: min haplotype coverage 3 -> {prefix}1.asm.*" in r1.stderr and "asm:" not in r0.stderr
    got = _asm_files(prefix + "1")
    pu = _engine(genome, reads, partitions=True)
    assert got == pu.asm_bed(pu.asm(min_cov=3))
    _comb, _cov, want = _expect(P, genome, reads, parts, min_cov=3)
    assert len(want) >= 200
    seen = 0
    for m, c in enumerate(CTX):
        rows = [r for r in want if r[6] == m]
        lines = got[c].splitlines()
        assert len(lines) == len(rows) and rows
        for line, (sid, soff, p1, n1, p2, n2, _m) in zip(lines, rows):
            f = line.split("\t")
            assert len(f) == 9
            assert (f[0], int(f[1]), int(f[2]), [int(x) for x in f[5:]]) == (genome[sid][0], soff, soff + 1, [p1, n1, p2, n2])
            assert f[3] == "%g" % float(_np_diff(p1, n1, p2, n2))
            assert _rel_err(float(f[4]), fisher_exact(p1, n1, p2, n2)) <= 1e-5      # six printed digits
            seen += 1
    assert seen == len(want)
    # the default -a is 5
    _run_cli(["-H", "-A", fa, bam, prefix + "5"])
    assert _asm_files(prefix + "5") == pu.asm_bed(pu.asm())
    pu.close()
    # usage errors: decided while parsing, nothing written
    for k, args in enumerate((["-A"], ["-H", "-A", "-a", "0"], ["-H", "-a", "4"], ["-a", "4"])):
        bad = str(tmp_path / f"bad{k}")
        r = _run_cli([*args, fa, bam, bad], ok=False)
        assert "USAGE" in r.stderr
        assert not [f for f in os.listdir(tmp_path) if f.startswith(f"bad{k}")]
    assert "-H" in _run_cli(["-A", fa, bam, str(tmp_path / "bad")], ok=False).stderr.split("USAGE")[0]


def _dist_env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HM_FORCE_COLLECTIVES"):
        env.pop(k, None)
    env.update(kw)
    return env


def test_pileup_dist_asm(tmp_path):
    """python -m hifimeth_amd.pileup_dist -H -A: a world of one (plain, and with forced collectives) and two gloo ranks sharing
    the card -- all twelve files identical to the CLI's; the two ranks' border lies inside chr2 with tested loci on both sides"""
    from bamutil import write_fasta
    genome, reads = _phased_reads()
    bam, fa = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    _run_cli(["-H", "-A", "-a", "3", fa, bam, str(tmp_path / "cli")])
    want = (_cov_files(str(tmp_path / "cli")), _asm_files(str(tmp_path / "cli")))
    n_loci = sum(len(s) for _, s in genome)
    border = (n_loci + 1) // 2 - len(genome[0][1])           # chunk border of two ranks, as an offset into chr2
    assert 0 < border < len(genome[1][1])
    chr2 = [int(line.split("\t")[1]) for c in CTX for line in want[1][c].splitlines() if line.startswith(genome[1][0] + "\t")]
    assert min(chr2) < border <= max(chr2) and all(want[1][c] for c in CTX)
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", "-H", "-A", "-a", "3", "--slab", "7"]
    for name, env in (("one", _dist_env()),
                      ("rccl", _dist_env(HM_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29581"))):
        prefix = str(tmp_path / name)
        r = subprocess.run([*mod, fa, bam, prefix], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert (_cov_files(prefix), _asm_files(prefix)) == want, name
    prefix = str(tmp_path / "gloo")
    procs = [subprocess.Popen([*mod, "--backend", "gloo", fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                                            MASTER_PORT="29583"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert (_cov_files(prefix), _asm_files(prefix)) == want


def test_asm_abi_errors():
    import torch
    from hifimeth_amd.pileup import ASM_DTYPE, MethylationPileup
    genome = [("c", "ACGT" * 50)]
    t = [torch.zeros(200, dtype=torch.int32, device="cuda") for _ in range(5)]
    ptr = [ctypes.c_void_p(x.data_ptr()) for x in t]
    none = [None] * 5
    out = np.zeros(4, ASM_DTYPE)
    po = out.ctypes.data_as(ctypes.c_void_p)

    plain = MethylationPileup(genome)
    f = plain._L.hm_pileup_fetch_asm
    assert f(plain._h, *none, 0, 0, 200, 5, None, 0) == HM_ESTATE          # own planes asked for, partitions off
    assert b"partitions" in plain._L.hm_pileup_last_error(plain._h)
    assert f(plain._h, *ptr, 0, 0, 200, 5, None, 0) == 0                   # caller planes need no partitions
    assert f(plain._h, *ptr, 0, 0, 200, 0, None, 0) == HM_EINVAL           # min_cov < 1
    assert f(plain._h, *ptr, 0, 0, 200, -3, None, 0) == HM_EINVAL
    assert f(plain._h, *ptr, 0, 10, 9, 5, None, 0) == HM_EINVAL            # lo > hi
    assert f(plain._h, *ptr, 0, -1, 9, 5, None, 0) == HM_EINVAL
    for k in range(5):                                                     # a mix of NULL and non-NULL planes
        mix = list(ptr)
        mix[k] = None
        assert f(plain._h, *mix, 0, 0, 200, 5, None, 0) == HM_EINVAL
        one = list(none)
        one[k] = ptr[k]
        assert f(plain._h, *one, 0, 0, 200, 5, None, 0) == HM_EINVAL
    assert f(plain._h, *ptr, 0, 7, 7, 5, po, 4) == 0                       # empty range
    assert f(None, *ptr, 0, 0, 200, 5, None, 0) == HM_EINVAL
    plain.close()

    hp = MethylationPileup(genome, partitions=True)
    assert f(hp._h, *none, 0, 0, 200, 5, po, 4) == 0                       # nothing counted yet: no tested locus
    assert f(hp._h, *none, 0, 0, 200, 0, po, 4) == HM_EINVAL
    assert f(hp._h, *none, 0, 0, 201, 5, po, 4) == HM_EINVAL               # own planes end with the reference
    assert len(hp.asm()) == 0 and hp.asm().dtype == ASM_DTYPE
    hp.close()
