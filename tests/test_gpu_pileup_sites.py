"""The per-locus binomial test (`pileup -B / -e`): control sums, the histogram of (motif, pcov, pcov + ncov) with its list of loci
beyond 255 reads, rows written by table lookup, the CLI and the distributed driver.

The device part has no arithmetic to tolerate: sums, bins, the big list and the rows' counts must equal the pure-Python
reference below exactly, and a row's pvalue / qvalue must be the bits of the table entry (hm_sites_table; its arithmetic is
checked against exact fractions in test_pileup_sites_cpu.py, which shares the reference functions of this file)."""
import ctypes
import os
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
HM_EINVAL = -1


# ---- the reference --------------------------------------------------------------------------------------------------------------
def binomial_tail_exact(k: int, n: int, e: float) -> Fraction:
    """P(X >= k), X ~ Binomial(n, e), for the exact value of the double e = a / b: the integer terms C(n, x) a^x (b - a)^(n - x),
    from x = n down (each from the one before by an exact division), over b^n"""
    a, b = Fraction(e).numerator, Fraction(e).denominator
    if k <= 0:
        return Fraction(1)
    if a == 0:
        return Fraction(0)
    term = total = a ** n
    for x in range(n, k, -1):                                 # term(x - 1) = term(x) * x (b - a) / ((n - x + 1) a)
        term = term * x * (b - a) // ((n - x + 1) * a)
        total += term
    return Fraction(total, b ** n)


def bh_by_sort(p: np.ndarray) -> np.ndarray:
    """textbook Benjamini-Hochberg, one p per locus: sort, p * m / rank, running minimum from the largest, capped at 1"""
    m = len(p)
    order = np.argsort(p, kind="stable")
    q = p[order] * float(m) / np.arange(1, m + 1, dtype=np.float64)
    q = np.minimum(np.minimum.accumulate(q[::-1])[::-1], 1.0)
    out = np.empty(m)
    out[order] = q
    return out


def counted(pcov, ncov):
    """loci that take part: both counters are counts, one is positive"""
    return (pcov >= 0) & (ncov >= 0) & ((pcov > 0) | (ncov > 0))


def ref_histogram(pcov, ncov, key, lo, hi, plane_base=0):
    """-> (bins [3, 256, 256] uint64, big loci as (gpos, pcov, ncov, motif) rows) of planes[lo, hi)"""
    p, n, ky = (np.asarray(x[lo:hi], np.int64) for x in (pcov, ncov, key))
    motif = np.minimum(ky & 3, 2)
    sel = counted(p, n)
    small = sel & (p + n < 256)
    bins = np.zeros((3, 256, 256), np.uint64)
    np.add.at(bins, (motif[small], (p + n)[small], p[small]), 1)
    b = np.nonzero(sel & (p + n >= 256))[0]
    return bins, np.stack([b + lo + plane_base, p[b], n[b], motif[b]], axis=1) if len(b) else np.zeros((0, 4), np.int64)


def ref_sums(pcov, ncov, key, lo, hi):
    p, n, ky = (np.asarray(x[lo:hi], np.int64) for x in (pcov, ncov, key))
    motif = np.minimum(ky & 3, 2)
    sel = counted(p, n)
    return np.array([p[sel & (motif == c)].sum() for c in range(3)] + [n[sel & (motif == c)].sum() for c in range(3)], np.uint64)


# ---- planes filled by hand ------------------------------------------------------------------------------------------------------
N_LOCI = 20480                                               # five blocks of 4 096 loci
SEQS = (("chrA", 9000), ("chrB", 6480), ("ctl", 5000))
DEAD = (18000, 19000)                                        # an all-uncovered range
NEGATIVE = 4099                                              # the locus with a negative counter


def _crafted():
    rng = np.random.default_rng(20)
    pcov, ncov = np.zeros(N_LOCI, np.int64), np.zeros(N_LOCI, np.int64)
    motif = rng.integers(0, 3, N_LOCI)
    # >= 10 000 loci on the one triple (CHH, 3, 30), spread over the first four blocks
    dense = rng.choice(16000, 10500, replace=False)
    pcov[dense], ncov[dense], motif[dense] = 3, 27, 2
    rest = np.setdiff1d(np.arange(N_LOCI), dense)
    rest = rest[(rest < DEAD[0]) | (rest >= DEAD[1])]
    pick = rng.choice(rest, 7000, replace=False)
    tot = rng.choice([1, 63, 64, 255, 256, 257, 70000, 30, 12, 100], len(pick))
    k = (rng.random(len(pick)) * (tot + 1)).astype(np.int64)
    k[:50], k[50:100] = 0, tot[50:100]
    pcov[pick], ncov[pick] = k, tot - k
    for i, t in zip((1, 4095, 4096, 4097, 8192, N_LOCI - 1), (256, 70000, 63, 257, 64, 255)):   # block edges
        pcov[i], ncov[i] = t // 3, t - t // 3
    pcov[NEGATIVE], ncov[NEGATIVE] = -1, 40
    order = rng.integers(0, 1 << 20, N_LOCI)
    key = (order << 2) | motif
    key[pick[100:110]] |= 3                                  # low bits 3: counted as CHH, like the BED writers do
    return pcov.astype(np.int32), ncov.astype(np.int32), key.astype(np.int32)


@pytest.fixture(scope="module")
def crafted():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    host = _crafted()
    pu = MethylationPileup([(n, "ACGT" * (L // 4)) for n, L in SEQS])
    assert pu.n_loci == N_LOCI
    dev = [torch.from_numpy(x.copy()).cuda() for x in host]
    yield pu, host, dev
    pu.close()


RANGES = ((0, 0), (1, 4097), (4095, 8193), DEAD, (0, N_LOCI), (7, 7), (12288, 20480))
BIG_SHIFTS = (0, (1 << 31) - 8192, (1 << 32) - 8192)         # plane_base of the whole crafted planes: 0, or locus 8192 lies on 2^31 / 2^32


def _big_rows(big):
    return np.stack([big["gpos"], big["pcov"], big["ncov"], big["motif"]], axis=1).astype(np.int64) if len(big) else np.zeros((0, 4), np.int64)


def test_crafted_planes_hold_the_cases():
    pcov, ncov, key = (x.astype(np.int64) for x in _crafted())
    tot, sel = pcov + ncov, counted(pcov, ncov)
    assert {1, 63, 64, 255, 256, 257, 70000} <= set(tot[sel].tolist())
    assert set((np.minimum(key & 3, 2))[sel].tolist()) == {0, 1, 2} and ((key & 3) == 3)[sel].any()
    dense = sel & (pcov == 3) & (tot == 30) & ((key & 3) == 2)
    assert dense.sum() >= 10000 and sum(dense[b * 4096:(b + 1) * 4096].sum() > 1000 for b in range(5)) >= 3
    assert pcov[NEGATIVE] < 0 and not sel[NEGATIVE] and not sel[DEAD[0]:DEAD[1]].any()
    assert 17000 <= sel.sum() and (sel & (tot >= 256)).sum() > 1000


def test_histogram_and_big_list(crafted):
    pu, host, dev = crafted
    for lo, hi in RANGES:
        want_bins, want_big = ref_histogram(*host, lo, hi)
        bins, big = pu.site_histogram(lo, hi, planes=dev)
        assert (bins == want_bins).all(), (lo, hi)
        assert (_big_rows(big) == want_big).all() and len(big) == len(want_big) and (big["reserved"] == 0).all(), (lo, hi)
    full, _ = pu.site_histogram(planes=dev)
    assert full[2, 30, 3] >= 10000 and full[:, 64:, :].sum() > 0 and full.sum() + len(_) == counted(host[0], host[1]).sum()
    # a rank's chunk: planes that start at locus `base`; the bins add into what the caller holds
    # `shift` is what locus 0 of the crafted planes is called: beyond 0 it puts locus 8192 on 2^31 / 2^32, inside the chunk's range
    base, lo, hi = 5000, 123, 9000
    for shift in BIG_SHIFTS:
        acc = np.full((3, 256, 256), 5, np.uint64)
        bins, big = pu.site_histogram(lo, hi, planes=[t[base:] for t in dev], plane_base=shift + base, bins=acc)
        want_bins, want_big = ref_histogram(*host, base + lo, base + hi, plane_base=shift)
        assert bins is acc and (acc == want_bins + 5).all() and (_big_rows(big) == want_big).all() and len(want_big) > 100
        assert shift == 0 or (want_big[:, 0] < shift + 8192).sum() > 100 < (want_big[:, 0] >= shift + 8192).sum()


def test_cap_overflow_leaves_everything_untouched(crafted):
    from hifimeth_amd.pileup import LOCUS_DTYPE
    pu, host, dev = crafted
    _bins, want_big = ref_histogram(*host, 0, N_LOCI)
    ptrs = [ctypes.c_void_p(t.data_ptr()) for t in dev]
    bins = np.full(3 * 256 * 256, 7, np.uint64)
    big = np.zeros(len(want_big), LOCUS_DTYPE)
    big["gpos"] = -7
    f = pu._L.hm_pileup_site_histogram
    for cap in (0, 1, len(want_big) - 1):
        assert f(pu._h, *ptrs, 0, 0, N_LOCI, bins.ctypes.data_as(ctypes.c_void_p), big.ctypes.data_as(ctypes.c_void_p), cap) == len(want_big)
        assert (bins == 7).all() and (big["gpos"] == -7).all() and (big["pcov"] == 0).all()
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, bins.ctypes.data_as(ctypes.c_void_p), None, 1 << 20) == len(want_big)   # no list to write to
    assert (bins == 7).all()
    assert f(pu._h, *ptrs, 0, 0, N_LOCI, bins.ctypes.data_as(ctypes.c_void_p), big.ctypes.data_as(ctypes.c_void_p), len(big)) == len(big)
    assert (bins.reshape(3, 256, 256) == _bins + 7).all() and (_big_rows(big) == want_big).all()
    assert f(pu._h, *ptrs, 0, 9, 8, bins.ctypes.data_as(ctypes.c_void_p), None, 0) == HM_EINVAL
    assert f(pu._h, *ptrs, 0, 0, 8, None, None, 0) == HM_EINVAL


def test_control_sums(crafted):
    pu, host, dev = crafted
    for lo, hi in ((4100, 9000), (0, N_LOCI), (15480, N_LOCI), DEAD, (33, 33)):     # the first starts inside a block
        assert (pu.control_sums(lo, hi, planes=dev) == ref_sums(*host, lo, hi)).all(), (lo, hi)
    assert ref_sums(*host, 4100, 9000).min() > 0
    base = 3000
    assert (pu.control_sums(100, 9000, planes=[t[base:] for t in dev]) == ref_sums(*host, base + 100, base + 9000)).all()


@pytest.mark.parametrize("rates", [(0.02, 0.05, 0.013), (0.02, float("nan"), 0.013)])
def test_rows_by_table_lookup(crafted, rates):
    from hifimeth_amd.pileup import rates_from_sums, sites_table
    pu, host, dev = crafted
    pcov, ncov, key = (x.astype(np.int64) for x in host)
    bins, big = pu.site_histogram(planes=dev)
    table = sites_table(rates, bins, big)
    tested = np.array([not np.isnan(r) for r in rates])
    assert table.ctx_mask == sum(1 << c for c in range(3) if tested[c])
    motif = np.minimum(key & 3, 2)
    big_at = {int(g): i for i, g in enumerate(big["gpos"])}

    def check(rows, lo, hi, base=0):
        sel = np.nonzero(counted(pcov[lo:hi], ncov[lo:hi]) & tested[motif[lo:hi]])[0] + lo
        assert len(rows) == len(sel) and (rows["gpos"] == sel).all()
        assert (rows["pcov"] == pcov[sel]).all() and (rows["ncov"] == ncov[sel]).all() and (rows["motif"] == motif[sel]).all()
        assert (rows["reserved"] == 0).all()
        tot = pcov[sel] + ncov[sel]
        small = tot < 256
        wp, wq = np.empty(len(sel)), np.empty(len(sel))
        wp[small] = table.ptab[motif[sel][small], tot[small], pcov[sel][small]]
        wq[small] = table.qtab[motif[sel][small], tot[small], pcov[sel][small]]
        at = [big_at[int(g)] for g in sel[~small]]
        wp[~small], wq[~small] = table.big_p[at], table.big_q[at]
        assert (rows["pvalue"].view(np.uint64) == wp.view(np.uint64)).all() and (rows["qvalue"].view(np.uint64) == wq.view(np.uint64)).all()
        assert not np.isnan(rows["pvalue"]).any() and not np.isnan(rows["qvalue"]).any()
        assert ((rows["pvalue"] >= DBL_MIN) & (rows["pvalue"] <= 1) & (rows["qvalue"] >= rows["pvalue"]) & (rows["qvalue"] <= 1)).all()
        return len(sel)

    for lo, hi in RANGES:
        n = check(pu.sites(table, lo, hi, planes=dev), lo, hi)
        assert (n == 0) == (lo == hi or (lo, hi) == DEAD)
    assert NEGATIVE not in pu.sites(table, 4096, 4200, planes=dev)["gpos"]
    base, lo, hi = 5000, 123, 9000
    check(pu.sites(table, lo, hi, planes=[t[base:] for t in dev], plane_base=base), base + lo, base + hi)
    # the job's loci called shift + i: the rows' gpos and the binary search by gpos in the big list (more than 1000 entries, on both
    # sides of 2^31 / 2^32) must give the rows above, moved
    from hifimeth_amd.pileup import SitesTable
    for shift in BIG_SHIFTS[1:]:
        moved_big = big.copy()
        moved_big["gpos"] += shift
        _bins, got_big = pu.site_histogram(planes=dev, plane_base=shift)
        assert got_big.tobytes() == moved_big.tobytes()
        B = shift + 8192
        assert (moved_big["gpos"] < B).sum() > 100 and (moved_big["gpos"] >= B).sum() > 100
        moved = SitesTable(table.rates, table.ptab, table.qtab, moved_big, table.big_p, table.big_q, table.m)
        for (lo, hi), start in [(r, 0) for r in RANGES] + [((123, 9000), 5000)]:
            want = pu.sites(table, lo, hi, planes=[t[start:] for t in dev], plane_base=start)
            want["gpos"] += shift
            got = pu.sites(moved, lo, hi, planes=[t[start:] for t in dev], plane_base=shift + start)
            assert got.tobytes() == want.tobytes(), (shift, lo, hi)
    # cap below the count: the count comes back, nothing is written; a list that lacks a big locus gives NaN there
    from hifimeth_amd.pileup import SITE_DTYPE
    out = np.zeros(4, SITE_DTYPE)
    out["gpos"] = -7
    vp = ctypes.c_void_p
    args = (*[vp(t.data_ptr()) for t in dev], 0, 0, 100, table.ctx_mask, *(x.ctypes.data_as(vp) for x in (table.ptab, table.qtab)))
    f = pu._L.hm_pileup_fetch_sites
    n100 = f(pu._h, *args, None, None, None, 0, None, 0)
    assert n100 > 4 and f(pu._h, *args, None, None, None, 0, out.ctypes.data_as(vp), 4) == n100 and (out["gpos"] == -7).all()
    out = np.zeros(n100, SITE_DTYPE)
    assert f(pu._h, *args, None, None, None, 0, out.ctypes.data_as(vp), n100) == n100
    is_big = out["pcov"].astype(np.int64) + out["ncov"] >= 256
    assert is_big.any() and np.isnan(out["pvalue"][is_big]).all() and not np.isnan(out["pvalue"][~is_big]).any()
    assert rates_from_sums(pu.control_sums(15480, N_LOCI, planes=dev))[0] > 0


# ---- through reads: the CLI, the Python mirror, the distributed driver --------------------------------------------------------
CONTROL = "chr1"


@pytest.fixture(scope="module")
def aligned(tmp_path_factory):
    """the phased reads of the -A tests (three sequences, 300 reads) as a mod-BAM; chr1, the shortest, serves as the control"""
    from bamutil import write_fasta
    from test_gpu_pileup_asm import _phased_reads, _write_bam
    d = tmp_path_factory.mktemp("sites")
    genome, reads = _phased_reads()
    bam, fa = str(d / "mod.bam"), str(d / "ref.fa")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    return genome, reads, bam, fa, d


def _files(prefix, names):
    return {n: open(f"{prefix}.{n}", "rb").read() for n in names}


COV = [f"{c}.cov.bed" for c in CTX]
HAP = [f"hap{p}.{c}.cov.bed" for p in (1, 2) for c in CTX] + [f"asm.{c}.bed" for c in CTX]
SITES = [f"sites.{c}.bed" for c in CTX] + ["sites.rates.tsv"]


def _run_cli(args):
    r = subprocess.run([CLI, "pileup", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _mirror(genome, reads, control=None, rates=None):
    """the Python mirror's text of the four sites files"""
    from hifimeth_amd.pileup import MethylationPileup, rates_from_sums, sites_rates_tsv, sites_table
    pu = MethylationPileup(genome)
    for r in reads:
        pu.add(r)
    pu.flush()
    pu.count(pu.resolve_thresholds(pu.histograms()))
    sums = np.zeros(6, np.uint64)
    if control is not None:
        sid = pu.names.index(control)
        sums = pu.control_sums(int(pu.offsets[sid]), int(pu.offsets[sid + 1]))
        rates = rates_from_sums(sums)
    table = sites_table(rates, *pu.site_histogram())
    text = pu.sites_bed(pu.sites(table))
    cov = pu.bed(pu.loci())
    pu.close()
    out = {f"sites.{c}.bed": text[c].encode() for c in CTX}
    out["sites.rates.tsv"] = sites_rates_tsv(sums, rates, table.m).encode()
    return out, cov, rates


def test_cli_sites(aligned):
    genome, reads, bam, fa, d = aligned
    p0, p1, p2, p3 = (str(d / f"cli{k}") for k in range(4))
    e0 = _run_cli(["-H", "-A", "-a", "3", fa, bam, p0])
    e1 = _run_cli(["-H", "-A", "-a", "3", "-B", CONTROL, fa, bam, p1])
    assert _files(p0, COV + HAP) == _files(p1, COV + HAP)                      # the twelve files do not notice -B
    assert not [f for f in os.listdir(d) if f.startswith("cli0.sites")] and "sites:" not in e0 and "sites:" in e1
    got = _files(p1, SITES)
    want, cov, rates = _mirror(genome, reads, control=CONTROL)
    assert got == want
    assert all(0 < r < 1 for r in rates) and all(got[n].count(b"\n") >= 100 for n in SITES[:3])
    for c in CTX:                                                                 # the cov.bed row, byte for byte, then two columns
        rows, base = got[f"sites.{c}.bed"].decode().splitlines(), cov[c].splitlines()
        assert len(rows) == len(base) and all(r.startswith(b + "\t") and r[len(b):].count("\t") == 2 for r, b in zip(rows, base))
    tsv = [line.split("\t") for line in got["sites.rates.tsv"].decode().splitlines()]
    assert [t[0] for t in tsv] == list(CTX) and [int(t[4]) for t in tsv] == [len(cov[c].splitlines()) for c in CTX]
    # the printed rates replayed with -e: the same rows, and counts of 0 in the rates file
    _run_cli(["-e", ",".join(t[3] for t in tsv), fa, bam, p2])
    again = _files(p2, SITES)
    assert all(again[n] == got[n] for n in SITES[:3])
    assert again["sites.rates.tsv"] == "".join(f"{t[0]}\t0\t0\t{t[3]}\t{t[4]}\n" for t in tsv).encode()
    assert _files(p2, COV) == _files(p0, COV)
    # a context that is not tested keeps an empty file; -q and -f pass through
    e3 = _run_cli(["-q", "5", "-f", "80", "-e", f"{tsv[0][3]},nan,0", fa, bam, p3])
    f3 = _files(p3, SITES)
    assert f3["sites.CHG.bed"] == b"" and f3["sites.CpG.bed"] and f3["sites.CHH.bed"] and e3.count("WARNING: CHG is not tested") == 1
    assert f3["sites.rates.tsv"].decode().splitlines()[1].split("\t")[3] == "nan"
    pv = {line.split("\t")[6] for line in f3["sites.CHH.bed"].decode().splitlines() if int(line.split("\t")[4]) > 0}
    assert pv == {"2.22507e-308"}                                                 # rate 0 and a methylated read: DBL_MIN
    # an unknown control sequence: an error after the FASTA is read, nothing written
    r = subprocess.run([CLI, "pileup", "-B", "chrNone", fa, bam, str(d / "bad")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "chrNone" in r.stderr and "Load 3 sequences" in r.stderr
    assert not [f for f in os.listdir(d) if f.startswith("bad")]


def _dist_env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HM_FORCE_COLLECTIVES"):
        env.pop(k, None)
    env.update(kw)
    return env


def test_pileup_dist_sites(aligned):
    """python -m hifimeth_amd.pileup_dist -H -A -B: a world of one and two gloo ranks sharing the card write the CLI's sixteen
    files; the ranks' border lies inside chr2, so the control sequence (chr1) and the loci are split over both"""
    genome, _reads, bam, fa, d = aligned
    _run_cli(["-H", "-A", "-a", "3", "-B", CONTROL, fa, bam, str(d / "ref")])
    want = _files(str(d / "ref"), COV + HAP + SITES)
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", "-H", "-A", "-a", "3", "-B", CONTROL, "--slab", "7"]
    r = subprocess.run([*mod, fa, bam, str(d / "one")], capture_output=True, text=True, env=_dist_env(), cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _files(str(d / "one"), COV + HAP + SITES) == want
    procs = [subprocess.Popen([*mod, "--backend", "gloo", fa, bam, str(d / "gloo")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29601"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert _files(str(d / "gloo"), COV + HAP + SITES) == want
    # -e on two ranks: the rates file carries no counts
    rates = ",".join(line.split("\t")[3] for line in want["sites.rates.tsv"].decode().splitlines())
    r = subprocess.run([*mod[:3], "-e", rates, fa, bam, str(d / "given")], capture_output=True, text=True, env=_dist_env(), cwd=ROOT,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert all(_files(str(d / "given"), SITES[:3])[n] == want[n] for n in SITES[:3])
    r = subprocess.run([*mod[:3], "-B", "chrNone", fa, bam, str(d / "none")], capture_output=True, text=True, env=_dist_env(), cwd=ROOT,
                       timeout=300)
    assert r.returncode == 1 and "chrNone" in r.stderr and not [f for f in os.listdir(d) if f.startswith("none")]


from test_gpu_pileup_fused import data  # noqa: E402,F401  (the fused tests' fixture: kinetics reads and their calls)


def test_cli_fused_sites(data, tmp_path):  # noqa: F811
    """`pileup -K -B` on the kinetics BAM of the fused tests: the cov files do not notice -B, every sites row is its cov.bed row
    plus two columns, and the rates file holds the control sequence's column sums"""
    from test_gpu_pileup_fused import _cli_input
    bam, fa = _cli_input(data, tmp_path)
    plain, sites = str(tmp_path / "plain"), str(tmp_path / "sites")
    _run_cli(["-t", "4", "-K", "-T", "1", fa, bam, plain])
    _run_cli(["-t", "4", "-K", "-T", "1", "-B", "chr2", fa, bam, sites])
    cov = _files(sites, COV)
    assert cov == _files(plain, COV)
    got = _files(sites, SITES)
    tsv = [line.split("\t") for line in got["sites.rates.tsv"].decode().splitlines()]
    for c, t in zip(CTX, tsv):
        base = cov[f"{c}.cov.bed"].decode().splitlines()
        ctl = [b.split("\t") for b in base if b.startswith("chr2\t")]
        assert t[0] == c and int(t[1]) == sum(int(x[4]) for x in ctl) and int(t[2]) == sum(int(x[5]) for x in ctl) and int(t[4]) == len(base)
        rows = got[f"sites.{c}.bed"].decode().splitlines()
        if t[3] == "nan":
            assert not rows and not ctl
            continue
        assert float(t[3]) == int(t[1]) / (int(t[1]) + int(t[2]))
        assert len(rows) == len(base) and all(r.startswith(b + "\t") and r[len(b):].count("\t") == 2 for r, b in zip(rows, base))
    assert got["sites.CpG.bed"].count(b"\n") >= 100
