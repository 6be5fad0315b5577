"""`pileup -E` on the device: the rows of hm_pileup_fetch_patterns equal those of the textbook restatement (tests/patterns_ref.py),
integers and all, on the hand-built inputs of tests/patterns_cases.py (test_pileup_patterns_cpu.py asserts that each of them holds
the condition it is named for); then the CLI against the Python front end and the fused path, byte for byte, and every file from
before this option unchanged by it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import patterns_cases as K
import patterns_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL, HM_ESTATE = -1, -5
_WANT = {}


def _want(name, genome, reads, k, **kw):
    key = (name, k, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = R.rows([K.as_dict(r) for r in reads], genome, k, **kw)
    return _WANT[key]


def _engine(genome, reads, k, span=150, batch=None, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(genome, patterns=k, pattern_span=span, **kw)
    for i, r in enumerate(reads):
        pu.add(r)
        if batch and (i + 1) % batch == 0:
            pu.flush()
    pu.flush()
    return pu


def _tuples(rows):
    return [(int(r["start"]), int(r["end"]), tuple(int(x) for x in r["counts"]), int(r["n"]), int(r["k"])) for r in rows]


@pytest.mark.parametrize("thr", [K.THR, 0, 255])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_rows_equal_the_restatement(k, thr):
    """every case of patterns_cases.reads() in one engine: both strands, a probability equal to the threshold, deletion, mismatch at
    C and at G, missing call, insertion, run break inside a later locus, reads ending mid-window, span 150 and 151, the first and
    the last CpG of the job, a sequence with fewer than k CpGs, C | G across two sequences, secondary and unmapped records, loci on
    both sides of the 1024-column tile edge under a run that straddles it"""
    genome, reads = K.genome(), K.reads()
    want = _want("all", genome, reads, k, thr=thr)
    pu = _engine(genome, reads, k)
    assert pu.num_pattern_records() > 0
    pu.count([thr, 128, 128])
    assert pu.num_pattern_records() == 0
    got = _tuples(pu.patterns(min_reads=1))
    assert got == want
    starts = {s for s, *_ in got}
    off2, off3 = len(genome[0][1]), len(genome[0][1]) + len(genome[1][1])
    assert 0 in starts and 1010 in starts and 1018 in starts and (300 in starts) == (k == 2) and 450 not in starts
    assert not any(off2 <= s < off3 for s in starts) and off3 + 50 in starts
    assert pu.patterns_bed(pu.patterns(min_reads=1)) == R.bed_text(want, genome)
    pu.close()


@pytest.mark.parametrize("k", [2, 4])
def test_filters_and_two_batches(k):
    """-q and -f take the records they take out of the counters out of the windows too; two hm_pileup_run batches (and a flush
    per record) before one count give the same rows"""
    genome, reads = K.genome(), K.reads()
    plain = _want("all", genome, reads, k, thr=K.THR)
    want = _want("all", genome, reads, k, thr=K.THR, min_mapq=20, min_pi=97.0)
    assert want != plain
    for batch in (None, len(reads) // 2, 1):
        pu = _engine(genome, reads, k, batch=batch, min_mapq=20, min_pi=97.0)
        pu.count([K.THR, 128, 128])
        assert _tuples(pu.patterns(min_reads=1)) == want, batch
        pu.close()


def test_span_option_min_reads_ranges_and_cap():
    from hifimeth_amd.pileup import PATTERN_DTYPE
    genome, reads = K.genome(), K.reads()
    for span in (149, 150, 151, 1, 65536):
        want = _want("all", genome, reads, 2, thr=K.THR, max_span=span)
        pu = _engine(genome, reads, 2, span=span)
        pu.count([K.THR, 128, 128])
        got = _tuples(pu.patterns(min_reads=1))
        assert got == want, span
        assert (300 in {s for s, *_ in got}) == (span >= 150) and (450 in {s for s, *_ in got}) == (span >= 151)
        if span != 150:
            pu.close()
            continue
        n = next(r[3] for r in want if r[0] == 100)                       # min_reads at n and n + 1
        assert n > 3
        for m in (n, n + 1):
            exp = [r for r in want if r[3] >= m]
            assert _tuples(pu.patterns(min_reads=m)) == exp and (100 in {r[0] for r in exp}) == (m == n)
        for lo, hi in ((0, 1), (1, 101), (100, 101), (101, 1600), (1599, 1601), (1600, 2400), (104, 104), (2399, 2400)):
            assert _tuples(pu.patterns(lo, hi, min_reads=1)) == [r for r in want if lo <= r[0] < hi], (lo, hi)
        L, h = pu._L, pu._h
        assert L.hm_pileup_fetch_patterns(h, 0, pu.n_loci, 1, None, 0) == len(want)          # count only
        buf = np.zeros(len(want), PATTERN_DTYPE)
        assert L.hm_pileup_fetch_patterns(h, 0, pu.n_loci, 1, buf.ctypes.data_as(ctypes.c_void_p), len(want) - 1) == len(want)
        assert not buf.view(np.uint8).any()                                                  # over cap: nothing written
        assert L.hm_pileup_fetch_patterns(h, 0, pu.n_loci, 1, buf.ctypes.data_as(ctypes.c_void_p), len(want)) == len(want)
        assert _tuples(buf) == want
        assert L.hm_pileup_fetch_patterns(h, 5, 4, 1, None, 0) == HM_EINVAL
        assert L.hm_pileup_fetch_patterns(h, -1, 4, 1, None, 0) == HM_EINVAL
        assert L.hm_pileup_fetch_patterns(h, 0, 4, 0, None, 0) == HM_EINVAL
        pu.close()


def test_crowd_on_one_window():
    """300 reads on the loci 100 .. 120: every one of them an atomic on the same 64 bytes of bins"""
    genome, reads = K.genome(), K.crowd(300)
    for k in (2, 4):
        want = _want("crowd", genome, reads, k, thr=K.THR)
        assert want[0][3] == 300
        pu = _engine(genome, reads, k)
        pu.count([K.THR, 128, 128])
        assert _tuples(pu.patterns(min_reads=300)) == [r for r in want if r[3] >= 300] and _tuples(pu.patterns(min_reads=1)) == want
        pu.close()


def test_dense_reference_more_records_than_one_grid_trip():
    """5000 reference CpGs (two 4096 blocks of ranks) and 279 860 window records: pattern_count_kernel's 1024 x 256 threads take
    more than one trip; range fetches that start and end off the block edges"""
    genome, reads = K.dense()
    want = _want("dense", genome, reads, 2, thr=K.THR, max_span=2)
    pu = _engine(genome, reads, 2, span=2, batch=70)
    assert pu.num_pattern_records() == 140 * 1999 > 1024 * 256
    pu.count([K.THR, 128, 128])
    got = pu.patterns(min_reads=1)
    assert _tuples(got) == want and len(want) > 4096
    for lo, hi in ((1001, 9001), (8191, 8193), (8192, 10000), (3, 8192)):
        assert _tuples(pu.patterns(lo, hi, min_reads=36)) == [r for r in want if lo <= r[0] < hi and r[3] >= 36], (lo, hi)
    pu.close()
    wide = _want("dense4", genome, reads[:8], 4, thr=K.THR, max_span=6)
    pu = _engine(genome, reads[:8], 4, span=6)
    pu.count([K.THR, 128, 128])
    assert _tuples(pu.patterns(min_reads=1)) == wide and wide
    pu.close()


def test_call_order_and_option_ranges():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import MethylationPileup
    L = lib()
    genome, reads = K.genome(), K.reads()
    off = MethylationPileup(genome)                                        # the option is off
    assert L.hm_pileup_fetch_patterns(off._h, 0, 10, 1, None, 0) == HM_ESTATE
    assert L.hm_pileup_set_option(off._h, b"patterns", 2.0) == HM_ESTATE  # after the reference
    assert L.hm_pileup_set_option(off._h, b"pattern_span", 100.0) == HM_ESTATE
    assert off.num_pattern_records() == 0
    off.close()
    h = ctypes.c_void_p()
    assert L.hm_pileup_create(ctypes.byref(h), 0) == 0
    for key, bad, good in ((b"patterns", (1.0, 5.0, -2.0, 2.5), (0.0, 2.0, 3.0, 4.0)),
                           (b"pattern_span", (0.0, 65537.0, -1.0, 10.5, float("nan")), (1.0, 150.0, 65536.0))):
        for v in bad:
            assert L.hm_pileup_set_option(h, key, v) == HM_EINVAL, (key, v)
        for v in good:
            assert L.hm_pileup_set_option(h, key, v) == 0, (key, v)
    L.hm_pileup_destroy(h)
    pu = _engine(genome, reads[:6], 3)
    assert L.hm_pileup_fetch_patterns(pu._h, 0, 10, 1, None, 0) == HM_ESTATE     # before hm_pileup_count
    assert b"hm_pileup_count" in L.hm_pileup_last_error(pu._h)
    pu.count([K.THR, 128, 128])
    assert L.hm_pileup_fetch_patterns(pu._h, 0, pu.n_loci, 1, None, 0) > 0
    pu.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _cli(args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    return r.returncode, r.stderr


def _files(prefix):
    d, b = os.path.dirname(prefix), os.path.basename(prefix) + "."
    return {n[len(b):]: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.startswith(b)}


def test_cli_equals_python_and_leaves_the_other_files_alone(tmp_path):
    """`pileup -E 4` writes pu.patterns_bed's text; a run with -E next to -H -A -B -D writes every other file as the run without it"""
    from bamutil import write_fasta
    from test_gpu_pileup_hp import _write_bam
    genome, reads = K.genome(), K.reads() + K.crowd(30)
    reads = sorted(reads, key=lambda r: (r.tid, r.pos))
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    _write_bam(bam, genome, reads, [[("i", (1, 2)[i % 2])] for i in range(len(reads))])
    write_fasta(fa, genome)
    pu = _engine(genome, reads, 4, span=120)
    pu.count(pu.resolve_thresholds(pu.histograms()))
    want = pu.patterns_bed(pu.patterns(min_reads=3))
    pu.close()
    assert want.count("\n") >= 3
    rc, err = _cli(["pileup", "-E", "4", "-w", "120", "-o", "3", "-b", "20", fa, bam, str(tmp_path / "e")])
    assert rc == 0, err[-2000:]
    assert open(tmp_path / "e.patterns.CpG.bed").read() == want
    rc, err = _cli(["pileup", "-b", "20", fa, bam, str(tmp_path / "p")])
    assert rc == 0, err[-2000:]
    plain, with_e = _files(str(tmp_path / "p")), _files(str(tmp_path / "e"))
    assert "patterns.CpG.bed" not in plain and set(with_e) == set(plain) | {"patterns.CpG.bed"}
    assert all(with_e[n] == plain[n] for n in plain) and plain["CpG.cov.bed"]
    many = ["-H", "-A", "-a", "1", "-B", "chr2", "-D", "-b", "20"]
    rc, err = _cli(["pileup", *many, fa, bam, str(tmp_path / "m")])
    assert rc == 0, err[-2000:]
    rc, err = _cli(["pileup", *many, "-E", "2", fa, bam, str(tmp_path / "me")])
    assert rc == 0, err[-2000:]
    a, b = _files(str(tmp_path / "m")), _files(str(tmp_path / "me"))
    assert set(b) == set(a) | {"patterns.CpG.bed"} and len(a) >= 15 and all(b[n] == a[n] for n in a)
    assert b["patterns.CpG.bed"] and a["asm.CpG.bed"] and a["domains.CpG.bed"] and a["sites.CpG.bed"]
    for args in (["-w", "100"], ["-o", "5"], ["-E", "5"], ["-E", "2", "-w", "0"], ["-E", "2", "-o", "0"], ["-E", "x"]):
        rc, err = _cli(["pileup", *args, fa, bam, str(tmp_path / "bad")])
        assert rc != 0 and "-E" in err, args


from test_gpu_pileup_fused import data  # noqa: E402,F401  (the module-scoped fixture: genome, reads with kinetics, their calls)


def test_cli_fused_equals_call_then_pileup(data, tmp_path):  # noqa: F811
    """`call` then `pileup -E` against `pileup -K -E`, explicit -T: the window records come from the same plane words"""
    from test_gpu_pileup_fused import _cli_input
    bam, fa = _cli_input(data, tmp_path)
    mod, two, one = str(tmp_path / "mod.bam"), str(tmp_path / "two"), str(tmp_path / "one")
    opts = ["-E", "3", "-w", "200", "-o", "1"]
    for args in (["call", "-t", "4", "-T", "1", bam, mod], ["pileup", "-t", "4", *opts, fa, mod, two],
                 ["pileup", "-t", "4", "-K", "-T", "1", *opts, fa, bam, one]):
        rc, err = _cli(args)
        assert rc == 0, err[-2000:]
    got, want = _files(one), _files(two)
    assert set(got) == set(want) and all(got[n] == want[n] for n in want)
    assert want["patterns.CpG.bed"].count(b"\n") >= 50
