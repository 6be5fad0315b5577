"""`pileup -M` on the device: the rows of hm_pileup_fetch_bedmethyl equal those of the textbook restatement (tests/bedmethyl_ref.py),
integers and all, on the hand-built inputs of tests/bedmethyl_cases.py (test_pileup_bedmethyl_cpu.py asserts that each of them
holds the rule it is named for); then the CLI against the Python front end and the fused path, byte for byte, and every file from
before this option unchanged by it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bedmethyl_cases as K
import bedmethyl_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL, HM_ESTATE = -1, -5
_WANT = {}


def _want(name, genome, reads, **kw):
    """the restatement's rows, computed once per argument set and shared"""
    key = (name, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))
    if key not in _WANT:
        _WANT[key] = R.rows([K.as_dict(r) for r in reads], genome, **kw)
    return _WANT[key]


def _engine(genome, reads, batch=None, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(genome, bedmethyl=True, **kw)
    for i, r in enumerate(reads):
        pu.add(r)
        if batch and (i + 1) % batch == 0:
            pu.flush()
    pu.flush()
    return pu


def _tuples(rows):
    assert not rows["reserved"].any()
    return [tuple(int(r[f]) for f in ("gpos", "n_mod", "n_canon", "n_nocall", "n_diff", "n_delete")) for r in rows]


@pytest.mark.parametrize("thr", [K.THR, 0, 255])
def test_rows_equal_the_restatement(thr):
    """every case of bedmethyl_cases.reads() in one engine: both strands, an ML byte equal to the threshold, a dropped call, mismatch
    at C and at G, insertion between C and G, D over the G, over the C, over both and over three CpGs, N over a CpG and over its G,
    = / X / M as one run, alignments that end on the C (with and without more behind) and begin on the G, the first and the last
    CpG of the job, C | G across two sequences, soft clips, secondary and unmapped records, a record without entries, CpGs on both
    sides of the 1024-column tile edge, a reference CGG under a reverse read"""
    genome, reads = K.genome(), K.reads()
    want = _want("all", genome, reads, thr=thr, min_valid=0)
    pu = _engine(genome, reads)
    pu.count([thr, 128, 128])
    got = _tuples(pu.bedmethyl(min_valid=0))
    assert got == want
    by = {r[0]: r for r in got}
    off2, off3 = len(genome[0][1]), len(genome[0][1]) + len(genome[1][1])
    assert 0 in by and off3 + 498 in by and off2 - 1 not in by and off2 + 150 in by
    assert by[104][4] >= 10 and by[104][5] >= 4 and by[110][3] >= 2 and by[1023][3] == 1 and by[1030][3] == 1 and by[447][4] == 1
    assert all(by[off3 + g][5] == 2 for g in K.CHR3[:4])
    if thr == 0:
        assert all(r[2] == 0 for r in got)
    if thr == 255:
        assert sum(r[1] for r in got) < sum(r[2] for r in got)
    assert pu.bedmethyl_bed(pu.bedmethyl(min_valid=0)) == R.bed_text(want, genome)
    pu.close()


def test_filters_batches_and_cycles():
    """-q and -f take a record out of every class; one batch, two batches and a flush per record before one count give the same
    rows; two run / count cycles accumulate"""
    genome, reads = K.genome(), K.reads()
    plain = _want("all", genome, reads, thr=K.THR, min_valid=0)
    want = _want("all", genome, reads, thr=K.THR, min_valid=0, min_mapq=20, min_pi=97.0)
    assert want != plain
    for batch in (None, len(reads) // 2, 1):
        pu = _engine(genome, reads, batch=batch, min_mapq=20, min_pi=97.0)
        pu.count([K.THR, 128, 128])
        assert _tuples(pu.bedmethyl(min_valid=0)) == want, batch
        pu.close()
    pu = _engine(genome, reads)
    pu.count([K.THR, 128, 128])
    for r in reads:
        pu.add(r)
    pu.flush()
    pu.count([K.THR, 128, 128])
    assert _tuples(pu.bedmethyl(min_valid=0)) == [(g, *(2 * x for x in n)) for g, *n in plain]
    pu.close()


def test_valid_calls_equal_the_cpg_records():
    """independently of the restatement: the members are the motif-0 records the projection left"""
    genome, reads = K.genome(), K.reads()
    pu = _engine(genome, reads)
    gpos, _prob, motif, _order = pu.records()
    assert (motif == 1).any()
    pu.count([K.THR, 128, 128])
    rows = pu.bedmethyl(min_valid=0)
    assert int(rows["n_mod"].sum() + rows["n_canon"].sum()) == int((motif == 0).sum()) > 0
    loci, counts = np.unique(gpos[motif == 0], return_counts=True)
    valid = rows[rows["n_mod"] + rows["n_canon"] > 0]
    assert np.array_equal(valid["gpos"], loci) and np.array_equal(valid["n_mod"] + valid["n_canon"], counts)
    pu.close()


def test_partitions():
    genome, reads = K.genome(), K.with_hp(K.reads())
    hps = [r.hp or 0 for r in reads]
    pu = _engine(genome, reads, partitions=True)
    pu.count([K.THR, 128, 128])
    got = [_tuples(pu.bedmethyl(min_valid=0, partition=s)) for s in range(3)]
    for s in range(3):
        assert got[s] == _want("hp", genome, reads, thr=K.THR, min_valid=0, part=s, hps=hps), s
    assert got[0] == _want("all", genome, K.reads(), thr=K.THR, min_valid=0)               # set 0 holds every read
    for s in (1, 2):                                                                       # set s holds exactly the HP s reads
        assert got[s] == _want("only%d" % s, genome, [r for r in reads if r.hp == s], thr=K.THR, min_valid=0)
    tot = lambda rows: sum(sum(r[1:]) for r in rows)
    assert tot(got[1]) + tot(got[2]) < tot(got[0]) and tot(got[1]) and tot(got[2])        # HP 0 reads are in set 0 only
    pu.close()


def test_min_valid_ranges_cap_and_errors():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import BEDMETHYL_DTYPE, MethylationPileup
    L = lib()
    genome, reads = K.genome(), K.reads()
    want = _want("all", genome, reads, thr=K.THR, min_valid=0)
    pu = _engine(genome, reads)
    h = pu._h
    assert L.hm_pileup_fetch_bedmethyl(h, 0, 0, 10, 1, None, 0) == HM_ESTATE             # before hm_pileup_count
    assert b"hm_pileup_count" in L.hm_pileup_last_error(h)
    pu.count([K.THR, 128, 128])
    nv = next(r[1] + r[2] for r in want if r[0] == 120)
    assert nv > 3 and any(r[1] + r[2] == 0 for r in want)
    for m in (0, 1, nv, nv + 1):
        exp = [r for r in want if r[1] + r[2] >= m]
        assert _tuples(pu.bedmethyl(min_valid=m)) == exp and (120 in {r[0] for r in exp}) == (m <= nv)
    for lo, hi in ((0, 1), (1, 101), (100, 101), (101, 1600), (1599, 1601), (1600, 2400), (104, 104), (2399, 2400), (2398, 2399)):
        assert _tuples(pu.bedmethyl(lo, hi, min_valid=0)) == [r for r in want if lo <= r[0] < hi], (lo, hi)
    assert L.hm_pileup_fetch_bedmethyl(h, 0, 0, pu.n_loci, 0, None, 0) == len(want)          # count only
    buf = np.zeros(len(want), BEDMETHYL_DTYPE)
    assert L.hm_pileup_fetch_bedmethyl(h, 0, 0, pu.n_loci, 0, buf.ctypes.data_as(ctypes.c_void_p), len(want) - 1) == len(want)
    assert not buf.view(np.uint8).any()                                                       # over cap: nothing written
    assert L.hm_pileup_fetch_bedmethyl(h, 0, 0, pu.n_loci, 0, buf.ctypes.data_as(ctypes.c_void_p), len(want)) == len(want)
    assert _tuples(buf) == want
    for part, lo, hi, mv, rc in ((1, 0, 10, 1, HM_ESTATE), (2, 0, 10, 1, HM_ESTATE), (3, 0, 10, 1, HM_EINVAL), (-1, 0, 10, 1, HM_EINVAL),
                                 (0, -1, 10, 1, HM_EINVAL), (0, 5, 4, 1, HM_EINVAL), (0, 0, 10, -1, HM_EINVAL)):
        assert L.hm_pileup_fetch_bedmethyl(h, part, lo, hi, mv, None, 0) == rc, (part, lo, hi, mv)
    assert L.hm_pileup_set_option(h, b"bedmethyl", 0.0) == HM_ESTATE                          # after the reference
    pu.close()
    off = MethylationPileup(genome)                                                           # the option is off
    assert L.hm_pileup_fetch_bedmethyl(off._h, 0, 0, 10, 1, None, 0) == HM_ESTATE
    off.close()
    hh = ctypes.c_void_p()
    assert L.hm_pileup_create(ctypes.byref(hh), 0) == 0
    for v in (2.0, -1.0, 0.5, float("nan")):
        assert L.hm_pileup_set_option(hh, b"bedmethyl", v) == HM_EINVAL, v
    for v in (1.0, 0.0):
        assert L.hm_pileup_set_option(hh, b"bedmethyl", v) == 0
    L.hm_pileup_destroy(hh)


def test_dense_reference_crosses_a_selection_block():
    """5000 reference CpGs (two 4096 blocks of ranks), a deletion over 1500 of them in one thread, range fetches off the block edges"""
    genome, reads = K.dense()
    want = _want("dense", genome, reads, thr=K.THR, min_valid=0)
    pu = _engine(genome, reads, batch=4)
    pu.count([K.THR, 128, 128])
    assert _tuples(pu.bedmethyl(min_valid=0)) == want and len(want) > 4096
    assert sum(r[5] for r in want) == 1500 and sum(r[3] for r in want) == 500
    for lo, hi in ((1001, 9001), (8191, 8193), (8192, 10000), (3, 8192)):
        assert _tuples(pu.bedmethyl(lo, hi, min_valid=2)) == [r for r in want if lo <= r[0] < hi and r[1] + r[2] >= 2], (lo, hi)
    pu.close()


def test_next_to_patterns_the_cpg_list_is_shared():
    """both options on one engine: each output equals its single-option run"""
    from hifimeth_amd.pileup import BEDMETHYL_DTYPE, MethylationPileup
    genome, reads = K.genome(), K.reads()
    single_p = MethylationPileup(genome, patterns=3)
    both = _engine(genome, reads, patterns=3)
    for r in reads:
        single_p.add(r)
    single_p.flush()
    for pu in (single_p, both):
        pu.count([K.THR, 128, 128])
    assert both.bedmethyl(min_valid=0).tobytes() == np.array(
        [r + (0,) for r in _want("all", genome, reads, thr=K.THR, min_valid=0)], BEDMETHYL_DTYPE).tobytes()
    pat = both.patterns(min_reads=1)
    assert len(pat) and pat.tobytes() == single_p.patterns(min_reads=1).tobytes()
    single_p.close()
    both.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _cli(args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    return r.returncode, r.stderr


def _files(prefix):
    d, b = os.path.dirname(prefix), os.path.basename(prefix) + "."
    return {n[len(b):]: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.startswith(b)}


def test_cli_equals_python_and_leaves_the_other_files_alone(tmp_path):
    """`pileup -M` writes pu.bedmethyl_bed's text, with -H per haplotype too; a run with -M next to -H -A -B -D -E writes every other
    file as the run without it"""
    from bamutil import write_fasta
    from test_gpu_pileup_asm import _write_bam
    genome, reads = K.genome(), K.with_hp(K.reads())
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    pu = _engine(genome, reads, partitions=True)
    pu.count(pu.resolve_thresholds(pu.histograms()))
    want = {v: [pu.bedmethyl_bed(pu.bedmethyl(min_valid=v, partition=s)) for s in range(3)] for v in (1, 0, 3)}
    pu.close()
    assert want[0][0].count("\n") > want[1][0].count("\n") > want[3][0].count("\n") >= 5 and want[1][1] and want[1][2]
    rc, err = _cli(["pileup", "-M", "-b", "20", fa, bam, str(tmp_path / "m")])
    assert rc == 0 and "bedmethyl" in err, err[-2000:]
    assert open(tmp_path / "m.bedmethyl.CpG.bed").read() == want[1][0]
    rc, err = _cli(["pileup", "-b", "20", fa, bam, str(tmp_path / "p")])
    assert rc == 0, err[-2000:]
    plain, with_m = _files(str(tmp_path / "p")), _files(str(tmp_path / "m"))
    assert set(with_m) == set(plain) | {"bedmethyl.CpG.bed"} and all(with_m[n] == plain[n] for n in plain) and plain["CpG.cov.bed"]
    for v in (0, 3):
        rc, err = _cli(["pileup", "-M", "-v", str(v), "-H", fa, bam, str(tmp_path / ("h%d" % v))])
        assert rc == 0, err[-2000:]
        got = _files(str(tmp_path / ("h%d" % v)))
        assert [got[n].decode() for n in ("bedmethyl.CpG.bed", "hap1.bedmethyl.CpG.bed", "hap2.bedmethyl.CpG.bed")] == want[v], v
    many = ["-H", "-A", "-a", "1", "-B", "chr2", "-D", "-E", "2", "-o", "1", "-b", "20"]
    rc, err = _cli(["pileup", *many, fa, bam, str(tmp_path / "a")])
    assert rc == 0, err[-2000:]
    rc, err = _cli(["pileup", *many, "-M", fa, bam, str(tmp_path / "am")])
    assert rc == 0, err[-2000:]
    a, b = _files(str(tmp_path / "a")), _files(str(tmp_path / "am"))
    new = {"bedmethyl.CpG.bed", "hap1.bedmethyl.CpG.bed", "hap2.bedmethyl.CpG.bed"}
    assert set(b) == set(a) | new and len(a) >= 16 and all(b[n] == a[n] for n in a)
    assert [b[n].decode() for n in sorted(new, key=lambda n: ("hap" in n, n))] == want[1] and a["patterns.CpG.bed"] and a["asm.CpG.bed"]


from test_gpu_pileup_fused import data  # noqa: E402,F401  (the module-scoped fixture: genome, reads with kinetics, their calls)


def test_cli_fused_equals_call_then_pileup(data, tmp_path):  # noqa: F811
    """`call` then `pileup -M` against `pileup -K -M`, explicit -T: the classes come from the same plane words"""
    from test_gpu_pileup_fused import _cli_input
    bam, fa = _cli_input(data, tmp_path)
    mod, two, one = str(tmp_path / "mod.bam"), str(tmp_path / "two"), str(tmp_path / "one")
    opts = ["-M", "-v", "0", "-H"]
    for args in (["call", "-t", "4", "-T", "1", bam, mod], ["pileup", "-t", "4", *opts, fa, mod, two],
                 ["pileup", "-t", "4", "-K", "-T", "1", *opts, fa, bam, one]):
        rc, err = _cli(args)
        assert rc == 0, err[-2000:]
    got, want = _files(one), _files(two)
    assert set(got) == set(want) and all(got[n] == want[n] for n in want)
    assert want["bedmethyl.CpG.bed"].count(b"\n") >= 50 and want["hap1.bedmethyl.CpG.bed"] and want["hap2.bedmethyl.CpG.bed"]
