"""`pileup -L` on the device: the rows of hm_pileup_fetch_linkage equal those of the textbook restatement (tests/linkage_ref.py),
integers and all, on the hand-built inputs of tests/patterns_cases.py and tests/linkage_cases.py in one engine
(test_pileup_linkage_cpu.py asserts that each of them holds the condition it is named for); then the CLI against the Python front
end, the fused path and pileup_dist, byte for byte, and every file from before this option unchanged by it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import linkage_cases as C
import linkage_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL, HM_ESTATE = -1, -5
_WANT = {}


def _want(name, reads, max_dist, **kw):
    key = (name, max_dist, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = R.rows([C.as_dict(r) for r in reads], C.genome(), max_dist, **kw)
    return _WANT[key]


def _engine(reads, max_dist, batch=None, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(C.genome(), linkage=max_dist, **kw)
    for i, r in enumerate(reads):
        pu.add(r)
        if batch and (i + 1) % batch == 0:
            pu.flush()
    pu.flush()
    return pu


def _tuples(rows):
    assert not rows["reserved"].any()
    return [tuple(int(r[k]) for k in ("dist", "n_uu", "n_um", "n_mu", "n_mm")) for r in rows]


@pytest.mark.parametrize("thr", [C.THR, 0, 255])
def test_rows_equal_the_restatement(thr):
    """every case of patterns_cases.reads() and linkage_cases.own_reads() in one engine at max_dist 400: both strands, neighbouring
    records and two alignments of one name that must not pair, a record with one member, pairs at max_dist and one beyond, across a
    D and an N, across the 1024-column tile edge and the selection's 4096-column block edge, equal ML bytes, ML bytes at and one
    below the threshold, deletions, mismatches, missing calls, secondary and unmapped records"""
    reads = C.reads()
    want = _want("all", reads, C.MAX_DIST, thr=thr)
    pu = _engine(reads, C.MAX_DIST)
    pu.count([thr, 128, 128])
    rows = pu.linkage(min_pairs=1)
    assert _tuples(rows) == want
    by_d = {r[0]: r[1:] for r in want}
    assert 2 in by_d and C.MAX_DIST in by_d and max(by_d) == C.MAX_DIST and len(want) > 30
    if thr == C.THR:
        assert all(sum(r[k] for r in want) > 0 for k in (1, 2, 3, 4))        # every class occurs
    elif thr == 0:
        assert all(r[1:4] == (0, 0, 0) for r in want)                        # nothing is unmethylated
    assert pu.linkage_tsv(rows) == R.tsv_text(want)
    pu.close()


def test_filters_and_batch_cuts():
    """-q and -f take the records they take out of the counters out of the pairs too; one batch, two, and a flush per record give
    the same table: a record's members never straddle a batch"""
    reads = C.reads()
    plain = _want("all", reads, C.MAX_DIST, thr=C.THR)
    want = _want("all", reads, C.MAX_DIST, thr=C.THR, min_mapq=20, min_pi=97.0)
    assert want != plain
    for batch in (None, len(reads) // 2, 1):
        pu = _engine(reads, C.MAX_DIST, batch=batch, min_mapq=20, min_pi=97.0)
        pu.count([C.THR, 128, 128])
        assert _tuples(pu.linkage()) == want, batch
        pu.close()


def test_two_cycles_accumulate_under_the_last_threshold():
    reads = C.reads()
    half = len(reads) // 2
    pu = _engine(reads[:half], C.MAX_DIST)
    pu.count([3, 128, 128])
    assert _tuples(pu.linkage()) == _want("first", reads[:half], C.MAX_DIST, thr=3)
    for r in reads[half:]:
        pu.add(r)
    pu.flush()
    pu.count([C.THR, 128, 128])
    assert _tuples(pu.linkage()) == _want("all", reads, C.MAX_DIST, thr=C.THR)
    pu.close()


@pytest.mark.parametrize("max_dist", [2, 2000, 16384])
def test_max_dist(max_dist):
    """the smallest reach (CGCG alone), one beyond every chromosome of the small cases, and the cap: big's 100 | 16484 and
    102 | 16486 are the last row, 100 | 16486 is no pair"""
    reads = C.reads()
    want = _want("all", reads, max_dist, thr=C.THR)
    pu = _engine(reads, max_dist)
    pu.count([C.THR, 128, 128])
    got = _tuples(pu.linkage())
    assert got == want and want[0][0] == 2
    if max_dist == 16384:
        assert want[-1][0] == 16384 and sum(want[-1][1:]) == 4
    every = pu.linkage(min_pairs=0)
    assert len(every) == max_dist - 1 and list(every["dist"]) == list(range(2, max_dist + 1))
    assert [t for t in _tuples(every) if sum(t[1:])] == want
    pu.close()


def test_min_pairs_cap_and_null():
    from hifimeth_amd.pileup import LINKAGE_DTYPE
    reads = C.reads()
    want = _want("all", reads, C.MAX_DIST, thr=C.THR)
    pu = _engine(reads, C.MAX_DIST)
    pu.count([C.THR, 128, 128])
    top = max(sum(r[1:]) for r in want)
    assert top > 3
    for m in (0, 1, 2, top, top + 1):
        exp = [r for r in _want("all", reads, C.MAX_DIST, thr=C.THR, min_pairs=0) if sum(r[1:]) >= m]
        assert _tuples(pu.linkage(min_pairs=m)) == exp and (len(exp) == 0) == (m == top + 1) and (m != 0 or len(exp) == C.MAX_DIST - 1), m
    L, h = pu._L, pu._h
    assert L.hm_pileup_fetch_linkage(h, 1, None, 0) == len(want)                                   # count only
    buf = np.zeros(len(want), LINKAGE_DTYPE)
    assert L.hm_pileup_fetch_linkage(h, 1, buf.ctypes.data_as(ctypes.c_void_p), len(want) - 1) == len(want)
    assert not buf.view(np.uint8).any()                                                            # over cap: nothing written
    assert L.hm_pileup_fetch_linkage(h, 1, None, len(want)) == len(want)                           # no out: nothing written
    assert L.hm_pileup_fetch_linkage(h, 1, buf.ctypes.data_as(ctypes.c_void_p), len(want)) == len(want)
    assert _tuples(buf) == want
    assert L.hm_pileup_fetch_linkage(h, -1, None, 0) == HM_EINVAL
    pu.close()


def test_crowd_on_one_read():
    """300 copies of one record: each of its ten pairs' three bins takes 300 atomics"""
    reads = C.crowd(300)
    want = _want("crowd", reads, C.MAX_DIST + 11, thr=C.THR)
    assert len(want) == 10 and all(sorted(r[1:]) == [0, 0, 0, 300] for r in want) and all(sum(r[k] for r in want) for k in (1, 3, 4))
    pu = _engine(reads, C.MAX_DIST + 11, batch=128)
    pu.count([C.THR, 128, 128])
    assert _tuples(pu.linkage(min_pairs=300)) == want and len(pu.linkage(min_pairs=301)) == 0
    pu.close()


def test_call_order_and_option_range():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import MethylationPileup
    L = lib()
    off = MethylationPileup(C.genome())                                    # the option is off
    off.add(C.reads()[0])
    off.flush()
    off.count([C.THR, 128, 128])
    assert L.hm_pileup_fetch_linkage(off._h, 1, None, 0) == HM_ESTATE
    assert L.hm_pileup_set_option(off._h, b"linkage", 100.0) == HM_ESTATE  # after the reference
    off.close()
    h = ctypes.c_void_p()
    assert L.hm_pileup_create(ctypes.byref(h), 0) == 0
    for v in (1.0, -2.0, 16385.0, 2.5, float("nan")):
        assert L.hm_pileup_set_option(h, b"linkage", v) == HM_EINVAL, v
    for v in (2.0, 2000.0, 16384.0, 0.0):
        assert L.hm_pileup_set_option(h, b"linkage", v) == 0, v
    assert L.hm_pileup_fetch_linkage(h, 1, None, 0) == HM_ESTATE          # option off again, no reference
    L.hm_pileup_destroy(h)
    pu = _engine(C.reads()[:6], 100)
    assert L.hm_pileup_fetch_linkage(pu._h, 1, None, 0) == HM_ESTATE      # before hm_pileup_count
    assert b"hm_pileup_count" in L.hm_pileup_last_error(pu._h)
    pu.count([C.THR, 128, 128])
    assert L.hm_pileup_fetch_linkage(pu._h, 1, None, 0) > 0
    pu.close()


def test_next_to_patterns_and_bedmethyl():
    """one engine with -E, -M and -L: each output is what the engine with that option alone gives"""
    from hifimeth_amd.pileup import MethylationPileup
    reads = C.reads()
    outs = []
    for kw in (dict(patterns=3, bedmethyl=True, linkage=C.MAX_DIST), dict(patterns=3), dict(bedmethyl=True), dict(linkage=C.MAX_DIST)):
        pu = MethylationPileup(C.genome(), **kw)
        for i, r in enumerate(reads):
            pu.add(r)
            if i % 25 == 24:
                pu.flush()
        pu.flush()
        pu.count([C.THR, 128, 128])
        outs.append((pu.loci().tobytes(), pu.patterns(min_reads=1).tobytes() if "patterns" in kw else None,
                     pu.bedmethyl(min_valid=0).tobytes() if "bedmethyl" in kw else None, _tuples(pu.linkage()) if "linkage" in kw else None))
        pu.close()
    both, pat, bm, lk = outs
    assert both[0] == pat[0] == bm[0] == lk[0] and both[1] == pat[1] and both[2] == bm[2]
    assert both[3] == lk[3] == _want("all", reads, C.MAX_DIST, thr=C.THR)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _cli(args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    return r.returncode, r.stderr


def _files(prefix):
    d, b = os.path.dirname(prefix), os.path.basename(prefix) + "."
    return {n[len(b):]: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.startswith(b)}


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
    d = tmp_path_factory.mktemp("linkage")
    reads = sorted(C.reads() + C.crowd(30), key=lambda r: (r.tid, r.pos))
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    _write_bam(bam, C.genome(), reads, [[("i", (1, 2)[i % 2])] for i in range(len(reads))])
    write_fasta(fa, C.genome())
    rc, err = _cli(["pileup", "-L", "2000", "-z", "2", "-b", "20", fa, bam, str(d / "l")])
    assert rc == 0, err[-2000:]
    return reads, bam, fa, d


def test_cli_equals_python_and_leaves_the_other_files_alone(on_disk):
    """`pileup -L 2000 -z 2` writes pu.linkage_tsv's text; a run with -L next to -H -A -B -D -E -M writes every other file as the
    run without it"""
    reads, bam, fa, d = on_disk
    pu = _engine(reads, 2000)
    pu.count(pu.resolve_thresholds(pu.histograms()))
    want = pu.linkage_tsv(pu.linkage(min_pairs=2))
    every = pu.linkage_tsv(pu.linkage(min_pairs=0))
    pu.close()
    assert want.count("\n") >= 30 and "nan" in want and every.count("\n") == 2000
    assert open(d / "l.linkage.CpG.tsv").read() == want
    rc, err = _cli(["pileup", "-L", "2000", "-z", "0", fa, bam, str(d / "z")])
    assert rc == 0, err[-2000:]
    assert open(d / "z.linkage.CpG.tsv").read() == every
    rc, err = _cli(["pileup", "-b", "20", fa, bam, str(d / "p")])
    assert rc == 0, err[-2000:]
    plain, with_l = _files(str(d / "p")), _files(str(d / "l"))
    assert "linkage.CpG.tsv" not in plain and set(with_l) == set(plain) | {"linkage.CpG.tsv"}
    assert all(with_l[n] == plain[n] for n in plain) and plain["CpG.cov.bed"]
    many = ["-H", "-A", "-a", "1", "-B", "chr2", "-D", "-E", "2", "-M", "-b", "20"]
    rc, err = _cli(["pileup", *many, fa, bam, str(d / "m")])
    assert rc == 0, err[-2000:]
    rc, err = _cli(["pileup", *many, "-L", "2000", "-z", "2", fa, bam, str(d / "ml")])
    assert rc == 0, err[-2000:]
    a, b = _files(str(d / "m")), _files(str(d / "ml"))
    assert set(b) == set(a) | {"linkage.CpG.tsv"} and len(a) >= 19 and all(b[n] == a[n] for n in a)
    assert b["linkage.CpG.tsv"].decode() == want and a["patterns.CpG.bed"] and a["bedmethyl.CpG.bed"] and a["domains.CpG.bed"]


def test_pileup_dist_equals_the_cli(on_disk):
    """python -m hifimeth_amd.pileup_dist -L on two gloo ranks sharing the card, records dealt in slabs of 7: the four counts per
    distance add up over the ranks to the CLI's file, byte for byte"""
    _reads, bam, fa, d = on_disk
    want = open(d / "l.linkage.CpG.tsv").read()
    prefix = str(d / "gloo")
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", "-L", "2000", "-z", "2", "--slab", "7", "--backend", "gloo"]
    procs = [subprocess.Popen([*mod, fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29607"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert open(prefix + ".linkage.CpG.tsv").read() == want
    assert _files(prefix)["CpG.cov.bed"] == _files(str(d / "l"))["CpG.cov.bed"]


from test_gpu_pileup_fused import data  # noqa: E402,F401  (the module-scoped fixture: genome, reads with kinetics, their calls)


def test_cli_fused_equals_call_then_pileup(data, tmp_path):  # noqa: F811
    """`call` then `pileup -L` against `pileup -K -L`, explicit -T: the member list comes from the same plane words"""
    from test_gpu_pileup_fused import _cli_input
    bam, fa = _cli_input(data, tmp_path)
    mod, two, one = str(tmp_path / "mod.bam"), str(tmp_path / "two"), str(tmp_path / "one")
    opts = ["-L", "300"]
    for args in (["call", "-t", "4", "-T", "1", bam, mod], ["pileup", "-t", "4", *opts, fa, mod, two],
                 ["pileup", "-t", "4", "-K", "-T", "1", *opts, fa, bam, one]):
        rc, err = _cli(args)
        assert rc == 0, err[-2000:]
    got, want = _files(one), _files(two)
    assert set(got) == set(want) and all(got[n] == want[n] for n in want)
    assert want["linkage.CpG.tsv"].count(b"\n") >= 50
