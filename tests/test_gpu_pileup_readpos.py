"""`pileup -P` / `pileup -I` on the device: the rows of hm_pileup_fetch_readpos equal those of tests/readpos_ref.py, integers and all
(exact equality of every row), on the hand-computed records of test_pileup_readpos_cpu.py and on the edge alignments of
tests/pileup_cases.py; trimming against the same input with the entries deleted by the test; then the command line against the
Python front end and pileup_dist byte for byte, and every output from before these options unchanged by them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pileup_cases as C
import readpos_ref as R
import test_pileup_readpos_cpu as K
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL, HM_ESTATE = -1, -5
THR = (128, 100, 60)
D_SMALL = 4           # L = 1 .. 7 reads of pileup_cases.boundaries() overlap both ends, L = 4 = D among them
_CACHE = {}


def _reads(name="all"):
    if name not in _CACHE:
        _CACHE[name] = C.everything() if name == "all" else C.CLASSES[name]()
    return _CACHE[name]


def _want(name, D, thr=THR, min_calls=1, **kw):
    key = (name, D, tuple(thr), min_calls, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = R.rows([C.as_dict(r) for r in _reads(name)], C.genome(), D, thr, min_calls=min_calls, **kw)
    return _CACHE[key]


def _engine(genome, reads, batch=None, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(genome, **kw)
    for i, r in enumerate(reads):
        pu.add(r)
        if batch and (i + 1) % batch == 0:
            pu.flush()
    pu.flush()
    return pu


def _tuples(rows):
    assert not rows["reserved"].any()
    return [tuple(int(r[k]) for k in ("motif", "end", "dist", "n_m", "n_u", "sum_ml")) for r in rows]


def _count_and_check(pu, thr=THR):
    """count, fetch every row, and the two invariants: the rows hold every projected record once, and their methylated calls are
    the combined pcov plane"""
    n_recs = pu.num_records()
    pu.count(list(thr))
    rows = pu.readpos(min_calls=0)
    assert len(rows) == 3 * (2 * pu.profile + 1)
    assert int(rows["n_m"].sum() + rows["n_u"].sum()) == n_recs
    loci = pu.loci()
    assert int(rows["n_m"].sum()) == int(loci["pcov"].astype(np.int64).sum())
    return _tuples(rows)


def _known():
    """the dict records of test_pileup_readpos_cpu.py as MethylationPileup.add() takes them"""
    from hifimeth_amd.synth import AlignedRead
    return [AlignedRead("k%d" % i, d["flag"], d["tid"], d["pos"], d["mapq"], d["cigar"], d["seq"], d["mm"], np.array(d["ml"], np.uint8))
            for i, d in enumerate(K.READS)]


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def test_known_answer():
    """the three hand-computed records: a read shorter than 2 D with its middle base called (the tie), both strands, a reverse CpG
    whose G is the last stored base, a CHH call recorded at the read's G, d3 = D exactly"""
    pu = _engine(K.REF, _known(), profile=4)
    assert _count_and_check(pu) == R.rows(K.READS, K.REF, 4, THR, min_calls=0)
    assert _tuples(pu.readpos()) == K.WANT
    from hifimeth_amd.pileup import readpos_tsv
    assert readpos_tsv(pu.readpos()) == R.tsv_text(K.WANT)
    pu.close()
    for D in (1, 8, 2048):
        pu = _engine(K.REF, _known(), profile=D)
        assert [t for t in _count_and_check(pu) if t[3] + t[4]] == R.rows(K.READS, K.REF, D, THR), D
        pu.close()


@pytest.mark.parametrize("D", [D_SMALL, 30, 2048])
def test_rows_equal_the_restatement(D):
    """every class of pileup_cases in one engine: every CIGAR op, soft clips at both ends (p counts the clipped bases), insertions and
    deletions before called sites, both strands with C+m on every C and G-m on every G (all record kinds), reads of 1 .. 7 bases,
    secondary and supplementary records, foreign tag dialects"""
    reads = _reads()
    want = _want("all", D, min_calls=0)
    assert {1, D_SMALL, 7} <= {r.l_qseq for r in reads} and any(r.flag & 0x100 for r in reads) and any(r.flag & 16 for r in reads)
    assert any(r.cigar and r.cigar[0][0] == "S" and r.cigar[-1][0] == "S" for r in reads)
    kinds = {(t[0], t[1]) for t in want if t[3] + t[4]}
    # every context has 5' and 3' records, and interior ones unless D reaches past the middle of the longest read (600 bases)
    assert kinds == {(m, e) for m in range(3) for e in range(3 if D < 300 else 2)}
    pu = _engine(C.genome(), reads, profile=D)
    assert _count_and_check(pu) == want
    pu.close()


def test_filters_and_secondary():
    """a record failing -q or -f is absent, a secondary record is present as a record of its own"""
    reads = _reads()
    plain = _want("all", 30)
    want = _want("all", 30, min_mapq=20, min_pi=97.5)
    assert want != plain
    for batch in (None, 7):
        pu = _engine(C.genome(), reads, batch=batch, profile=30, min_mapq=20, min_pi=97.5)
        assert [t for t in _count_and_check(pu) if t[3] + t[4]] == want, batch
        pu.close()
    primary = R.rows([C.as_dict(r) for r in reads if not r.flag & 0x900], C.genome(), 30, THR)
    assert primary != plain                                                   # the secondary records are in the table


def test_many_short_reads_in_one_batch():
    """3 600 alignments of 1 .. 70 columns in one batch and in batches of 500: about fifty 1 024-column tiles, each flushing its
    interior rows behind the other tiles' atomics on the end rows; ten copies of a record add up tenfold"""
    base = _reads("tiny_crowd")
    reads = base * 10
    want = [(m, e, d, 10 * a, 10 * b, 10 * s) for m, e, d, a, b, s in _want("tiny_crowd", 8, min_calls=0)]
    assert sum(sum(n for op, n in r.cigar if op in "M=X") for r in reads) > 40 * 1024
    assert sum(t[3] + t[4] for t in want if t[1] == 2) > 2000 and sum(t[3] + t[4] for t in want if t[1] != 2) > 2000
    for batch in (None, 500):
        pu = _engine(C.genome(), reads, batch=batch, profile=8)
        assert _count_and_check(pu) == want, batch
        pu.close()


def test_two_cycles_accumulate_under_the_last_threshold():
    reads = _reads()
    half = len(reads) // 2
    _CACHE["first"] = reads[:half]
    pu = _engine(C.genome(), reads[:half], profile=30)
    first = (3, 250, 128)
    assert _count_and_check(pu, first) == _want("first", 30, thr=first, min_calls=0)
    for r in reads[half:]:
        pu.add(r)
    pu.flush()
    n_recs = pu.num_records()
    pu.count(list(THR))
    rows = pu.readpos(min_calls=0)
    assert _tuples(rows) == _want("all", 30, min_calls=0)
    assert n_recs < int(rows["n_m"].sum() + rows["n_u"].sum())                # the table holds both cycles
    pu.close()


def test_min_calls_cap_and_null():
    from hifimeth_amd.pileup import READPOS_DTYPE
    reads = _reads()
    every = _want("all", 30, min_calls=0)
    pu = _engine(C.genome(), reads, profile=30)
    pu.count(list(THR))
    top = max(t[3] + t[4] for t in every)
    assert top > 50 and len(every) == 3 * 61
    for m in (0, 1, 2, 50, top, top + 1):
        exp = [t for t in every if t[3] + t[4] >= m]
        assert _tuples(pu.readpos(min_calls=m)) == exp and (len(exp) == 0) == (m == top + 1), m
        assert m < 2 or len(exp) < len([t for t in every if t[3] + t[4]])     # 2 and up drop rows
    want = [t for t in every if t[3] + t[4]]
    L, h = pu._L, pu._h
    assert L.hm_pileup_fetch_readpos(h, 1, None, 0) == len(want)                                   # count only
    buf = np.zeros(len(want), READPOS_DTYPE)
    assert L.hm_pileup_fetch_readpos(h, 1, buf.ctypes.data_as(ctypes.c_void_p), len(want) - 1) == len(want)
    assert not buf.view(np.uint8).any()                                                            # over cap: nothing written
    assert L.hm_pileup_fetch_readpos(h, 1, None, len(want)) == len(want)                           # no out: nothing written
    assert L.hm_pileup_fetch_readpos(h, 1, buf.ctypes.data_as(ctypes.c_void_p), len(want)) == len(want)
    assert _tuples(buf) == want
    assert L.hm_pileup_fetch_readpos(h, -1, None, 0) == HM_EINVAL
    pu.close()


def test_tables_of_two_engines_add_up():
    """hm_pileup_add_readpos: the second engine's table plus the first's is the table of all records"""
    reads = _reads()
    half = len(reads) // 2
    a = _engine(C.genome(), reads[:half], profile=30)
    b = _engine(C.genome(), reads[half:], profile=30)
    ha = a.readpos_histograms()
    assert ha.shape == (3, 61, 256) and int(ha.sum()) == a.num_records()
    b.add_readpos(ha)
    b.count(list(THR))
    assert _tuples(b.readpos(min_calls=0)) == _want("all", 30, min_calls=0)
    assert b._L.hm_pileup_add_readpos(b._h, ha.ctypes.data_as(ctypes.c_void_p), ha.size - 1) == HM_EINVAL
    a.close()
    b.close()


# ---- trimming ----------------------------------------------------------------------------------------------------------------------
def _submit_entries(pu, read, mods, order):
    """hm_pileup_submit_read with the entries given as they are"""
    if not len(mods):
        return 0
    seq4 = np.ascontiguousarray(read.seq4, np.uint8)
    cig = np.ascontiguousarray(read.cigar_u32(), np.uint32)
    return pu._check(pu._L.hm_pileup_submit_read(pu._h, order, read.flag, read.tid, read.pos, read.mapq, len(read.seq), seq4.ctypes.data_as(ctypes.c_void_p),
                                                 len(cig), cig.ctypes.data_as(ctypes.c_void_p), len(mods), mods.ctypes.data_as(ctypes.c_void_p)))


def _state(pu, thr=THR):
    """what trimming must leave as the deleted input leaves it: threshold histograms, the planes' rows, the -M rows, the table"""
    bins = pu.histograms().copy()
    n = pu.num_records()
    pu.count(list(thr))
    rows = pu.readpos(min_calls=0)
    assert int(rows["n_m"].sum() + rows["n_u"].sum()) == n
    return bins.tobytes(), pu.loci().tobytes(), pu.bedmethyl(min_valid=0).tobytes(), _tuples(rows)


def _trim_case(genome, reads, dicts, D, trim, batch=None):
    from hifimeth_amd.pileup import MethylationPileup
    cut = _engine(genome, reads, batch=batch, profile=D, bedmethyl=True, trim=trim)
    got = _state(cut)
    cut.close()
    ref = MethylationPileup(genome, profile=D, bedmethyl=True)
    for i, (r, d) in enumerate(zip(reads, dicts)):
        if not r.flag & 4:
            _submit_entries(ref, r, R.surviving_entries(d, *trim), i)
    ref.flush()
    want = _state(ref)
    ref.close()
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3], trim
    assert got[3] == R.rows(dicts, genome, D, THR, min_calls=0, trim=trim), trim
    return got


@pytest.mark.parametrize("trim", [(0, 0), (1, 1), (2, 2), (0, 2), (3, 3), (4, 3), (3, 4), (20, 0), (0, 1 << 22)])
def test_trim_known_answer(trim):
    """n5 and n3 exactly on a called position (it stays) and one past it (it goes), n5 + n3 = L and beyond: the hand-computed rows"""
    got = _trim_case(K.REF, _known(), K.READS, 4, trim)
    assert [t for t in got[3] if t[3] + t[4]] == R.rows(K.READS, K.REF, 4, THR, trim=trim)
    if trim == (4, 3):
        assert [t for t in got[3] if t[3] + t[4]] == [K.WANT[4], K.WANT[6]]


@pytest.mark.parametrize("trim", [(3, 0), (0, 5), (7, 7), (64, 1), (1000, 1000)])
def test_trim_equals_deleted_entries(trim):
    """the edge alignments, every C and G of which carries an entry, so that every n5 and n3 lies on a called position of some read
    and one past one of another; reads of 1 .. 7 bases lose every entry at 7:7; with the -M counters next to it, where a trimmed call
    is an Nnocall"""
    reads = _reads()
    dicts = [C.as_dict(r) for r in reads]
    plain = _CACHE.setdefault("plain_state", _trim_case(C.genome(), reads, dicts, 30, (0, 0)))
    got = _trim_case(C.genome(), reads, dicts, 30, trim, batch=50)
    assert got[0] != plain[0] and got[1] != plain[1] and got[2] != plain[2] and got[3] != plain[3]
    if trim == (1000, 1000):
        assert not any(t[3] + t[4] for t in got[3]) and not np.frombuffer(got[0], np.uint64).any()


def test_trim_of_calls_equals_trim_of_mods():
    """the same records once with their MM / ML entries and once as calls (hm_pileup_submit_read_calls): PMod and PCall entries
    share the predicate"""
    from hifimeth_amd.caller import CALL_DTYPE
    from hifimeth_amd.pileup import MethylationPileup
    reads = [r for name in ("cigar_zoo", "boundaries", "tiny_crowd", "identity_ties") for r in _reads(name)]
    trim = (3, 5)
    outs = []
    for form in ("mods", "calls", "deleted"):
        pu = MethylationPileup(C.genome(), profile=8, bedmethyl=True, trim=(0, 0) if form == "deleted" else trim)
        for i, r in enumerate(reads):
            d = C.as_dict(r)
            if form == "mods":
                pu.add(r, order=i)
            elif form == "deleted":
                _submit_entries(pu, r, R.surviving_entries(d, *trim), i)
            else:
                ent = sorted((strand, q, prob) for q, strand, ub, code, prob in R.entries(d))
                assert all(code == "m" for *_x, code, _p in R.entries(d))
                calls = np.zeros(len(ent), CALL_DTYPE)
                for k, (strand, q, prob) in enumerate(ent):
                    calls[k]["qoff"], calls[k]["strand"], calls[k]["scaled_prob"] = q, strand, prob
                pu.add_called(r, calls, order=i)
        pu.flush()
        outs.append(_state(pu))
        pu.close()
    assert outs[0] == outs[1] == outs[2] and any(t[3] + t[4] for t in outs[0][3])


# ---- the off path and the options --------------------------------------------------------------------------------------------------
def test_off_path_and_option_range():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import MethylationPileup
    L = lib()
    reads = _reads()
    off = _engine(C.genome(), reads)                                       # profile 0, trim 0:0
    off.count(list(THR))
    assert L.hm_pileup_fetch_readpos(off._h, 0, None, 0) == HM_ESTATE
    assert L.hm_pileup_readpos_histograms(off._h, None, 0) == HM_ESTATE
    for k in (b"profile", b"trim5", b"trim3"):
        assert L.hm_pileup_set_option(off._h, k, 4.0) == HM_ESTATE, k      # after the reference
    on = _engine(C.genome(), reads, profile=30)
    assert L.hm_pileup_fetch_readpos(on._h, 0, None, 0) == HM_ESTATE       # before hm_pileup_count
    assert b"hm_pileup_count" in L.hm_pileup_last_error(on._h)
    on.count(list(THR))
    assert on.loci().tobytes() == off.loci().tobytes() and (on.histograms() == off.histograms()).all()
    assert on.bed(on.loci()) == off.bed(off.loci())
    on.close()
    off.close()
    only_trim = _engine(C.genome(), reads, trim=(2, 2))
    only_trim.count(list(THR))
    assert L.hm_pileup_fetch_readpos(only_trim._h, 0, None, 0) == HM_ESTATE
    only_trim.close()
    h = ctypes.c_void_p()
    assert L.hm_pileup_create(ctypes.byref(h), 0) == 0
    for v in (-1.0, 2049.0, 2.5, float("nan"), float("inf")):
        assert L.hm_pileup_set_option(h, b"profile", v) == HM_EINVAL, v
    for k in (b"trim5", b"trim3"):
        for v in (-1.0, 0.5, float("nan"), 2.0 ** 31):
            assert L.hm_pileup_set_option(h, k, v) == HM_EINVAL, (k, v)
        for v in (0.0, 1.0, 200.0, 2.0 ** 31 - 1):
            assert L.hm_pileup_set_option(h, k, v) == 0, (k, v)
    for v in (1.0, 1024.0, 2048.0, 0.0):
        assert L.hm_pileup_set_option(h, b"profile", v) == 0, v
    assert L.hm_pileup_fetch_readpos(h, 1, None, 0) == HM_ESTATE           # option off again, no reference
    L.hm_pileup_destroy(h)


# ---- the command line --------------------------------------------------------------------------------------------------------------
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


CLI_OPTS = ["-P", "30", "-y", "2", "-I", "3:5"]


@pytest.fixture(scope="module")
def on_disk(tmp_path_factory):
    from bamutil import aligned_to_bam, write_fasta
    d = tmp_path_factory.mktemp("readpos")
    reads = _reads()
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    aligned_to_bam(bam, C.genome(), reads)
    write_fasta(fa, C.genome())
    rc, err = _cli(["pileup", *CLI_OPTS, "-b", "20", fa, bam, str(d / "t")])
    assert rc == 0, err[-2000:]
    return reads, bam, fa, d


def test_cli_equals_the_restatement_and_python(on_disk):
    """`pileup -P 30 -y 2 -I 3:5` writes the restatement's text under the thresholds the run resolved, which is pu.readpos_tsv's; -I
    with one number trims both ends; without the options every file is what it was, with -P alone every other file too"""
    from hifimeth_amd.pileup import readpos_tsv
    reads, bam, fa, d = on_disk
    pu = _engine(C.genome(), reads, profile=30, trim=(3, 5))
    thr = pu.resolve_thresholds(pu.histograms())
    pu.count(thr)
    got = open(d / "t.readpos.tsv").read()
    assert got == readpos_tsv(pu.readpos(min_calls=2))
    assert got == R.tsv_text(R.rows([C.as_dict(r) for r in reads], C.genome(), 30, thr, min_calls=2, trim=(3, 5))) and got.count("\n") > 60
    every = readpos_tsv(pu.readpos(min_calls=0))
    cov = pu.bed(pu.loci())
    pu.close()
    assert {k: v.decode() for k, v in _files(str(d / "t")).items() if k.endswith("cov.bed")} == {k + ".cov.bed": v for k, v in cov.items()}
    rc, err = _cli(["pileup", "-P", "30", "-y", "0", "-I", "3:5", fa, bam, str(d / "z")])
    assert rc == 0, err[-2000:]
    assert open(d / "z.readpos.tsv").read() == every and every.count("\n") == 1 + 3 * 61 and "nan" in every
    for tag, args in (("p", []), ("P", ["-P", "30"]), ("I", ["-I", "4"]), ("I44", ["-I", "4:4"]), ("I00", ["-I", "0:0", "-P", "30"])):
        rc, err = _cli(["pileup", "-b", "20", *args, fa, bam, str(d / tag)])
        assert rc == 0, err[-2000:]
    plain, with_p, one, two, zero = (_files(str(d / t)) for t in ("p", "P", "I", "I44", "I00"))
    assert "readpos.tsv" not in plain and set(with_p) == set(plain) | {"readpos.tsv"} and plain["CpG.cov.bed"]
    assert all(with_p[n] == plain[n] for n in plain)                         # the cov.bed files without the new paths
    assert one == two and set(one) == set(plain) and one["CpG.cov.bed"] != plain["CpG.cov.bed"]
    assert zero == with_p
    many = ["-H", "-A", "-a", "1", "-B", "chr2", "-D", "-E", "2", "-M", "-L", "50", "-b", "20"]
    rc, err = _cli(["pileup", *many, "-I", "3:5", fa, bam, str(d / "m")])
    assert rc == 0, err[-2000:]
    rc, err = _cli(["pileup", *many, *CLI_OPTS, fa, bam, str(d / "mt")])
    assert rc == 0, err[-2000:]
    a, b = _files(str(d / "m")), _files(str(d / "mt"))
    assert set(b) == set(a) | {"readpos.tsv"} and all(b[n] == a[n] for n in a) and b["readpos.tsv"].decode() == got
    assert a["patterns.CpG.bed"] and a["bedmethyl.CpG.bed"] and a["linkage.CpG.tsv"] and a["domains.CpG.bed"]


def test_pileup_dist_world_of_one_equals_the_cli(on_disk):
    _reads_, bam, fa, d = on_disk
    prefix = str(d / "one")
    r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *CLI_OPTS, fa, bam, prefix], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=_dist_env())
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(prefix + ".readpos.tsv").read() == open(d / "t.readpos.tsv").read()
    assert _files(prefix)["CpG.cov.bed"] == _files(str(d / "t"))["CpG.cov.bed"]


def test_pileup_dist_two_ranks_equal_the_cli(on_disk):
    """two gloo ranks sharing the card, records dealt in slabs of 7: the three sums of a row add up over the ranks to the CLI's file"""
    _reads_, bam, fa, d = on_disk
    prefix = str(d / "gloo")
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", *CLI_OPTS, "--slab", "7", "--backend", "gloo"]
    procs = [subprocess.Popen([*mod, fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29611"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert open(prefix + ".readpos.tsv").read() == open(d / "t.readpos.tsv").read()
    assert _files(prefix)["CpG.cov.bed"] == _files(str(d / "t"))["CpG.cov.bed"]


from test_gpu_pileup_fused import data  # noqa: E402,F401  (the module-scoped fixture: genome, reads with kinetics, their calls)


def test_cli_fused_equals_call_then_pileup(data, tmp_path):  # noqa: F811
    """`call` then `pileup -P -I` against `pileup -K -P -I`, explicit -T: the calls enter through the same predicate and table"""
    from test_gpu_pileup_fused import _cli_input
    bam, fa = _cli_input(data, tmp_path)
    mod, two, one = str(tmp_path / "mod.bam"), str(tmp_path / "two"), str(tmp_path / "one")
    opts = ["-P", "300", "-I", "150:100"]
    for args in (["call", "-t", "4", "-T", "1", bam, mod], ["pileup", "-t", "4", *opts, fa, mod, two],
                 ["pileup", "-t", "4", "-K", "-T", "1", *opts, fa, bam, one]):
        rc, err = _cli(args)
        assert rc == 0, err[-2000:]
    got, want = _files(one), _files(two)
    assert set(got) == set(want) and all(got[n] == want[n] for n in want)
    text = want["readpos.tsv"].decode().splitlines()
    assert len(text) > 300 and not any(ln.split("\t")[1:3] == ["5p", "149"] for ln in text) and any(ln.split("\t")[1:3] == ["5p", "150"] for ln in text)
    assert not any(ln.split("\t")[1:3] == ["3p", "99"] for ln in text) and any(ln.split("\t")[1:3] == ["3p", "100"] for ln in text)
