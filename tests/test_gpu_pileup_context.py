"""`pileup -S` on the GPU: hm_pileup_fetch_context against the restatement (tests/context_ref.py) on a synthetic genome with short
sequences, Ns and a range of several workgroups and strides, on both accumulation paths, on chunks, on counters that need 64 bits,
on real records, and through the front ends.  Every integer is compared by equality."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import context_ref as X
import pileup_cases as C
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL, HM_ESTATE = -1, -5
LDS, GLOBAL = 0, 1
_CACHE = {}


def _random_seq(rng, n, n_rate=0.004):
    return "".join(rng.choice(list("ACGTN"), n, p=[(1 - n_rate) / 4] * 4 + [n_rate]))


def _case():
    """the genome (sequences of 1, 2, 3, 5, 7, 9 and 300 bases, one of more loci than one stride of the kernel's grid, one of 2),
    its engine, host planes (as test_gpu_pileup_regions.py::_synthetic: random contexts under random order bits; the short sequences
    and the last bases covered for certain), the same on the device, and the expected table per (flank, min_cov)"""
    if "case" not in _CACHE:
        import torch
        from hifimeth_amd.pileup import MethylationPileup, context_geometry
        span = context_geometry()[0]
        stride = span * torch.cuda.get_device_properties(0).multi_processor_count
        assert stride <= 400000                                                   # the long sequence stays a few hundred thousand bases
        rng = np.random.default_rng(23)
        seqs = [_random_seq(rng, n) for n in (1, 2, 3, 5, 7, 9, 300)] + [_random_seq(rng, stride + 3 * span + 77), _random_seq(rng, 2)]
        n = sum(len(s) for s in seqs)
        on = rng.random(n) < 0.12
        on[:340] = on[-14:] = True
        pc = np.where(on, rng.integers(0, 6, n), 0).astype(np.int32)
        nc = np.where(on, rng.integers(0, 6, n), 0).astype(np.int32)
        pc[:30] |= 1
        pc[-14:] |= 1
        ky = ((rng.integers(0, 1 << 20, n) << 2) | rng.integers(0, 3, n)).astype(np.int32)
        host = (pc, nc, ky)
        pu = MethylationPileup([(f"s{i}", s) for i, s in enumerate(seqs)])
        _CACHE["case"] = dict(seqs=seqs, n=n, span=span, stride=stride, host=host, dev=_dev(host), pu=pu, want={})
    return _CACHE["case"]


def _dev(planes):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes)


def _want(flank, min_cov=1):
    k = _case()
    if (flank, min_cov) not in k["want"]:
        k["want"][flank, min_cov] = X.context_table(*k["host"], k["seqs"], flank, min_cov=min_cov)
        k["want"][flank, min_cov].setflags(write=False)
    return k["want"][flank, min_cov]


def _paths(flank):
    from hifimeth_amd.pileup import CONTEXT_PATH_AUTO, context_geometry
    return [CONTEXT_PATH_AUTO, GLOBAL] + ([LDS] if flank <= context_geometry()[2] else [])


@pytest.mark.parametrize("flank", [0, 1, 2, 3])
def test_against_the_restatement(flank):
    k = _case()
    want = _want(flank)
    assert want.shape == (3, 4 ** (3 + 2 * flank) + 1, 4)
    assert (want[:, -1, 0] > 0).all()                                             # `other` rows
    pc, nc, ky = k["host"]
    is_g = np.frombuffer("".join(k["seqs"]).encode(), np.uint8) == ord("G")
    from_g = X.context_table(np.where(is_g, pc, 0), np.where(is_g, nc, 0), ky, k["seqs"], flank)
    assert from_g[:, :-1, 0].sum() > 100 and (want[:, :-1, 0] >= from_g[:, :-1, 0]).all()   # rows from G-loci
    assert X.near_ends(pc, nc, k["seqs"], flank) == (True, True)
    assert k["n"] > k["stride"] + k["span"]                                       # several workgroups, more than one stride of the grid
    for c in range(3):                                                            # the invariant
        assert want[c, :, 0].sum() == ((pc.astype(np.int64) + nc >= 1) & ((ky & 3) == c)).sum()
    for path in _paths(flank):
        got = k["pu"].context(flank, planes=k["dev"], hi=k["n"], path=path)
        assert got.dtype == np.int64 and got.shape == want.shape and (got == want).all(), path


@pytest.mark.parametrize("flank", [0, 2])
def test_non_zero_base_and_unaligned_range(flank):
    k = _case()
    base, lo, hi = 317, k["span"] // 2 + 7, k["n"] - 317 - 5                       # the planes start inside the 300-base sequence
    part = tuple(p[base:] for p in k["host"])
    want = X.context_table(*part, k["seqs"], flank, base=base, lo=lo, hi=hi)
    assert want.any() and not (want == _want(flank)).all()
    for path in _paths(flank):
        got = k["pu"].context(flank, lo=lo, hi=hi, planes=tuple(t[base:] for t in k["dev"]), plane_base=base, path=path)
        assert (got == want).all(), path


@pytest.mark.parametrize("flank", [0, 1, 3])
def test_chunks_add_up(flank):
    k = _case()
    n, span, pu = k["n"], k["span"], k["pu"]
    off = np.cumsum([len(s) for s in k["seqs"]])
    whole = _want(flank)
    for cut in (1, span - 1, span, span + 1, int(off[6]) - 1, int(off[6]), int(off[6]) + 1):
        left = pu.context(flank, lo=0, hi=cut, planes=k["dev"])
        right = pu.context(flank, lo=0, hi=n - cut, planes=tuple(t[cut:] for t in k["dev"]), plane_base=cut)
        assert (left + right == whole).all(), cut
        assert (left == X.context_table(*k["host"], k["seqs"], flank, hi=cut)).all(), cut
        assert (right == X.context_table(*(p[cut:] for p in k["host"]), k["seqs"], flank, base=cut)).all(), cut
        assert (pu.context(flank, lo=cut, hi=n, planes=k["dev"]) == right).all(), cut


def test_second_pass_of_the_unrolled_loop():
    """a thread takes eight strides of the grid before it comes round again: a range of more than eight strides, sparsely covered"""
    import torch
    from hifimeth_amd.pileup import MethylationPileup, context_geometry
    span = context_geometry()[0]
    eight = 8 * span * torch.cuda.get_device_properties(0).multi_processor_count
    n = eight + 5 * span + 3
    rng = np.random.default_rng(29)
    seq = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, n, p=[0.2495] * 4 + [0.002])].tobytes().decode()
    on = rng.random(n) < 0.01
    on[-3 * span:] |= rng.random(3 * span) < 0.3
    pc, nc = (np.where(on, rng.integers(0, 6, n), 0).astype(np.int32) for _ in range(2))
    ky = rng.integers(0, 3, n).astype(np.int32)
    want = X.context_table(pc, nc, ky, [seq], 1)
    assert X.context_table(pc[eight:], nc[eight:], ky[eight:], [seq], 1, base=eight)[:, :-1].any()   # loci of the second pass
    pu = MethylationPileup([("long", seq)])
    dev = _dev((pc, nc, ky))
    for path in (LDS, GLOBAL):
        assert (pu.context(1, planes=dev, path=path) == want).all(), path
    pu.close()


def test_64_bit_counters():
    from hifimeth_amd.pileup import MethylationPileup
    big = 2 ** 31 - 1
    seq = "ACCGT" * 4                                                             # C at 1, 6, 11, 16: the same ACCGT at flank 1
    pc, nc, ky = (np.zeros(20, np.int32) for _ in range(3))
    for g in (1, 6, 11, 16):
        pc[g], nc[g], ky[g] = big, big, 1
    pc[2], ky[2] = big, 0                                                         # a CpG with no unmethylated read
    pu = MethylationPileup([("r", seq)])
    dev = _dev((pc, nc, ky))
    row = X.kmer_rows(5)["ACCGT"]
    for flank, paths in ((1, (LDS, GLOBAL)), (2, (GLOBAL,))):
        want = X.context_table(pc, nc, ky, [seq], flank)
        for path in paths:
            for min_cov in (1, 2 * big):                                          # cov = 2^32 - 2 does not wrap, and still counts
                got = pu.context(flank, min_cov=min_cov, planes=dev, path=path)
                if flank == 1:
                    assert got[1, row].tolist() == [4, 4 * big, 4 * big, 2000000] and 4 * big > 2 ** 32
                assert (got[1] == want[1]).all() and (min_cov > 1 or (got == want).all())
                assert got[0].any() == (min_cov == 1)
    assert not pu.context(0, min_cov=2 * big + 1, planes=dev).any()
    pu.close()


def test_min_cov_above_every_coverage_and_repeats():
    k = _case()
    assert not k["pu"].context(1, min_cov=11, planes=k["dev"], hi=k["n"]).any() and _want(1, 10).any()
    for flank in (0, 3):                                                          # the device table is zeroed by every call
        a = k["pu"].context(flank, min_cov=3, planes=k["dev"], hi=k["n"])
        b = k["pu"].context(flank, min_cov=3, planes=k["dev"], hi=k["n"])
        assert (a == b).all() and (a == _want(flank, 3)).all()
    assert (k["pu"].context(0, planes=k["dev"], hi=k["n"]) == _want(0)).all()       # and a smaller table after a larger one


# ---- real records --------------------------------------------------------------------------------------------------------------------
def _tagged_reads():
    if "reads" not in _CACHE:
        _CACHE["reads"] = [dataclasses.replace(r, hp=(None, 1, 2)[i % 3]) for i, r in enumerate(C.everything())]
    return _CACHE["reads"]


def _real():
    if "real" not in _CACHE:
        from hifimeth_amd.pileup import MethylationPileup
        pu = MethylationPileup(C.genome(), partitions=True)
        for r in _tagged_reads():
            pu.add(r)
        pu.flush()
        pu.count(pu.resolve_thresholds(pu.histograms()))
        _CACHE["real"] = pu
    return _CACHE["real"]


def _planes_from_loci(loci, n):
    pc, nc, ky = (np.zeros(n, np.int64) for _ in range(3))
    g = np.asarray(loci["gpos"], np.int64)
    pc[g], nc[g], ky[g] = loci["pcov"], loci["ncov"], loci["motif"]
    return pc, nc, ky


@pytest.mark.parametrize("part", [0, 1, 2])
def test_real_records_and_partitions(part):
    """own planes, and a partition's counts with the combined key"""
    pu = _real()
    seqs = [s.upper() for _, s in C.genome()]
    loci = pu.loci(partition=part)
    assert len(loci) > 50
    bed = pu.bed(loci)
    for flank in (0, 1, 3):
        for min_cov in (1, 2):
            want = X.context_table(*_planes_from_loci(loci, pu.n_loci), seqs, flank, min_cov=min_cov)
            got = pu.context(flank, min_cov, partition=part)
            assert (got == want).all() and want[:, :-1, 0].sum() > (20 if min_cov == 1 else 0)
            if min_cov == 1:
                assert [int(got[c, :, 0].sum()) for c in range(3)] == [bed[ctx].count("\n") for ctx in X.CTX]


# ---- the ABI's refusals ----------------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.caller import HifimethError
    from hifimeth_amd.pileup import MethylationPileup
    L = lib()
    out = np.zeros(4 * 3 * 65, np.int64)
    h = ctypes.c_void_p()
    assert L.hm_pileup_create(ctypes.byref(h), 0) == 0
    assert L.hm_pileup_fetch_context(h, None, None, None, 0, 0, 10, 1, 0, out.ctypes.data_as(ctypes.c_void_p), 195) == HM_ESTATE
    assert b"hm_pileup_set_reference" in L.hm_pileup_last_error(h)
    L.hm_pileup_destroy(h)
    k = _case()
    pu, n, dev = k["pu"], k["n"], k["dev"]
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in dev]
    o = out.ctypes.data_as(ctypes.c_void_p)
    assert L.hm_pileup_fetch_context(pu._h, *ptr, 0, 0, n, 1, 0, None, 0) == 195                 # the size, nothing written
    assert L.hm_pileup_fetch_context(pu._h, *ptr, 0, 0, n, 1, 0, o, 194) == 195 and not out.any()
    assert L.hm_pileup_fetch_context(pu._h, *ptr, 0, 0, n, 1, 0, o, 195) == 195 and out.any()
    for bad in ((ptr[0], ptr[1], None), (None, ptr[1], ptr[2]), (ptr[0], None, None)):           # a mix of NULL and non-NULL planes
        assert L.hm_pileup_fetch_context(pu._h, *bad, 0, 0, n, 1, 0, o, 195) == HM_EINVAL
    for bad in (dict(flank=-1), dict(flank=4), dict(min_cov=0), dict(lo=5, hi=4), dict(lo=-1), dict(hi=n + 1), dict(plane_base=1),
                dict(plane_base=-1, hi=n - 1), dict(flank=2, path=LDS), dict(path=7)):
        with pytest.raises(HifimethError):
            pu.context(**{"planes": dev, "hi": n, **bad})
    assert (pu.context(0, planes=dev, hi=n) == _want(0)).all()                    # the engine still answers
    assert not pu.context(0, planes=dev, lo=7, hi=7).any()                        # an empty range
    planeless = MethylationPileup([("s", "ACGT")], planes=None)
    assert planeless.context(0).shape == (3, 65, 4)                               # own planes, nothing counted yet
    planeless.close()


# ---- the front ends --------------------------------------------------------------------------------------------------------------------
def _cli(args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    return r.returncode, r.stderr


def _files(prefix):
    d, b = os.path.dirname(prefix), os.path.basename(prefix) + "."
    return {n[len(b):]: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.startswith(b)}


def _ours(files):
    return {k: v for k, v in files.items() if "context." in k}


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
    d = tmp_path_factory.mktemp("context")
    reads = _tagged_reads()
    bam, fa = str(d / "in.bam"), str(d / "ref.fa")
    _write_bam(bam, C.genome(), reads, [[("C", r.hp)] if r.hp else [] for r in reads])
    write_fasta(fa, C.genome())
    rc, err = _cli(["pileup", "-S", "1", "-O", "2", "-b", "20", fa, bam, str(d / "t")])
    assert rc == 0, err[-2000:]
    return bam, fa, d


def test_cli_equals_the_binding(on_disk):
    from hifimeth_amd.pileup import context_tsv
    bam, fa, d = on_disk
    pu = _real()
    got = _ours(_files(str(d / "t")))
    assert sorted(got) == ["context.CHG.tsv", "context.CHH.tsv", "context.CpG.tsv"]
    want = context_tsv(pu.context(1, 2), 1)
    assert sum(text.count("\n") for text in want.values()) > 9
    for ctx, text in want.items():
        assert got[f"context.{ctx}.tsv"].decode() == text
    rc, err = _cli(["pileup", "-H", "-S", "0", "-b", "20", fa, bam, str(d / "h")])
    assert rc == 0, err[-2000:]
    got = _ours(_files(str(d / "h")))
    assert len(got) == 9
    for part, tag in enumerate(("", "hap1.", "hap2.")):
        for ctx, text in context_tsv(pu.context(0, partition=part), 0).items():
            assert got[f"{tag}context.{ctx}.tsv"].decode() == text
    assert got["context.CpG.tsv"] != got["hap1.context.CpG.tsv"]
    assert _files(str(d / "h"))["CpG.cov.bed"] == _files(str(d / "t"))["CpG.cov.bed"]


def test_pileup_dist_two_ranks_equal_the_cli(on_disk):
    """two gloo ranks sharing the card: each takes the table of its half of the planes, the sum is the CLI's files"""
    bam, fa, d = on_disk
    prefix = str(d / "gloo")
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", "-S", "1", "-O", "2", "--slab", "7", "--backend", "gloo"]
    procs = [subprocess.Popen([*mod, fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29623"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert len(_ours(_files(prefix))) == 3 and _ours(_files(prefix)) == _ours(_files(str(d / "t")))
    assert _files(prefix)["CpG.cov.bed"] == _files(str(d / "t"))["CpG.cov.bed"]


def test_usage_errors_are_reported(tmp_path):
    for args, what in ((["-O", "2"], "ERROR: -O needs -S"), (["-S", "4"], "ERROR: -S must"), (["-S", "1", "-O", "0"], "ERROR: -S must")):
        rc, err = _cli(["pileup", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"), str(tmp_path / "out")])
        assert rc != 0 and what in err.split("\n")[0], (args, err[:300])
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"),
                            str(tmp_path / "out")], capture_output=True, text=True, timeout=120, cwd=ROOT, env=_dist_env())
        assert r.returncode == 2 and "-O" in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(tmp_path)
