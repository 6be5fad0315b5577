"""Duplicate loci through the three loaders on the device: hm_pileup_load_loci, hm_pileup_load_sample_loci and hm_sample_load on the
cases of loader_dup_cases.py, whose rows stand in chosen wavefronts, workgroups, slabs and calls.  Of k counted rows that one
target gets for one locus exactly k - 1 are duplicates, whatever the geometry, the order of the rows or the slab size: every case
is loaded as placed and in three seeded permutations, and the answer is the same each time.

Everything is exact.  The return values, the message (the literal the engine writes, with sum (k - 1) duplicates in it) and the
voiding are checked for every case, loader and order.  `diff` adds a duplicate too, so its seven planes equal the restatement's
byte for byte in every case.  In the other two a duplicate adds nothing and which row of a locus wins is open: the loci that hold a
count afterwards are determined and are compared in every case, the planes themselves where every duplicate equals its partner
(identical-duplicates).  A call with bad rows returns HM_EDATA, not the number of rows that added, and the planes an engine keeps
to itself (moments, sample counts, levels) cannot be read from a void engine: the rows that added are seen in the returns of the
clean calls and in the caller's planes."""
import subprocess

import numpy as np
import pytest

import loader_dup_cases as D
from loader_dup_cases import HM_EDATA, HM_ESTATE, LOADERS
from test_gpu_pileup_asm import CLI
from test_gpu_pileup_diff import _load as _load_part
from test_gpu_pileup_groups import _begin, _load as _load_group
from test_gpu_pileup_loaders import LENGTHS, VOID, WHO, _engine, _err, _genome, _loaded_restatements, _rows
from test_gpu_pileup_samples import _open, _load as _load_sample

pytestmark = pytest.mark.gpu

assert LENGTHS == D.LENGTHS
GOOD = ([100], [1], [1], [0])
DIFF_PLANES = ("pcov", "ncov", "key", "pcov1", "ncov1", "pcov2", "ncov2")


def _run(case, loader, order, calls=None):
    """a fresh engine on the caller's planes, minimum coverage 1, the case's slab; its calls (or `calls`) in turn -> (engine,
    planes, returns)"""
    pu, _load, t = _engine(loader, planes=True, slab=case.slab)
    returns, opened = [], 1                                   # _engine opened the first sample
    for target, rows in case.calls(loader, order) if calls is None else calls:
        if loader == "diff":
            returns.append(_load_part(pu, target, rows))
            continue
        while opened < target:
            assert (_begin(pu, 1) if loader == "groupdiff" else _open(pu)) == opened
            opened += 1
        returns.append((_load_group if loader == "groupdiff" else _load_sample)(pu, rows))
    return pu, t, returns


def _duplicates_in(text, loader):
    """the number in front of the duplicates' words in the engine's message"""
    head, _sep, _tail = text.partition(" " + D.DUP_TEXT[loader])
    return int(head.rsplit(" ", 1)[1])


@pytest.mark.parametrize("loader", LOADERS)
@pytest.mark.parametrize("case", D.cases(), ids=repr)
def test_the_rows_that_add_are_counted_by_the_engine(case, loader):
    """a call with bad rows returns HM_EDATA, so the engine never tells how many rows of a case added.  The case without its bad
    rows and duplicates -- of every target and locus the first counted row -- is clean: every call returns its number of rows, the
    restatement's, and for the two sample loaders their sum is the `added` of the case itself; the planes are the restatement's"""
    calls = D.clean_calls(case, loader)
    got, ref = D.by_restatement(case, loader, calls=calls)
    pu, t, returns = _run(case, loader, 0, calls)
    try:
        print(case, loader, returns)
        assert returns == got["returns"] == [len(rows[0]) for _t, rows in calls] and all(r > 0 for r in returns), _err(pu)
        assert loader == "diff" or sum(returns) == D.by_counts(case, loader)["added"] == got["added"]
        for x, name in zip(t, DIFF_PLANES):
            assert x.cpu().numpy().tobytes() == ref.planes[name].astype(np.int32).tobytes(), name
    finally:
        pu.close()


def test_retargeting_a_part_forgets_its_rows():
    """rows into both parts, then other planes for part 1 (hm_pileup_use_partition_planes after the load): the same loci are no
    duplicates for part 1, whose new planes then hold exactly these rows, and still are for part 2, each row once"""
    import ctypes
    import torch
    rows = _rows()
    ref, want = _loaded_restatements()["diff"]
    pu, _load, t = _engine("diff", planes=True)
    try:
        assert _load_part(pu, 1, rows) == want and _load_part(pu, 2, rows) == want
        fresh = [torch.zeros(D.TOTAL, dtype=torch.int32, device="cuda") for _ in range(2)]
        assert pu._L.hm_pileup_use_partition_planes(pu._h, 1, *(ctypes.c_void_p(x.data_ptr()) for x in fresh)) == 0
        assert _load_part(pu, 1, rows) == want, _err(pu)
        for x, name in zip(fresh, ("pcov1", "ncov1")):
            assert x.cpu().numpy().tobytes() == ref.planes[name].astype(np.int32).tobytes() and x.any(), name
        assert t[3].cpu().numpy().tobytes() == fresh[0].cpu().numpy().tobytes()      # the planes it left keep the first load
        assert _load_part(pu, 2, rows) == HM_EDATA
        assert _err(pu).decode() == D.message("diff", 0, 0, 0, 0, want)
    finally:
        pu.close()


@pytest.mark.parametrize("loader", LOADERS)
@pytest.mark.parametrize("case", D.cases(), ids=repr)
def test_duplicates_are_counted_exactly(case, loader):
    for order in range(D.N_ORDERS):
        want = D.by_counts(case, loader, order)
        got, ref = D.by_restatement(case, loader, order)
        pu, t, returns = _run(case, loader, order)
        try:
            text = _err(pu).decode()
            print(case, loader, order, returns, text)
            assert returns == want["returns"] == got["returns"] and returns[-1] == HM_EDATA
            assert _duplicates_in(text, loader) == want["dup"] == got["dup"]
            assert text == want["message"] == got["message"]
            planes = [x.cpu().numpy() for x in t]
            if loader == "diff":                              # a duplicate still adds: every plane is the restatement's
                for x, name in zip(planes, DIFF_PLANES):
                    assert x.tobytes() == ref.planes[name].astype(np.int32).tobytes(), (order, name)
            else:                                             # one row per locus and target added: the covered loci are determined
                covered = np.flatnonzero(planes[0].astype(np.int64) + planes[1])
                assert (covered == want["covered"]).all() and (covered == got["covered"]).all() and got["added"] == want["added"]
                if case.name == "identical-duplicates":
                    for x, name in zip(planes, DIFF_PLANES):
                        assert x.tobytes() == ref.planes[name].astype(np.int32).tobytes(), (order, name)
            # void: the next load and the next fetch refuse, in the words they always had
            assert (_load_part(pu, 1, GOOD) if loader == "diff" else _load_group(pu, GOOD) if loader == "groupdiff" else _load_sample(pu, GOOD)) == HM_ESTATE
            assert _err(pu) == WHO[loader] + VOID
            assert pu._L.hm_pileup_fetch_loci(pu._h, None, None, None, 0, 0, D.TOTAL, None, 0) == HM_ESTATE and _err(pu) == VOID[2:]
        finally:
            pu.close()


def _clean_load_gives_the_planes(loader):
    ref, want = _loaded_restatements()[loader]
    pu, load, t = _engine(loader, planes=True)
    try:
        assert load(_rows()) == want > 0, _err(pu)
        for x, name in zip(t, DIFF_PLANES):
            assert x.cpu().numpy().tobytes() == ref.planes[name].astype(np.int32).tobytes(), name
    finally:
        pu.close()


@pytest.mark.parametrize("loader", LOADERS)
def test_a_fresh_engine_knows_nothing_of_the_one_before(loader):
    """the duplicate-free rows of test_gpu_pileup_loaders.py through a fresh engine, an engine voided by duplicates, the rows again
    through a fresh engine: nothing an engine has seen -- the first one saw these very loci -- outlives it"""
    _clean_load_gives_the_planes(loader)
    case = D.case("pairs-across")
    pu, _t, returns = _run(case, loader, 0)
    try:
        assert returns == [HM_EDATA] and _err(pu).decode() == D.by_counts(case, loader)["message"]
    finally:
        pu.close()
    _clean_load_gives_the_planes(loader)
    pu, load, _t = _engine(loader, planes=True)               # and within one engine: the other partition, the next sample
    try:
        rows = _rows()
        want = _loaded_restatements()[loader][1]
        assert load(rows) == want
        if loader == "diff":
            assert _load_part(pu, 2, rows) == want
        else:
            assert (_begin(pu, 1) if loader == "groupdiff" else _open(pu)) == 1 and load(rows) == want
    finally:
        pu.close()


# ---- the command ------------------------------------------------------------------------------------------------------------------------
RUNS = 8


def _bed(rows):
    names = [n for n, _ in _genome()]
    s = np.searchsorted(D.OFFSETS, rows[0], side="right") - 1
    return "".join("%s\t%d\t%d\t%g\t%d\t%d\n" % (names[c], g - D.OFFSETS[c], g - D.OFFSETS[c] + 1, 100.0 * p / max(p + n, 1), p, n)
                   for c, g, p, n in zip(s.tolist(), rows[0].tolist(), rows[1].tolist(), rows[2].tolist()))


def _sets():
    """{name: the CpG rows of sample A}: a locus in two rows of a small file; a locus as a pcov-only row in workgroup 0 and an
    ncov-only row in the last workgroup of a file of 4 202 rows, which -t 1 hands to the loader in one call, one launch"""
    rng = np.random.default_rng(31)
    loci = rng.choice(D.TOTAL, 4201, replace=False)
    p, n = rng.integers(1, 30, 4201), rng.integers(0, 30, 4201)
    small = (np.array([10, 41, 700, 41]), np.array([9, 2, 3, 1]), np.array([1, 9, 3, 1]))
    large = (np.concatenate([loci, loci[:1]]), np.concatenate([[3], p[1:], [0]]), np.concatenate([[0], n[1:], [5]]))
    assert len(large[0]) >= 4096 and (len(large[0]) - 1) // 256 > 0
    return {"two rows of one locus": small, "pcov-only and ncov-only row, workgroups apart": large}


@pytest.mark.parametrize("which", list(_sets()))
def test_the_command_refuses_a_duplicate_every_time(which, tmp_path):
    """8 runs of `diff` on the same files: the exit status and the line that names the duplicates are the same each time, and are
    what the Python path says.  The check of a value, eight times; a wrong count in any run fails."""
    from bamutil import write_fasta
    from hifimeth_amd.caller import HifimethError
    from hifimeth_amd.pileup import MethylationPileup, read_cov_bed
    rows = _sets()[which]
    genome = _genome()
    fa, A, B, out = (str(tmp_path / x) for x in ("ref.fa", "A", "B", "out"))
    write_fasta(fa, genome)
    with open(A + ".CpG.cov.bed", "w") as f:
        f.write(_bed(rows))
    with open(B + ".CpG.cov.bed", "w") as f:
        f.write(_bed((np.array([10, 41]), np.array([1, 8]), np.array([9, 1]))))
    pu = MethylationPileup(genome, partitions=True)
    try:
        loaded = read_cov_bed(A + ".CpG.cov.bed", [n for n, _ in genome], pu.offsets)
        assert (loaded[0] == rows[0]).all() and (loaded[1] == rows[1]).all() and (loaded[2] == rows[2]).all()
        with pytest.raises(HifimethError):
            pu.load_loci(1, *loaded)
        said = _err(pu).decode()
    finally:
        pu.close()
    assert said == "hm_pileup_load_loci: 1 bad rows: 1 locus given twice for one part"
    want = (1, ["ERROR: %s.CpG.cov.bed: %s" % (A, said)])
    got = []
    for _ in range(RUNS):
        r = subprocess.run([CLI, "diff", "-t", "1", fa, A, B, out], capture_output=True, text=True, timeout=120)
        got.append((r.returncode, [x for x in r.stderr.splitlines() if "given twice" in x or "bad rows" in x]))
    print(got)
    assert got == [want] * RUNS
