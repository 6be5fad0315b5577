"""`diff` without a GPU: the numpy restatement of the loader (diff_ref.Loader) against tables written by hand, the two BED parsers
-- the package's read_cov_bed and the restatement's -- on every kind of line they must reject, and the command's usage text."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from diff_ref import HM_EDATA, HM_ESTATE, Loader, parse_cov_bed

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
NAMES, LENGTHS = ["chrA", "chrB", "c3"], [100, 50, 7]
OFFSETS = [0, 100, 150, 157]


def _planes(ld):
    return {k: {int(i): int(v[i]) for i in np.nonzero(v)[0]} for k, v in ld.planes.items()}


def test_loader_adds_to_the_part_and_to_the_pool():
    ld = Loader(157)
    assert ld.load(1, [5, 0, 156], [3, 0, 1], [1, 2, 0], [0, 1, 2]) == 3
    assert ld.load(2, [156, 5, 99], [4, 2, 7], [4, 0, 7], [2, 0, 1]) == 3
    assert _planes(ld) == {
        "pcov1": {5: 3, 156: 1}, "ncov1": {5: 1, 0: 2}, "pcov2": {156: 4, 5: 2, 99: 7}, "ncov2": {156: 4, 99: 7},
        "pcov": {5: 5, 156: 5, 99: 7}, "ncov": {5: 1, 0: 2, 156: 4, 99: 7}, "key": {0: 1, 156: 2, 99: 1}}
    assert ld.tested(1) == [(5, 3, 1, 2, 0, 0), (156, 1, 0, 4, 4, 2)] and ld.tested(5) == []
    g, p, n, m = ld.loci()
    assert (g.tolist(), p.tolist(), n.tolist(), m.tolist()) == ([0, 5, 99, 156], [0, 5, 7, 5], [2, 1, 7, 4], [1, 0, 1, 2])
    assert [x.tolist() for x in ld.loci(2)] == [[5, 99, 156], [2, 7, 4], [0, 7, 4], [0, 1, 2]]


def test_loader_ignores_rows_without_a_count():
    ld = Loader(10)
    assert ld.load(1, [3, 4, 3], [0, 1, 0], [0, 0, 0], [2, 0, 3]) == 1      # twice on locus 3 without a count: no duplicate, no key
    assert _planes(ld) == {"pcov1": {4: 1}, "ncov1": {}, "pcov2": {}, "ncov2": {}, "pcov": {4: 1}, "ncov": {}, "key": {}}
    assert ld.load(1, [3], [0], [2], [1]) == 1 and ld.load(2, [], [], [], []) == 0


def test_loader_motif_conflict_keeps_the_larger_code():
    ld = Loader(10)
    assert ld.load(1, [2, 3, 4], [1, 1, 1], [0, 0, 0], [0, 1, 2]) == 3      # CpG / CHG / CHH in sample 1
    assert ld.load(2, [2, 3, 4], [1, 1, 1], [0, 0, 0], [1, 0, 3]) == 3      # CHG / CpG / a reverse CHH in sample 2
    assert ld.planes["key"][2:5].tolist() == [1, 1, 3]
    assert [r[5] for r in ld.tested(1)] == [1, 1, 2]                         # the file a row goes to: min(key & 3, 2)


@pytest.mark.parametrize("rows,kind,n_bad", [
    (([4, -1], [1, 1], [1, 1], [0, 0]), "gpos", 1), (([10], [1], [1], [0]), "gpos", 1), (([9, 1], [1, -1], [1, 5], [0, 0]), "count", 1),
    (([1], [1], [-1], [0]), "count", 1), (([1], [-2], [2], [0]), "count", 1), (([1, 2], [1, 1], [1, 1], [4, 3]), "motif", 1),
    (([7, 3, 7], [1, 1, 0], [0, 0, 2], [0, 0, 0]), "dup", 1), (([7, 7, 7], [1, 1, 1], [0, 0, 0], [0, 0, 0]), "dup", 2),
    (([-5], [-1], [0], [9]), "gpos", 1)])                                    # the first failing check names the row
def test_loader_bad_rows(rows, kind, n_bad):
    ld = Loader(10)
    assert ld.load(2, [0], [1], [1], [0]) == 1
    assert ld.load(1, *rows) == HM_EDATA
    assert ld.bad == {**dict.fromkeys(("gpos", "count", "motif", "dup"), 0), kind: n_bad}
    assert ld.load(1, [8], [1], [1], [0]) == HM_ESTATE and ld.load(2, [8], [1], [1], [0]) == HM_ESTATE


def test_loader_duplicates_across_calls_and_parts():
    ld = Loader(10)
    assert ld.load(1, [4], [0], [3], [0]) == 1 and ld.load(2, [4], [2], [0], [0]) == 1      # the other part's count is no duplicate
    assert ld.load(2, [5], [1], [0], [0]) == 1
    assert ld.load(1, [6, 4], [1, 1], [0, 0], [0, 0]) == HM_EDATA and ld.bad["dup"] == 1   # ncov1 held 3 from the first call
    assert ld.planes["pcov1"][4] == 1 and ld.planes["ncov1"][4] == 3 and ld.planes["pcov"][4] == 3   # a duplicate still adds
    ld = Loader(10)
    assert ld.load(1, [4], [1], [0], [0]) == 1
    assert ld.load(1, [4, 4], [1, 1], [0, 0], [0, 0]) == HM_EDATA and ld.bad["dup"] == 2   # both meet the earlier call's count


# ---- the parsers -------------------------------------------------------------------------------------------------------------------
GOOD = "chrA\t0\t1\t75\t3\t1\nchrA\t99\t100\t0\t0\t4\n\nchrB\t49\t50\tnan\t2\t2\r\nc3\t6\t7\t100\t2147483647\t0\n"
GOOD_ROWS = [(0, 3, 1), (99, 0, 4), (149, 2, 2), (156, 2147483647, 0)]
REJECTED = {
    "five columns": "chrA\t1\t2\t50\t1\n", "spaces instead of tabs": "chrA 1 2 50 1 1\n", "an unknown sequence": "chrX\t1\t2\t50\t1\t1\n",
    "a name with a blank behind it": "chrA \t1\t2\t50\t1\t1\n", "start at the sequence's length": "chrB\t50\t51\t50\t1\t1\n",
    "start far outside": "c3\t1000\t1001\t50\t1\t1\n", "a negative start": "chrA\t-1\t0\t50\t1\t1\n", "start no integer": "chrA\t1.0\t2\t50\t1\t1\n",
    "an empty start": "chrA\t\t2\t50\t1\t1\n", "end == start": "chrA\t5\t5\t50\t1\t1\n", "end == start + 2": "chrA\t5\t7\t50\t1\t1\n",
    "end no integer": "chrA\t5\tx\t50\t1\t1\n", "a negative count": "chrA\t5\t6\t50\t-1\t1\n", "a negative ncov": "chrA\t5\t6\t50\t1\t-3\n",
    "a decimal count": "chrA\t5\t6\t50\t1.5\t1\n", "a count with an exponent": "chrA\t5\t6\t50\t1e3\t1\n", "an empty count": "chrA\t5\t6\t50\t\t1\n",
    "a count with a sign": "chrA\t5\t6\t50\t+1\t1\n", "a count of 2^31": "chrA\t5\t6\t50\t2147483648\t1\n",
    "a count with a blank": "chrA\t5\t6\t50\t1 \t1\n", "ncov followed by a blank": "chrA\t5\t6\t50\t1\t1 \n"}


def _both(path, motif=0):
    from hifimeth_amd.pileup import read_cov_bed
    got = read_cov_bed(str(path), NAMES, OFFSETS, motif)
    want = parse_cov_bed(str(path), NAMES, LENGTHS, motif)
    assert [a.dtype for a in got] == [np.int64, np.int32, np.int32, np.uint32]
    assert all((a == b).all() and len(a) == len(b) for a, b in zip(got, want))
    return got


def test_parsers_accept(tmp_path):
    p = tmp_path / "s.CHG.cov.bed"
    p.write_text(GOOD)
    g, pc, nc, m = _both(p, 1)
    assert list(zip(g.tolist(), pc.tolist(), nc.tolist())) == GOOD_ROWS and (m == 1).all()
    from hifimeth_amd.pileup import read_cov_bed
    assert (read_cov_bed(str(p), NAMES, OFFSETS)[3] == 1).all()             # the context from the file name
    p.write_bytes(GOOD.encode()[:-1])                                       # no newline behind the last row
    assert _both(p)[0].tolist() == [r[0] for r in GOOD_ROWS]
    p.write_text("")
    assert len(_both(p)[0]) == 0


def test_parsers_read_gzip(tmp_path):
    p = tmp_path / "s.CpG.cov.bed"
    p.write_bytes(gzip.compress(GOOD.encode()))
    g, pc, nc, m = _both(p)
    assert list(zip(g.tolist(), pc.tolist(), nc.tolist())) == GOOD_ROWS and (m == 0).all()


def test_parsers_ignore_the_columns_behind_the_sixth(tmp_path):
    p = tmp_path / "s.CHH.cov.bed"
    p.write_text("chrA\t7\t8\t66.6667\t2\t1\tCAA\nchrB\t0\t1\t0\t0\t9\tCTT\textra\t\n")       # cov2bed's seventh column
    g, pc, nc, m = _both(p, 2)
    assert (g.tolist(), pc.tolist(), nc.tolist(), m.tolist()) == ([7, 100], [2, 0], [1, 9], [2, 2])


@pytest.mark.parametrize("what", list(REJECTED))
def test_parsers_reject(tmp_path, what):
    from hifimeth_amd.pileup import read_cov_bed
    p = tmp_path / "s.CpG.cov.bed"
    p.write_text("chrA\t0\t1\t75\t3\t1\n\n" + REJECTED[what] + "chrA\t9\t10\t0\t1\t1\n")
    for parse, args in ((read_cov_bed, (NAMES, OFFSETS, 0)), (parse_cov_bed, (NAMES, LENGTHS, 0))):
        with pytest.raises(ValueError) as e:
            parse(str(p), *args)
        assert str(e.value).startswith(f"{p}:3: "), (what, str(e.value))    # the file and the line, empty lines counted


def test_cli_diff_without_arguments_prints_its_usage():
    r = subprocess.run([CLI, "diff"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == ""
    assert "hifimeth-hip diff [OPTIONS] reference prefix1 prefix2 output-prefix" in r.stderr
    assert all(f"  {o}" in r.stderr for o in ("-a <int>", "-Q", "-G", "-s <p>", "-g <bp>", "-n <int>", "-t <CPU threads>", "-d <int>"))
    for args in (["ref.fa", "a", "b"], ["-a", "0", "ref.fa", "a", "b", "out"], ["-s", "0.5", "ref.fa", "a", "b", "out"],
                 ["-G", "-n", "0", "ref.fa", "a", "b", "out"], ["-x", "1", "ref.fa", "a", "b", "out"]):
        r = subprocess.run([CLI, "diff", *args], capture_output=True, text=True)
        assert r.returncode == 1 and "USAGE" in r.stderr and " diff " in r.stderr, args
    assert "diff" in subprocess.run([CLI], capture_output=True, text=True).stderr     # the program's own usage lists the command


def test_library_exports_the_loader():
    from hifimeth_amd import _lib
    L = _lib.lib()
    assert "hm_pileup_load_loci" in L._hm_symbols and L.hm_pileup_load_loci.restype is not None
    header = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    assert "int64_t hm_pileup_load_loci(hm_pileup_t* p, int32_t part, const hm_locus_t* rows, int64_t n);" in header
    assert _lib.HM_ABI_VERSION == 5 and "#define HM_ABI_VERSION 5" in header       # an addition: the version stays
