"""`smooth` without a GPU: the two formulations of tests/smooth_ref.py against each other and against windows written out by hand,
the struct's layout as a C compiler sees it, the symbols, hm_smooth_stats (host only) bit for bit, and the command's usage, option
errors and recorded command lines (tests/golden/cli_options_smooth.json)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
RANGE_RULE = "ERROR: -W must be an integer in [1, 16384], -a an integer in [1, 2147483647], -i an integer >= 1\n"


def test_windows_written_out_by_hand():
    # two sequences [0, 10) and [10, 14); CpG at 2, 5, 9 | 10, 13; a CHG locus at 4 and a CpG without a call's worth at 7 (cov 1)
    rows = S.locus_rows([2, 4, 5, 7, 9, 10, 13], [1, 9, 2, 1, 4, 8, 16], [3, 9, 0, 0, 1, 0, 2], [0, 1, 0, 0, 0, 0, 0])
    off = [0, 10, 14]
    for f in (S.smooth_direct, S.smooth_prefix):
        got = f(rows, off, 0, 4, min_cov=2)                   # 7 does not count; weights 4 - distance; 9 and 10 do not see each other
        assert got.tolist() == [(2, 1, 3, 2, 4 * 1 + 1 * 2, 4 * 3), (5, 2, 0, 2, 1 * 1 + 4 * 2, 1 * 3),       # 9 is exactly 4 from 5: outside
                                (9, 4, 1, 1, 4 * 4, 4 * 1), (10, 8, 0, 2, 4 * 8 + 1 * 16, 1 * 2), (13, 16, 2, 2, 1 * 8 + 4 * 16, 4 * 2)]
        assert f(rows, off, 0, 5, min_cov=2).tolist()[1] == (5, 2, 0, 3, 2 * 1 + 5 * 2 + 1 * 4, 2 * 3 + 1 * 1)  # at h = 5 it has weight 1
        assert f(rows, off, 0, 4, min_cov=2, min_loci=2)["gpos"].tolist() == [2, 5, 10, 13]                   # min_loci only drops rows
        assert f(rows, off, 0, 4)["gpos"].tolist() == [2, 5, 7, 9, 10, 13] and f(rows, off, 1, 4).tolist() == [(4, 9, 9, 1, 36, 36)]
        assert f(rows, off, 0, 1, min_cov=2).tolist() == [(g, p, n, 1, p, n) for g, p, n in ((2, 1, 3), (5, 2, 0), (9, 4, 1), (10, 8, 0), (13, 16, 2))]
        assert f(rows, off, 0, 4, min_cov=2, lo=5, hi=10).tobytes() == got[1:3].tobytes()


def test_the_two_formulations_agree_on_the_boundary_set():
    rows, off = S.boundary_rows()
    assert off.tolist() == [0, 1, 3, 8, 3008, 73008] and 0.2 * off[-1] < len(rows) < 0.35 * off[-1]
    n = 0
    for ctx in (0, 1, 2):
        pos = S.counting(rows, ctx, 1)[0]
        for h in S.HALF_WIDTHS:
            for min_cov, min_loci in ((1, 1), (3, 1), (1, 5), (3, 2)):
                if (min_cov, min_loci) != (1, 1) and not (ctx == 0 or h == 500):
                    continue
                a = S.smooth_direct(rows, off, ctx, h, min_cov, min_loci)
                b = S.smooth_prefix(rows, off, ctx, h, min_cov, min_loci)
                assert a.tobytes() == b.tobytes() and (len(a) > 0 or (min_loci > 1 and h < 500)), (ctx, h, min_cov, min_loci)
                n += len(a)
            if h > 1:                                         # loci exactly h - 1 (weight 1) and exactly h (weight 0) apart exist
                d = set(pos.tolist())
                assert any(g + h - 1 in d for g in pos.tolist()) and any(g + h in d for g in pos.tolist()), (ctx, h)
        whole = S.smooth_prefix(rows, off, ctx, 16384)
        assert (whole["loci"][whole["gpos"] < 8] <= 3).all()  # nothing leaks out of the short sequences
        assert whole["loci"].max() > 2000 and S.smooth_prefix(rows, off, ctx, 1)["loci"].max() == 1
    assert n > 100000


def test_the_two_formulations_agree_where_the_sums_are_largest():
    for mirror in (False, True):
        rows, off = S.exact_rows(mirror)
        b = S.smooth_prefix(rows, off, 0, 16384)
        assert len(b) == 40000
        for lo, hi in ((0, 40), (16380, 16390), (19990, 20010), (23610, 23620), (39960, 40000)):
            a = S.smooth_direct(rows, off, 0, 16384, lo=lo, hi=hi)
            assert a.tobytes() == b[lo:hi].tobytes()
        mid = b[20000]
        assert int(mid["wn" if mirror else "wp"]) == (2 ** 31 - 1) * 16384 ** 2 > 2 ** 58 and int(mid["wp" if mirror else "wn"]) == 0
        assert int(mid["loci"]) == 2 * 16384 - 1 and int(b[0]["loci"]) == 16384


def test_struct_layout_as_the_compiler_sees_it(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hifimeth_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(hm_smooth_t), offsetof(hm_smooth_t, gpos), '
                   'offsetof(hm_smooth_t, pcov), offsetof(hm_smooth_t, ncov), offsetof(hm_smooth_t, loci), offsetof(hm_smooth_t, wp), '
                   'offsetof(hm_smooth_t, wn), HM_ABI_VERSION, HM_SMOOTH_MAX_HALF_WIDTH, HM_SMOOTH_SPAN); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["40", "0", "8", "12", "16", "24", "32", "5", "16384", "32768"]
    from hifimeth_amd.pileup import SMOOTH_DTYPE
    assert SMOOTH_DTYPE == S.SMOOTH_DTYPE and SMOOTH_DTYPE.itemsize == 40
    assert [SMOOTH_DTYPE.fields[k][1] for k in SMOOTH_DTYPE.names] == [0, 8, 12, 16, 24, 32]


def test_symbols_header_and_python_names():
    from hifimeth_amd import pileup as P
    from hifimeth_amd._lib import HM_ABI_VERSION, lib
    L = lib()
    assert L.hm_abi_version() == 5 == HM_ABI_VERSION
    for name in ("hm_smooth_fetch", "hm_smooth_stats"):
        assert hasattr(L, name) and name in L._hm_symbols, name
    assert hasattr(P.MethylationPileup, "fetch_smooth") and callable(P.smooth_stats)
    header = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    assert "} hm_smooth_t;" in header and "int hm_smooth_stats(" in header and "#define HM_ABI_VERSION 5\n" in header


def test_smooth_stats_equals_the_formula_bit_for_bit():
    from hifimeth_amd.caller import HifimethError
    from hifimeth_amd.pileup import smooth_stats
    rng = np.random.default_rng(5)
    pairs = [(1, 0), (0, 1), (1, 1), (2 ** 60, 0), (0, 2 ** 60), (2 ** 60, 2 ** 60), (2 ** 60 - 1, 2 ** 60 - 1), (2 ** 53 + 1, 2 ** 53 + 3),
             (2 ** 59 + 2 ** 5 + 1, 3), ((2 ** 31 - 1) * 16384 ** 2, 0), (1, 2 ** 60), (3, 2 ** 54 + 1)]
    pairs += [(int(rng.integers(0, 2 ** 60, endpoint=True)), int(rng.integers(0, 2 ** 60, endpoint=True))) for _ in range(300)]
    pairs += [(int(a) >> int(s), int(b) >> int(t)) for a, b, s, t in zip(rng.integers(1, 2 ** 60, 300), rng.integers(1, 2 ** 60, 300),
                                                                          rng.integers(0, 60, 300), rng.integers(0, 60, 300)) if (int(a) >> int(s)) + (int(b) >> int(t))]
    row = np.zeros(1, S.SMOOTH_DTYPE)
    for wp, wn in pairs:
        for h in (1, 7, 500, 16384):
            row["wp"], row["wn"] = wp, wn
            got = smooth_stats(row[0], h)
            want = (100.0 * float(wp) / (float(wp) + float(wn)), (float(wp) + float(wn)) / h)
            assert np.array(got).tobytes() == np.array(want).tobytes() == np.array(S.stats(row[0], h)).tobytes(), (wp, wn, h)
    row["wp"], row["wn"] = 0, 0
    with pytest.raises(HifimethError):
        smooth_stats(row[0], 5)
    row["wp"] = 5
    for h in (0, -1):
        with pytest.raises(HifimethError):
            smooth_stats(row[0], h)


def _run(args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def test_usage_of_the_command():
    r = _run(["smooth", "-h"])
    assert r.returncode == 0 and r.stdout == "" and "smooth [OPTIONS] reference prefix output-prefix" in r.stderr
    assert [x.strip() for x in r.stderr.splitlines() if x.startswith("  -")] == ["-W <bp>", "-a <int>", "-i <int>", "-t <CPU threads>", "-d <int>"]
    assert "Default: 500" in r.stderr and "smooth.summary.tsv" in r.stderr
    tail = ["ref.fa", "a", "o"]
    for args in (["-W", "0"], ["-W", "16385"], ["-W", "x"], ["-W", "2.5"], ["-W", ""], ["-a", "0"], ["-a", "2147483648"], ["-i", "0"], ["-i", "-3"]):
        r = _run(["smooth", *args, *tail])
        assert r.returncode == 1 and r.stderr.startswith(RANGE_RULE + "USAGE:"), (args, r.stderr[:200])
    for args in (["-Q"], ["-G"], ["-R", "x.bed"], ["-H"]):
        r = _run(["smooth", *args, *tail])
        assert r.returncode == 1 and r.stderr.startswith("ERROR: unrecognised option %s\n" % args[0]), (args, r.stderr[:200])
    assert _run(["smooth", "ref.fa", "a"]).returncode == 1 and _run(["smooth", "ref.fa", "a", "o", "more"]).returncode == 1
    r = _run(["smooth", "-W", "16384", "-a", "2", "-i", "3", *tail])     # a good line gets as far as the missing files
    assert r.returncode == 1 and "half-width 16384, min coverage 2, min loci per window 3" in r.stderr
    assert r.stderr.endswith("ERROR: no context has a cov.bed file of the sample\n") and "USAGE:" not in r.stderr
    assert "smooth [OPTIONS] reference prefix output-prefix" in _run([]).stderr


def test_recorded_command_lines(tmp_path):
    """tests/golden/cli_options_smooth.json holds the command's matrix of tools/make_cli_options.py: replayed byte for byte; per flag
    of the usage text one case ends in the usage and one gets past the checks"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_cli_options as M
    usage, cases = M.load(M.SMOOTH_FIXTURE)
    assert list(usage) == ["smooth"] and [(c[0], c[1]) for c in cases] == M.matrix(M.SMOOTH_COMMANDS) and len(cases) > 60
    prefix = str(tmp_path / "out")
    assert M.run_case(CLI, "smooth", ["-h"], prefix) == (0, usage["smooth"], "")
    for cmd, args, code, follows, stderr in cases:
        assert M.run_case(CLI, cmd, args, prefix) == (code, usage[cmd] if follows else None, stderr), args
    flags = re.findall(r"^  (-\w)(?: |$)", usage["smooth"], re.M)
    assert flags == ["-W", "-a", "-i", "-t", "-d"]
    for flag in flags:
        assert {c[3] for c in cases if flag in c[1]} == {0, 1}, flag
    assert not os.listdir(tmp_path)
    assert {c[0] for c in M.matrix()} == {"pileup", "diff"}   # the older fixture's matrix is what it was
