"""`pileup -S` without a GPU: a hand-written table for the restatement (tests/context_ref.py), the k-mer names, the TSV writer, the
header's declaration and the errors the command line reports before it touches a device."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import context_ref as X
from conftest import ROOT

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")

# Two sequences back to back, global coordinates 0 .. 19:
#   chrA  T C C G A T G N C G A C      chrB  G T A C C T A G
#         0 1 2 3 4 5 6 7 8 9 10 11          12 13 14 15 16 17 18 19
SEQS = ["TCCGATGNCGAC", "GTACCTAG"]
# locus: (pcov, ncov, context), and where it goes at flank 0
#   1  C, window CCG                                   (3, 1, CHG)  ppm (6e6 + 4) / 8 = 750 000
#   4  A: neither C nor G -> other                     (1, 0, CHG)  1 000 000
#   6  G, window ATG, reverse complement CAT           (1, 1, CHH)  500 000
#   8  C, window CGA                                   (0, 5, CpG)  0
#   9  G, window NCG: an N inside -> other             (2, 0, CpG)  1 000 000
#  11  C, window would be C + chrB's GT -> other       (1, 2, CHH)  (2e6 + 3) / 6 = 333 333
#  12  G, first of chrB, window would start in chrA -> other   (4, 0, CHH)  1 000 000
#  15  C, window CCT                                   (2, 2, CHH)  500 000
#  16  C, window CTA                                   (1, 0, CHH)  1 000 000
#  19  G, window TAG, reverse complement CTA           (0, 1, CHH)  0
LOCI = {1: (3, 1, 1), 4: (1, 0, 1), 6: (1, 1, 2), 8: (0, 5, 0), 9: (2, 0, 0), 11: (1, 2, 2), 12: (4, 0, 2), 15: (2, 2, 2), 16: (1, 0, 2),
        19: (0, 1, 2)}
ROW = {"CAT": 1 * 16 + 0 * 4 + 3, "CCG": 1 * 16 + 1 * 4 + 2, "CCT": 1 * 16 + 1 * 4 + 3, "CGA": 1 * 16 + 2 * 4 + 0, "CTA": 1 * 16 + 3 * 4 + 0, "other": 64}
WANT = {(0, "CGA"): [1, 0, 5, 0], (0, "other"): [1, 2, 0, 1000000],
        (1, "CCG"): [1, 3, 1, 750000], (1, "other"): [1, 1, 0, 1000000],
        (2, "CAT"): [1, 1, 1, 500000], (2, "CCT"): [1, 2, 2, 500000], (2, "CTA"): [2, 1, 1, 1000000], (2, "other"): [2, 5, 2, 1333333]}


def _planes():
    pc, nc, ky = (np.zeros(20, np.int32) for _ in range(3))
    for g, (p, n, c) in LOCI.items():
        pc[g], nc[g], ky[g] = p, n, c | (g << 2)                                  # order bits above the context: ignored
    return pc, nc, ky


def _literal(want, rows, n_rows):
    tab = np.zeros((3, n_rows, 4), np.int64)
    for (c, name), v in want.items():
        tab[c, rows[name]] = v
    return tab


def test_known_answer_flank_0():
    assert X.reverse_complement("ATG") == "CAT" and X.reverse_complement("TAG") == "CTA"  # the two G-loci, spelled out
    assert X.kmer_rows(3)["CAT"] == ROW["CAT"] == 19 and X.kmer_rows(3)["CTA"] == 28
    got = X.context_table(*_planes(), SEQS, 0)
    assert got.shape == (3, 65, 4) and (got == _literal(WANT, ROW, 65)).all()


def test_known_answer_flank_1():
    """k = 5: loci 1, 15 and 16 keep a window (TCCGA, ACCTA, CCTAG); 6 gets the N (GATGN), 8 too (NCGAC), 19's leaves chrB"""
    code = lambda s: int("".join(str("ACGT".index(ch)) for ch in s), 4)  # noqa: E731
    assert code("TCCGA") == 3 * 256 + 64 + 16 + 8 == 856 and code("ACCTA") == 92 and code("CCTAG") == 370
    rows = {"TCCGA": 856, "ACCTA": 92, "CCTAG": 370, "other": 1024}
    want = {(1, "TCCGA"): [1, 3, 1, 750000], (2, "ACCTA"): [1, 2, 2, 500000], (2, "CCTAG"): [1, 1, 0, 1000000],
            (0, "other"): [2, 2, 5, 1000000], (1, "other"): [1, 1, 0, 1000000], (2, "other"): [4, 6, 4, 1833333]}
    got = X.context_table(*_planes(), SEQS, 1)
    assert got.shape == (3, 1025, 4) and (got == _literal(want, rows, 1025)).all()


def test_min_cov_range_and_base():
    pc, nc, ky = _planes()
    two = X.context_table(pc, nc, ky, SEQS, 0, min_cov=2)                         # loci 4, 16 and 19 (coverage 1) fall out
    want = dict(WANT)
    del want[(1, "other")]
    want[(2, "CTA")] = [0, 0, 0, 0]
    assert (two == _literal(want, ROW, 65)).all()
    whole = X.context_table(pc, nc, ky, SEQS, 0)
    for cut in (1, 9, 12, 13, 19):                                                # a chunk's planes with a base: the halves add up
        left = X.context_table(pc[:cut], nc[:cut], ky[:cut], SEQS, 0)
        right = X.context_table(pc[cut:], nc[cut:], ky[cut:], SEQS, 0, base=cut)
        assert (left + right == whole).all(), cut
        assert (X.context_table(pc, nc, ky, SEQS, 0, lo=cut) == right).all(), cut


@pytest.mark.parametrize("flank", [0, 1, 2, 3])
def test_invariant_counted_loci_per_context(flank):
    rng = np.random.default_rng(flank)
    seqs = ["".join(rng.choice(list("ACGTN"), n, p=[0.24, 0.24, 0.24, 0.24, 0.04])) for n in (1, 2, 3, 2 * flank + 3, 40, 0, 60)]
    n = sum(len(s) for s in seqs)
    pc, nc, ky = rng.integers(0, 3, n), rng.integers(0, 3, n), rng.integers(0, 1 << 10, n)
    for min_cov in (1, 2, 3):
        tab = X.context_table(pc, nc, ky, seqs, flank, min_cov=min_cov, lo=2, hi=n - 1)
        counted = (pc + nc >= min_cov)[2:n - 1]
        for c in range(3):
            assert tab[c, :, 0].sum() == (counted & ((ky & 3)[2:n - 1] == c)).sum() > 0
        assert tab[:, -1, 0].sum() > 0 and tab[:, :-1, 0].sum() > 0


def test_kmer_names_round_trip():
    from hifimeth_amd.pileup import context_code, context_kmer
    assert context_kmer(0, 3) == "AAA" and context_kmer(63, 3) == "TTT" and context_kmer(22, 3) == "CCG" and context_kmer(64, 3) == "other"
    assert context_kmer(856, 5) == "TCCGA" and context_code("TCCGA") == 856
    for k in (3, 5, 7, 9):
        names = X.kmer_rows(k) if k < 9 else None
        for code in ([*range(64)] if k == 3 else []) + [0, 1, 4 ** k // 3, 4 ** k - 1]:
            text = context_kmer(code, k)
            assert len(text) == k and context_code(text) == code and (names is None or names[text] == code)
        assert context_kmer(4 ** k, k) == "other"
        with pytest.raises(ValueError):
            context_kmer(4 ** k + 1, k)


def test_tsv_text():
    from hifimeth_amd.pileup import context_tsv
    text = context_tsv(X.context_table(*_planes(), SEQS, 0), 0)
    head = "#context\tn_loci\tpcov\tncov\tweighted\tmean\n"
    assert text["CpG"] == head + "CGA\t1\t0\t5\t0\t0\nother\t1\t2\t0\t100\t100\n"
    assert text["CHG"] == head + "CCG\t1\t3\t1\t75\t75\nother\t1\t1\t0\t100\t100\n"
    assert text["CHH"] == head + "CAT\t1\t1\t1\t50\t50\nCCT\t1\t2\t2\t50\t50\nCTA\t2\t1\t1\t50\t50\nother\t2\t5\t2\t71.4286\t66.6667\n"
    empty = context_tsv(np.zeros((3, 1025, 4), np.int64), 1)
    assert empty == {c: head for c in X.CTX}                                      # no row without a counted locus, `other` included


def test_header_and_symbols():
    from hifimeth_amd import _lib
    from hifimeth_amd.pileup import context_geometry
    src = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    assert "#define HM_ABI_VERSION 5" in src                                      # no struct changed
    m = re.search(r"int64_t hm_pileup_fetch_context\((.*?)\);", src, re.S)
    assert m and " ".join(m.group(1).split()) == (
        "hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo, int64_t hi, "
        "int64_t min_cov, int32_t flank, hm_region_sum_t* out, int64_t cap")
    for word in ("strand-split", "tests between contexts", "IUPAC", "sequence", "k above 9"):
        assert word in src[src.index("`pileup -S`"):]
    L = _lib.lib()
    assert L.hm_abi_version() == 5
    assert {"hm_pileup_fetch_context", "hm_pileup_fetch_context_path", "hm_context_geometry"} <= set(L._hm_symbols)
    assert len(L.hm_pileup_fetch_context.argtypes) == 11
    span, lds_flank, lds_max = context_geometry()
    assert span == 1024 and 0 <= lds_flank <= lds_max == 1                        # flank 0 never pays global atomics on 64 rows


def test_cli_usage_errors(tmp_path):
    """-O without -S, either out of range: before any file is opened"""
    for args, what in ((["-O", "2"], "-O needs -S"), (["-S", "4"], "-S must"), (["-S", "-1"], "-S must"), (["-S", "x"], "-S must"),
                       (["-S", "1.5"], "-S must"), (["-S", "1", "-O", "0"], "-S must"), (["-S", "0", "-O", "x"], "-S must")):
        r = subprocess.run([CLI, "pileup", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"), str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and f"ERROR: {what}" in r.stderr.split("\n")[0], (args, r.stderr[:300])
    assert not os.listdir(tmp_path)
    r = subprocess.run([CLI, "pileup", "-C", "2", str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "ERROR: -C and -J need -R" in r.stderr.split("\n")[0]       # -C keeps its meaning
    r = subprocess.run([CLI, "pileup"], capture_output=True, text=True, timeout=60)
    assert all(t in r.stderr + r.stdout for t in ("-S <flank>", "-O <int>", "context.<ctx>.tsv"))


def test_pileup_dist_refusals(tmp_path):
    for args in (["-O", "2"], ["-S", "4"], ["-S", "-1"], ["-S", "1", "-O", "0"]):
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"),
                            str(tmp_path / "out")], capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 2 and "-O" in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(tmp_path)
