"""The fused call-and-pileup path (`pileup -K`, hm_pileup_submit_read_calls), the parts that need no GPU: the ABI symbol, the
command line, the aligned-kinetics BAM generator, and the one fact about `call` the fused record loop relies on for records
the call engine passes through."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


def test_header_declares_and_library_exports_submit_read_calls():
    from hifimeth_amd import _lib
    src = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    m = re.search(r"int\s+hm_pileup_submit_read_calls\s*\(([^;]*)\)\s*;", src)
    assert m, "include/hifimeth_hip.h does not declare hm_pileup_submit_read_calls"
    args = " ".join(m.group(1).split())
    assert args == ("hm_pileup_t* p, uint32_t order, int32_t flag, int32_t sid, int64_t pos, int32_t mapq, int32_t l_qseq, "
                    "const uint8_t* seq4, int32_t n_cigar, const uint32_t* cigar, int64_t n_calls, const hm_call_t* calls, int32_t hp")
    assert "#define HM_ABI_VERSION 5" in src                       # no struct changed
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hm_pileup_submit_read_calls")
    L = _lib.lib()
    assert "hm_pileup_submit_read_calls" in L._hm_symbols
    assert len(L.hm_pileup_submit_read_calls.argtypes) == 13


def test_usage_lists_the_fused_options():
    r = subprocess.run([CLI, "pileup"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    for opt in ("-K\n", "-m <dir>", "-c <list>", "-l <int>", "-p <0|1|2>", "-T <0|1>"):
        assert "  " + opt in r.stderr, opt
    assert "byte-identical" in r.stderr                            # the guarantee is part of the usage text
    for opt in ("-q <mapQ>", "-H\n", "-A\n", "-a <int>"):          # and nothing went missing
        assert "  " + opt in r.stderr, opt


@pytest.mark.parametrize("opt", [["-m", "x"], ["-c", "cpg"], ["-l", "500"], ["-p", "0"], ["-T", "1"]])
def test_caller_options_without_K_are_a_usage_error(opt, tmp_path):
    """refused while the command line is parsed: no file is opened and no device asked for"""
    r = subprocess.run([CLI, "pileup", *opt, str(tmp_path / "no.fa"), str(tmp_path / "no.bam"), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "need -K" in r.stderr and "USAGE:" in r.stderr
    assert "HIP" not in r.stderr and "no.bam" not in r.stderr and "no.fa" not in r.stderr
    assert not list(tmp_path.iterdir())


def test_bad_caller_option_values_with_K(tmp_path):
    for opt in (["-c", "cpg,xyz"], ["-p", "3"], ["-T", "2"], ["-l", "-5"]):
        r = subprocess.run([CLI, "pileup", "-K", *opt, str(tmp_path / "no.fa"), str(tmp_path / "no.bam"), str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "USAGE:" in r.stderr and "HIP" not in r.stderr, opt


def _core(raw):
    tid, pos, l_rn, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", raw, 0)
    cig = np.frombuffer(raw, "<u4", n_cig, 32 + l_rn)
    return tid, pos, mapq, flag, l_seq, cig


def test_write_aligned_kinetics_bam_roundtrip(tmp_path):
    import dataclasses

    from bamutil import parse_aux, read_bam
    from hifimeth_amd.synth import (AlignedRead, aligned_kinetics, kinetics_read, synth_alignments, synth_genome,
                                    write_aligned_kinetics_bam)
    genome = synth_genome(n_chr=2, length=6000)
    reads = synth_alignments(genome, 14, seed=9, median_len=900)
    reads = [dataclasses.replace(r, hp=(None, 1, 2)[i % 3]) for i, r in enumerate(reads)]
    # a hard-clipped supplementary record: its tags keep the whole read's length
    r0 = next(r for r in reads if not r.flag & 4)
    reads.append(dataclasses.replace(r0, name="supp", flag=r0.flag | 0x800, cigar=[("H", 40)] + list(r0.cigar)))
    wide, stale = {1, 4}, {2, 3}
    assert all(reads[i].mm is not None for i in stale)
    path = str(tmp_path / "k.bam")
    kin = aligned_kinetics(reads, seed=4, wide=wide)
    n = write_aligned_kinetics_bam(path, genome, reads, kinetics=kin, keep_mods=stale, threads=2)
    text, recs = read_bam(path)
    assert n > 0 and "SO:coordinate" in text and [f"SN:{nm}" in text for nm, _ in genome] == [True, True]
    assert len(recs) == len(reads)
    for i, (r, rec) in enumerate(zip(reads, recs)):
        tid, pos, mapq, flag, l_seq, cig = _core(rec["raw"])
        assert (rec["name"], tid, pos, mapq, flag, l_seq) == (r.name, r.tid, r.pos, r.mapq, r.flag, r.l_qseq)
        assert (cig == r.cigar_u32()).all() and (rec["seq4"] == r.seq4).all()
        aux = {t: (ty, v) for t, ty, v in parse_aux(rec["aux"])}
        full = r.l_qseq + (40 if r.name == "supp" else 0)
        for t, a in zip(("fi", "fp", "ri", "rp"), kin[i]):
            ty, v = aux[t]
            assert ty == ("BS" if i in wide else "BC") and len(v) == full and (v == a).all()
        assert ("MM" in aux, "ML" in aux, "MN" in aux) == ((i in stale),) * 3
        if i in stale:
            assert aux["MM"][1] == r.mm and (aux["ML"][1] == r.ml).all()
        assert ("HP" in aux) == (r.hp is not None) and (r.hp is None or aux["HP"] == ("i", r.hp))
        # the view the call engine gets: SEQ as stored, kinetics complete only when they match SEQ
        rd = kinetics_read(r, kin[i])
        assert rd.l_qseq == r.l_qseq and rd.flag == r.flag and rd.has_kinetics() == (r.name != "supp")
    # default kinetics: drawn from `seed`, reproducible
    write_aligned_kinetics_bam(str(tmp_path / "a.bam"), genome, reads, seed=5)
    write_aligned_kinetics_bam(str(tmp_path / "b.bam"), genome, reads, seed=5)
    assert open(tmp_path / "a.bam", "rb").read() == open(tmp_path / "b.bam", "rb").read()
    assert isinstance(reads[0], AlignedRead)


def test_call_strips_the_tags_of_a_read_it_passes_through(tmp_path):
    """`call` hands every record through apply_calls, with no calls for a read the engine did not accept: its kinetics AND its own
    MM / ML go (build_mod_bam.cpp:87-109).  So in `call` + `pileup` such a record contributes nothing, and `pileup -K` skips it."""
    from bamutil import parse_aux, read_bam
    from hifimeth_amd.synth import synth_alignments, synth_genome, write_aligned_kinetics_bam
    genome = synth_genome(n_chr=1, length=3000)
    reads = [r for r in synth_alignments(genome, 6, seed=2, median_len=500, frac_no_mods=0) if not r.flag & 4][:2]
    src, dst, empty = str(tmp_path / "in.bam"), str(tmp_path / "out.bam"), str(tmp_path / "calls.bin")
    write_aligned_kinetics_bam(src, genome, reads, keep_mods={0, 1})
    open(empty, "wb").close()
    r = subprocess.run([CLI, "tagtest", src, empty, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    tags_in = [{t for t, _ty, _v in parse_aux(rec["aux"])} for rec in read_bam(src)[1]]
    tags_out = [{t for t, _ty, _v in parse_aux(rec["aux"])} for rec in read_bam(dst)[1]]
    assert all({"MM", "ML", "fi", "rp"} <= t for t in tags_in)
    assert all(not t & {"MM", "ML", "fi", "fp", "ri", "rp"} for t in tags_out)
