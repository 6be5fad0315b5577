"""The fused call-and-pileup path: hm_pileup_submit_read_calls / MethylationPileup.add_called / `pileup -K`.

The specification is one equivalence: handing a read's calls to the pileup engine has the effect of writing them into the
record as MM / ML, parsing those back and submitting the parsed lists.  The ABI tests build exactly that pair (tags written
by oracle/modtags.py, parsed by the host mirror's parse_mods) and compare everything the engine exposes; the CLI test compares
`pileup -K` with `call` followed by `pileup`, byte for byte.  Inputs are the smallest that keep every path alive: 2 chromosomes
of 20 / 26 kb, ~40 alignments of ~1.5 kb on both strands with indels and soft clips."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
CTX = ("CpG", "CHG", "CHH")
HM_EINVAL, HM_EDATA, HM_ESTATE = -1, -4, -5


@pytest.fixture(scope="module")
def data():
    """genome, mapped reads of >= 1000 bases with kinetics, and their calls from the caller mirror (dense trunk fixed, so the
    kernel path does not depend on the sample); computed once, never modified"""
    from hifimeth_amd import MethylationCaller
    from hifimeth_amd.synth import aligned_kinetics, kinetics_read, revcomp, synth_alignments, synth_genome
    from oracle.modtags import expected_tags
    genome = synth_genome(n_chr=2, length=20000)
    reads = [r for r in synth_alignments(genome, 48, seed=17, median_len=1500, frac_unmapped=0) if r.l_qseq >= 1000]
    kin = aligned_kinetics(reads, seed=18, wide={3})
    with MethylationCaller(device=0) as mc:
        mc.set_option("trunk", 1)
        calls = mc.call([kinetics_read(r, k) for r, k in zip(reads, kin)])
    per_read = [calls[calls["read_id"] == i] for i in range(len(reads))]
    tagged = []                                  # the same reads carrying their calls as MM / ML
    for r, c in zip(reads, per_read):
        t = expected_tags((revcomp(r.seq) if r.flag & 16 else r.seq).encode(), c["qoff"], c["strand"], c["scaled_prob"])
        tagged.append(dataclasses.replace(r, mm=t["MM"] if t else None, ml=t["ML"] if t else None))
    thr = [int(np.median(calls["scaled_prob"][calls["ctx"] == c])) for c in range(3)]
    return dict(genome=genome, reads=reads, kin=kin, calls=per_read, tagged=tagged, thr=thr)


def test_inputs_cover_the_paths(data):
    reads, calls = data["reads"], data["calls"]
    assert 36 <= len(reads) <= 48 and all(len(c) > 0 for c in calls)
    assert sum(1 for r in reads if r.flag & 16) * 3 >= len(reads) and any(not r.flag & 16 for r in reads)
    ops = {op for r in reads for op, _n in r.cigar}
    assert {"I", "D", "S", "=", "X"} <= ops
    assert any(r.flag & 0x900 for r in reads)                      # non-primary: projected, not in the histograms
    for c in calls:                                                # the order hm_fetch promises
        f, v = c[c["strand"] == 0], c[c["strand"] == 1]
        assert len(f) and len(v) and (c["strand"][:len(f)] == 0).all()
        assert (np.diff(f["qoff"]) > 0).all() and (np.diff(v["qoff"]) > 0).all()


def _sorted_records(pu):
    g, p, m, o = pu.records()
    k = np.lexsort((p, m, g, o))
    return g[k], p[k], m[k], o[k]


def _state(pu, thr, partitions=False):
    """everything the engine exposes: histograms, projected records, loci (and partition loci) after count"""
    out = dict(bins=pu.histograms(), recs=_sorted_records(pu))
    pu.count(thr)
    out["loci"] = pu.loci()
    if partitions:
        out["hap"] = [pu.loci(partition=1), pu.loci(partition=2)]
    return out


def _same(a, b):
    assert (a["bins"] == b["bins"]).all()
    assert all((x == y).all() and len(x) == len(y) for x, y in zip(a["recs"], b["recs"]))
    assert len(a["loci"]) == len(b["loci"]) and (a["loci"] == b["loci"]).all()
    for x, y in zip(a.get("hap", ()), b.get("hap", ())):
        assert len(x) == len(y) and (x == y).all()


@pytest.mark.parametrize("partitions", [False, True])
def test_calls_equal_written_and_parsed_tags(data, partitions):
    from hifimeth_amd.pileup import MethylationPileup
    rng = np.random.default_rng(5)
    hps = [int(x) for x in rng.integers(0, 3, len(data["reads"]))] if partitions else [0] * len(data["reads"])
    a, b = MethylationPileup(data["genome"], partitions=partitions), MethylationPileup(data["genome"], partitions=partitions)
    for i, (r, t, c, hp) in enumerate(zip(data["reads"], data["tagged"], data["calls"], hps)):
        assert a.add(dataclasses.replace(t, hp=hp or None)) == 1
        assert b.add_called(r, c, hp=hp) == 1
        if i % 16 == 15:                        # several runs: plane offsets restart, records accumulate
            a.flush()
            b.flush()
    a.flush()
    b.flush()
    assert a.num_records() == b.num_records() > 0
    sa, sb = _state(a, data["thr"], partitions), _state(b, data["thr"], partitions)
    _same(sa, sb)
    loci = sb["loci"]
    assert sb["bins"].sum(axis=1).min() > 0
    assert (loci["motif"] == 0).sum() >= 100 and all((loci["motif"] == m).any() for m in range(3))
    assert loci["pcov"].sum() > 0 and loci["ncov"].sum() > 0       # thresholds at the medians: both sides populated
    if partitions:
        assert all(len(h) > 0 for h in sb["hap"]) and sum(h["pcov"].sum() + h["ncov"].sum() for h in sb["hap"]) < \
            loci["pcov"].sum() + loci["ncov"].sum()
    a.close()
    b.close()


def test_mixed_batch(data):
    """one flush holds reads added with mods (even) and reads added with calls (odd)"""
    from hifimeth_amd.pileup import MethylationPileup
    genome, n = data["genome"], len(data["reads"])
    mixed, mods_only, calls_only, all_mods = (MethylationPileup(genome) for _ in range(4))
    for i in range(n):
        r, t, c = data["reads"][i], data["tagged"][i], data["calls"][i]
        all_mods.add(t, order=i)
        if i % 2 == 0:
            mixed.add(t, order=i)
            mods_only.add(t, order=i)
        else:
            mixed.add_called(r, c, order=i)
            calls_only.add_called(r, c, order=i)
    for pu in (mixed, mods_only, calls_only, all_mods):
        pu.flush()
    assert mods_only.num_records() > 0 and calls_only.num_records() > 0
    assert mixed.num_records() == mods_only.num_records() + calls_only.num_records()
    sm, s1, s2, sa = (_state(pu, data["thr"]) for pu in (mixed, mods_only, calls_only, all_mods))
    assert (sm["bins"] == s1["bins"] + s2["bins"]).all()
    both = [np.concatenate([x, y]) for x, y in zip(s1["recs"], s2["recs"])]
    k = np.lexsort((both[1], both[2], both[0], both[3]))
    assert all((x == y[k]).all() for x, y in zip(sm["recs"], both))
    dense = np.zeros((2, mixed.n_loci), np.int64)
    for s in (s1, s2):
        np.add.at(dense[0], s["loci"]["gpos"], s["loci"]["pcov"])
        np.add.at(dense[1], s["loci"]["gpos"], s["loci"]["ncov"])
    got = np.zeros_like(dense)
    got[0, sm["loci"]["gpos"]], got[1, sm["loci"]["gpos"]] = sm["loci"]["pcov"], sm["loci"]["ncov"]
    assert (got == dense).all()
    _same(sm, sa)                               # and, motif keys included, the batch where every read came with mods
    for pu in (mixed, mods_only, calls_only, all_mods):
        pu.close()


# ---- the command line ---------------------------------------------------------------------------------------------------
def _cli_input(data, tmp_path):
    """the fixture's reads + the special records, as an aligned kinetics BAM"""
    from bamutil import write_fasta
    from hifimeth_amd.synth import AlignedRead, aligned_kinetics, synth_alignments, write_aligned_kinetics_bam
    genome = data["genome"]
    reads = [dataclasses.replace(r, hp=(1, 2, None)[i % 3]) for i, r in enumerate(data["reads"])]
    short = next(r for r in synth_alignments(genome, 8, seed=23, median_len=600, frac_unmapped=0, frac_supp=0, frac_no_mods=0)
                 if 300 <= r.l_qseq < 1000)
    short = dataclasses.replace(short, name="short_own_mods", hp=1)
    stale = next(r for r in reads if r.mm is not None and not r.flag & 0x900)
    donor = next(r for r in reads if r is not stale and not r.flag & 0x900 and r.mm is not None)
    supp = dataclasses.replace(donor, name="supp_hard_clip", flag=donor.flag | 0x800, cigar=[("H", 50)] + list(donor.cigar), hp=2)
    reads = sorted(reads + [short, supp], key=lambda r: (r.tid, r.pos))
    rng = np.random.default_rng(29)
    reads.append(AlignedRead("unmapped", 4, -1, -1, 0, [], "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 1200)), None, None))
    idx = {r.name: i for i, r in enumerate(reads)}
    wide = {idx[next(r.name for r in reads if r.l_qseq >= 1000 and not r.flag & 4 and r.name not in (stale.name, supp.name))]}
    keep = {idx[short.name], idx[stale.name], idx[supp.name]}
    kin = aligned_kinetics(reads, seed=31, wide=wide)
    assert len(kin[idx[supp.name]][0]) == supp.l_qseq + 50 and len(kin[idx["unmapped"]][0]) == 1200
    assert 300 <= short.l_qseq < 1000 and short.mm and stale.l_qseq >= 1000
    bam, fa = str(tmp_path / "aligned.kinetics.bam"), str(tmp_path / "ref.fa")
    write_aligned_kinetics_bam(bam, genome, reads, kinetics=kin, keep_mods=keep)
    write_fasta(fa, genome)
    return bam, fa


def _run(args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _threshold_lines(err):
    return [x for x in err.splitlines() if x.startswith(CTX + ("Not enough",))]


def _read(prefix, names):
    return {n: open(f"{prefix}.{n}", "rb").read() for n in names}


def test_cli_identity(data, tmp_path):
    bam, fa = _cli_input(data, tmp_path)
    cov = [f"{c}.cov.bed" for c in CTX]
    hap = [f"hap{p}.{c}.cov.bed" for p in (1, 2) for c in CTX]
    asm = [f"asm.{c}.bed" for c in CTX]
    for tag, call_opts, pile_opts, names in (("all", [], [], cov),
                                             ("hap", [], ["-H", "-A", "-a", "1"], cov + hap + asm),
                                             ("cpg", ["-c", "cpg"], [], cov)):
        mod, two, one = str(tmp_path / f"{tag}.mod.bam"), str(tmp_path / f"{tag}.two"), str(tmp_path / f"{tag}.one")
        if tag != "hap":                        # (the -H run piles up the mod-BAM of the first)
            _run(["call", "-t", "4", "-T", "1", *call_opts, bam, mod])
        else:
            mod = str(tmp_path / "all.mod.bam")
        e2 = _run(["pileup", "-t", "4", *pile_opts, fa, mod, two])
        e1 = _run(["pileup", "-t", "4", "-K", "-T", "1", *call_opts, *pile_opts, fa, bam, one])
        got, want = _read(one, names), _read(two, names)
        for n in names:
            assert got[n] == want[n], (tag, n)
        assert len(_threshold_lines(e1)) == 6 and _threshold_lines(e1) == _threshold_lines(e2)
        assert "kinetics:" in e1 and "kinetics:" not in e2
        if tag == "all":
            assert want["CpG.cov.bed"].count(b"\n") >= 100 and want["CHG.cov.bed"] and want["CHH.cov.bed"]
        if tag == "hap":
            assert all(want[n] for n in hap) and any(want[n] for n in asm)
        if tag == "cpg":
            assert want["CpG.cov.bed"] and not want["CHG.cov.bed"] and not want["CHH.cov.bed"]


# ---- host-side rejections -----------------------------------------------------------------------------------------------
def test_submit_read_calls_errors():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.caller import CALL_DTYPE
    from hifimeth_amd.pileup import MethylationPileup
    L = lib()
    genome = [("c", "ACGT" * 50)]
    seq4 = np.frombuffer(bytes([0x12, 0x48] * 5), np.uint8).copy()        # ACGT x 5
    cig = np.array([(20 << 4) | 0], np.uint32)

    def calls(*rows):
        a = np.zeros(len(rows), CALL_DTYPE)
        for k, (q, s, p) in enumerate(rows):
            a[k]["qoff"], a[k]["strand"], a[k]["scaled_prob"], a[k]["read_id"] = q, s, p, 7
        return a

    def submit(pu, c, hp=0, order=0, n=None):
        return L.hm_pileup_submit_read_calls(pu._h, order, 0, 0, 0, 60, 20, seq4.ctypes.data, 1, cig.ctypes.data,
                                             len(c) if n is None else n, c.ctypes.data, hp)

    good1 = calls((1, 0, 200), (5, 0, 30), (9, 0, 250), (2, 1, 90), (6, 1, 10))
    good2 = calls((13, 0, 100), (17, 0, 220))
    dirty, clean = MethylationPileup(genome), MethylationPileup(genome)
    assert submit(dirty, good1) == 1
    for bad, code in ((calls((1, 0, 200), (5, 0, 30), (20, 0, 1)), HM_EDATA),          # past the read, after valid calls
                      (calls((-1, 0, 200)), HM_EDATA),
                      (calls((1, 0, 200), (2, 1, 30), (21, 1, 1)), HM_EDATA),
                      (calls((5, 0, 200), (1, 0, 30)), HM_EINVAL),                     # descending within FWD
                      (calls((5, 0, 200), (5, 0, 30)), HM_EINVAL),                     # not strictly increasing
                      (calls((1, 0, 200), (6, 1, 30), (2, 1, 30)), HM_EINVAL),         # descending within REV
                      (calls((2, 1, 200), (1, 0, 30)), HM_EINVAL),                     # REV before FWD
                      (calls((1, 2, 200)), HM_EINVAL)):                                # no such strand
        assert submit(dirty, bad, order=1) == code, bad
        assert L.hm_pileup_last_error(dirty._h)
    assert submit(dirty, good1, hp=1) == HM_ESTATE                                      # no partitions option
    assert submit(dirty, good1, hp=3) == HM_EINVAL
    assert submit(dirty, good1, n=0) == 0                                               # like a record without MM
    assert submit(dirty, good2, order=2) == 1
    assert submit(clean, good1) == 1 and submit(clean, good2, order=2) == 1
    dirty.flush()
    clean.flush()
    assert clean.num_records() > 0
    _same(_state(dirty, [128, 128, 128]), _state(clean, [128, 128, 128]))
    dirty.close()
    clean.close()
