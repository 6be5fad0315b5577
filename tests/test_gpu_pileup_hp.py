"""Haplotype-resolved `pileup` (-H): records tagged HP 1 / 2 are also counted into per-haplotype planes with the combined
thresholds, and <prefix>.hap1.* / <prefix>.hap2.* list each locus in its combined context.  The expectation is built from the
CPU oracle (oracle/pileup_oracle.py): thresholds and motifs of `pileup` over all records, partition counts from
`read_contribution` over the records of that haplotype, text from `bed_text`."""
import ctypes
import dataclasses
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
CTX = ("CpG", "CHG", "CHH")
_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}


@pytest.fixture(scope="module")
def P():
    from oracle import pileup_oracle
    return pileup_oracle


def _as_dict(r):
    return dict(flag=r.flag, tid=r.tid, pos=r.pos, mapq=r.mapq, cigar=r.cigar, seq=r.seq, mm=r.mm, ml=r.ml)


def _partition(tags):
    """partition of a record from its HP fields [(type, value)] in aux order: the first one, integer-typed, value 1 or 2"""
    if not tags:
        return 0
    t, v = tags[0]
    return v if t in _FMT and v in (1, 2) else 0


def _hp_aux(tags):
    out = b""
    for t, v in tags:
        out += b"HP" + t.encode() + (str(v).encode() + b"\0" if t == "Z" else struct.pack("<" + _FMT[t], v))
    return out


def _write_bam(path, genome, reads, hp_tags):
    """bamutil.aligned_to_bam with HP fields behind MM / ML / MN (hp_tags[i]: [(type, value)] of read i)"""
    from bamutil import aux_B, aux_i, aux_Z, write_bgzf
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{len(s)}\n" for n, s in genome)
    parts = [b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(genome))]
    for n, s in genome:
        nm = n.encode() + b"\0"
        parts.append(struct.pack("<I", len(nm)) + nm + struct.pack("<I", len(s)))
    for r, tags in zip(reads, hp_tags):
        aux = aux_Z("RG", "rg0")
        if r.mm is not None:
            aux += aux_Z("MM", r.mm) + aux_B("ML", np.asarray(r.ml, np.uint8)) + aux_i("MN", r.l_qseq)
        aux += _hp_aux(tags)
        qn = r.name.encode() + b"\0"
        cig = r.cigar_u32()
        core = struct.pack("<iiBBHHHiiii", r.tid, r.pos, len(qn), r.mapq, 4680, len(cig), r.flag, r.l_qseq, -1, -1, 0)
        body = core + qn + cig.astype("<u4").tobytes() + bytes(r.seq4) + b"\xff" * r.l_qseq + aux
        parts.append(struct.pack("<I", len(body)) + body)
    write_bgzf(path, b"".join(parts))


def _expect(P, genome, reads, parts, min_mapq=0, min_pi=0.0):
    """-> (combined oracle result, {1: (loci, bed), 2: (loci, bed)}); loci = [(sid, soff, pcov, ncov, motif)]"""
    recs = [_as_dict(r) for r in reads]
    comb = P.pileup(recs, genome, min_mapq=min_mapq, min_pi=min_pi)
    thr = comb["thresholds"]
    motif = {(sid, soff): m for sid, soff, _p, _n, m in comb["loci"]}
    out = {}
    for part in (1, 2):
        cov = {}
        for rec, hp in zip(recs, parts):
            if hp != part:
                continue
            for sid, soff, prob, m in P.read_contribution(rec, genome, min_mapq, min_pi)[1]:
                e = cov.setdefault((sid, soff), [0, 0])
                e[0 if prob >= thr[m] else 1] += 1
        loci = sorted((sid, soff, p, n, motif[(sid, soff)]) for (sid, soff), (p, n) in cov.items())
        out[part] = (loci, P.bed_text([(genome[sid][0], soff, p, n, m) for sid, soff, p, n, m in loci]))
    return comb, out


def _rows(pu, loci):
    return [(int(l["gpos"]), int(l["pcov"]), int(l["ncov"]), int(l["motif"])) for l in loci]


def _oracle_rows(pu, loci):
    return [(int(pu.offsets[sid] + soff), p, n, m) for sid, soff, p, n, m in loci]


def _engine(genome, reads, batch=16, **kw):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(genome, **kw)
    for i, r in enumerate(reads):
        pu.add(r)
        if (i + 1) % batch == 0:
            pu.flush()                    # several batches: records carrying hp accumulate in HBM across runs
    pu.flush()
    pu.count(pu.resolve_thresholds(pu.histograms()))
    return pu


def _tagged_reads(n, seed, median_len=1500, length=12000):
    """synth_alignments reads with hp drawn from {None, 1, 2, 3} and extra secondary / supplementary flags"""
    from hifimeth_amd.synth import synth_alignments, synth_genome
    genome = synth_genome(n_chr=3, length=length, seed=seed)
    reads = synth_alignments(genome, n, seed=seed + 1, median_len=median_len)
    rng = np.random.default_rng(seed + 2)
    out = []
    for r in reads:
        hp = [None, 1, 2, 3][int(rng.integers(0, 4))]
        flag = r.flag
        if not flag & 4 and rng.random() < 0.1:
            flag |= 0x100 if rng.random() < 0.5 else 0x800
        out.append(dataclasses.replace(r, hp=hp, flag=flag))
    return genome, out


def test_partitions_python_api(P):
    genome, reads = _tagged_reads(70, seed=41)
    assert {r.hp for r in reads} == {None, 1, 2, 3}
    assert any(r.flag & 0x100 for r in reads) and any(r.flag & 0x800 for r in reads)
    assert any(r.flag & 16 for r in reads) and any(not r.flag & 16 for r in reads)
    parts = [r.hp if r.hp in (1, 2) else 0 for r in reads]
    comb, want = _expect(P, genome, reads, parts)
    plain = _engine(genome, reads)
    pu = _engine(genome, reads, partitions=True)
    loci = pu.loci()
    assert (loci == plain.loci()).all()                        # the combined output does not see the partitions
    assert _rows(pu, loci) == _oracle_rows(pu, comb["loci"])
    assert pu.bed(loci) == comb["bed"]
    total = np.zeros((len(loci), 2), np.int64)
    for part in (1, 2):
        got = pu.loci(partition=part)
        assert len(got) > 100
        assert _rows(pu, got) == _oracle_rows(pu, want[part][0])
        assert pu.bed(got) == want[part][1]
        # per sequence, as the CLI fetches them
        per_seq = [pu.loci(int(pu.offsets[s]), int(pu.offsets[s + 1]), partition=part) for s in range(len(genome))]
        assert (np.concatenate(per_seq) == got).all()
        j = np.searchsorted(loci["gpos"], got["gpos"])
        assert (loci["gpos"][j] == got["gpos"]).all()
        total[j, 0] += got["pcov"]
        total[j, 1] += got["ncov"]
    assert (total[:, 0] <= loci["pcov"]).all() and (total[:, 1] <= loci["ncov"]).all()
    assert (total[:, 0] + total[:, 1] < loci["pcov"] + loci["ncov"]).any()     # untagged / HP 3 reads count only combined
    plain.close()
    pu.close()


def _cli_reads(seed=61, n=80):
    """reads + their HP fields in every integer type, HP:Z, two HP fields (the first decides) and none"""
    from hifimeth_amd.synth import synth_alignments, synth_genome
    genome = synth_genome(n_chr=3, length=12000, seed=seed)
    reads = synth_alignments(genome, n, seed=seed + 1)
    kinds = [[("c", 1)], [("C", 2)], [("s", 1)], [("S", 2)], [("i", 1)], [("I", 2)], [("i", 3)], [("Z", "1")], [],
             [("c", 2), ("i", 1)], [("Z", "2"), ("i", 2)], [("C", 0)]]
    tags = [kinds[i % len(kinds)] for i in range(len(reads))]
    return genome, reads, tags


def _run_cli(args):
    r = subprocess.run([CLI, "pileup", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def _files(prefix, haps=True):
    tags = ["", "hap1.", "hap2."] if haps else [""]
    return {t + c: open(f"{prefix}.{t}{c}.cov.bed").read() for t in tags for c in CTX}


def test_cli_haplotypes(P, tmp_path):
    from bamutil import write_fasta
    genome, reads, tags = _cli_reads()
    parts = [_partition(t) for t in tags]
    assert set(parts) == {0, 1, 2}
    bam, fa, prefix = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "out")
    _write_bam(bam, genome, reads, tags)
    write_fasta(fa, genome)
    for kw, args in ((dict(), ["-t", "4", "-b", "25"]), (dict(min_mapq=20, min_pi=98.5), ["-q", "20", "-f", "98.5"])):
        tag = "q" if kw else "a"
        r0 = _run_cli([*args, fa, bam, prefix + tag + "0"])
        r1 = _run_cli([*args, "-H", fa, bam, prefix + tag + "1"])
        plain, haps = _files(prefix + tag + "0", haps=False), _files(prefix + tag + "1")
        comb, want = _expect(P, genome, reads, parts, **kw)
        for c in CTX:
            assert haps[c] == plain[c] == comb["bed"][c]
            for part in (1, 2):
                assert haps[f"hap{part}.{c}"] == want[part][1][c], (part, c)
        assert sum(len(want[p][0]) for p in (1, 2)) > 100
        # one set of thresholds: the same stderr lines, one more parameter line
        lines = lambda e: [x for x in e.splitlines() if x.startswith(CTX + ("Not enough",))]  # noqa: E731
        assert len(lines(r0.stderr)) == 6 and lines(r0.stderr) == lines(r1.stderr)
        assert "haplotypes:" in r1.stderr and "haplotypes:" not in r0.stderr
        assert not os.path.exists(f"{prefix}{tag}0.hap1.CpG.cov.bed")
    # no HP anywhere: six empty partition files
    _write_bam(bam, genome, reads, [[] for _ in reads])
    _run_cli(["-H", fa, bam, prefix + "n"])
    got = _files(prefix + "n")
    assert all(got[f"hap{p}.{c}"] == "" for p in (1, 2) for c in CTX)
    assert {c: got[c] for c in CTX} == _files(prefix + "a0", haps=False)


def test_thresholds_shared_across_partitions(P, tmp_path):
    """a dataset whose combined histograms resolve real thresholds: the partitions use them, not their own"""
    from bamutil import write_fasta
    from hifimeth_amd.synth import synth_alignments, synth_genome
    genome = synth_genome(n_chr=2, length=60000, seed=71)
    reads = synth_alignments(genome, 600, seed=72, median_len=3000)
    rng = np.random.default_rng(73)
    tags = [[("i", int(v))] if v else [] for v in rng.integers(0, 3, len(reads))]
    parts = [_partition(t) for t in tags]
    recs = [_as_dict(r) for r in reads]
    bins = {k: np.zeros((3, 256), np.uint64) for k in (0, 1, 2)}      # 0 = all records
    for rec, part in zip(recs, parts):
        for c, p in P.read_contribution(rec, genome)[0]:
            bins[0][c, p] += 1
            if part:
                bins[part][c, p] += 1
    thr = {k: [P.resolve_threshold(bins[k][c])[0] for c in range(3)] for k in bins}
    assert any(t != 128 for t in thr[0]), thr
    assert thr[1] != thr[0] or thr[2] != thr[0], thr
    bam, fa, prefix = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "out")
    _write_bam(bam, genome, reads, tags)
    write_fasta(fa, genome)
    r = _run_cli(["-H", fa, bam, prefix])
    for c in range(3):
        if thr[0][c] != 128:
            assert f"{CTX[c]} scaled probability threshold: {thr[0][c]}" in r.stderr
    comb, want = _expect(P, genome, reads, parts)
    assert comb["thresholds"] == thr[0]
    got = _files(prefix)
    for c in CTX:
        assert got[c] == comb["bed"][c]
        for part in (1, 2):
            assert got[f"hap{part}.{c}"] == want[part][1][c], (part, c)


def _dist_env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HM_FORCE_COLLECTIVES"):
        env.pop(k, None)
    env.update(kw)
    return env


def test_pileup_dist_haplotypes(tmp_path):
    """python -m hifimeth_amd.pileup_dist -H: a world of one (plain, and over RCCL), and two gloo ranks sharing the card --
    all nine files identical to the CLI's"""
    from bamutil import write_fasta
    genome, reads, tags = _cli_reads(seed=81, n=60)
    bam, fa = str(tmp_path / "mod.bam"), str(tmp_path / "ref.fa")
    _write_bam(bam, genome, reads, tags)
    write_fasta(fa, genome)
    _run_cli(["-H", fa, bam, str(tmp_path / "cli")])
    want = _files(str(tmp_path / "cli"))
    assert all(want[f"hap{p}.{c}"] for p in (1, 2) for c in CTX)
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", "-H", "--slab", "7"]
    for name, env in (("one", _dist_env()),
                      ("rccl", _dist_env(HM_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29571"))):
        prefix = str(tmp_path / name)
        r = subprocess.run([*mod, fa, bam, prefix], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert _files(prefix) == want, name
    prefix = str(tmp_path / "gloo")
    procs = [subprocess.Popen([*mod, "--backend", "gloo", fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                                            MASTER_PORT="29573"))
             for k in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], [e[-2000:] for _o, e in outs]
    assert _files(prefix) == want


def test_partition_abi_errors():
    import torch
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import MOD_DTYPE, MethylationPileup
    HM_EINVAL, HM_ESTATE = -1, -5
    L = lib()
    genome = [("c", "ACGT" * 50)]
    mods = np.zeros(1, MOD_DTYPE)
    mods["unmod_base"], mods["code"], mods["prob"] = b"C", b"m", 200
    seq4 = np.frombuffer(bytes([0x12, 0x48] * 5), np.uint8).copy()      # ACGT x 5
    cig = np.array([(20 << 4) | 0], np.uint32)

    def submit(pu, hp):
        return L.hm_pileup_submit_read_hp(pu._h, 0, 0, 0, 0, 60, 20, seq4.ctypes.data, 1, cig.ctypes.data, 1,
                                          mods.ctypes.data, hp)

    plain = MethylationPileup(genome)
    assert L.hm_pileup_set_option(plain._h, b"partitions", 2.0) == HM_ESTATE       # after the reference
    assert submit(plain, 3) == HM_EINVAL
    assert submit(plain, -1) == HM_EINVAL
    assert submit(plain, 1) == HM_ESTATE
    assert submit(plain, 0) == 1
    pc, nc = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.hm_pileup_partition_planes(plain._h, 1, None, None) == HM_ESTATE
    assert L.hm_pileup_use_partition_planes(plain._h, 1, pc.data_ptr(), nc.data_ptr()) == HM_ESTATE
    plain.close()

    hp = MethylationPileup(genome, partitions=True)
    assert submit(hp, 3) == HM_EINVAL
    assert submit(hp, 2) == 1 and submit(hp, 1) == 1 and submit(hp, 0) == 1
    assert L.hm_pileup_partition_planes(hp._h, 3, None, None) == HM_EINVAL
    assert L.hm_pileup_partition_planes(hp._h, 0, None, None) == HM_EINVAL
    assert L.hm_pileup_set_option(hp._h, b"partitions", 0.0) == HM_ESTATE
    hp.close()

    # "partitions" accepts 0 or 2 only, and only before hm_pileup_use_planes as well
    planes = [torch.zeros(200, dtype=torch.int32, device="cuda") for _ in range(3)]
    h = ctypes.c_void_p()
    assert L.hm_pileup_create(ctypes.byref(h), 0) == 0
    assert L.hm_pileup_set_option(h, b"partitions", 3.0) == HM_EINVAL
    assert L.hm_pileup_use_planes(h, *(t.data_ptr() for t in planes)) == 0
    assert L.hm_pileup_set_option(h, b"partitions", 2.0) == HM_ESTATE
    L.hm_pileup_destroy(h)
