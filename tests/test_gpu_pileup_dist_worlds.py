"""`python -m hifimeth_amd.pileup_dist` on three, five and eight gloo ranks sharing the card, with every output the driver has at once,
against the files of the C++ CLI over the same input (tests/dist_cases.py): a middle rank with neighbours on both sides, a -D
segment, a -G region and a -R interval over whole chunks, a padded tail, chunks inside one sequence and over three, empty "big"
lists in the middle of the rank order, ranks that are dealt no record, and the agreement on an error that only a middle rank sees.
No tolerance anywhere: every comparison is byte equality of files."""
import os
import subprocess
import sys

import pytest

import dist_cases as D
from conftest import ROOT
from test_dist_gloo import _free_port

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
CTX = ("CpG", "CHG", "CHH")
CLI_ONLY = frozenset()             # the files only the CLI writes under these options: none
# what the option list must give: the plain and the per-haplotype tables, and the outputs of -A -Q -G, -B, -D -Y, -L, -P
NAMES = {f"{t}{kind}.{c}.{ext}" for t in ("", "hap1.", "hap2.") for kind, ext in (("regions", "tsv"), ("metaplot", "tsv"), ("context", "tsv"))
         for c in CTX} | {f"{t}{c}.cov.bed" for t in ("", "hap1.", "hap2.") for c in CTX} \
    | {f"{kind}.{c}.bed" for kind in ("asm", "asm.regions", "sites", "domains") for c in CTX} \
    | {"asm.summary.tsv", "sites.rates.tsv", "domains.fit.tsv", "linkage.CpG.tsv", "readpos.tsv"}


def _files(prefix):
    d, b = os.path.dirname(prefix), os.path.basename(prefix) + "."
    return {n[len(b):]: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.startswith(b)}


def _dist_env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HM_FORCE_COLLECTIVES"):
        env.pop(k, None)
    env.update(kw)
    return env


def _launch(world, args, slab, fa, bam, prefix):
    """`world` gloo ranks sharing the card -> (return codes, stderr texts), in rank order"""
    mod = [sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "--slab", str(slab), "--backend", "gloo"]
    port = str(_free_port())
    procs = [subprocess.Popen([*mod, fa, bam, prefix], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=_dist_env(RANK=str(k), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=port))
             for k in range(world)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return [p.returncode for p in procs], [e for _o, e in outs]


def _cli(args):
    r = subprocess.run([CLI, "pileup", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.fixture(scope="module")
def on_disk(tmp_path_factory):
    """the FASTA, the BAM and the BED file, and the CLI's files of the option list: the expectation of every world"""
    from bamutil import write_fasta
    from test_gpu_pileup_hp import _write_bam
    d = tmp_path_factory.mktemp("worlds")
    fa, bam, bed = str(d / "ref.fa"), str(d / "in.bam"), str(d / "iv.bed")
    write_fasta(fa, D.genome())
    _write_bam(bam, D.genome(), D.reads(), D.hp_tags(D.reads()))
    D.write_bed(bed)
    _cli([*D.options(bed), "-b", "20", fa, bam, str(d / "cli")])
    return dict(dir=d, fa=fa, bam=bam, bed=bed, want=_files(str(d / "cli")))


def test_the_cli_writes_every_file_and_the_oracles_counts(on_disk):
    """the expectation is anchored outside the two front ends: the nine *.cov.bed are the CPU oracle's text"""
    want = on_disk["want"]
    assert set(want) == NAMES | CLI_ONLY
    ref = D.reference()
    for tag, text in ref["bed"].items():
        for c in CTX:
            assert want[f"{tag}{c}.cov.bed"].decode() == text[c] and text[c], (tag, c)
    assert all(want[n] for n in NAMES if not n.startswith("asm.regions.CH"))          # no file is empty (regions are asked of CpG)


def test_the_clis_files_hold_the_cases(on_disk):
    """what test_dist_cases_cpu.py asserts of the references, on the expectation itself: a -D H segment and a -G region over a
    whole chunk of every world, and big -B loci on two ranks of eight with ranks between them that have none"""
    from hifimeth_amd.pileup import locus_ranges
    want, off = on_disk["want"], {n: int(o) for n, o in zip(D.NAMES, D.offsets())}
    rows = lambda name: [f.split("\t") for f in want[name].decode().splitlines()]  # noqa: E731
    high = [(off[f[0]] + int(f[1]), off[f[0]] + int(f[2])) for c in CTX for f in rows(f"domains.{c}.bed") if f[4] == "H"]
    regs = [(off[f[0]] + int(f[1]), off[f[0]] + int(f[2])) for c in CTX for f in rows(f"asm.regions.{c}.bed")]
    for world in D.WORLDS:
        ranges = locus_ranges(D.N_LOCI, world)
        for what in (high, regs):
            assert any(a <= lo and hi <= b for a, b in what for lo, hi in ranges if lo < hi), world
    chunk = locus_ranges(D.N_LOCI, 8)[0][1]
    deep = sorted({(off[f[0]] + int(f[1])) // chunk for c in CTX for f in rows(f"{c}.cov.bed") if int(f[4]) + int(f[5]) >= 256})
    assert len(deep) == 2 and deep[1] - deep[0] >= 3


@pytest.mark.parametrize("world", D.WORLDS)
def test_every_file_of_a_world_equals_the_clis(on_disk, world):
    from hifimeth_amd.bamio import read_bam
    prefix = str(on_disk["dir"] / f"w{world}")
    records = list(read_bam(on_disk["bam"])[2])
    slab = D.slab(world, len(records))
    staged = [sum(1 for i, r in enumerate(records) if (i // slab) % world == k and not r.flag & 4 and r.mm is not None) for k in range(world)]
    assert sum(staged) == len(D.reads())
    assert all(staged) if world < 8 else (all(staged[:5]) and staged[5:] == [0, 0, 0])    # eight: the ranks 5 .. 7 stage no record
    codes, errs = _launch(world, D.options(on_disk["bed"]), slab, on_disk["fa"], on_disk["bam"], prefix)
    assert codes == [0] * world, [e[-2000:] for e in errs]
    got, want = _files(prefix), on_disk["want"]
    assert set(got) == set(want) - CLI_ONLY
    assert [n for n in sorted(got) if got[n] != want[n]] == []


def test_eight_ranks_with_contexts_left_out(on_disk):
    """-e with a nan rate and -u with a nan pair: CHG is neither tested nor segmented, so every rank's pieces skip a context"""
    d = on_disk["dir"]
    _cli([*D.NAN_OPTIONS, "-b", "20", on_disk["fa"], on_disk["bam"], str(d / "nan_cli")])
    want = _files(str(d / "nan_cli"))
    assert want["domains.CpG.bed"] and want["domains.CHH.bed"] and not want.get("domains.CHG.bed")
    assert want["sites.CpG.bed"] and want["sites.CHH.bed"] and not want.get("sites.CHG.bed")
    codes, errs = _launch(8, D.NAN_OPTIONS, D.slab(8, len(D.reads())), on_disk["fa"], on_disk["bam"], str(d / "nan8"))
    assert codes == [0] * 8, [e[-2000:] for e in errs]
    got = _files(str(d / "nan8"))
    assert set(got) == set(want) - CLI_ONLY
    assert [n for n in sorted(got) if got[n] != want[n]] == []


def test_three_ranks_agree_on_a_middle_ranks_error(on_disk, tmp_path):
    """a record on a sequence the FASTA lacks, in a slab of rank 1: all three leave with status 1, rank 1 says why, nothing is written"""
    from test_gpu_pileup_hp import _write_bam
    g, rs, name = D.ghost()
    bam = str(tmp_path / "ghost.bam")
    _write_bam(bam, g, rs, D.hp_tags(rs))
    codes, errs = _launch(3, D.options(on_disk["bed"]), D.SMALL_SLAB, on_disk["fa"], bam, str(tmp_path / "out"))
    assert codes == [1, 1, 1], [e[-2000:] for e in errs]
    assert f"Sequence name {name} does not exist" in errs[1] and "does not exist" not in errs[0] + errs[2]
    assert not [n for n in os.listdir(tmp_path) if n.endswith((".bed", ".tsv"))]
