#!/usr/bin/env python3
"""End-to-end rate of `hifimeth-hip pileup` (BGZF/BAM decode, MM/ML parsing, GPU projection + counting, BED text) on a
synthetic aligned mod-BAM.  usage: e2e_pileup_bench.py [genome_mb] [coverage] [threads]
--fused (anywhere on the line): the A/B of the fused path instead -- ONE synthetic aligned BAM with kinetics, `call` + `pileup` (with the
mod-BAM between them) against `pileup -K` on that file, same box, back to back, twice; checks that the BED files are identical and
prints wall times, the size of the intermediate mod-BAM the fused path never writes, and sites/s (one JSON line at the end)."""
import os, subprocess, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bamutil
from hifimeth_amd.synth import AlignedRead, revcomp

fused = "--fused" in sys.argv
argv = [a for a in sys.argv if a != "--fused"]
gmb = float(argv[1]) if len(argv) > 1 else 5
cov = float(argv[2]) if len(argv) > 2 else 10
threads = argv[3] if len(argv) > 3 else "16"
tmp = os.environ.get("TMPDIR", "/tmp")
rng = np.random.default_rng(2)
G, L = int(gmb * 1e6), 15000
chrom = np.frombuffer(b"ACGT", np.uint8)[rng.choice(4, G, p=[0.32, 0.18, 0.18, 0.32])].tobytes().decode()
genome = [("chr1", chrom)]
cli = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


def fused_leg():
    import json, re
    from hifimeth_amd.synth import write_aligned_kinetics_bam
    t = time.time()
    reads = [AlignedRead(f"r{i}", 16 if rng.random() < 0.5 else 0, 0, int(s), 60, [("=", L)], chrom[s:s + L], None, None)
             for i, s in enumerate(np.sort(rng.integers(0, G - L, int(G * cov / L))))]
    bam, fa, mod = os.path.join(tmp, "puk_in.bam"), os.path.join(tmp, "puk_ref.fa"), os.path.join(tmp, "puk_mod.bam")
    write_aligned_kinetics_bam(bam, genome, reads, threads=int(threads))
    bamutil.write_fasta(fa, genome)
    print(f"synthetic aligned kinetics BAM: {len(reads)} reads, {len(reads) * L / 1e6:.1f} Mbases, {os.path.getsize(bam) / 1e6:.1f} MB, "
          f"built in {time.time() - t:.1f} s", flush=True)

    def run(args):
        t0 = time.time()
        p = subprocess.run([cli, *args], stderr=subprocess.PIPE, text=True)
        if p.returncode:
            sys.exit(f"{' '.join(args)}: exit {p.returncode}\n{p.stderr[-2000:]}")
        return time.time() - t0, p.stderr

    res = []
    for rep in range(2):        # back to back; the second pass has the page cache and the code objects warm on both sides
        t_call, e = run(["call", "-t", threads, "-T", "1", bam, mod])
        sites = sum(int(x) for x in re.findall(r"## C\w\w samples: (\d+)", e))
        t_pile, _ = run(["pileup", "-t", threads, fa, mod, os.path.join(tmp, "puk_two")])
        t_fused, e = run(["pileup", "-K", "-T", "1", "-t", threads, fa, bam, os.path.join(tmp, "puk_one")])
        same = all(open(os.path.join(tmp, f"puk_one.{c}.cov.bed"), "rb").read() == open(os.path.join(tmp, f"puk_two.{c}.cov.bed"), "rb").read()
                   for c in ("CpG", "CHG", "CHH"))
        rows = sum(1 for c in ("CpG", "CHG", "CHH") for _ in open(os.path.join(tmp, f"puk_one.{c}.cov.bed")))
        r = dict(pass_=rep, call_s=round(t_call, 2), pileup_s=round(t_pile, 2), two_step_s=round(t_call + t_pile, 2), fused_s=round(t_fused, 2),
                 mod_bam_MB=round(os.path.getsize(mod) / 1e6, 1), sites=sites, two_step_sites_per_s=round(sites / (t_call + t_pile)),
                 fused_sites_per_s=round(sites / t_fused), bed_rows=rows, bed_identical=same)
        res.append(r)
        print(f"pass {rep}: call {t_call:.2f} s + pileup {t_pile:.2f} s = {t_call + t_pile:.2f} s ({r['two_step_sites_per_s'] / 1e6:.1f} M sites/s, "
              f"mod-BAM {r['mod_bam_MB']} MB) | pileup -K {t_fused:.2f} s ({r['fused_sites_per_s'] / 1e6:.1f} M sites/s) | {rows} BED rows, "
              f"identical: {same}", flush=True)
        for l in e.splitlines():
            if "##" in l:
                print("   ", l.strip())
    print(json.dumps(dict(bench="pileup_fused_ab", genome_mb=gmb, coverage=cov, threads=int(threads), input_MB=round(os.path.getsize(bam) / 1e6, 1),
                          passes=res)))
    if not all(r["bed_identical"] for r in res):
        sys.exit("pileup -K and call + pileup wrote different BED files")


if fused:
    fused_leg()
    sys.exit(0)
t = time.time()
reads = []
for i, s in enumerate(np.sort(rng.integers(0, G - L, int(G * cov / L)))):
    seq = chrom[s:s + L]
    rev = bool(rng.random() < 0.5)
    fwd = np.frombuffer((revcomp(seq) if rev else seq).encode(), np.uint8)
    parts, mls = [], []
    for base, head in ((67, "C+m"), (71, "G-m")):          # every C / G called: an upper bound on the tag volume
        n = int((fwd == base).sum())
        parts.append(head + ",0" * n + ";")
        mls.append(np.where(rng.random(n) < 0.5, rng.integers(0, 60, n), rng.integers(196, 256, n)).astype(np.uint8))
    reads.append(AlignedRead(f"r{i}", 16 if rev else 0, 0, int(s), 60, [("=", L)], seq, "".join(parts), np.concatenate(mls)))
bam, fa, prefix = os.path.join(tmp, "pu_in.bam"), os.path.join(tmp, "pu_ref.fa"), os.path.join(tmp, "pu_out")
bamutil.aligned_to_bam(bam, genome, reads, level=1)
bamutil.write_fasta(fa, genome)
print(f"synthetic mod-BAM: {len(reads)} reads, {len(reads) * L / 1e6:.1f} Mbases aligned, {os.path.getsize(bam) / 1e6:.1f} MB, "
      f"built in {time.time() - t:.1f} s", flush=True)
for b in ("512", "4096"):
    t = time.time()
    p = subprocess.run([cli, "pileup", "-t", threads, "-b", b, fa, bam, prefix], stderr=subprocess.PIPE, text=True)
    dt = time.time() - t
    rows = sum(1 for c in ("CpG", "CHG", "CHH") for _ in open(f"{prefix}.{c}.cov.bed"))
    print(f"-b {b}: exit {p.returncode}, {dt:.2f} s wall, {len(reads) * L / dt / 1e6:.1f} M aligned bases/s, {rows} BED rows", flush=True)
    for l in p.stderr.splitlines():
        if "##" in l:
            print("   ", l.strip())
