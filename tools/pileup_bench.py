#!/usr/bin/env python3
"""Throughput of the `pileup` device path on one GPU, synthetic data.

A random genome, error-free reads (one '=' CIGAR op each, both strands) with call-like MM/ML tags; the MM/ML lists are
parsed once on the host and the staged batches are replayed, so the timed region is what the GPU does per batch:
H2D of the staged records, plane memset, entries_kernel, project_kernel, then count_kernel and the covered-loci
compaction at the end.  Prints one JSON object; `--check` verifies that the per-locus counters add up to the number of projected calls.
`--partitions`: the haplotype-resolved engine (`pileup -H`), every read tagged with a random HP of {none, 1, 2}; the loci
fetch then also compacts the two partitions' planes.
`--asm` (with `--partitions`): the allele-specific test of `pileup -H -A` over the counted planes: select + Fisher test + D2H per pass.
`--asm-q` (with `--asm`): the q-values of `pileup -H -A -Q`: histogram + bin p-values + table (host) + rows with q (D2H included) per pass.
`--asm-regions` (with `--asm`): the regions of `pileup -H -A -G`: per context, select + test + chain + D2H of the region rows per pass.
`--sites`: the binomial test of `pileup -B / -e` over the counted planes: histogram + table + rows (D2H included) per pass.
`--domains`: the segmentation of `pileup -D` over the counted planes: per context, select + two scans + heads + D2H of the segments per pass.
`--fit` (with `--domains`): one state-sums pass (`pileup -D -Y`: select + two scans + one reduction, 48 bytes back) next to one fetch of the
segments over the same planes, and the fit of the three contexts from the default levels: iterations, status, seconds.
`--patterns K`: the read-level CpG patterns of `pileup -E K`: the timed passes run on an engine without the option first and then on one
with it; the leg is what the option adds to projection and counting plus one fetch of the rows (D2H included): window records per second,
rows, share of a pass.
`--linkage D`: the within-read co-methylation by distance of `pileup -L D`, timed like `--patterns`: the leg is what the option adds to
a pass (the member list through the selection skeleton -- one 8-byte count copy per batch -- and the pair kernel) plus one fetch of
all rows (reduce per distance, LinkSel, D2H): pairs per second, rows, share of a pass.
`--readpos D`: methylation by position in the read of `pileup -P D`, timed like `--patterns`: the leg is what the profiling variant of the
projection adds to a pass (an LDS atomic per interior record, a global one per end record, one flush per workgroup) plus one fetch of all
rows (reduce per row, ReadPosSel, D2H): records per second, rows, share of a pass.
`--bedmethyl`: the depth classes of `pileup -M`, timed like `--patterns`: the passes on an engine without the option, then on one with
it; the leg is what the option adds to projection and counting plus one fetch of the rows (D2H included).  The synthetic reads are
error-free: the column kernel and the record count run at full size, the deletion kernel has nothing to do.
`--digest`: a sha256 of every output that must not depend on the build -- the records of one pass (sorted by order, gpos, motif: the
append order is not fixed), the loci of the combined set and of each partition, and the rows of `--patterns`, `--bedmethyl` (each set)
and `--linkage` -- under "digest" in the JSON object, for comparing two builds of the library (HM_LIB_PATH) byte for byte.
`--load`: the loader of `diff` (hm_pileup_load_loci) on an engine of its own behind the main run: 2^24 rows on distinct loci of a
reference of 2^28 bases, part 1 in ascending order (a *.cov.bed file's) and part 2 shuffled, whole calls -- the H2D of 24 bytes per row
from pageable memory slab by slab, the kernel, the counters' download -- in rows per second, beside the main run's `records_per_s_count`
(count_kernel over its resident 12-byte records: no H2D, one or two atomic adds and an atomic max per record) as the yardstick.
`--parts N` (with `--domains`): the same segments chained from N equal pieces next to the single fetch (three stateless passes per piece).

    python tools/pileup_bench.py --genome-mb 20 --coverage 10 [--partitions [--asm [--asm-q] [--asm-regions]]] [--sites] [--domains [--fit] [--parts N]] [--patterns K] [--bedmethyl] [--linkage D] [--readpos D] [--load]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from hifimeth_amd.pileup import MOD_DTYPE, MethylationPileup  # noqa: E402
from hifimeth_amd.synth import pack_codes  # noqa: E402

_ASCII = np.frombuffer(b"ACGT", np.uint8)
_COMP = np.zeros(256, np.uint8)
_COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]


def call_like_mods(fwd: np.ndarray, rng) -> np.ndarray:
    """C+m on CpG/CHG/CHH cytosines, G-m on the G of [AGT][AGT]G (what `hifimeth call` writes), already parsed"""
    L = len(fwd)
    C_, G_ = 67, 71
    n1 = np.concatenate([fwd[1:], [0]])
    n2 = np.concatenate([fwd[2:], [0, 0]])
    p1 = np.concatenate([[0], fwd[:-1]])
    p2 = np.concatenate([[0, 0], fwd[:-2]])
    isH = lambda x: (x == 65) | (x == 67) | (x == 84)  # noqa: E731
    isD = lambda x: (x == 65) | (x == 71) | (x == 84)  # noqa: E731
    fc = np.nonzero((fwd == C_) & ((n1 == G_) | (isH(n1) & ((n2 == G_) | isH(n2)))))[0]
    rg = np.nonzero((fwd == G_) & isD(p1) & isD(p2) & (np.arange(L) >= 2))[0]
    m = np.zeros(len(fc) + len(rg), MOD_DTYPE)
    m["qoff"] = np.concatenate([fc, rg])
    m["strand"][len(fc):] = 1
    m["unmod_base"][:len(fc)] = b"C"
    m["unmod_base"][len(fc):] = b"G"
    m["code"] = b"m"
    m["prob"] = np.where(rng.random(len(m)) < 0.5, rng.integers(0, 60, len(m)), rng.integers(196, 256, len(m)))
    return m


def cpu_baseline(genome, chrom, starts, staged, read_len, n_sample=600, repeat=12):
    """The reference's BamQuerySequence::init + BamMapInfo::init + extract_{cpg,chg,chh}_mapped_samples
    (src/corelib/bam_info.cpp:169-439, 5mc_motif_finder.cpp), built from its sources by oracle/ref_build, one thread."""
    import subprocess
    import tempfile
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "_ref", "ref_align")
    if not os.path.exists(exe):
        return None
    n = min(n_sample, len(staged))
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "g.fa")
        with open(fa, "w") as f:
            f.write(">chr1\n" + genome[0][1] + "\n")
        recs = "".join(f"{staged[i][0]} 0 {int(starts[i])} {read_len}= {chrom[int(starts[i]):int(starts[i]) + read_len].tobytes().decode()}\n"
                       for i in range(n))
        r = subprocess.run([exe, "-t", str(repeat), fa], input=recs.encode(), capture_output=True, check=True)
    t = r.stdout.decode().split()
    cols, secs = int(t[4]), float(t[-1])
    return dict(value=round(cols / secs), unit="aligned columns/s", cores=1, kind="reference",
                sample=f"{n} reads x {repeat} passes = {cols} columns through the reference's alignment projection "
                       f"(ref_align -t), {secs:.1f} s")


def context_leg(log2_loci, repeat, check):
    """`pileup -S`: hm_pileup_fetch_context over planes of 2^log2_loci loci, about 5 % of them covered, for flank 0 .. 3 and each
    accumulation path that exists for the flank, next to the yardstick: one hm_pileup_fetch_regions call of one interval, whose
    region_block_sums_kernel streams the same pcov / ncov / key and adds neither reference reads nor atomics.  Times are whole
    calls (memset of the device table, the kernel, the table's download); the kernels' own times come from a run of this leg
    under a kernel trace (context_kernel<flank, lds> against region_block_sums_kernel)."""
    import torch
    from hifimeth_amd.pileup import CONTEXT_PATH_GLOBAL, CONTEXT_PATH_LDS, context_geometry
    n = 1 << log2_loci
    rng = np.random.default_rng(3)
    bases = _ASCII[rng.integers(0, 4, n, dtype=np.uint8)]
    pu = MethylationPileup([("chr1", n)], bases=bases)
    gen = torch.Generator(device="cuda").manual_seed(5)
    on = torch.rand(n, device="cuda", generator=gen) < 0.05
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    pc = torch.where(on, torch.randint(0, 30, (n,), dtype=torch.int32, device="cuda", generator=gen), zero)
    nc = torch.where(on, torch.randint(0, 30, (n,), dtype=torch.int32, device="cuda", generator=gen), zero)
    ky = torch.randint(0, 3, (n,), dtype=torch.int32, device="cuda", generator=gen)
    del on, zero
    torch.cuda.synchronize()
    planes = (pc, nc, ky)
    span, lds_flank, lds_max = context_geometry()
    legs = {"regions_index": lambda: pu.regions([0], [1], planes=planes, hi=n)}
    for f in range(4):
        for name, path in (("lds", CONTEXT_PATH_LDS), ("global", CONTEXT_PATH_GLOBAL)):
            if path == CONTEXT_PATH_GLOBAL or f <= lds_max:
                legs[f"flank{f}_{name}"] = lambda f=f, path=path: pu.context(f, planes=planes, hi=n, path=path)
    times = {k: [] for k in legs}
    for leg in legs.values():
        leg()                                      # warm-up: the buffers, the code objects
    for _ in range(max(repeat, 5)):                # the legs alternate, so that a drift of the machine falls on all of them
        for k, leg in legs.items():
            t0 = time.perf_counter()
            leg()
            times[k].append(time.perf_counter() - t0)
    best = {k: min(v) for k, v in times.items()}
    out = dict(context_loci=n, context_covered=round(float(((pc + nc) > 0).float().mean()), 4), context_span=span,
               context_lds_flank=lds_flank, context_call_s={k: [round(x, 5) for x in v] for k, v in times.items()},
               context_call_ratio_to_regions_index={k: round(v / best["regions_index"], 3) for k, v in best.items()},
               context_table_bytes={f"flank{f}": 3 * (4 ** (3 + 2 * f) + 1) * 32 for f in range(4)})
    if check:                                      # both paths give one table, and it holds every counted locus
        same = all((pu.context(f, planes=planes, hi=n, path=CONTEXT_PATH_LDS) == pu.context(f, planes=planes, hi=n, path=CONTEXT_PATH_GLOBAL)).all()
                   for f in range(lds_max + 1))
        counted = int(((pc + nc) > 0).sum())
        out["check_context_paths_agree"] = bool(same)
        out["check_context_holds_the_loci"] = all(int(pu.context(f, planes=planes, hi=n)[:, :, 0].sum()) == counted for f in range(4))
    pu.close()
    print(json.dumps(out))


def load_leg(check):
    """`diff`: hm_pileup_load_loci of LOAD_ROWS rows into a reference of LOAD_BASES bases -> the leg's entries of the JSON object"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    LOAD_BASES, LOAD_ROWS = 1 << 28, 1 << 24
    rng = np.random.default_rng(11)
    step = LOAD_BASES // LOAD_ROWS
    rows = np.zeros(LOAD_ROWS, LOCUS_DTYPE)
    rows["gpos"] = np.arange(LOAD_ROWS, dtype=np.int64) * step + rng.integers(0, step, LOAD_ROWS)   # distinct and ascending
    rows["pcov"], rows["ncov"] = rng.integers(1, 30, LOAD_ROWS), rng.integers(0, 30, LOAD_ROWS)
    rows["motif"] = rng.integers(0, 3, LOAD_ROWS)
    shuffled = rows[rng.permutation(LOAD_ROWS)]
    pu = MethylationPileup([("chr1", LOAD_BASES)], partitions=True, bases=np.full(LOAD_BASES, ord("N"), np.uint8))
    none = np.zeros(1, LOCUS_DTYPE)
    assert pu._L.hm_pileup_load_loci(pu._h, 1, none.ctypes.data_as(C.c_void_p), 1) == 0       # warm-up: the slab, the code object
    secs = {}
    for name, part, r in (("sorted", 1, rows), ("shuffled", 2, shuffled)):
        t0 = time.perf_counter()
        n = pu._L.hm_pileup_load_loci(pu._h, part, r.ctypes.data_as(C.c_void_p), LOAD_ROWS)
        secs[name] = time.perf_counter() - t0
        assert n == LOAD_ROWS, pu._L.hm_pileup_last_error(pu._h)
    out = dict(load_rows=LOAD_ROWS, load_reference_bases=LOAD_BASES, load_call_s={k: round(v, 4) for k, v in secs.items()},
               load_rows_per_s={k: round(LOAD_ROWS / v) for k, v in secs.items()})
    if check:                                      # the pooled planes hold both parts' counts, each part's its own
        pooled, parts = pu.loci(), [pu.loci(partition=k) for k in (1, 2)]
        out["check_load_planes_hold_the_rows"] = bool(
            all(len(x) == LOAD_ROWS and (x["gpos"] == rows["gpos"]).all() for x in [pooled] + parts)
            and (parts[0]["pcov"] == rows["pcov"]).all() and (parts[1]["ncov"] == rows["ncov"]).all()
            and (pooled["pcov"] == 2 * rows["pcov"]).all() and (pooled["motif"] == rows["motif"]).all())
    pu.close()
    return out


def sample_intervals_leg(check):
    """`regiondiff`: hm_sample_fetch_intervals of N = 6 samples over 2^20 tiles of 256 bases of a reference of 2^28 bases, one
    context, both modes, beside hm_pileup_fetch_regions on the same intervals over the combined planes (all three contexts at
    once, twelve sums per interval) in the same run; a leg of its own: nothing else is run.  Both calls include the copies of the
    intervals to the device and of the sums back."""
    BASES, TILE, N, ROWS = 1 << 28, 256, 6, 1 << 23
    rng = np.random.default_rng(13)
    step = BASES // ROWS
    pu = MethylationPileup([("chr1", BASES)], samples=N, bases=np.full(BASES, ord("N"), np.uint8))
    g = np.arange(ROWS, dtype=np.int64) * step + rng.integers(0, step, ROWS)          # a locus per 32 bases, the same in every sample
    motif = rng.integers(0, 3, ROWS)
    for s in range(N):
        cov = rng.integers(1, 30, ROWS)
        p = rng.binomial(cov, 0.6)
        assert pu.open_sample() == s and pu.load_sample(g, p, cov - p, motif) == ROWS
    start = np.arange(0, BASES, TILE, dtype=np.int64)
    end = start + TILE
    pu.sample_intervals(start[:8], end[:8], 0)                # warm-up: the code objects, the buffers
    pu.regions(start[:8], end[:8])
    secs = {}
    for name, call in (("sample_intervals_pairwise", lambda: pu.sample_intervals(start, end, 0)),
                       ("sample_intervals_complete", lambda: pu.sample_intervals(start, end, 0, complete=True)),
                       ("fetch_regions", lambda: pu.regions(start, end, min_cov=1))):
        t0 = time.perf_counter()
        got = call()
        secs[name] = time.perf_counter() - t0
        if name == "sample_intervals_pairwise":
            sums = got
    out = dict(sample_intervals_samples=N, sample_intervals_reference_bases=BASES, sample_intervals_tiles=len(start), sample_intervals_tile=TILE,
               sample_intervals_call_s={k: round(v, 4) for k, v in secs.items()},
               sample_intervals_tiles_per_s={k: round(len(start) / v) for k, v in secs.items()})
    if check:                                      # every counting locus of context 0 lies in exactly one tile
        planes = [pu.sample_plane(s) for s in range(N)]
        key0 = np.zeros(BASES, bool)
        key0[g[motif == 0]] = True
        out["check_tiles_hold_the_loci"] = bool(all(int(sums[:, s, 0].sum()) == int(((planes[s] != 0) & (planes[s] != 0xFFFF) & key0).sum()) for s in range(N)))
    pu.close()
    print(json.dumps(out))


def group_regions_leg(repeat, check):
    """`groupdmr`: hm_dmr_fetch_regions of one context over a reference of 2^26 bases with 2^22 loci per sample (3 + 3
    samples; stretches of 2^12 bases in which group 1 lies above group 2, below it or level with it), beside hm_pileup_fetch_groups
    over the same range in the same run -- the rows of all three contexts copied to the host, which `groupdmr` without -F and -L
    never does; a leg of its own: nothing else is run.  Each call is timed `repeat` times after one warm-up call."""
    BASES, ROWS, STRETCH = 1 << 26, 1 << 22, 1 << 12
    rng = np.random.default_rng(17)
    step = BASES // ROWS
    pu = MethylationPileup([("chr1", BASES)], partitions=True, groups=True, bases=np.full(BASES, ord("N"), np.uint8))
    g = np.arange(ROWS, dtype=np.int64) * step + rng.integers(0, step, ROWS)          # a locus per 16 bases, the same in every sample
    motif = rng.choice(3, ROWS, p=[0.6, 0.2, 0.2])
    state = rng.choice([1, -1, 0], BASES // STRETCH, p=[0.2, 0.2, 0.6])[g // STRETCH]
    for part in (1, 2):
        for s in range(3):
            cov = rng.integers(5, 40, ROWS)
            p = rng.binomial(cov, 0.5 + (0.3 if part == 1 else -0.3) * state)
            assert pu.begin_sample(part) == s and pu.load_sample_loci(g, p, cov - p, motif) == ROWS
    calls = (("fetch_groups", lambda: pu.group_tests(0, BASES, 2)),
             ("fetch_group_regions", lambda: pu.group_regions(0, 0, BASES, 2, 0.01, 0.0, 500, 3)))
    secs, got = {}, {}
    for name, call in calls:
        call()                                                # warm-up: the code objects, the buffers
        secs[name] = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            got[name] = call()
            secs[name].append(time.perf_counter() - t0)
    rows, (regions, n_ctx_rows, n_hits) = got["fetch_groups"], got["fetch_group_regions"]
    out = dict(group_regions_reference_bases=BASES, group_regions_loci_per_sample=ROWS, group_regions_tested_rows=len(rows),
               group_regions_ctx_rows=n_ctx_rows, group_regions_hits=n_hits, group_regions_regions=len(regions),
               group_regions_call_s={k: [round(x, 4) for x in v] for k, v in secs.items()},
               group_regions_best_s={k: round(min(v), 4) for k, v in secs.items()})
    if check:                                      # the context's rows and hits are those of the per-locus fetch
        r0 = rows[np.minimum(rows["motif"], 2) == 0]
        out["check_group_regions_counts"] = bool(len(r0) == n_ctx_rows and int(((r0["pvalue"] <= 0.01) & (r0["diff"] != 0)).sum()) == n_hits
                                                 and int(regions["n_loci"].sum()) <= n_hits and len(regions) > 0)
    pu.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=20)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--read-len", type=int, default=15000)
    ap.add_argument("--batch", type=int, default=512, help="reads per hm_pileup_run")
    ap.add_argument("--repeat", type=int, default=3, help="timed passes over the staged read set")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--partitions", action="store_true", help="haplotype partitions on, reads tagged with random HP")
    ap.add_argument("--asm", action="store_true", help="with --partitions: time the per-locus haplotype test (pileup -H -A)")
    ap.add_argument("--asm-min-cov", type=int, default=5)
    ap.add_argument("--asm-q", action="store_true", help="with --asm: time the Benjamini-Hochberg q-values of the test (pileup -H -A -Q)")
    ap.add_argument("--asm-regions", action="store_true", help="with --asm: time the chaining of tested loci into regions (pileup -H -A -G)")
    ap.add_argument("--regions-max-p", type=float, default=0.01)
    ap.add_argument("--regions-max-gap", type=int, default=500)
    ap.add_argument("--regions-min-loci", type=int, default=3)
    ap.add_argument("--sites", action="store_true", help="time the per-locus binomial test (pileup -B / -e)")
    ap.add_argument("--sites-rate", type=float, default=0.013, help="with --sites: the false-positive rate of all three contexts")
    ap.add_argument("--domains", action="store_true", help="time the low / high segmentation of the covered loci (pileup -D, its default weights)")
    ap.add_argument("--fit", action="store_true",
                    help="with --domains: also one state-sums pass (hm_pileup_domain_sums) next to one fetch, and the fit of the levels (pileup -D -Y)")
    ap.add_argument("--fit-iter", type=int, default=50, help="with --fit: the largest number of iterations per context")
    ap.add_argument("--parts", type=int, default=0, metavar="N",
                    help="with --domains: also the same segments chained from N equal pieces (hm_pileup_fetch_domains_part, what pileup_dist -D runs)")
    ap.add_argument("--patterns", type=int, default=0, metavar="K", choices=(0, 2, 3, 4),
                    help="time what the read-level CpG patterns over windows of K reference CpGs add (pileup -E K, default span and min reads)")
    ap.add_argument("--linkage", type=int, default=0, metavar="D",
                    help="time what the within-read co-methylation by distance up to D bases adds (pileup -L D, min_pairs 1)")
    ap.add_argument("--readpos", type=int, default=0, metavar="D",
                    help="time what the methylation by position in the read adds, D bases from either end resolved (pileup -P D, min_calls 1)")
    ap.add_argument("--regions", type=int, default=0, metavar="N",
                    help="time the interval sums and the metaplot (pileup -R / -J 20:2000:10): N gene-like intervals of 0.5 - 20 kb, "
                         "and a tiling of the reference in 1 kb windows")
    ap.add_argument("--context", type=int, default=0, metavar="LOG2",
                    help="time the k-mer tables (pileup -S 0 .. 3) on both accumulation paths over synthetic planes of 2^LOG2 loci, 5 %% "
                         "covered, against the interval index build over the same planes; a leg of its own: nothing else is run")
    ap.add_argument("--load", action="store_true",
                    help="time the loader of `diff` (hm_pileup_load_loci): 2^24 rows into a reference of 2^28 bases on an engine of its own, "
                         "reported beside records_per_s_count of this run")
    ap.add_argument("--bedmethyl", action="store_true", help="time what the per-CpG depth classes add (pileup -M, min_valid 1)")
    ap.add_argument("--digest", action="store_true", help="add a sha256 of the records, the loci and the rows of the timed options")
    ap.add_argument("--cpu-baseline", action="store_true",
                    help="time the reference's own projection code (oracle/_ref/ref_align -t) on a bounded sample")
    ap.add_argument("--sample-intervals", action="store_true",
                    help="time the interval sums of `regiondiff` (hm_sample_fetch_intervals): 6 samples, 2^20 tiles of 256 bases over 2^28 bases, "
                         "against hm_pileup_fetch_regions on the same tiles over the combined planes; a leg of its own: nothing else is run")
    ap.add_argument("--group-regions", action="store_true",
                    help="time the regions of `groupdmr` (hm_dmr_fetch_regions): 3 + 3 samples of 2^22 loci over 2^26 bases, one context, "
                         "against hm_pileup_fetch_groups over the same range; a leg of its own: nothing else is run")
    a = ap.parse_args()
    if a.group_regions:
        return group_regions_leg(a.repeat, a.check)
    if a.context:
        return context_leg(a.context, a.repeat, a.check)
    if a.sample_intervals:
        return sample_intervals_leg(a.check)
    if a.asm and not a.partitions:
        ap.error("--asm needs --partitions")
    if a.asm_q and not a.asm:
        ap.error("--asm-q needs --asm")
    if a.asm_regions and not a.asm:
        ap.error("--asm-regions needs --asm")

    rng = np.random.default_rng(1)
    G = int(a.genome_mb * 1e6)
    gc = 0.36
    codes = rng.choice(4, G, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]).astype(np.uint8)
    chrom = _ASCII[codes]
    genome = [("chr1", chrom.tobytes().decode())]
    n_reads = int(G * a.coverage / a.read_len)
    starts = np.sort(rng.integers(0, G - a.read_len, n_reads))
    t0 = time.perf_counter()
    staged = []
    lut = np.zeros(256, np.uint8)
    lut[[65, 67, 71, 84]] = [0, 1, 2, 3]
    for i, s in enumerate(starts):
        seq = chrom[s:s + a.read_len]
        rev = bool(rng.random() < 0.5)
        fwd = _COMP[seq][::-1] if rev else seq
        mods = call_like_mods(fwd, rng)
        staged.append((16 if rev else 0, int(s), pack_codes(lut[seq]), np.array([(a.read_len << 4) | 7], np.uint32), mods))
    t_prep = time.perf_counter() - t0
    n_mods = sum(len(x[4]) for x in staged)
    hp = np.random.default_rng(2).integers(0, 3, n_reads) if a.partitions else np.zeros(n_reads, np.int64)

    pu = MethylationPileup(genome, partitions=a.partitions)
    L = pu._L

    def one_pass(pu=pu):
        for i, (flag, pos, seq4, cig, mods) in enumerate(staged):
            args = (pu._h, i, flag, 0, pos, 60, a.read_len, seq4.ctypes.data_as(C.c_void_p), 1,
                    cig.ctypes.data_as(C.c_void_p), len(mods), mods.ctypes.data_as(C.c_void_p))
            rc = L.hm_pileup_submit_read_hp(*args, int(hp[i])) if a.partitions else L.hm_pileup_submit_read(*args)
            assert rc == 1
            if (i + 1) % a.batch == 0:
                pu.flush()
        pu.flush()

    if a.patterns or a.bedmethyl or a.linkage or a.readpos:  # the same passes without the option(s) first: the leg is the difference
        one_pass()
        pu.count([128, 128, 128])
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            one_pass()
        t_project_off = time.perf_counter() - t0
        t0 = time.perf_counter()
        pu.count([128, 128, 128])
        t_count_off = time.perf_counter() - t0
        pu.close()
        pu = MethylationPileup(genome, partitions=a.partitions, patterns=a.patterns, bedmethyl=a.bedmethyl, linkage=a.linkage, profile=a.readpos)
    one_pass(pu)                                   # warm-up (allocations)
    wins_per_pass = pu.num_pattern_records()
    recs_per_pass = pu.num_records()
    digest = {}

    def sha(rows):
        return hashlib.sha256(np.ascontiguousarray(rows).tobytes()).hexdigest()

    if a.digest:                                   # the warm-up pass's records, still resident
        g, p, m, o = pu.records()
        at = np.lexsort(((g << 2) | m, o))
        digest["records"] = sha(np.rec.fromarrays([o[at], g[at], m[at], p[at]]))
    pu.count([128, 128, 128])
    t0 = time.perf_counter()
    for _ in range(a.repeat):
        one_pass(pu)
    t_project = time.perf_counter() - t0
    t0 = time.perf_counter()
    pu.count([128, 128, 128])
    t_count = time.perf_counter() - t0
    t0 = time.perf_counter()
    loci = pu.loci()
    t_loci = time.perf_counter() - t0
    hp_loci = []
    if a.partitions:
        t0 = time.perf_counter()
        hp_loci = [pu.loci(partition=k) for k in (1, 2)]
        t_hp_loci = time.perf_counter() - t0
    cols = n_reads * a.read_len
    out = dict(genome_bases=G, reads=n_reads, aligned_columns=cols, mods=n_mods, records_per_pass=recs_per_pass,
               host_prep_s=round(t_prep, 2),
               stage_and_project_s_per_pass=round(t_project / a.repeat, 4),
               aligned_columns_per_s=round(cols * a.repeat / t_project),
               count_s=round(t_count, 4), records_counted=recs_per_pass * a.repeat,
               records_per_s_count=round(recs_per_pass * a.repeat / t_count),
               covered_loci=int(len(loci)), loci_fetch_s=round(t_loci, 4),
               loci_scan_bases_per_s=round(G / t_loci), partitions=a.partitions)
    if a.partitions:
        out.update(partition_loci=[int(len(x)) for x in hp_loci], partition_loci_fetch_s=round(t_hp_loci, 4))
    if a.patterns:
        pu.patterns()                              # warm-up: the row buffer
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            rows = pu.patterns()
        t_rows = (time.perf_counter() - t0) / a.repeat
        t_leg = max((t_project - t_project_off + t_count - t_count_off) / a.repeat, 0.0) + t_rows
        t_pass = (t_project_off + t_count_off) / a.repeat + t_loci
        out.update(patterns_k=a.patterns, patterns_window_records_per_pass=int(wins_per_pass), patterns_rows=int(len(rows)),
                   patterns_project_s_per_pass=[round(t_project_off / a.repeat, 4), round(t_project / a.repeat, 4)],
                   patterns_count_s=[round(t_count_off, 4), round(t_count, 4)], patterns_rows_s=round(t_rows, 4),
                   patterns_leg_s_per_pass=round(t_leg, 4), patterns_window_records_per_s=round(wins_per_pass / t_leg) if t_leg else 0,
                   patterns_share_of_pass=round(t_leg / (t_pass + t_leg), 4))
        if a.check:                                # a row's reads are window records: all of them at min_reads 1
            n_all = int(pu.patterns(min_reads=1)["n"].astype(np.int64).sum())
            out["check_patterns_rows_hold_the_records"] = bool(n_all == wins_per_pass * (a.repeat + 1))
    if a.linkage:
        pu.linkage()                               # warm-up: the table and the row buffer
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            rows = pu.linkage()
        t_rows = (time.perf_counter() - t0) / a.repeat
        pairs = int(sum(int(rows[k].astype(np.uint64).sum()) for k in ("n_uu", "n_um", "n_mu", "n_mm"))) // (a.repeat + 1)
        t_leg = max((t_project - t_project_off + t_count - t_count_off) / a.repeat, 0.0) + t_rows
        t_pass = (t_project_off + t_count_off) / a.repeat + t_loci
        out.update(linkage_max_dist=a.linkage, linkage_pairs_per_pass=pairs, linkage_rows=int(len(rows)),
                   linkage_project_s_per_pass=[round(t_project_off / a.repeat, 4), round(t_project / a.repeat, 4)],
                   linkage_count_s=[round(t_count_off, 4), round(t_count, 4)], linkage_rows_s=round(t_rows, 4),
                   linkage_leg_s_per_pass=round(t_leg, 4), linkage_pairs_per_s=round(pairs / t_leg) if t_leg else 0,
                   linkage_share_of_pass=round(t_leg / (t_pass + t_leg), 4), linkage_also=[a.patterns, a.bedmethyl])
        if a.check:                                # every pass adds the same pairs; the distances are ascending and within reach
            n_all = sum(int(rows[k].astype(np.uint64).sum()) for k in ("n_uu", "n_um", "n_mu", "n_mm"))
            out["check_linkage_rows"] = bool(len(rows) and n_all == pairs * (a.repeat + 1) and (np.diff(rows["dist"].astype(np.int64)) > 0).all()
                                             and rows["dist"][0] >= 2 and rows["dist"][-1] <= a.linkage)
    if a.readpos:
        pu.readpos()                               # warm-up: the three sums per row and the row buffer
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            rows = pu.readpos()
        t_rows = (time.perf_counter() - t0) / a.repeat
        n_all = int(rows["n_m"].sum() + rows["n_u"].sum())
        ends = int((rows["n_m"] + rows["n_u"])[rows["end"] != 2].sum()) // (a.repeat + 1)
        t_leg = max((t_project - t_project_off + t_count - t_count_off) / a.repeat, 0.0) + t_rows
        t_pass = (t_project_off + t_count_off) / a.repeat + t_loci
        out.update(readpos_reach=a.readpos, readpos_table_bytes=3 * (2 * a.readpos + 1) * 2048, readpos_rows=int(len(rows)),
                   readpos_end_records_per_pass=ends,
                   readpos_project_s_per_pass=[round(t_project_off / a.repeat, 4), round(t_project / a.repeat, 4)],
                   readpos_count_s=[round(t_count_off, 4), round(t_count, 4)], readpos_rows_s=round(t_rows, 4),
                   readpos_leg_s_per_pass=round(t_leg, 4), readpos_records_per_s=round(recs_per_pass / t_leg) if t_leg else 0,
                   readpos_share_of_pass=round(t_leg / (t_pass + t_leg), 4), readpos_also=[a.patterns, a.bedmethyl, a.linkage])
        if a.check:                                # every pass adds its records once; the methylated ones are the pcov plane
            out["check_readpos_rows"] = bool(n_all == recs_per_pass * (a.repeat + 1) and int(rows["n_m"].sum()) == int(loci["pcov"].astype(np.int64).sum()))
    if a.bedmethyl:
        pu.bedmethyl()                             # warm-up: the row buffer
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            rows = pu.bedmethyl()
        t_rows = (time.perf_counter() - t0) / a.repeat
        t_leg = max((t_project - t_project_off + t_count - t_count_off) / a.repeat, 0.0) + t_rows
        t_pass = (t_project_off + t_count_off) / a.repeat + t_loci
        out.update(bedmethyl_rows=int(len(rows)), bedmethyl_project_s_per_pass=[round(t_project_off / a.repeat, 4), round(t_project / a.repeat, 4)],
                   bedmethyl_count_s=[round(t_count_off, 4), round(t_count, 4)], bedmethyl_rows_s=round(t_rows, 4),
                   bedmethyl_leg_s_per_pass=round(t_leg, 4), bedmethyl_share_of_pass=round(t_leg / (t_pass + t_leg), 4),
                   bedmethyl_also_patterns=a.patterns)
        if a.check:                                # Nvalid of a row is the coverage of its locus; a reference CGG also takes CHG records there
            valid = pu.bedmethyl(min_valid=1)
            j = np.minimum(np.searchsorted(loci["gpos"], valid["gpos"]), len(loci) - 1)
            nv = valid["n_mod"].astype(np.int64) + valid["n_canon"]
            cov = loci["pcov"].astype(np.int64)[j] + loci["ncov"][j]
            plain = chrom[np.minimum(valid["gpos"] + 2, G - 1)] != 71
            out["check_bedmethyl_valid_is_the_cpg_coverage"] = bool(
                len(valid) and (loci["gpos"][j] == valid["gpos"]).all() and (nv <= cov).all() and (nv[plain] == cov[plain]).all()
                and not valid["n_diff"].any() and not valid["n_delete"].any())
    if a.asm:                                      # select + test + fetch of every tested locus, as the CLI does per sequence
        pu.asm(min_cov=a.asm_min_cov)              # warm-up: the log n! table and the row buffer
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            rows = pu.asm(min_cov=a.asm_min_cov)
        t_asm = (time.perf_counter() - t0) / a.repeat
        t0 = time.perf_counter()
        for _ in range(a.repeat):                  # the count-only call: predicate + scan, no test
            n_rows = pu._L.hm_pileup_fetch_asm(pu._h, None, None, None, None, None, 0, 0, G, a.asm_min_cov, None, 0)
        t_sel = (time.perf_counter() - t0) / a.repeat
        assert n_rows == len(rows)
        steps = np.minimum(np.minimum(rows["pcov1"] + rows["ncov1"], rows["pcov2"] + rows["ncov2"]),
                           np.minimum(rows["pcov1"] + rows["pcov2"], rows["ncov1"] + rows["ncov2"])).astype(np.int64) + 1
        out.update(asm_min_cov=a.asm_min_cov, asm_rows=int(len(rows)), asm_s_per_pass=round(t_asm, 4),
                   asm_count_only_s=round(t_sel, 4), asm_rows_per_s=round(len(rows) / t_asm),
                   asm_mean_tables_per_row=round(float(steps.mean()), 1) if len(rows) else 0.0,
                   asm_share_of_pass=round(t_asm / (t_project / a.repeat + t_count / a.repeat + t_loci + t_hp_loci + t_asm), 4))
    if a.asm_q:                                    # histogram, p per tuple, q-values (host), rows of every tested locus, as the CLI does
        from hifimeth_amd.pileup import asm_qvalues

        def q_pass():
            t = [time.perf_counter()]
            bins, big = pu.asm_histogram(min_cov=a.asm_min_cov)
            t.append(time.perf_counter())
            tab = pu.asm_bin_pvalues(bins)
            t.append(time.perf_counter())
            table = asm_qvalues(tab, big)
            t.append(time.perf_counter())
            rows_q = pu.asm(min_cov=a.asm_min_cov, table=table)
            t.append(time.perf_counter())
            return np.diff(t), table, rows_q

        q_pass()                                   # warm-up: the 104 MB of bins, the row buffers
        legs = np.zeros(4)
        for _ in range(a.repeat):
            dt, table, rows_q = q_pass()
            legs += dt
        legs /= a.repeat
        t_q = float(legs.sum())
        t_hp_pass = t_project / a.repeat + t_count / a.repeat + t_loci + t_hp_loci + t_asm     # a -H -A pass
        out.update(asmq_rows=int(len(rows_q)), asmq_big_loci=int(len(table.big)), asmq_tuples=int(len(table.tab)),
                   asmq_histogram_s=round(float(legs[0]), 4), asmq_bin_pvalues_s=round(float(legs[1]), 4),
                   asmq_table_s=round(float(legs[2]), 4), asmq_rows_s=round(float(legs[3]), 4), asmq_s_per_pass=round(t_q, 4),
                   asmq_rows_per_s=round(len(rows_q) / t_q) if t_q else 0, asmq_share_of_asm_pass=round(t_q / t_hp_pass, 4),
                   asmq_significant=[int((rows_q["qvalue"] <= x).sum()) for x in (0.05, 0.01)])
        if a.check:                                # the rows of --asm with a q each; the table's weights are the rows
            plain = np.ascontiguousarray(rows_q[list(rows.dtype.names)]).astype(rows.dtype)
            out["check_asmq_rows_are_the_asm_rows"] = bool(plain.tobytes() == rows.tobytes() and not np.isnan(rows_q["qvalue"]).any()
                                                           and int(table.m.sum()) == len(rows))
    if a.asm_regions:                              # the three contexts over the whole sequence, as the CLI does
        def regions_pass():
            return [pu.asm_regions(c, min_cov=a.asm_min_cov, max_p=a.regions_max_p, max_gap=a.regions_max_gap,
                                   min_loci=a.regions_min_loci) for c in range(3)]

        regions_pass()                             # warm-up: the row buffers
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            found = regions_pass()
        t_reg = (time.perf_counter() - t0) / a.repeat
        ctx_rows = sum(n for _r, n in found)
        t_hp_pass = t_project / a.repeat + t_count / a.repeat + t_loci + t_hp_loci + t_asm     # a -H -A pass
        out.update(regions_max_p=a.regions_max_p, regions_max_gap=a.regions_max_gap, regions_min_loci=a.regions_min_loci,
                   regions_ctx_rows=int(ctx_rows), regions=[int(len(r)) for r, _n in found],
                   regions_longest_chain=int(max((int(r["n_loci"].max()) for r, _n in found if len(r)), default=0)),
                   regions_s_per_pass=round(t_reg, 4), regions_rows_per_s=round(ctx_rows / t_reg) if t_reg else 0,
                   regions_share_of_asm_pass=round(t_reg / t_hp_pass, 4))
        if a.check:                                # every tested row belongs to exactly one context
            out["check_regions_rows_are_the_asm_rows"] = bool(ctx_rows == len(rows))
    if a.sites:                                    # histogram, table (host), rows of every covered locus, as the CLI does
        from hifimeth_amd.pileup import sites_table
        pu.sites(sites_table([a.sites_rate] * 3, *pu.site_histogram()))    # warm-up: buffers, the log n! table
        t_hist = t_tab = t_rows = 0.0
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            bins, big = pu.site_histogram()
            t1 = time.perf_counter()
            table = sites_table([a.sites_rate] * 3, bins, big)
            t2 = time.perf_counter()
            rows = pu.sites(table)
            t_hist, t_tab, t_rows = t_hist + t1 - t0, t_tab + t2 - t1, t_rows + time.perf_counter() - t2
        t_sites = (t_hist + t_tab + t_rows) / a.repeat
        t_pass = t_project / a.repeat + t_count / a.repeat + t_loci
        out.update(sites_rate=a.sites_rate, sites_rows=int(len(rows)), sites_big_loci=int(len(big)), sites_triples=int((bins > 0).sum()),
                   sites_histogram_s=round(t_hist / a.repeat, 4), sites_table_s=round(t_tab / a.repeat, 4),
                   sites_rows_s=round(t_rows / a.repeat, 4), sites_s_per_pass=round(t_sites, 4),
                   sites_loci_per_s=round(len(rows) / t_sites) if t_sites else 0,
                   sites_share_of_pass=round(t_sites / (t_pass + t_sites), 4))
        if a.check:
            out["check_sites_rows_are_the_loci"] = bool(len(rows) == len(loci) and (rows["gpos"] == loci["gpos"]).all()
                                                        and int(bins.sum()) + len(big) == len(loci))
    if a.domains:                                  # the three contexts over the whole sequence, as the CLI does
        def domains_pass():
            return [pu.domains(c) for c in range(3)]

        domains_pass()                             # warm-up: the row buffers
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            found = domains_pass()
        t_dom = (time.perf_counter() - t0) / a.repeat
        ctx_rows = sum(n for _r, n in found)
        t_pass = t_project / a.repeat + t_count / a.repeat + t_loci
        out.update(domains_ctx_rows=int(ctx_rows), domains=[int(len(r)) for r, _n in found],
                   domains_high=[int((r["state"] == 1).sum()) for r, _n in found],
                   domains_longest=int(max((int(r["n_loci"].max()) for r, _n in found if len(r)), default=0)),
                   domains_s_per_pass=round(t_dom, 4), domains_rows_per_s=round(ctx_rows / t_dom) if t_dom else 0,
                   domains_share_of_pass=round(t_dom / (t_pass + t_dom), 4))
        if a.fit:                                  # the sums pass the fit repeats, and the fit itself from the default levels
            from hifimeth_amd.pileup import DOMAIN_LEVELS, DOMAIN_MAX_GAP, DOMAIN_PENALTY

            def sums_pass():
                return [pu.domain_sums(c) for c in range(3)]

            sums_pass()
            t0 = time.perf_counter()
            for _ in range(a.repeat):
                state_sums = sums_pass()
            t_sums = (time.perf_counter() - t0) / a.repeat
            t0 = time.perf_counter()
            fits = [pu.fit_domain_levels(c, *DOMAIN_LEVELS[c], DOMAIN_PENALTY, DOMAIN_MAX_GAP, a.fit_iter) for c in range(3)]
            t_fit = time.perf_counter() - t0
            out.update(domains_sums_s_per_pass=round(t_sums, 4), domains_sums_rows_per_s=round(ctx_rows / t_sums) if t_sums else 0,
                       domains_sums_over_fetch=round(t_sums / t_dom, 3) if t_dom else 0, domains_fit_s=round(t_fit, 4),
                       domains_fit_iterations=[len(f[3]) for f in fits], domains_fit_status=[f[2] for f in fits],
                       domains_fit_levels=[[float("%.6g" % f[0]), float("%.6g" % f[1])] for f in fits])
            if a.check:                            # the sums are those of the fetched segments, state by state
                out["check_domains_sums_equal_the_segments"] = bool(all(
                    s == tuple(int(r[f][r["state"] == z].sum()) for z in (0, 1) for f in ("pcov", "ncov", "n_loci"))
                    for s, (r, _n) in zip(state_sums, found)))
        if a.parts:                                # the same segments from a.parts equal pieces: three stateless passes each, chained
            from functools import partial

            from hifimeth_amd.pileup import DOMAIN_LEVELS, DOMAIN_MAX_GAP, chain_domain_parts, domain_scores, stitch_domains
            edges = [pu.n_loci * k // a.parts for k in range(a.parts + 1)]

            def chained_pass():
                rows = []
                for c in range(3):
                    A, B, S = domain_scores(*DOMAIN_LEVELS[c])
                    pieces = [partial(pu.domains_part, c, lo, hi) for lo, hi in zip(edges, edges[1:])]
                    rows.append(stitch_domains(chain_domain_parts(pieces, A, B, S, DOMAIN_MAX_GAP), A, B))
                return rows

            chained_pass()
            t0 = time.perf_counter()
            for _ in range(a.repeat):
                chained = chained_pass()
            t_parts = (time.perf_counter() - t0) / a.repeat
            out.update(domains_parts=a.parts, domains_parts_s_per_pass=round(t_parts, 4),
                       domains_parts_rows_per_s=round(ctx_rows / t_parts) if t_parts else 0,
                       domains_parts_over_single=round(t_parts / t_dom, 3) if t_dom else 0)
            if a.check:
                out["check_domains_parts_equal_the_single_fetch"] = bool(all(x.tobytes() == r.tobytes() for x, (r, _n) in zip(chained, found)))
        if a.check:                                # the segments partition the covered loci and their counts
            out["check_domains_partition_the_loci"] = bool(
                ctx_rows == len(loci) == sum(int(r["n_loci"].sum()) for r, _n in found)
                and sum(int(r["pcov"].sum()) for r, _n in found) == int(loci["pcov"].astype(np.int64).sum())
                and sum(int(r["ncov"].sum()) for r, _n in found) == int(loci["ncov"].astype(np.int64).sum()))
    if a.regions:
        from hifimeth_amd.pileup import locate, region_geometry
        rng_iv = np.random.default_rng(17)
        length = np.exp(rng_iv.uniform(np.log(500), np.log(20000), a.regions)).astype(np.int64)
        start = rng_iv.integers(0, max(G - 20000, 1), a.regions)
        sid, _ = locate(pu.offsets, start)
        s0, s1 = pu.offsets[sid], pu.offsets[sid + 1]
        genes = dict(start=start, end=np.minimum(start + length, s1), seq_start=s0, seq_end=s1, strand=bytes(rng_iv.choice([43, 45], a.regions).astype(np.uint8)))
        tiles = np.concatenate([np.arange(pu.offsets[k], pu.offsets[k + 1], 1000) for k in range(len(pu.offsets) - 1)])
        sid, _ = locate(pu.offsets, tiles)
        tile_end = np.minimum(tiles + 1000, pu.offsets[sid + 1])
        legs = {"genes": lambda: pu.regions(genes["start"], genes["end"]),
                "metaplot": lambda: pu.metaplot(**genes, bins=20, flank=2000, flank_bins=10),
                "tiles": lambda: pu.regions(tiles, tile_end),
                "index": lambda: pu.regions(tiles[:1], tile_end[:1])}              # one interval: the index build and the fixed costs
        times = {}
        for name, leg in legs.items():
            leg()                                  # warm-up: the buffers, the code objects
            t = []
            for _ in range(max(a.repeat, 5)):
                t0 = time.perf_counter()
                leg()
                t.append(time.perf_counter() - t0)
            times[name] = t
        t_pass = t_project / a.repeat + t_count + t_loci
        best = {k: min(v) for k, v in times.items()}
        out.update(regions_block=region_geometry()[0], regions_intervals=a.regions, regions_tiles=int(len(tiles)),
                   regions_s={k: [round(x, 5) for x in v] for k, v in times.items()},
                   regions_index_bytes=int(12 * G), regions_index_bytes_per_s=round(12 * G / best["index"]),
                   regions_ns_per_interval={"genes": round(1e9 * max(best["genes"] - best["index"], 0) / a.regions, 1),
                                            "metaplot": round(1e9 * max(best["metaplot"] - best["index"], 0) / a.regions, 1),
                                            "tiles": round(1e9 * max(best["tiles"] - best["index"], 0) / len(tiles), 1)},
                   regions_share_of_pass={k: round(v / (t_pass + v), 4) for k, v in best.items()})
        if a.check:                                # the tiles partition the reference: their sums are the covered loci's
            t_sum = pu.regions(tiles, tile_end)
            out["check_regions_tiles_hold_the_loci"] = bool(
                int(t_sum["n_loci"].sum()) == len(loci) and int(t_sum["pcov"].sum()) == int(loci["pcov"].astype(np.int64).sum())
                and int(t_sum["ncov"].sum()) == int(loci["ncov"].astype(np.int64).sum()))
        if a.digest:
            digest["regions"] = [sha(pu.regions(genes["start"], genes["end"])), sha(pu.metaplot(**genes, bins=20, flank=2000, flank_bins=10)[0])]
    if a.check:                                    # every pass (and the warm-up) adds the same records
        total = int((loci["pcov"].astype(np.int64) + loci["ncov"]).sum())
        out["check_total_records"] = total == recs_per_pass * (a.repeat + 1)
        if a.partitions:                           # hap1 + hap2 <= combined at every locus, and the tagged share is counted once
            add = np.zeros((len(loci), 2), np.int64)
            for x in hp_loci:                      # both lists ascending; a partition locus is a combined locus
                j = np.searchsorted(loci["gpos"], x["gpos"])
                np.add.at(add, (j, 0), x["pcov"])
                np.add.at(add, (j, 1), x["ncov"])
            out["check_partitions_within_combined"] = bool((add[:, 0] <= loci["pcov"]).all() and (add[:, 1] <= loci["ncov"]).all())
    if a.digest:
        digest["loci"] = sha(loci)
        digest["partition_loci"] = [sha(x) for x in hp_loci]
        if a.patterns:
            digest["patterns"] = sha(pu.patterns())
        if a.bedmethyl:
            digest["bedmethyl"] = [sha(pu.bedmethyl(partition=k)) for k in ((0, 1, 2) if a.partitions else (0,))]
        if a.linkage:
            digest["linkage"] = sha(pu.linkage())
        if a.readpos:
            digest["readpos"] = sha(pu.readpos())
        out["digest"] = digest
    if a.cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(genome, chrom, starts, staged, a.read_len)
    if a.load:
        pu.close()                                 # the leg's engine holds 28 B per base of its own reference
        out.update(load_leg(a.check))
        out["load_rows_per_s_to_count_records_per_s"] = {k: round(v / out["records_per_s_count"], 3) for k, v in out["load_rows_per_s"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
