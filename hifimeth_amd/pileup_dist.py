"""`hifimeth pileup` over N GPUs of one node, one process per GPU (the path's only exchange step).

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        -m hifimeth_amd.pileup_dist [-q mapQ] [-f identity] [-H [-A [-a min-cov] [-Q] [-G [-s max-p] [-g max-gap] [-n min-loci]]]] [-B control | -e r,r,r] [-D [-u lo:hi[,lo:hi,lo:hi]] [-x nats] [-j bp]] [-L bp [-z min-pairs]] [-P bp [-y min-calls]] [-I n5[:n3]] [-R bed [-C min-cov] [-J bins[:flank:flank_bins]]] [-S flank [-O min-cov]] reference.fa mod.bam output-prefix

Records are dealt to the ranks in slabs of `--slab` records (round-robin, like the `call` path).  Each rank projects its
records and histograms them on its own GPU; then
  1. all-reduce(sum) of the 3 x 256 histograms (6 KB)           -> every rank resolves the same thresholds,
  2. per-rank counting into planes laid out as world x chunk loci,
  3. reduce-scatter(sum) of pcov / ncov and reduce-scatter(max) of the motif key over RCCL
                                                                 -> rank r owns loci [r*chunk, (r+1)*chunk),
  4. every rank compacts and formats its range; rank 0 concatenates the parts in rank order (= locus order).
A single process (no torchrun) runs the same code with the collectives skipped.
-H (haplotypes): four more planes (pcov / ncov of HP 1 and HP 2) are counted with the same thresholds, reduce-scattered
with SUM next to the three above, and rank 0 also writes <prefix>.hap1.<ctx>.cov.bed / <prefix>.hap2.<ctx>.cov.bed.
-A (with -H): every rank tests its own chunk of the reduce-scattered haplotype planes (hm_pileup_fetch_asm, plane_base = the
chunk's first locus) and rank 0 also writes <prefix>.asm.<ctx>.bed; no further collective.
-Q (with -A): every rank counts the tested loci of its chunk per (context, pcov1, ncov1, pcov2, ncov2) (all-reduce of 12 979 200
int64; the few loci beyond the bins by all_gather_object), computes the p of every tuple that occurs on its own device, solves the same
Benjamini-Hochberg q-values (hm_asm_qvalues) and writes its rows with the tenth column; rank 0 also writes <prefix>.asm.summary.tsv.
-G (with -A): every rank chains the tested loci of each (sequence, context) inside its chunk (hm_pileup_fetch_asm_regions with
keep_edges), the chains and the numbers of tested rows travel by all_gather_object, and rank 0 stitches the chains that cross a
chunk boundary (stitch_asm_regions) and writes <prefix>.asm.regions.<ctx>.bed.
-B control / -e rates: the per-locus binomial test.  After step 3 every rank sums the control sequence's part of its chunk
(all-reduce of 6 int64 -> the same rates everywhere), histograms its chunk per (motif, pcov, pcov + ncov) (all-reduce of
196 608 int64; the few loci beyond the histogram by all_gather_object), solves the same table (hm_sites_table) and writes its
chunk's rows by lookup; rank 0 also writes <prefix>.sites.<ctx>.bed and <prefix>.sites.rates.tsv.  No p-value crosses ranks.
-D: methylation domains of the combined planes.  A rank's pieces are its chunk cut at the sequence starts, one per (sequence,
context); a domain may cross any number of chunks.  Every rank runs pass S of hm_pileup_fetch_domains_part on its pieces, the
summaries travel by all_gather_object, every rank walks the same carries from left to right (domain_forward_carries), runs pass C,
gathers (d_last, back), walks from right to left (domain_backward_carries), runs pass G; the segments are gathered and rank 0 joins
those that cross a chunk boundary (stitch_domains) and writes <prefix>.domains.<ctx>.bed: three small exchanges in all, and
files byte-identical to `pileup -D`.
-D -Y n: the two levels fitted from the data first.  Per iteration passes S and C and the two walks as above, then
hm_pileup_domain_sums_part per piece (no segment is built) and one all-reduce of 18 int64, the three contexts' state sums; every
rank runs the same hm_domain_refit and stop rule (DomainFit) on them, so no level crosses ranks.  Rank 0 writes
<prefix>.domains.fit.tsv; it and the segments are byte-identical to `pileup -D -Y n`.
-L bp: within-read co-methylation by distance.  A record lives on one rank, so the four counts per distance are sums over the ranks:
every rank fetches all its distances (min_pairs 0), the [bp + 1, 4] int64 table goes through one all-reduce, and rank 0 applies -z
and writes <prefix>.linkage.CpG.tsv, byte-identical to `pileup -L bp`.
-P bp: methylation by position in the read.  A record lives on one rank and every rank counts with the same thresholds, so the three
sums of a row (n_m, n_u, sum_ml) are sums over the ranks: every rank fetches all its rows (min_calls 0), the [3 (2 bp + 1), 3] int64
table goes through one all-reduce, and rank 0 applies -y and writes <prefix>.readpos.tsv, byte-identical to `pileup -P bp`.
-I n5[:n3]: every rank's engine drops the entries at the read ends, as `pileup -I` does.
-R bed [-C min-cov] [-J bins[:flank:flank_bins]]: methylation of given intervals and the metaplot.  Every rank reads the same BED file
(before the device is touched: a bad file ends all ranks alike) and queries its own chunk of the reduce-scattered planes
(hm_pileup_fetch_regions / hm_pileup_fetch_metaplot with plane_base = the chunk's first locus: every interval and bin is clamped to
the chunk), the integer columns go through one all-reduce each -- they are exact sums, so the parts add up to the whole -- and rank 0
writes <prefix>.regions.<ctx>.tsv and <prefix>.metaplot.<ctx>.tsv, under -H per haplotype too, byte-identical to `pileup -R`.  The
metaplot's n_regions depends on neither planes nor chunk: every rank computes the same value and it is not summed.
-S flank [-O min-cov]: methylation by the k = 3 + 2 flank bases around each cytosine.  Every rank takes the table of its own chunk of
the reduce-scattered planes (hm_pileup_fetch_context with plane_base = the chunk's first locus; the whole reference is on every
rank's device, so a window reads across a chunk boundary like anywhere else), the [3, 4^k + 1, 4] integer tables go through one
all-reduce per set of planes, and rank 0 writes <prefix>.context.<ctx>.tsv, under -H per haplotype too, byte-identical to `pileup -S`.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import dist as D
from .bamio import is_coordinate_sorted, load_fasta, read_bam
from .caller import HifimethError
from .pileup import (ASM_DTYPE, CONTEXT_MAX_FLANK, CTX_NAMES, context_tsv, LINKAGE_DTYPE, LINKAGE_MAX_DIST, linkage_tsv, READPOS_MAX, readpos_tsv, REGION_SUM_DTYPE, metaplot_tsv, parse_metaplot, parse_regions_bed, regions_tsv, DOMAIN_LEVELS, DOMAIN_MAX_GAP, DOMAIN_PASS_CODES, DOMAIN_PASS_SEGMENTS, DOMAIN_PASS_SUMMARY,
                     DOMAIN_PENALTY, LOCUS_DTYPE, DomainFit, MethylationPileup, allreduce_histograms, asm_qvalues, asm_summary_tsv,
                     domain_backward_carries, domain_forward_carries, domain_scores, domains_fit_tsv, locus_ranges, parse_domain_levels, parse_rates,
                     rates_from_sums, reduce_scatter_planes, reduce_scatter_sum, resolve_threshold, sites_rates_tsv, sites_table,
                     stitch_asm_regions, stitch_domains)


def run(reference: str, bam: str, prefix: str, min_mapq: int = 0, min_pi: float = 0.0, slab: int = 256,
        batch: int = 256, backend: str | None = None, log=sys.stderr, haplotypes: bool = False, asm: bool = False,
        asm_min_cov: int = 5, control: str | None = None, rates=None, asm_q: bool = False,
        asm_regions: bool = False, max_p: float = 0.01, max_gap: int = 500, min_loci: int = 3, domain_rules=None,
        domain_max_gap: int = DOMAIN_MAX_GAP, domain_fit=None, linkage: int = 0, linkage_min_pairs: int = 1, profile: int = 0,
        profile_min_calls: int = 1, trim=(0, 0), regions_bed: str | None = None, region_min_cov: int = 1, metaplot=None,
        context_flank: int | None = None, context_min_cov: int = 1):
    """domain_rules (-D): per context (A, B, S) of domain_scores, or None for a context that is not segmented.  domain_fit (-Y):
    {"levels": per context (lo, hi) or None, "penalty", "max_iter"}: the levels are fitted from those and replace domain_rules.
    regions_bed (-R), region_min_cov (-C), metaplot (-J): (bins, flank, flank_bins) or None.  context_flank (-S): 0 .. 3 or None,
    context_min_cov (-O)"""
    import torch
    rank, local_rank, world = D.env_world()
    dist = D.init_process_group(backend, force=bool(os.environ.get("HM_FORCE_COLLECTIVES")))
    on_gpu = dist is None or dist.get_backend() == "nccl"
    text, refs, records = read_bam(bam)
    def leave(code):
        if dist is not None:
            dist.destroy_process_group()
        return code

    if not refs or not is_coordinate_sorted(text):          # s_bam_is_mapped_and_sorted (pileup.cpp:438-459)
        if rank == 0:
            print("ERROR: Methylation frequency could not be computed due to the following errors:", file=log)
            if not refs:
                print("BAM is not mapped", file=log)
            if not is_coordinate_sorted(text):
                print("BAM is not sorted", file=log)
        return leave(1)                                      # every rank sees the same header: all leave together
    genome = load_fasta(reference)
    sid_of = {n: i for i, (n, _) in enumerate(genome)}
    if control is not None and control not in sid_of:       # every rank reads the same FASTA: all leave together, before the device
        if rank == 0:
            print(f"ERROR: control sequence {control} (-B) is not in {reference}", file=log)
        return leave(1)
    regions = None
    if regions_bed is not None:                             # every rank reads the same file: all leave together, before the device
        try:
            regions = parse_regions_bed(regions_bed, [n for n, _ in genome], [len(s) for _, s in genome])
        except (OSError, ValueError) as e:
            if rank == 0:
                print(f"ERROR: {e}", file=log)
            return leave(1)
    missing = None
    n_loci = sum(len(s) for _, s in genome)
    ranges = locus_ranges(n_loci, world)
    chunk = max(1, (n_loci + world - 1) // world)
    ndev = max(torch.cuda.device_count(), 1)
    dev = torch.device("cuda", local_rank % ndev)
    torch.cuda.set_device(dev)
    planes = [torch.zeros(world * chunk, dtype=torch.int32, device=dev) for _ in range(3)]
    hp_planes = [torch.zeros(world * chunk, dtype=torch.int32, device=dev) for _ in range(4)] if haplotypes else []
    torch.cuda.synchronize()
    pu = MethylationPileup(genome, device=dev.index, min_mapq=min_mapq, min_pi=min_pi, planes=planes, partitions=haplotypes,
                           partition_planes=(hp_planes[0:2], hp_planes[2:4]) if haplotypes else None, linkage=linkage,
                           profile=profile, trim=trim)
    staged = 0
    for order, rec in enumerate(records):
        if (order // slab) % world != rank or rec.flag & 4 or rec.mm is None:
            continue
        name = refs[rec.tid][0]
        if name not in sid_of:                               # only the rank that owns the record sees it: flag, do not exit
            missing = name
            break
        rec.tid = sid_of[name]
        staged += pu.add(rec, order=order)
        if staged >= batch:
            pu.flush()
            staged = 0
    pu.flush()
    # a failed rank must not leave the others waiting in the collectives below: agree on the error first
    bad = torch.tensor([1 if missing else 0], dtype=torch.int32, device=dev if on_gpu else "cpu")
    if dist is not None:
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
    if int(bad.item()):
        if missing:
            print(f"ERROR: Sequence name {missing} does not exist", file=log)
        pu.close()
        return leave(1)
    bins = allreduce_histograms(dist, pu.histograms(), device=str(dev) if on_gpu else "cpu") if dist is not None \
        else pu.histograms()
    thr = []
    for c in range(3):
        t, samples = resolve_threshold(bins[c])
        thr.append(t)
        if rank == 0:
            print(f"{CTX_NAMES[c]} samples: {samples}\n{CTX_NAMES[c]} scaled probability threshold: {t}", file=log)
    pu.count(thr)
    torch.cuda.synchronize()
    if dist is not None:
        if not on_gpu:                                      # gloo rehearsal: collectives on host copies
            host = [t.cpu() for t in planes]
            pc, nc, key, base = reduce_scatter_planes(dist, *host)
            pc, nc, key = (t.to(dev) for t in (pc, nc, key))
            hp = [t.to(dev) for t in reduce_scatter_sum(dist, [t.cpu() for t in hp_planes])[0]] if haplotypes else []
        else:
            pc, nc, key, base = reduce_scatter_planes(dist, *planes, force=True)
            hp = reduce_scatter_sum(dist, hp_planes, force=True)[0] if haplotypes else []
        torch.cuda.synchronize()
    else:
        pc, nc, key, base = planes[0], planes[1], planes[2], 0
        hp = hp_planes
    lo, hi = ranges[rank]
    loci = pu.loci(0, hi - lo, planes=(pc, nc, key), plane_base=base)
    part = {"": pu.bed(loci)}                               # file tag -> {context: text}
    for k in range(len(hp) // 2):                           # a partition: its counts, the combined key's motif
        part[f"hap{k + 1}."] = pu.bed(pu.loci(0, hi - lo, planes=(hp[2 * k], hp[2 * k + 1], key), plane_base=base))
    where = "cpu" if dist is not None and not on_gpu else dev

    def allreduce_i64(a):
        if dist is None:
            return a
        t = torch.from_numpy(a.astype(np.int64).reshape(-1)).to(where)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.cpu().numpy().astype(np.uint64).reshape(a.shape)

    if asm:                                                 # the two partitions' chunks and the key's lie on the same range
        asm_planes, table = (*hp, key), None
        if asm_q:
            bins, big = pu.asm_histogram(0, hi - lo, asm_min_cov, planes=asm_planes, plane_base=base)
            bins = allreduce_i64(bins)
            if dist is not None:
                bigs = [None] * world
                dist.all_gather_object(bigs, big)
                big = np.concatenate(bigs).astype(ASM_DTYPE)  # rank order = locus order
            table = asm_qvalues(pu.asm_bin_pvalues(bins), big)
            del bins
            if rank == 0:
                with open(f"{prefix}.asm.summary.tsv", "w") as f:
                    f.write(asm_summary_tsv(table))
        part["asm."] = pu.asm_bed(pu.asm(0, hi - lo, asm_min_cov, planes=asm_planes, plane_base=base, table=table))
    if asm_regions:                                         # per (sequence, context): this rank's chains, edge chains kept
        chains = {}
        for sid in range(len(genome)):
            a, b = max(int(pu.offsets[sid]), lo), min(int(pu.offsets[sid + 1]), hi)
            for c in range(3 if a < b else 0):
                chains[sid, c] = pu.asm_regions(c, a - base, b - base, asm_min_cov, max_p, max_gap, min_loci, planes=(*hp, key),
                                              plane_base=base, keep_edges=True)
        every = [chains]
        if dist is not None:
            every = [None] * world
            dist.all_gather_object(every, chains)             # rank order = locus order
        if rank == 0:
            for c in range(3):
                with open(f"{prefix}.asm.regions.{CTX_NAMES[c]}.bed", "w") as f:
                    for sid in range(len(genome)):
                        rows, _ = stitch_asm_regions([m[sid, c] for m in every if (sid, c) in m], max_gap, min_loci)
                        f.write(pu.asm_regions_bed(rows)[CTX_NAMES[c]])
    if domain_rules is not None:                            # per (sequence, context): this rank's piece of the combined planes
        pieces = {}
        for sid in range(len(genome)):
            a, b = max(int(pu.offsets[sid]), lo), min(int(pu.offsets[sid + 1]), hi)
            for c in range(3 if a < b else 0):
                if domain_rules[c] is not None:
                    pieces[sid, c] = (a - base, b - base)

        def run_pass(pass_, carries=None):
            """one pass over this rank's pieces (after pass S: over those with rows) -> every rank's results, in rank order"""
            got = {k: pu.domains_part(k[1], a, b, pass_, carries and carries[k], *domain_rules[k[1]], domain_max_gap, planes=(pc, nc, key),
                                      plane_base=base) if carries is None or k in carries else {"n_rows": 0}
                   for k, (a, b) in pieces.items()}
            every = [got]
            if dist is not None:
                every = [None] * world
                dist.all_gather_object(every, got)
            return every

        def chains(every):                                   # (sequence, context) -> [(rank, result)], rank order = locus order
            out = {}
            for r, m in enumerate(every):
                for k, v in m.items():
                    out.setdefault(k, []).append((r, v))
            return out

        def segment_carries():
            """passes S and C under domain_rules with the two walks -> the carry of every piece of this rank that has rows"""
            sums = chains(run_pass(DOMAIN_PASS_SUMMARY))
            fwd = {k: domain_forward_carries([v for _, v in ch], domain_rules[k[1]][2], domain_max_gap) for k, ch in sums.items()}
            mine_of = lambda k: [r for r, _ in sums[k]].index(rank)  # noqa: E731  this rank's place in the chain of pieces k
            carry = {k: fwd[k][mine_of(k)] for k in pieces if sums[k][mine_of(k)][1]["n_rows"]}
            codes = chains(run_pass(DOMAIN_PASS_CODES, carry))
            bwd = {k: domain_backward_carries([v for _, v in sums[k]], [v for _, v in ch], domain_rules[k[1]][2], domain_max_gap)
                   for k, ch in codes.items()}
            return {k: {**f, **bwd[k][mine_of(k)]} for k, f in carry.items()}

        if domain_fit is not None:                           # -Y: every rank walks the same iteration, only the sums travel
            every_piece, domain_rules = pieces, list(domain_rules)
            fits = [None if lv is None else DomainFit(*lv, domain_fit["penalty"], domain_fit["max_iter"]) for lv in domain_fit["levels"]]
            while any(f is not None and f.status is None for f in fits):
                active = [f is not None and f.status is None for f in fits]
                pieces = {k: v for k, v in every_piece.items() if active[k[1]]}
                for c in range(3):
                    if active[c]:
                        domain_rules[c] = fits[c].rule
                carry = segment_carries()
                mine = np.zeros((3, 6), np.int64)
                for k, cr in carry.items():
                    mine[k[1]] += np.array(pu.domain_sums(k[1], *pieces[k], *domain_rules[k[1]], domain_max_gap, planes=(pc, nc, key),
                                                          plane_base=base, carry=cr), np.int64)
                total = allreduce_i64(mine).astype(np.int64)
                for c in range(3):
                    if active[c]:
                        fits[c].step(total[c])
            pieces = every_piece
            for c in range(3):
                if fits[c] is not None:
                    domain_rules[c] = fits[c].rule
            if rank == 0:
                with open(f"{prefix}.domains.fit.tsv", "w") as f:
                    f.write(domains_fit_tsv([None if x is None else (x.lo, x.hi, x.status, x.history) for x in fits]))
        segs = chains(run_pass(DOMAIN_PASS_SEGMENTS, segment_carries()))
        if rank == 0:
            for c in range(3):
                with open(f"{prefix}.domains.{CTX_NAMES[c]}.bed", "w") as f:
                    for sid in range(len(genome)):
                        if (sid, c) in segs:
                            rows = stitch_domains([v["segments"] for _, v in segs[sid, c] if v["n_rows"]], *domain_rules[c][:2])
                            f.write(pu.domains_bed(rows)[CTX_NAMES[c]])
    if linkage:                                             # records are dealt whole: the counts per distance add up over the ranks
        mine = pu.linkage(min_pairs=0)
        table = np.zeros((linkage + 1, 4), np.int64)
        table[mine["dist"]] = np.stack([mine[k] for k in ("n_uu", "n_um", "n_mu", "n_mm")], axis=1).astype(np.int64)
        table = allreduce_i64(table)
        if rank == 0:
            rows = np.zeros(linkage + 1, LINKAGE_DTYPE)
            rows["dist"] = np.arange(linkage + 1)
            for c, k in enumerate(("n_uu", "n_um", "n_mu", "n_mm")):
                rows[k] = table[:, c]
            rows = rows[2:]
            with open(f"{prefix}.linkage.CpG.tsv", "w") as f:
                f.write(linkage_tsv(rows[table[2:].sum(axis=1) >= linkage_min_pairs]))
    if profile:                                             # records are dealt whole and the thresholds are shared: the rows add up
        rows = pu.readpos(min_calls=0)
        table = allreduce_i64(np.stack([rows[k] for k in ("n_m", "n_u", "sum_ml")], axis=1).astype(np.int64))
        if rank == 0:
            for c, k in enumerate(("n_m", "n_u", "sum_ml")):
                rows[k] = table[:, c]
            with open(f"{prefix}.readpos.tsv", "w") as f:
                f.write(readpos_tsv(rows[table[:, 0] + table[:, 1] >= profile_min_calls]))
    if regions is not None:                                 # every interval and bin clamped to this rank's chunk: the parts add up
        xy = regions.coords(pu.offsets)
        sets = [("", (pc, nc, key))] + [(f"hap{k + 1}.", (hp[2 * k], hp[2 * k + 1], key)) for k in range(len(hp) // 2)]
        for tag, pl in sets:
            sums = pu.regions(xy["start"], xy["end"], region_min_cov, 0, hi - lo, planes=pl, plane_base=base)
            table = allreduce_i64(np.stack([sums[k] for k in REGION_SUM_DTYPE.names], axis=-1)).astype(np.int64)
            if metaplot is not None:
                bins, flank, flank_bins = metaplot
                rows, n_used = pu.metaplot(**xy, bins=bins, flank=flank, flank_bins=flank_bins, min_cov=region_min_cov, lo=0, hi=hi - lo,
                                           planes=pl, plane_base=base)
                mtab = allreduce_i64(np.stack([rows[k] for k in REGION_SUM_DTYPE.names], axis=-1)).astype(np.int64)
            if rank == 0:
                for c, k in enumerate(REGION_SUM_DTYPE.names):
                    sums[k] = table[..., c]
                for ctx, text in regions_tsv(regions, pu.names, sums).items():
                    with open(f"{prefix}.{tag}regions.{ctx}.tsv", "w") as f:
                        f.write(text)
                if metaplot is not None:
                    for c, k in enumerate(REGION_SUM_DTYPE.names):
                        rows[k] = mtab[..., c]                  # n_regions stays: the same on every rank
                    for ctx, text in metaplot_tsv(rows, n_used, len(regions) - n_used, bins, flank_bins).items():
                        with open(f"{prefix}.{tag}metaplot.{ctx}.tsv", "w") as f:
                            f.write(text)
    if context_flank is not None:                           # exact integer sums per k-mer: the chunks' tables add up to the whole's
        sets = [("", (pc, nc, key))] + [(f"hap{k + 1}.", (hp[2 * k], hp[2 * k + 1], key)) for k in range(len(hp) // 2)]
        for tag, pl in sets:
            mine = pu.context(context_flank, context_min_cov, 0, hi - lo, planes=pl, plane_base=base) if hi > lo \
                else np.zeros((3, 4 ** (3 + 2 * context_flank) + 1, 4), np.int64)
            table = allreduce_i64(mine).astype(np.int64)
            if rank == 0:
                for ctx, text in context_tsv(table, context_flank).items():
                    with open(f"{prefix}.{tag}context.{ctx}.tsv", "w") as f:
                        f.write(text)
    if control is not None or rates is not None:
        mine, n_mine = (pc, nc, key), hi - lo               # this rank's chunk: element 0 is locus `base`
        sums = np.zeros(6, np.uint64)
        if control is not None:
            c0 = int(pu.offsets[sid_of[control]])
            c1 = c0 + len(genome[sid_of[control]][1])
            a, b = min(max(c0 - base, 0), n_mine), min(max(c1 - base, 0), n_mine)
            sums = allreduce_i64(pu.control_sums(a, b, planes=mine) if a < b else sums)
            rates = rates_from_sums(sums)
        bins, big = pu.site_histogram(0, n_mine, planes=mine, plane_base=base)
        bins = allreduce_i64(bins)
        if dist is not None:
            bigs = [None] * world
            dist.all_gather_object(bigs, big)
            big = np.concatenate(bigs).astype(LOCUS_DTYPE)  # rank order = locus order
        table = sites_table(rates, bins, big)
        part["sites."] = pu.sites_bed(pu.sites(table, 0, n_mine, planes=mine, plane_base=base))
        if rank == 0:
            for c in range(3):
                print(f"WARNING: {CTX_NAMES[c]} is not tested: no rate" if np.isnan(rates[c])
                      else f"{CTX_NAMES[c]} false-positive rate: {rates[c]:.17g}", file=log)
            with open(f"{prefix}.sites.rates.tsv", "w") as f:
                f.write(sites_rates_tsv(sums, rates, table.m))
    if dist is not None:
        parts = [None] * world if rank == 0 else None
        dist.gather_object(part, parts, dst=0)
    else:
        parts = [part]
    if rank == 0:
        for tag in parts[0]:
            for c in CTX_NAMES:
                with open(f"{prefix}.{tag}{c}" + (".bed" if tag in ("asm.", "sites.") else ".cov.bed"), "w") as f:
                    for p in parts:
                        f.write(p[tag][c])
    pu.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m hifimeth_amd.pileup_dist")
    ap.add_argument("-q", type=int, default=0, help="minimum mapping quality")
    ap.add_argument("-f", type=float, default=0.0, help="minimum alignment identity (percent)")
    ap.add_argument("--slab", type=int, default=256, help="records per slab dealt to a rank")
    ap.add_argument("--backend", default=None, help="nccl (RCCL, default on GPUs) or gloo")
    ap.add_argument("-H", dest="haplotypes", action="store_true",
                    help="haplotype-resolved output: also <prefix>.hap1.* / <prefix>.hap2.* from the HP tag")
    ap.add_argument("-A", dest="asm", action="store_true",
                    help="with -H: per-locus haplotype difference + Fisher exact test -> <prefix>.asm.<ctx>.bed")
    ap.add_argument("-a", dest="asm_min_cov", type=int, default=None, help="with -A: minimum coverage of each haplotype (default 5)")
    ap.add_argument("-Q", dest="asm_q", action="store_true",
                    help="with -A: Benjamini-Hochberg q-value per tested locus (tenth column), <prefix>.asm.summary.tsv")
    ap.add_argument("-G", dest="asm_regions", action="store_true",
                    help="with -A: runs of tested loci with p <= -s and a difference of one sign -> <prefix>.asm.regions.<ctx>.bed")
    ap.add_argument("-s", dest="max_p", type=float, default=None, help="with -G: largest p-value of a locus in a region, in (0, 1] (default 0.01)")
    ap.add_argument("-g", dest="max_gap", type=int, default=None, help="with -G: largest distance between consecutive loci, >= 1 (default 500)")
    ap.add_argument("-n", dest="min_loci", type=int, default=None, help="with -G: smallest number of loci of a region, >= 1 (default 3)")
    ap.add_argument("-B", dest="control", default=None, metavar="NAME",
                    help="per-locus binomial test against the false-positive rates measured on this unmethylated control sequence "
                         "-> <prefix>.sites.<ctx>.bed, <prefix>.sites.rates.tsv")
    ap.add_argument("-e", dest="rates", default=None, metavar="R,R,R",
                    help="instead of -B: the three rates (CpG,CHG,CHH), each a decimal in [0, 1] or nan (context not tested)")
    ap.add_argument("-D", dest="domains", action="store_true",
                    help="cut the covered loci of each context into low (L) and high (H) methylated stretches -> <prefix>.domains.<ctx>.bed")
    ap.add_argument("-u", dest="domain_levels", default=None, metavar="LO:HI[,LO:HI,LO:HI]",
                    help="with -D: the low and the high methylation level, 0 < lo < hi < 1, once or per context (CpG,CHG,CHH); nan instead "
                         "of a pair: that context is not segmented (default 0.1:0.8,0.05:0.5,0.02:0.2)")
    ap.add_argument("-x", dest="domain_penalty", type=float, default=None, help="with -D: penalty of a change of state in nats, in [0, 256] (default 8)")
    ap.add_argument("-j", dest="domain_max_gap", type=int, default=None, help="with -D: largest distance between two loci that still links them, >= 1 (default 1000)")
    ap.add_argument("-Y", dest="domain_fit", type=int, default=None, metavar="N",
                    help="with -D: fit the two levels of every segmented context from the data, starting from -u, at most N iterations "
                         "-> also <prefix>.domains.fit.tsv")
    ap.add_argument("-L", dest="linkage", type=int, default=None, metavar="BP",
                    help="within-read co-methylation by distance up to BP bases, in [2, 16384] -> <prefix>.linkage.CpG.tsv")
    ap.add_argument("-z", dest="linkage_min_pairs", type=int, default=None, help="with -L: smallest number of pairs of a distance that is written, >= 0 (default 1)")
    ap.add_argument("-P", dest="profile", type=int, default=None, metavar="BP",
                    help="methylation by position in the read, the BP bases at either end a row each, in [1, 2048] -> <prefix>.readpos.tsv")
    ap.add_argument("-y", dest="profile_min_calls", type=int, default=None, help="with -P: smallest number of calls of a row that is written, >= 0 (default 1)")
    ap.add_argument("-I", dest="trim", default=None, metavar="N5[:N3]",
                    help="leave the calls in the first N5 and the last N3 bases of every read out of all outputs (one number: both ends)")
    ap.add_argument("-R", dest="regions_bed", default=None, metavar="BED",
                    help="methylation of the intervals of this BED file (plain or gzip) -> <prefix>.regions.<ctx>.tsv")
    ap.add_argument("-C", dest="region_min_cov", type=int, default=None, help="with -R: smallest coverage of a locus that counts, >= 1 (default 1)")
    ap.add_argument("-J", dest="metaplot", default=None, metavar="BINS[:FLANK_BP:FLANK_BINS]",
                    help="with -R: the metaplot over all intervals and their flanks -> <prefix>.metaplot.<ctx>.tsv")
    ap.add_argument("-S", dest="context_flank", type=int, default=None, metavar="FLANK",
                    help="methylation by the 3 + 2 FLANK bases around each cytosine, FLANK in 0 .. 3 -> <prefix>.context.<ctx>.tsv")
    ap.add_argument("-O", dest="context_min_cov", type=int, default=None, help="with -S: smallest coverage of a locus that counts, >= 1 (default 1)")
    ap.add_argument("reference")
    ap.add_argument("mod_bam")
    ap.add_argument("output_prefix")
    a = ap.parse_args(argv)
    if a.asm and not a.haplotypes:
        ap.error("-A needs -H")
    if a.asm_min_cov is not None and not a.asm:
        ap.error("-a needs -A")
    if a.asm_min_cov is not None and a.asm_min_cov < 1:
        ap.error("-a must be >= 1")
    if a.asm_q and not a.asm:
        ap.error("-Q needs -A")
    if a.asm_regions and not a.asm:
        ap.error("-G needs -A")
    if not a.asm_regions and not (a.max_p is None and a.max_gap is None and a.min_loci is None):
        ap.error("-s, -g and -n need -G")
    if a.max_p is not None and not 0.0 < a.max_p <= 1.0:
        ap.error("-s must be in (0, 1]")
    if (a.max_gap is not None and a.max_gap < 1) or (a.min_loci is not None and not 1 <= a.min_loci < 2 ** 31):
        ap.error("-g and -n must be >= 1")
    if a.control is not None and a.rates is not None:
        ap.error("-B and -e exclude each other")
    rates = None
    if a.rates is not None:
        try:
            rates = parse_rates(a.rates)
        except ValueError as e:
            ap.error(f"-e: {e}")
    if not a.domains and not (a.domain_levels is None and a.domain_penalty is None and a.domain_max_gap is None):
        ap.error("-u, -x and -j need -D")
    if a.domain_fit is not None and not a.domains:
        ap.error("-Y needs -D")
    if a.domain_fit is not None and a.domain_fit < 1:
        ap.error("-Y takes the largest number of iterations, an integer >= 1")
    if a.linkage_min_pairs is not None and a.linkage is None:
        ap.error("-z needs -L")
    if (a.linkage is not None and not 2 <= a.linkage <= LINKAGE_MAX_DIST) or (a.linkage_min_pairs is not None and a.linkage_min_pairs < 0):
        ap.error("-L must be an integer in [2, 16384], -z an integer >= 0")
    if a.profile_min_calls is not None and a.profile is None:
        ap.error("-y needs -P")
    parts = (a.trim or "0").split(":")
    bad_trim = not 1 <= len(parts) <= 2 or not all(t.isascii() and t.isdigit() and int(t) < 2 ** 31 for t in parts)
    trim = (0, 0) if bad_trim else (int(parts[0]), int(parts[-1]))
    if bad_trim or (a.profile is not None and not 1 <= a.profile <= READPOS_MAX) or (a.profile_min_calls is not None and a.profile_min_calls < 0):
        ap.error("-P must be an integer in [1, 2048], -y an integer >= 0, -I n5[:n3] with integers >= 0")
    if a.regions_bed is None and not (a.region_min_cov is None and a.metaplot is None):
        ap.error("-C and -J need -R")
    metaplot = None
    try:
        if a.region_min_cov is not None and a.region_min_cov < 1:
            raise ValueError
        metaplot = None if a.metaplot is None else parse_metaplot(a.metaplot)
    except ValueError:
        ap.error("-C must be an integer >= 1, -J bins[:flank_bp:flank_bins] with bins in [1, 1000] and flank_bp a multiple of flank_bins in [1, 1000]")
    if a.context_flank is None and a.context_min_cov is not None:
        ap.error("-O needs -S")
    if (a.context_flank is not None and not 0 <= a.context_flank <= CONTEXT_MAX_FLANK) or (a.context_min_cov is not None and a.context_min_cov < 1):
        ap.error("-S must be an integer in [0, 3], -O an integer >= 1")
    domain_rules = domain_fit = None
    if a.domains:
        bad = "-u takes lo:hi with 0 < lo < hi < 1 (levels a 2^24-th of a nat apart at least) or nan, once or per context; " \
              "-x must be in [0, 256], -j an integer >= 1"
        penalty = DOMAIN_PENALTY if a.domain_penalty is None else a.domain_penalty
        if not 0.0 <= penalty <= 256.0 or (a.domain_max_gap is not None and a.domain_max_gap < 1):
            ap.error(bad)
        try:
            levels = list(DOMAIN_LEVELS) if a.domain_levels is None else parse_domain_levels(a.domain_levels)
            domain_rules = [None if lv is None else domain_scores(*lv, penalty) for lv in levels]
            if a.domain_fit is not None:
                domain_fit = {"levels": levels, "penalty": penalty, "max_iter": a.domain_fit}
        except (ValueError, HifimethError):
            ap.error(bad)
    return run(a.reference, a.mod_bam, a.output_prefix, a.q, a.f, slab=a.slab, backend=a.backend, haplotypes=a.haplotypes,
               asm=a.asm, asm_min_cov=5 if a.asm_min_cov is None else a.asm_min_cov, control=a.control, rates=rates,
               asm_q=a.asm_q, asm_regions=a.asm_regions, max_p=0.01 if a.max_p is None else a.max_p,
               max_gap=500 if a.max_gap is None else a.max_gap, min_loci=3 if a.min_loci is None else a.min_loci,
               domain_rules=domain_rules, domain_max_gap=DOMAIN_MAX_GAP if a.domain_max_gap is None else a.domain_max_gap,
               domain_fit=domain_fit, linkage=a.linkage or 0, linkage_min_pairs=1 if a.linkage_min_pairs is None else a.linkage_min_pairs,
               profile=a.profile or 0, profile_min_calls=1 if a.profile_min_calls is None else a.profile_min_calls, trim=trim,
               regions_bed=a.regions_bed, region_min_cov=1 if a.region_min_cov is None else a.region_min_cov, metaplot=metaplot,
               context_flank=a.context_flank, context_min_cov=1 if a.context_min_cov is None else a.context_min_cov)


if __name__ == "__main__":
    sys.exit(main())
