"""Pileup on a real reference of more than 2^31 and more than 2^32 bases: a small job, then the same job behind a pad of 'N' that
puts a boundary B on a chosen locus (tests/bigref.py), and every result of the big job must equal the small job's with the loci
translated -- exactly, floats as bits.  The engine's results may not depend on where in the concatenated reference a contig lies.

Six cases: B = 2^31 with haplotype partitions (7 planes, about 65 GB on the card), B = 2^32 without (3 planes, about 61 GB), each
with the boundary on a covered CpG, on a reverse-strand CHH record (decided two columns below B) and on a contig start.  One
big engine is alive at a time; the 4 GB host buffers are built once per boundary.  A case skips, naming both numbers, when the
card has less free memory than it needs plus 8 GB.  The small job is itself checked against oracle/pileup_oracle.py.

A stage argument orders the work from safe to less safe: the projection only reads the reference (stage "records"), counting
writes the planes ("count"), the fetches read them ("fetch"), and so do the outputs that came after those ("extras": domains and
their sums, allele-specific regions, interval sums and metaplots, the k-mer table), on the same engine and with no option set.

Three more cases give the big engine the options behind patterns, bedMethyl, linkage and the read-position table (2^32 cpg_at_B and
contig_at_B plain, 2^31 cpg_at_B with partitions), each against a small job built with the same options."""
import ctypes
import time

import numpy as np
import pytest

import bigref as R

pytestmark = pytest.mark.gpu
MIN_COV = 1                                                    # of the haplotype test: at 3x coverage the rows must not run out
STAGES = ("records", "count", "fetch", "extras")


class HostBuffers:
    """the reference ('N') and the label array (-1) of one boundary, HOST_LEN long; place() writes the small job behind the pad
    and takes the previous placement's bytes out again"""
    def __init__(self, B):
        self.B = B
        self.ref = np.full(R.HOST_LEN[B], ord("N"), np.uint8)
        self.labels = np.full(R.HOST_LEN[B], -1, np.int8)
        self.at = (0, 0)

    def place(self, P, small_ref, small_lab):
        lo, hi = self.at
        self.ref[lo:hi], self.labels[lo:hi] = ord("N"), -1
        total = P + len(small_ref)
        assert total <= len(self.ref)
        self.ref[P:total], self.labels[P:total] = small_ref, small_lab
        self.at = (P, total)
        return self.ref[:total], self.labels[:total]


class HostCache:
    """one boundary's buffers at a time: the host never holds more than 2 x (2^32 + 40000) bytes of them"""
    def __init__(self):
        self.held = None

    def get(self, B):
        if self.held is None or self.held.B != B:
            self.held = None
            self.held = HostBuffers(B)
        return self.held


class Small:
    """the small job on the device: what is only there before count() is kept, the counted engine stays for the range fetches"""
    def __init__(self, partitions, options=None):
        """options: None, or the engine options of R.option_sets -- then the outputs they switch on are fetched and checked too"""
        from hifimeth_amd.pileup import AsmTable, MethylationPileup, asm_qvalues, sites_table
        genome, reads = R.small_job()
        want, _n = R.oracle_small()
        self.partitions, self.n = partitions, sum(len(s) for _, s in genome)
        self.ref = np.frombuffer("".join(s for _, s in genome).encode(), np.uint8)
        self.lab = R.small_labels(self.n)
        self.options = options
        pu = self.pu = MethylationPileup(genome, min_pi=R.MIN_PI, partitions=partitions, **(options or {}))
        off = pu.offsets
        feed(pu, reads)
        self.n_pattern_records = pu.num_pattern_records() if options else 0
        self.hist = pu.histograms()
        self.records = R.sorted_records(*pu.records())
        self.label_hist = pu.label_histograms(self.lab)
        self.thr = pu.resolve_thresholds(self.hist)
        # ... against the oracle, as test_gpu_pileup.py::_check does: bins, records, thresholds, loci, BED text
        assert (self.hist == want["bins"]).all() and self.thr == want["thresholds"]
        exp = sorted((int(off[sid] + soff), prob, motif) for sid, soff, prob, motif in want["records"])
        assert list(zip(self.records["gpos"].tolist(), self.records["prob"].tolist(), self.records["motif"].tolist())) == exp
        assert self.label_hist.sum() > 1000 and (self.label_hist.sum(axis=(1, 2)) > 0).all()
        pu.count(self.thr)
        self.loci = pu.loci()
        R.assert_same_rows(self.loci, R.oracle_locus_rows(want, off), "small loci against the oracle")
        self.bed = pu.bed(self.loci)
        assert self.bed == want["bed"]
        self.site_bins, self.site_big = pu.site_histogram()
        self.sites_table = sites_table(R.RATES, self.site_bins, self.site_big)
        self.asm_table = None
        if partitions:
            self.asm_bins, self.asm_big = pu.asm_histogram(min_cov=MIN_COV)
            self.asm_tab = pu.asm_bin_pvalues(self.asm_bins)
            self.asm_table = asm_qvalues(self.asm_tab, self.asm_big)
            assert isinstance(self.asm_table, AsmTable) and len(self.asm_tab) > 10
        self.cache = {}
        self.extras = {}
        if partitions:                                         # the rows of the haplotype test against the oracle's counts and the
            got, exp = self.rows("asm", 0, self.n), R.expected_asm_rows()     # exact p: the chains' reference is fed with the device's rows
            assert len(got) == len(exp) and all((got[f] == exp[f]).all() for f in ("gpos", "pcov1", "ncov1", "pcov2", "ncov2", "motif"))
            assert got["diff"].tobytes() == exp["diff"].tobytes() and np.allclose(got["pvalue"], exp["pvalue"], rtol=1e-9, atol=0)
            assert ((got["pvalue"] <= R.ASM_MAX_P) == (exp["pvalue"] <= R.ASM_MAX_P)).all()
        if options:
            self.check_options()

    def option_rows(self, kind, *args):
        """patterns / bedmethyl / linkage / readpos / readpos_histograms of the small job, fetched once"""
        if (kind,) + args not in self.cache:
            self.cache[(kind,) + args] = getattr(self.pu, kind)(*args)
        return self.cache[(kind,) + args]

    def check_options(self):
        """the outputs behind the engine options against their CPU restatements (tests/bigref.py)"""
        opts, n_sets = R.option_sets(self.partitions)
        assert self.options == opts and self.n_pattern_records > 1000
        R.assert_same_rows(self.option_rows("patterns", 0, self.n, 1), R.expected_patterns(opts["patterns"]), "small patterns")
        for part in range(n_sets):
            for min_valid in (0, 1):
                R.assert_same_rows(self.option_rows("bedmethyl", 0, self.n, min_valid, part), R.expected_bedmethyl(min_valid, part),
                                   "small bedMethyl, set %d, min_valid %d" % (part, min_valid))
        R.assert_same_rows(self.option_rows("linkage", 0), R.expected_linkage(0), "small linkage")
        R.assert_same_rows(self.option_rows("readpos", 0), R.expected_readpos(0), "small read position")
        assert (self.option_rows("readpos_histograms") == R.expected_readpos_histograms()).all()

    def extra(self, key, make, check):
        """one of the newer outputs of the small job, fetched once and checked against its CPU restatement"""
        if key not in self.extras:
            self.extras[key] = make(self.pu)
            check(self.extras[key])
        return self.extras[key]

    def tables(self, P):
        """the two lookup tables as the big job needs them: their big lists moved by P"""
        from hifimeth_amd.pileup import AsmTable, SitesTable
        s, a = self.sites_table, self.asm_table
        st = SitesTable(s.rates, s.ptab, s.qtab, R.translate(s.big, P), s.big_p, s.big_q, s.m)
        return st, a and AsmTable(a.tab, R.translate(a.big, P), a.big_q, a.m)

    def rows(self, kind, lo, hi):
        if (kind, lo, hi) not in self.cache:
            self.cache[kind, lo, hi] = fetch(self.pu, kind, lo, hi, self.sites_table, self.asm_table)
        return self.cache[kind, lo, hi]

    def close(self):
        self.pu.close()


def feed(pu, reads, batch=16):
    for i, r in enumerate(reads):
        pu.add(r)
        if (i + 1) % batch == 0:
            pu.flush()                    # several batches: records accumulate in HBM across runs
    pu.flush()


def kinds(partitions):
    return ("loci", "sites") + (("part1", "part2", "asm", "asmq") if partitions else ())


def fetch(pu, kind, lo, hi, sites_tab, asm_tab):
    if kind == "loci":
        return pu.loci(lo, hi)
    if kind in ("part1", "part2"):
        return pu.loci(lo, hi, partition=int(kind[-1]))
    if kind == "sites":
        return pu.sites(sites_tab, lo, hi)
    if kind == "asm":
        return pu.asm(lo, hi, min_cov=MIN_COV)
    if kind == "asmq":
        return pu.asm(lo, hi, min_cov=MIN_COV, table=asm_tab)
    raise ValueError(kind)


# ---- the outputs that need no engine option ---------------------------------------------------------------------------------------------
def context_runs():
    from hifimeth_amd.pileup import CONTEXT_PATH_AUTO, CONTEXT_PATH_GLOBAL
    return [(f, CONTEXT_PATH_AUTO) for f in R.CONTEXT_FLANKS] + [(f, CONTEXT_PATH_GLOBAL) for f in (0, 1, 2)]


ROW_CAP = 4096                                                 # rows of one fetch of this job: a few hundred at the most


def rows_once(pu, fn, dtype, *args):
    """a row fetch of the C ABI in ONE call, into a buffer that holds every row of this job -> (rows, n_ctx_rows).  pu.domains and
    pu.asm_regions ask for the number first and fetch then: each is a whole pass over the planes, 20 ms at this size"""
    out, n_ctx_rows = np.zeros(ROW_CAP, dtype), ctypes.c_int64(0)
    n = pu._check(fn(pu._h, *args, ctypes.byref(n_ctx_rows), out.ctypes.data_as(ctypes.c_void_p), ROW_CAP))
    assert n <= ROW_CAP
    return out[:n].copy(), int(n_ctx_rows.value)


def row_extras(pu, partitions, lo, hi):
    """{name: (rows, n_ctx_rows) or the six sums} of [lo, hi): the outputs of the row-scan skeleton"""
    from hifimeth_amd.pileup import ASM_REGION_DTYPE, DOMAIN_DTYPE, DOMAIN_MAX_GAP
    out = {}
    for ctx in range(3):
        out["domains%d" % ctx] = rows_once(pu, pu._L.hm_pileup_fetch_domains, DOMAIN_DTYPE, None, None, None, 0, lo, hi, ctx,
                                           *R.domain_scores_of(ctx), DOMAIN_MAX_GAP)
        out["domain_sums%d" % ctx] = pu.domain_sums(ctx, lo, hi)
        if partitions:
            out["asm_regions%d" % ctx] = rows_once(pu, pu._L.hm_pileup_fetch_asm_regions, ASM_REGION_DTYPE, None, None, None, None, None, 0,
                                                   lo, hi, MIN_COV, ctx, R.ASM_MAX_P, R.ASM_MAX_GAP, R.ASM_MIN_LOCI, 1)
    return out


def check_row_extras(small, lo, hi):
    def check(got):
        for ctx in range(3):
            if (lo, hi) == (0, small.n):                       # the Python entry points give what the single call gave
                R.assert_same_rows(small.pu.domains(ctx, lo, hi)[0], got["domains%d" % ctx][0], "pu.domains")
                if small.partitions:
                    R.assert_same_rows(small.pu.asm_regions(ctx, lo, hi, min_cov=MIN_COV, max_p=R.ASM_MAX_P, max_gap=R.ASM_MAX_GAP,
                                                            min_loci=R.ASM_MIN_LOCI, keep_edges=True)[0], got["asm_regions%d" % ctx][0], "pu.asm_regions")
            seg, n_rows, sums = R.expected_domains(R.oracle_loci(), ctx, lo, hi)
            R.assert_same_rows(got["domains%d" % ctx][0], seg, "small domains %d [%d, %d)" % (ctx, lo, hi))
            assert got["domains%d" % ctx][1] == n_rows and got["domain_sums%d" % ctx] == sums
            if small.partitions:
                chains, n_rows = R.expected_asm_regions(small.rows("asm", 0, small.n), ctx, lo, hi)
                R.assert_same_rows(got["asm_regions%d" % ctx][0], chains, "small asm regions %d [%d, %d)" % (ctx, lo, hi))
                assert got["asm_regions%d" % ctx][1] == n_rows
    return check


def same_row_extras(got, want, P, what):
    assert got.keys() == want.keys()
    for k in got:
        if k.startswith("domain_sums"):
            assert got[k] == want[k], (what, k)
        else:
            R.assert_same_rows(got[k][0], R.translate(want[k][0], P), "%s %s" % (k, what))
            assert got[k][1] == want[k][1], (what, k)


def sum_extras(pu, partitions, P, g, lo, hi, meta=True):
    """{name: int64 table} of [lo, hi): the sums of the fixed intervals around the placed locus g (moved by P) per min_cov and
    partition, and the metaplot with its n_used"""
    start, end = R.intervals(g)
    out = {}
    for part in (0, 1, 2) if partitions else (0,):
        for min_cov in R.REGION_MIN_COVS:
            out["regions", part, min_cov] = R.region_table(pu.regions(start + P, end + P, min_cov, lo, hi, partition=part))
    if meta:
        a, b, s0, s1, strand = R.meta_intervals()
        rows, n_used = pu.metaplot(a + P, b + P, s0 + P, s1 + P, strand, lo=lo, hi=hi, **R.META)
        out["metaplot"] = R.meta_table(rows)
        out["n_used"] = np.array([n_used])
    return out


def check_sum_extras(small, g, lo, hi):
    def check(got):
        start, end = R.intervals(g)
        for (_r, part, min_cov) in [k for k in got if k[0] == "regions"]:
            if part == 0:
                assert (got["regions", 0, min_cov] == R.expected_regions(start, end, min_cov, 0, lo, hi)).all(), (min_cov, lo, hi)
            else:                                          # a partition's own loci, through the restatement
                import regions_ref
                run = regions_ref.Running(*regions_ref.planes_from_loci(small.rows("part%d" % part, 0, small.n), small.n), min_cov=min_cov)
                assert (got["regions", part, min_cov] == regions_ref.region_sums(run, start, end, lo, hi)).all(), (part, min_cov, lo, hi)
        if "metaplot" in got:
            tab, used = R.expected_metaplot(*R.meta_intervals(), 1, 0, lo, hi)
            assert (got["metaplot"] == tab).all() and got["n_used"][0] == used
    return check


def context_extras(pu, lo, hi):
    return {(f, path): pu.context(f, lo=lo, hi=hi, path=path) for f, path in context_runs()}


def check_context_extras(lo, hi):
    def check(got):
        for (f, path), tab in got.items():
            assert (tab == R.expected_context(f, lo, hi)).all(), (f, path, lo, hi)
    return check


def same_tables(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)


def small_extra(small, kind, g, lo, hi):
    """the small job's side of one extras fetch over its [lo, hi), checked against the CPU restatements on first use"""
    part = small.partitions
    if kind == "rows":
        return small.extra((kind, lo, hi), lambda spu: row_extras(spu, part, lo, hi), check_row_extras(small, lo, hi))
    if kind in ("sums", "sums+meta"):
        meta = kind == "sums+meta"
        return small.extra((kind, g, lo, hi), lambda spu: sum_extras(spu, part, 0, g, lo, hi, meta), check_sum_extras(small, g, lo, hi))
    return small.extra((kind, lo, hi), lambda spu: context_extras(spu, lo, hi), check_context_extras(lo, hi))


def extras_plan(small, B, P, g):
    """[(kind, name, (big lo, big hi), (small lo, small hi))].  Every output runs over the whole reference; the row outputs also
    over `around` and `near`, the interval sums over `near` (off the block grid) and the halves at B, which must add up, the k-mer
    table over the halves at 2^31, where the stage has the room.  A whole-range pass costs 10 to 25 ms of plane reads.  With every
    range of R.ranges and the single sequences for every output the stage took 0.6 s at 2^31 and 0.75 s at 2^32 against 0.4 s and
    0.28 s of fetches; as it is, 0.25 s and 0.27 s (profiles/bigref_outputs.txt).  What is left out are ranges, no output: the
    halves and the single sequences of the row outputs, and at 2^32 the halves of the k-mer table."""
    rngs = R.ranges(B, P, small.n)
    plan = [("rows", nm, big, sm) for nm, big, sm in rngs if nm in ("all", "around", "near")]
    plan += [("sums" if nm == "near" else "sums+meta", nm, big, sm) for nm, big, sm in rngs if nm in ("all", "below", "above", "near")]
    plan += [("context", nm, big, sm) for nm, big, sm in rngs if nm == "all" or (B == R.B31 and nm in ("below", "above"))]
    return plan


def run_extras(pu, small, B, P, g):
    """the big job's newer outputs against the small job's (fetched and checked before the big engine's clock started)"""
    part = small.partitions
    got, secs = {}, {}
    for kind, nm, (blo, bhi), (slo, shi) in extras_plan(small, B, P, g):
        t0 = time.perf_counter()
        want = small_extra(small, kind, g, slo, shi)
        what = "%s %s [%d, %d)" % (kind, nm, blo, bhi)
        if kind == "rows":
            got[kind, nm] = row_extras(pu, part, blo, bhi)
            same_row_extras(got[kind, nm], want, P, what)
        elif kind == "context":
            got[kind, nm] = context_extras(pu, blo, bhi)
            same_tables(got[kind, nm], want, what)
        else:
            got["sums", nm] = sum_extras(pu, part, P, g, blo, bhi, kind == "sums+meta")
            same_tables(got["sums", nm], want, what)
        secs[kind[:4]] = secs.get(kind[:4], 0.0) + time.perf_counter() - t0
    print("bigref extras: " + ", ".join("%s %.2f s" % kv for kv in secs.items()))
    for ctx in range(3):                                       # the boundary lies inside a segment (and a chain) of every context
        rows = got["rows", "all"]["domains%d" % ctx][0]
        assert ((rows["start"] <= B) & (B < rows["end"])).sum() == 1
        assert (rows["end"] <= B).any() and (rows["start"] > B).any()
        if part:
            chains = got["rows", "all"]["asm_regions%d" % ctx][0]
            assert ((chains["start"] <= B) & (B < chains["end"])).sum() == 1
    if part:
        assert sum(int((got["rows", "all"]["asm_regions%d" % c][0]["n_loci"] >= 2).sum()) for c in range(3)) >= 3
    assert (B - 5000) % R.region_block()                       # `near` begins off the block grid of the region index
    for k, whole in got["sums", "all"].items():                # the halves at B add up
        lo_, hi_ = got["sums", "below"][k], got["sums", "above"][k]
        if k == "metaplot":                                    # n_regions is no range's business: every part reports all of it
            assert (lo_[:, :, 0] == whole[:, :, 0]).all() and (hi_[:, :, 0] == whole[:, :, 0]).all()
            assert (lo_[:, :, 1:] + hi_[:, :, 1:] == whole[:, :, 1:]).all() and lo_[:, :, 1].any() and hi_[:, :, 1].any()
        elif k == "n_used":
            assert lo_ == hi_ == whole
        else:
            assert (lo_ + hi_ == whole).all() and lo_.any() and hi_.any(), k
    for k, tab in got["context", "all"].items():                # nothing moves and the pad adds nothing: the table is the small job's
        assert tab[:, :-1, 0].any() and tab.shape == (3, 4 ** (3 + 2 * k[0]) + 1, 4), k
        if ("context", "below") in got:                        # the halves at B add up
            lo_, hi_ = got["context", "below"][k], got["context", "above"][k]
            assert (lo_ + hi_ == tab).all() and lo_.any() and hi_.any(), k


def run_options(pu, small, B, P, name):
    """the outputs behind the engine options: the big job's against the small job's (checked against the CPU restatements)"""
    total = P + small.n
    _opts, n_sets = R.option_sets(small.partitions)
    rngs = R.ranges(B, P, small.n)
    rngs += [("seq%d" % s, (int(pu.offsets[s]), int(pu.offsets[s + 1])), (max(int(pu.offsets[s]) - P, 0), int(pu.offsets[s + 1]) - P))
             for s in range(len(pu.names))]
    got = {}
    for nm, (blo, bhi), (slo, shi) in rngs:
        got[nm] = pu.patterns(blo, bhi, 1)
        if nm == "seq0":                                       # the pad: no reference CpG, no row of any set
            assert len(got[nm]) == 0 and all(len(pu.bedmethyl(blo, bhi, 0, part)) == 0 for part in range(n_sets))
            continue
        R.assert_same_rows(got[nm], R.translate(small.option_rows("patterns", slo, shi, 1), P), "patterns %s [%d, %d)" % (nm, blo, bhi))
        for part in range(n_sets):
            for min_valid in (0, 1):
                R.assert_same_rows(pu.bedmethyl(blo, bhi, min_valid, part), R.translate(small.option_rows("bedmethyl", slo, shi, min_valid, part), P),
                                   "bedMethyl %s [%d, %d), set %d, min_valid %d" % (nm, blo, bhi, part, min_valid))
    assert len(got["seq0"]) == 0 and len(got["all"]) > 1000 and len(got["below"]) >= 100 and len(got["above"]) >= 100
    R.assert_same_rows(np.concatenate([got["seq%d" % s] for s in range(len(pu.names))]), got["all"], "patterns per sequence")
    R.assert_same_rows(np.concatenate([got["below"], got["above"]]), got["all"], "patterns, the halves at B")
    if name == "cpg_at_B":                                     # a window begins on B, and one lies across it
        assert (got["all"]["start"] == B).sum() == 1 and ((got["all"]["start"] < B) & (B < got["all"]["end"])).any()
        assert (pu.bedmethyl(B, B + 1, 0)["gpos"] == B).all() and len(pu.bedmethyl(B, B + 1, 0)) == 1
    whole = pu.bedmethyl(0, total, 0)
    assert (whole["gpos"] < B).sum() >= 100 and (whole["gpos"] >= B).sum() >= 100
    R.assert_same_rows(pu.linkage(0), small.option_rows("linkage", 0), "linkage")     # distances, tables: nothing in these three moves
    R.assert_same_rows(pu.readpos(0), small.option_rows("readpos", 0), "read position")
    assert (pu.readpos_histograms() == small.option_rows("readpos_histograms")).all()
    assert pu.patterns_bed(got["all"]) == small.pu.patterns_bed(small.option_rows("patterns", 0, small.n, 1))
    assert pu.bedmethyl_bed(whole) == small.pu.bedmethyl_bed(small.option_rows("bedmethyl", 0, small.n, 0, 0))


def run_case(B, name, small, host, upto="extras", options=None, plain=None):
    """one big job against the small one; `upto` ends it after that stage.  -> seconds per stage.  With `options` (those of
    `small`) the big engine gets them too, `plain` is the option-free small job, and the stages are records, count, options"""
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    genome, reads = R.small_job()
    want, _n = R.oracle_small()
    P, g = R.placement(name, B, genome, reads, want)
    R.check_preconditions(name, B, P, small.records["gpos"], small.loci["gpos"])
    total, planes = P + small.n, 7 if small.partitions else 3
    # reference, planes, labels, and a GB for everything batch-sized.  The extras stay inside that GB: the region index takes 96 B per
    # HM_REGION_BLOCK loci (101 MB at 2^32), the k-mer table 25 MB at flank 3, the domains 34 B per row of a context
    need = total * (1 + 4 * planes + 1) + (1 << 30)
    assert 96 * (total // R.region_block() + 1) + (25 << 20) + 34 * len(small.loci) < (1 << 29)
    if options:                                                # ... and so does what the options allocate: per reference CpG 8 + 64 B
        n_cpg = sum(s.count("CG") for _n, s in genome)         # for the patterns and 20 B per bedMethyl set (the pad has none), 6144 B
        n_sets = R.option_sets(small.partitions)[1]            # per linkage distance, 12.6 MB of read-position table
        need += (72 + 20 * n_sets) * n_cpg + (options["linkage"] + 1) * 6144 + 3 * (2 * options["profile"] + 1) * 2048
        assert need - total * (1 + 4 * planes + 1) < (1 << 30) + (1 << 25)
    free, _all = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip("the card has %.1f GB free, the case needs %.1f GB plus 8 GB" % (free / 1e9, need / 1e9))
    ref, labels = host.get(B).place(P, small.ref, small.lab)
    if upto == "extras" and not options:                       # the small side of the last stage, outside the big engine's clock
        for kind, _nm, _big, (slo, shi) in extras_plan(small, B, P, g):
            small_extra(small, kind, g, slo, shi)
    t = [time.perf_counter()]
    pu = MethylationPileup([("pad", P)] + [(n, len(s)) for n, s in genome], min_pi=R.MIN_PI, partitions=small.partitions, bases=ref,
                           **(options or {}))
    plain = plain or small
    try:
        assert pu.names == ["pad"] + [n for n, _ in genome] and pu.offsets.tolist() == [0] + (P + R.offsets_of(genome)).tolist()
        assert pu.n_loci == total > B
        # ---- the projection: reads the reference, writes records
        feed(pu, R.shifted_reads(reads))
        assert (pu.histograms() == plain.hist).all()             # the options change neither the histograms nor the records
        R.assert_same_rows(R.sorted_records(*pu.records()), R.translate(plain.records, P), "records")
        assert pu.resolve_thresholds(pu.histograms()) == plain.thr
        assert not options or pu.num_pattern_records() == small.n_pattern_records > 0
        t.append(time.perf_counter())
        assert (pu.label_histograms(labels) == small.label_hist).all()
        t.append(time.perf_counter())
        if upto == "records":
            return np.diff(t)
        # ---- counting: writes the planes
        pu.count(small.thr)
        assert pu.num_records() == 0
        loci = pu.loci()
        R.assert_same_rows(loci, R.translate(plain.loci, P), "loci")
        assert pu.bed(loci) == small.bed                       # the names follow the contigs, the pad has no row
        t.append(time.perf_counter())
        if options:
            run_options(pu, small, B, P, name)
            t.append(time.perf_counter())
            return np.diff(t)
        if upto == "count":
            return np.diff(t)
        # ---- the fetches: read the planes
        sites_tab, asm_tab = small.tables(P)
        rngs = R.ranges(B, P, small.n)
        for kind in kinds(small.partitions):
            got = {}
            for nm, (blo, bhi), (slo, shi) in rngs:
                got[nm] = fetch(pu, kind, blo, bhi, sites_tab, asm_tab)
                R.assert_same_rows(got[nm], R.translate(small.rows(kind, slo, shi), P), "%s %s [%d, %d)" % (kind, nm, blo, bhi))
            assert len(got["all"]) > 100 and len(got["below"]) and len(got["above"]) and len(got["near"]), kind
            if name != "contig_at_B" and kind in ("loci", "sites"):
                assert len(got["around"]) >= 1 and B in got["around"]["gpos"]
            per_seq = [fetch(pu, kind, int(pu.offsets[s]), int(pu.offsets[s + 1]), sites_tab, asm_tab) for s in range(len(pu.names))]
            assert len(per_seq[0]) == 0 and all(len(x) for x in per_seq[1:]), kind
            R.assert_same_rows(np.concatenate(per_seq), got["all"], kind + " per sequence")
        for nm, (blo, bhi), (slo, shi) in rngs:
            assert (pu.control_sums(blo, bhi) == small.pu.control_sums(slo, shi)).all(), nm
        assert small.pu.control_sums(0, small.n).min() > 0
        bins, big = pu.site_histogram()
        assert (bins == small.site_bins).all()
        R.assert_same_rows(big, R.translate(small.site_big, P), "site_histogram's big list")
        halves, _big = pu.site_histogram(0, B)
        pu.site_histogram(B, total, bins=halves)
        assert (halves == small.site_bins).all()
        assert pu.sites_bed(pu.sites(sites_tab)) == small.pu.sites_bed(small.rows("sites", 0, small.n))
        if small.partitions:
            bins, big = pu.asm_histogram(min_cov=MIN_COV)
            assert (bins == small.asm_bins).all()
            R.assert_same_rows(big, R.translate(small.asm_big, P), "asm_histogram's big list")
            bins[:] = 0
            pu.asm_histogram(0, B, MIN_COV, bins=bins)
            pu.asm_histogram(B, total, MIN_COV, bins=bins)
            assert (bins == small.asm_bins).all()
            R.assert_same_rows(pu.asm_bin_pvalues(bins), small.asm_tab, "asm_bin_pvalues")
            rq = pu.asm(min_cov=MIN_COV, table=asm_tab)
            assert not np.isnan(rq["qvalue"]).any() and (rq["gpos"] < B).any() and (rq["gpos"] >= B).any()
            assert pu.asm_bed(rq) == small.pu.asm_bed(small.rows("asmq", 0, small.n))
        t.append(time.perf_counter())
        if upto == "fetch":
            return np.diff(t)
        # ---- the newer outputs: read the planes (and, for the k-mer table, the reference)
        run_extras(pu, small, B, P, g)
        t.append(time.perf_counter())
        return np.diff(t)
    finally:
        pu.close()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def host():
    cache = HostCache()
    yield cache
    cache.held = None


@pytest.fixture(scope="module")
def smalls():
    made = {}

    def get(partitions, with_options):
        if (partitions, with_options) not in made:
            made[partitions, with_options] = Small(partitions, R.option_sets(partitions)[0] if with_options else None)
        return made[partitions, with_options]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("B,name", R.CASES, ids=R.CASE_IDS)
def test_big_reference_equals_translated_small_job(B, name, smalls, host):
    secs = run_case(B, name, smalls(B == R.B31, False), host)
    print("bigref %s %s: engine + projection %.2f s, labels %.2f s, count + loci %.2f s, fetches %.2f s, extras %.2f s" % (
        R.CASE_IDS[R.CASES.index((B, name))], "partitions" if B == R.B31 else "plain", *secs))


@pytest.mark.parametrize("B,name", R.OPTION_CASES, ids=R.OPTION_CASE_IDS)
def test_big_reference_with_engine_options(B, name, smalls, host):
    """patterns (k = 4 plain, k = 2 with partitions), bedMethyl (one set plain, three with partitions), linkage up to 2000 and the
    read-position table at 1024 on engines of their own: profile instantiates another projection kernel, so the six cases above
    go on testing the one they tested.  No trimming run: it acts on read offsets only."""
    part = B == R.B31
    secs = run_case(B, name, smalls(part, True), host, options=R.option_sets(part)[0], plain=smalls(part, False))
    print("bigref %s %s: engine + projection %.2f s, labels %.2f s, count + loci %.2f s, options %.2f s" % (
        R.OPTION_CASE_IDS[R.OPTION_CASES.index((B, name))], "partitions" if part else "plain", *secs))
