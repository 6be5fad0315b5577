"""Pileup on a real reference of more than 2^31 and more than 2^32 bases: a small job, then the same job behind a pad of 'N' that
puts a boundary B on a chosen locus (tests/bigref.py), and every result of the big job must equal the small job's with the loci
translated -- exactly, floats as bits.  The engine's results may not depend on where in the concatenated reference a contig lies.

Six cases: B = 2^31 with haplotype partitions (7 planes, about 65 GB on the card), B = 2^32 without (3 planes, about 61 GB), each
with the boundary on a covered CpG, on a reverse-strand CHH record (decided two columns below B) and on a contig start.  One
big engine is alive at a time; the 4 GB host buffers are built once per boundary.  A case skips, naming both numbers, when the
card has less free memory than it needs plus 8 GB.  The small job is itself checked against oracle/pileup_oracle.py.

A stage argument orders the work from safe to less safe: the projection only reads the reference (stage "records"), counting
writes the planes ("count"), the fetches read them ("fetch")."""
import time

import numpy as np
import pytest

import bigref as R

pytestmark = pytest.mark.gpu
MIN_COV = 1                                                    # of the haplotype test: at 3x coverage the rows must not run out
STAGES = ("records", "count", "fetch")


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
    def __init__(self, partitions):
        from hifimeth_amd.pileup import AsmTable, MethylationPileup, asm_qvalues, sites_table
        genome, reads = R.small_job()
        want, _n = R.oracle_small()
        self.partitions, self.n = partitions, sum(len(s) for _, s in genome)
        self.ref = np.frombuffer("".join(s for _, s in genome).encode(), np.uint8)
        self.lab = R.small_labels(self.n)
        pu = self.pu = MethylationPileup(genome, min_pi=R.MIN_PI, partitions=partitions)
        off = pu.offsets
        feed(pu, reads)
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


def run_case(B, name, small, host, upto="fetch"):
    """one big job against the small one; `upto` ends it after that stage.  -> seconds per stage"""
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    genome, reads = R.small_job()
    want, _n = R.oracle_small()
    P, g = R.placement(name, B, genome, reads, want)
    R.check_preconditions(name, B, P, small.records["gpos"], small.loci["gpos"])
    total, planes = P + small.n, 7 if small.partitions else 3
    need = total * (1 + 4 * planes + 1) + (1 << 30)            # reference, planes, labels, and a GB for everything batch-sized
    free, _all = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip("the card has %.1f GB free, the case needs %.1f GB plus 8 GB" % (free / 1e9, need / 1e9))
    ref, labels = host.get(B).place(P, small.ref, small.lab)
    t = [time.perf_counter()]
    pu = MethylationPileup([("pad", P)] + [(n, len(s)) for n, s in genome], min_pi=R.MIN_PI, partitions=small.partitions, bases=ref)
    try:
        assert pu.names == ["pad"] + [n for n, _ in genome] and pu.offsets.tolist() == [0] + (P + R.offsets_of(genome)).tolist()
        assert pu.n_loci == total > B
        # ---- the projection: reads the reference, writes records
        feed(pu, R.shifted_reads(reads))
        assert (pu.histograms() == small.hist).all()
        R.assert_same_rows(R.sorted_records(*pu.records()), R.translate(small.records, P), "records")
        assert pu.resolve_thresholds(pu.histograms()) == small.thr
        t.append(time.perf_counter())
        assert (pu.label_histograms(labels) == small.label_hist).all()
        t.append(time.perf_counter())
        if upto == "records":
            return np.diff(t)
        # ---- counting: writes the planes
        pu.count(small.thr)
        assert pu.num_records() == 0
        loci = pu.loci()
        R.assert_same_rows(loci, R.translate(small.loci, P), "loci")
        assert pu.bed(loci) == small.bed                       # the names follow the contigs, the pad has no row
        t.append(time.perf_counter())
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

    def get(partitions):
        if partitions not in made:
            made[partitions] = Small(partitions)
        return made[partitions]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("B,name", R.CASES, ids=R.CASE_IDS)
def test_big_reference_equals_translated_small_job(B, name, smalls, host):
    secs = run_case(B, name, smalls(B == R.B31), host)
    print("bigref %s %s: engine + projection %.2f s, labels %.2f s, count + loci %.2f s, fetches %.2f s" % (
        R.CASE_IDS[R.CASES.index((B, name))], "partitions" if B == R.B31 else "plain", *secs))
