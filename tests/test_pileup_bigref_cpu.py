"""Host-side arithmetic of pileup on references beyond 2^31 and 2^32 bases (no GPU): the rank ranges, the two host solvers with
big lists whose loci straddle 2^32, the locus -> (sequence, position) mapping behind the BED writers, and the expected side of
test_gpu_pileup_bigref.py -- its placements, its preconditions and the proof that a 32-bit locus cannot pass its comparison."""
import numpy as np
import pytest

import bigref as R
from asm_q_ref import cases

B32 = 1 << 32


# ---- locus_ranges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("n", [2 ** 31 + 1, 2 ** 32 + 5, 3_100_000_000])
def test_locus_ranges_cover_a_big_reference(n, world):
    from hifimeth_amd.pileup import locus_ranges
    r = locus_ranges(n, world)
    assert len(r) == world and r[0][0] == 0 and r[-1][1] == n
    for (a, b), (c, _d) in zip(r, r[1:] + [(n, n)]):
        assert type(a) is int and type(b) is int               # Python ints: no fixed-width wrap anywhere
        assert a < b and b == c                                # none empty; contiguous, hence disjoint and covering
    chunk = -(-n // world)
    assert all(b - a == chunk for a, b in r[:-1]) and r[-1][1] - r[-1][0] <= chunk


# ---- hm_sites_table / hm_asm_qvalues with big lists across 2^32 -----------------------------------------------------------------------
def _straddle(k):
    """k ascending loci, half of them below 2^32, one exactly on it"""
    return B32 - 3 * (k // 2) + 3 * np.arange(k, dtype=np.int64)


def test_sites_table_with_big_loci_across_2_32():
    from hifimeth_amd.pileup import LOCUS_DTYPE, sites_table
    rng = np.random.default_rng(5)
    bins = np.zeros((3, 256, 256), np.uint64)
    n = rng.integers(1, 256, 4000)
    k = (rng.random(4000) * (n + 1)).astype(np.int64)
    np.add.at(bins, (rng.integers(0, 3, 4000), n, k), 1)
    big = np.zeros(64, LOCUS_DTYPE)
    big["gpos"] = _straddle(64)
    tot = rng.choice([256, 257, 1000, 4096], 64)
    big["pcov"] = (rng.random(64) * (tot + 1)).astype(np.int64)
    big["ncov"] = tot - big["pcov"]
    big["motif"] = rng.integers(0, 3, 64)
    big[[10, 11]] = big[[10, 10]]                              # the same counts on neighbours (the value is reused), ...
    big["gpos"] = _straddle(64)                                # ... the loci still ascending
    assert (big["gpos"] < B32).sum() == 32 and (big["gpos"] == B32).sum() == 1 and (np.diff(big["gpos"]) > 0).all()
    low = big.copy()
    low["gpos"] = big["gpos"] - B32 + 1000
    assert (low["gpos"] >= 0).all() and low["gpos"].max() < 2 ** 31
    a, b = sites_table(R.RATES, bins, big), sites_table(R.RATES, bins, low)
    for f in ("ptab", "qtab", "big_p", "big_q", "m"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert not np.isnan(a.big_p).any() and not np.isnan(a.big_q).any() and (a.big["gpos"] == big["gpos"]).all()


def test_asm_qvalues_with_big_loci_across_2_32():
    from hifimeth_amd.caller import HifimethError
    from hifimeth_amd.pileup import asm_qvalues
    tab, big = cases()["random"]
    big = big.copy()
    big["gpos"] = _straddle(len(big))
    assert len(big) >= 100 and (big["gpos"] < B32).any() and (big["gpos"] >= B32).sum() > 10
    low = big.copy()
    low["gpos"] = big["gpos"] - B32 + 1000
    a, b = asm_qvalues(tab, big), asm_qvalues(tab, low)
    assert a.tab.tobytes() == b.tab.tobytes() and a.big_q.tobytes() == b.big_q.tobytes() and a.m.tobytes() == b.m.tobytes()
    assert not np.isnan(a.big_q).any() and (a.big["gpos"] == big["gpos"]).all()
    swapped = tab.copy()                                       # a table that is not ascending is refused, whatever the loci are
    swapped[[2, 3]] = swapped[[3, 2]]
    with pytest.raises(HifimethError):
        asm_qvalues(swapped, big)


# ---- locus -> (sequence, position): what the BED writers print ------------------------------------------------------------------------
def _mirror_without_engine(names, lengths):
    """a MethylationPileup that holds names and offsets only: the text writers read nothing else"""
    from hifimeth_amd.pileup import MethylationPileup
    pu = object.__new__(MethylationPileup)
    pu._h = None
    pu.names = list(names)
    pu.lengths = np.array(lengths, np.int64)
    pu.offsets = np.concatenate([[0], np.cumsum(pu.lengths)])
    return pu


@pytest.mark.parametrize("P", [0, B32 - 12000, B32 - 17, 2 ** 31 - 5, B32 + 123456789])
def test_locate_and_bed_text_behind_a_pad(P):
    from hifimeth_amd.pileup import ASMQ_DTYPE, LOCUS_DTYPE, SITE_DTYPE, locate
    names, lengths = ["chr1", "chr2", "chr3"], [12000, 15600, 19200]
    small = _mirror_without_engine(names, lengths)
    big = _mirror_without_engine(["pad"] + names, [P] + lengths) if P else small
    at = np.array([0, 1, 11999, 12000, 12001, 27599, 27600, 46799], np.int64)       # both sides of every sequence start
    sid, soff = locate(small.offsets, at)
    assert sid.tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and soff.tolist() == [0, 1, 11999, 0, 1, 15599, 0, 19199]
    bsid, bsoff = locate(big.offsets, at + P)
    assert bsid.dtype == np.int64 and bsoff.dtype == np.int64
    assert (bsid == sid + (1 if P else 0)).all() and (bsoff == soff).all()
    if P:
        psid, psoff = locate(big.offsets, [0, P - 1])           # the pad's own loci
        assert psid.tolist() == [0, 0] and psoff.tolist() == [0, P - 1]
        assert (at + P).max() > 2 ** 31
    loci = np.zeros(len(at), LOCUS_DTYPE)
    loci["gpos"], loci["pcov"], loci["ncov"], loci["motif"] = at, 1 + np.arange(len(at)), 3, np.arange(len(at)) % 3
    sites = np.zeros(len(at), SITE_DTYPE)
    for f in ("gpos", "pcov", "ncov", "motif"):
        sites[f] = loci[f]
    sites["pvalue"], sites["qvalue"] = 0.25, 0.5
    asm = np.zeros(len(at), ASMQ_DTYPE)
    asm["gpos"], asm["pcov1"], asm["ncov1"], asm["pcov2"], asm["ncov2"], asm["motif"] = at, 5, 1, 2, 4, loci["motif"]
    asm["diff"], asm["pvalue"], asm["qvalue"] = 50.0, 0.125, 0.25
    for rows, writer in ((loci, "bed"), (sites, "sites_bed"), (asm, "asm_bed")):
        want = getattr(small, writer)(rows)
        assert getattr(big, writer)(R.translate(rows, P)) == want
        assert sum(t.count("\n") for t in want.values()) == len(at) and "pad" not in "".join(want.values())
    assert small.bed(loci)["CpG"].startswith("chr1\t0\t1\t25\t1\t3\n")               # the text of a str genome, pinned
    assert small.bed(loci)["CpG"].endswith("chr3\t0\t1\t70\t7\t3\n")


# ---- the expected side of the big-reference GPU test ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    genome, reads = R.small_job()
    want, n_unfiltered = R.oracle_small()
    return genome, reads, want, n_unfiltered


def test_small_job_holds_what_the_placements_need(small):
    genome, reads, want, n_unfiltered = small
    assert [len(s) for _, s in genome] == [12000, 15600, 19200]
    assert 0 < len(want["records"]) < n_unfiltered              # the identity filter drops some reads, not all
    assert {r.hp for r in reads} == {None, 1, 2, 3} and any(r.flag & 16 for r in reads) and any(r.flag & 0x900 for r in reads)
    shifted = R.shifted_reads(reads)
    assert all(s.tid == r.tid + 1 for s, r in zip(shifted, reads) if not r.flag & 4)
    assert all(dict(R.as_dict(s), tid=0) == dict(R.as_dict(r), tid=0) for s, r in zip(shifted, reads))


@pytest.mark.parametrize("B,name", R.CASES, ids=R.CASE_IDS)
def test_expected_side_sees_a_32_bit_locus(small, B, name):
    """the placement's preconditions hold, the translation puts the oracle's loci where the big job must have them, and the
    comparison the GPU test uses fails for expectations whose locus went through 32 bits, unsigned or signed"""
    genome, reads, want, _n = small
    off = R.offsets_of(genome)
    P, g = R.placement(name, B, genome, reads, want)
    assert P + int(off[-1]) <= R.HOST_LEN[B] and 0 < g < off[-1]
    rec, loc = R.record_gpos(want, off), R.loci_gpos(want, off)
    R.check_preconditions(name, B, P, rec, loc)
    rows = R.oracle_locus_rows(want, off)
    big = R.translate(rows, P)
    assert (big["gpos"] - P == rows["gpos"]).all() and (np.diff(big["gpos"]) > 0).all()
    assert R.same_rows(big, big.copy())
    casts = (True,) if B < B32 else (True, False)               # an int32 wraps from 2^31 on, a uint32 from 2^32 on
    for signed in casts:
        bad = R.truncate32(big, signed)
        assert not R.same_rows(bad, big)
        with pytest.raises(AssertionError):
            R.assert_same_rows(bad, big, "loci")
    recs = R.sorted_records(rec + P, *(np.array(x) for x in zip(*[(p, m, 0) for _s, _o, p, m in want["records"]])))
    for signed in casts:
        bad = R.truncate32(recs, signed)
        assert not R.same_rows(np.sort(bad, order=["gpos", "prob", "motif", "order"]), recs)
    for _nm, (blo, bhi), (slo, shi) in R.ranges(B, P, int(off[-1])):
        assert bhi - P == shi and (blo - P == slo if blo else slo == 0)      # a range from 0 on takes the pad with it: no rows there
    if name == "rev_chh_at_B":                                  # the record sits on the G, the deciding column two below
        assert genome[1][1][g - int(off[1])] == "G" and any(o + off[s] == g and m == 2 for s, o, _p, m in want["records"])
    if name == "contig_at_B":
        assert g == off[1]


# ---- the newer outputs (-G, -D, -E, -M, -L, -P, -R / -J, -S): what makes their big cases worth the memory -------------------------------
COORD_OUTPUTS = ("patterns2", "patterns4", "bedmethyl", "domains0", "domains1", "domains2", "asm_regions0", "asm_regions1", "asm_regions2")


def _expected_rows(what):
    """the small job's expected rows of one coordinate-carrying output, from its CPU restatement"""
    n = int(R.offsets_of(R.small_job()[0])[-1])
    if what.startswith("patterns"):
        return R.expected_patterns(int(what[-1]))
    if what == "bedmethyl":
        return R.expected_bedmethyl(0)
    if what.startswith("domains"):
        return R.expected_domains(R.oracle_loci(), int(what[-1]), 0, n)[0]
    return R.expected_asm_regions(R.expected_asm_rows(), int(what[-1]), 0, n)[0]


def test_small_job_fills_the_newer_outputs(small):
    genome, _reads, want, _n = small
    assert R.expected_thresholds() == want["thresholds"] == [128, 128, 128]
    assert len(R.expected_patterns(2)) >= 1000 and len(R.expected_patterns(4)) >= 1000       # min_reads 1, span 150
    assert R.expected_patterns(2)["k"].tolist() == [2] * len(R.expected_patterns(2))
    assert len(R.expected_bedmethyl(0)) >= 1000 and len(R.expected_bedmethyl(0)) > len(R.expected_bedmethyl(1)) > 0
    sets = R.expected_bedmethyl_counters()
    assert all(len(s) > 100 for s in sets) and set(sets[1]) <= set(sets[0]) and set(sets[2]) <= set(sets[0])
    assert len(R.expected_bedmethyl(0, 1)) > 100 and len(R.expected_bedmethyl(0, 2)) > 100
    pairs = R.expected_linkage_pairs()
    assert len(pairs) >= 1000 and max(pairs) == R.LINKAGE_DIST and len(R.expected_linkage(0)) == R.LINKAGE_DIST - 1
    hist = R.expected_readpos_histograms()
    assert (hist.sum(axis=(1, 2)) > 1000).all() and hist[:, :R.PROFILE_D].any() and hist[:, R.PROFILE_D:-1].any() and hist[:, -1].any()
    assert len(R.expected_readpos(0)) == 3 * (2 * R.PROFILE_D + 1) > len(R.expected_readpos(1)) > 1000
    for flank in R.CONTEXT_FLANKS:
        tab = R.expected_context(flank)
        assert (tab[:, :, 0].sum(axis=1) == [(R.oracle_loci()["motif"] == c).sum() for c in range(3)]).all()
    assert R.expected_context(3)[:, -1, 0].sum() > 0            # a covered cytosine within 5 bases of a sequence end: row `other`
    chains = np.concatenate([_expected_rows("asm_regions%d" % c) for c in range(3)])
    assert (chains["n_loci"] >= 2).sum() >= 3 and (chains["sign"] > 0).any() and (chains["sign"] < 0).any()
    pv = R.expected_asm_rows()["pvalue"]
    assert (pv <= R.ASM_MAX_P).any() and (pv > R.ASM_MAX_P).any() and not (np.abs(pv / R.ASM_MAX_P - 1) < 1e-6).any()   # the p filter decides, far from ties
    assert all(len(_expected_rows("domains%d" % c)) >= 5 for c in range(3))
    start, end, s0, s1, strand = R.meta_intervals()
    tab, used = R.expected_metaplot(start, end, s0, s1, strand)
    nb, fb = tab.shape[1], R.META["flank_bins"]
    assert used == len(start) == 6 and set(strand) == set(b"+-.")
    assert (tab[:, :fb - 1, 0] < used).all() and (tab[:, nb - fb + 1:, 0] < used).all()       # both flanks hit the sequence clamp ...
    assert (tab[:, fb:nb - fb, 0] == used).all() and tab[:, :, 1].sum(axis=0).all()            # ... the bodies never, and no bin is empty


@pytest.mark.parametrize("name", R.PLACEMENTS)
def test_newer_outputs_have_rows_on_both_sides_of_the_placed_locus(small, name):
    genome, reads, want, _n = small
    P, g = R.placement(name, B32, genome, reads, want)
    assert R.placement(name, R.B31, genome, reads, want)[1] == g                            # the locus is the same at either boundary
    n = int(R.offsets_of(genome)[-1])
    for k in (2, 4):
        p = R.expected_patterns(k)
        assert (p["start"] < g).sum() >= 100 and (p["start"] >= g).sum() >= 100
        if name == "cpg_at_B":
            assert ((p["start"] < g) & (g < p["end"])).sum() >= 1 and (p["start"] == g).sum() >= 1
    b = R.expected_bedmethyl(0)
    assert (b["gpos"] < g).sum() >= 100 and (b["gpos"] >= g).sum() >= 100
    if name == "cpg_at_B":
        assert (b["gpos"] == g).sum() == 1
        assert R.linkage_straddlers(g) >= 1                     # pairs of one record with members on both sides of B
    start, end = R.intervals(g)
    for min_cov in R.REGION_MIN_COVS:
        filled = R.expected_regions(start, end, min_cov)[:, :, 0].sum(axis=1) > 0
        assert ((start < g) & (g < end) & filled).any() and ((start == g) & filled).any() and ((end == g) & filled).any()
    assert ((end - start) == n).any() and len(start) == 21 + 3 + 1
    blk = R.region_block()
    assert {g - 1, g, g + 1, g - blk, g + blk, g - blk - 1, g + blk + 1} <= set(start.tolist()) | set(end.tolist())
    for what in COORD_OUTPUTS[3:]:                              # a segment and a chain of every context contain the placed locus
        rows = _expected_rows(what)
        assert ((rows["start"] <= g) & (g < rows["end"])).sum() == 1, what
    for c in range(3):                                          # ... and either side of it has loci that are counted
        loci = R.oracle_loci()
        assert ((loci["gpos"] < g) & (loci["motif"] == c)).sum() >= 100 and ((loci["gpos"] >= g) & (loci["motif"] == c)).sum() >= 100


@pytest.mark.parametrize("B,name", R.CASES, ids=R.CASE_IDS)
def test_expected_side_of_the_newer_outputs_sees_a_32_bit_locus(small, B, name):
    """for every output that carries coordinates, the expectation whose coordinates went through 32 bits is another one: rows by
    their own fields, the sums of -R / -J by the intervals they are asked for"""
    genome, reads, want, _n = small
    P, g = R.placement(name, B, genome, reads, want)
    n = int(R.offsets_of(genome)[-1])
    casts = (True,) if B < B32 else (True, False)
    for what in COORD_OUTPUTS:
        rows = _expected_rows(what)
        big = R.translate(rows, P)
        fields = [f for f in R.COORDS if f in rows.dtype.names]
        assert all((big[f] - P == rows[f]).all() for f in fields) and R.same_rows(big, big.copy()), what
        others = [f for f in rows.dtype.names if f not in fields]
        assert all(big[f].tobytes() == rows[f].tobytes() for f in others), what
        for signed in casts:
            bad = R.truncate32(big, signed)
            assert not R.same_rows(bad, big), what
            with pytest.raises(AssertionError):
                R.assert_same_rows(bad, big, what)
    start, end = R.intervals(g)
    m = R.meta_intervals()
    want_sums = R.expected_regions(start + P, end + P, base=P)
    assert (want_sums == R.expected_regions(start, end)).all()  # untranslated: the sums do not know where the planes lie
    want_meta, used = R.expected_metaplot(*(x + P for x in m[:4]), m[4], base=P)
    assert used == 6 and (want_meta == R.expected_metaplot(*m)[0]).all()
    for signed in casts:
        assert (R.expected_regions(R.wrap32(start + P, signed), R.wrap32(end + P, signed), base=P) != want_sums).any()
        a, b, s0, s1 = (R.wrap32(x + P, signed) for x in m[:4])
        assert (R.expected_metaplot(a, b, s0, s1, m[4], base=P)[0] != want_meta).any()
