"""Inputs and the catalogue of readers for the call-sequence tests of the pileup engine (plain module, imported by
test_sequence_cases_cpu.py and test_gpu_pileup_sequences.py; it imports without a GPU).

The engine's outputs share mutable device state (struct hm_pileup: the staging of every row fetch in d_rows / d_blk / d_offs, the
tables "in hand" of the context and the interval fetches, scratch filled by whichever call comes first).  The other test files ask
an engine for one family of outputs; here every read-only entry point is an entry of one CATALOGUE, so that a test can call them in
any order on one engine and hold every answer to the one a fresh engine gives.

    record_input(which)      a genome of three contigs (about 6 kb), 60 alignments on both strands with an insertion, a deletion,
                             soft clips and HP 0 / 1 / 2, in three slabs; `which` 0 is the input of most tests, 1 a second, different one
    RECORD_OPTIONS           every option on: partitions, patterns, bedmethyl, linkage, profile and a -I trim
    feed_slab / feed         run + count per slab at the medians of the engine's histograms
    load_genome / feed_load  the 3 + 3 samples of groups_ref.dataset() through begin_sample / load_sample_loci
    ladder_planes / LADDER   crafted caller planes and nested ranges whose row counts at least triple per step
    CATALOGUE, LOAD_CATALOGUE  [(name, fn(engine) -> tuple of numpy arrays / ints)], CALLS name -> the exports the entry calls
    EXPORTS                  every hm_pileup_* / hm_group_* / hm_asm_* / hm_sites_* / hm_domain_* function of the header by class

An engine that uses caller planes finds them in its attribute `crafted` (seven torch tensors, set by the GPU test).
"""
import ctypes
import dataclasses
import functools

import numpy as np

import groups_ref as G
import pileup_cases as C
from hifimeth_amd import pileup as M
from hifimeth_amd.synth import revcomp, synth_genome

HM_EINVAL, HM_EDATA, HM_ESTATE = -1, -4, -5
TRIM = (5, 7)
RECORD_OPTIONS = dict(partitions=True, patterns=2, bedmethyl=True, linkage=64, profile=16, trim=TRIM)
N_SLABS = 3
ASM_MIN_COV = 2


# ---- the record input ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def record_input(which=0):
    """-> (genome, reads): three contigs of 1500 / 1950 / 2400 bases (1300 / 1690 / 2080 for the second input) and 60 alignments of
    500 .. 900 columns, each M I M D M with soft clips on some, every C and G of the read called (pileup_cases.make_read), HP by turns"""
    g = synth_genome(n_chr=3, length=(1500, 1300)[which], gc=0.5, seed=(301, 401)[which], n_frac=0.0)
    rng = np.random.default_rng((302, 402)[which])
    reads = []
    for i in range(60):
        tid = i % 3
        a, b, c = (int(x) for x in rng.integers(150, 300, 3))
        ni, nd = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        spec = ([("S", int(rng.integers(1, 20)))] if i % 4 == 0 else []) + [("M", a), ("I", ni), ("M", b), ("D", nd), ("M", c)] \
            + ([("S", int(rng.integers(1, 20)))] if i % 5 == 0 else [])
        pos = int(rng.integers(0, len(g[tid][1]) - (a + b + c + nd) + 1))
        r = C.make_read("seq%d_%d" % (which, i), 16 if (i // 3) % 2 else 0, tid, pos, spec, g, rng, mapq=int(rng.integers(20, 61)))
        reads.append(dataclasses.replace(r, hp=(i // 6) % 3))
    reads.sort(key=lambda r: (r.tid, r.pos))
    return g, reads


def slabs(reads):
    n = (len(reads) + N_SLABS - 1) // N_SLABS
    return [reads[k * n:(k + 1) * n] for k in range(N_SLABS)]


def trimmed(read, trim=TRIM):
    """the read with the MM / ML entries `-I n5:n3` drops deleted from its tags: what the restatements without a trim argument take"""
    fwd = revcomp(read.seq) if read.flag & 16 else read.seq
    L = len(fwd)
    keep = lambda _k, q: trim[0] <= q <= L - 1 - trim[1]  # noqa: E731
    mm, ml, at = "", [], 0
    for base, head in (("C", "C+m"), ("G", "G-m")):
        qs = [q for q, ch in enumerate(fwd) if ch == base]
        text, kept = C._positions_mm(fwd, base, head, keep)
        mm += text
        ml += [read.ml[at + k] for k, q in enumerate(qs) if keep(k, q)]
        assert kept == [q for k, q in enumerate(qs) if keep(k, q)]
        at += len(qs)
    assert at == len(read.ml)
    return dataclasses.replace(read, mm=mm, ml=np.array(ml, np.uint8))


def median_thresholds(bins):
    """per context the smallest ML byte at which the running count reaches half of the histogram's total (128 for an empty one),
    kept inside 1 .. 255"""
    out = []
    for c in range(3):
        h = np.asarray(bins[c], np.uint64).astype(np.int64)
        run, total = np.cumsum(h), int(h.sum())
        out.append(128 if not total else min(max(int(np.searchsorted(run, (total + 1) // 2)), 1), 255))
    return out


def feed_slab(pu, slab, stop=None):
    """run and count one slab at the medians of the histograms so far -> the thresholds; stop = "run": return before the count"""
    for r in slab:
        pu.add(r)
    pu.flush()
    thr = median_thresholds(pu.histograms())
    if stop != "run":
        pu.count(thr)
    return thr


def feed(pu, reads):
    return [feed_slab(pu, s) for s in slabs(reads)]


# ---- the load input ------------------------------------------------------------------------------------------------------------
LOAD_OPTIONS = dict(partitions=True, groups=True, group_min_cov=G.MIN_COV)


@functools.lru_cache(maxsize=None)
def load_genome():
    rng = np.random.default_rng(303)
    return [("ctg%d" % (s + 1), "".join(rng.choice(list("ACGT"), n))) for s, n in enumerate(G.LENGTHS)]


def feed_load(pu):
    for (g, s), rows in sorted(G.dataset().items()):
        assert pu.begin_sample(g) == s
        pu.load_sample_loci(*rows)


# ---- crafted caller planes and the ladder ---------------------------------------------------------------------------------------
LADDER_N = 3 ** 9 + 5
PLANE_BASE = 100000
LADDER_MIN_COV = 5


def ladder_planes():
    """-> (pcov, ncov, key, pcov1, ncov1, pcov2, ncov2) int32 numpy planes of LADDER_N loci, every locus covered and tested: the
    haplotypes lean 9 : 1 against 1 : 9, the direction turning every 40 loci (hits of both signs for the regions); unphased reads add
    8 methylated or 8 unmethylated calls by turns of 50 loci (high and low domains); every locus is a CpG, so that the rows of
    context 0 triple with the range as the loci do"""
    i = np.arange(LADDER_N)
    lean = (i // 40) % 2 == 0
    p1, n1 = np.where(lean, 9, 1), np.where(lean, 1, 9)
    p2, n2 = n1.copy(), p1.copy()
    up = (i // 50) % 2 == 0
    pc, nc = p1 + p2 + np.where(up, 8, 0), n1 + n2 + np.where(up, 0, 8)
    return tuple(np.ascontiguousarray(x, np.int32) for x in (pc, nc, 0 * i, p1, n1, p2, n2))


def _ladder():
    mid, out = LADDER_N // 2, []
    for k in range(9):
        h = (3 ** k - 1) // 2
        out.append((mid - h, mid + h + 1))
    return out + [(0, LADDER_N)]


LADDER = _ladder()                                   # 1, 3, 9, .. 6561 loci around the middle, then all 19 688


def ladder_rows(kind, lo, hi, planes=None):
    """the number of rows the device selects over [lo, hi) of the crafted planes: covered loci, tested loci, rows of context 0"""
    pc, nc, key, p1, n1, p2, n2 = (x[lo:hi].astype(np.int64) for x in (planes or ladder_planes()))
    if kind == "loci":
        return int((pc + nc > 0).sum())
    if kind == "asm":
        return int(((p1 + n1 >= LADDER_MIN_COV) & (p2 + n2 >= LADDER_MIN_COV)).sum())
    return int(((pc + nc > 0) & ((key & 3) == 0)).sum())


# ---- the catalogue -------------------------------------------------------------------------------------------------------------
CATALOGUE, LOAD_CATALOGUE, CALLS = [], [], {}
_vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def reader(name, *exports, load=False, record=True):
    def wrap(fn):
        CALLS[name] = exports
        if record:
            CATALOGUE.append((name, fn))
        if load:
            LOAD_CATALOGUE.append((name, fn))
        return fn
    return wrap


def _ptrs(pu, names):
    """the caller planes of the engine: device pointers of its `crafted` tensors, by index"""
    return [ctypes.c_void_p(pu.crafted[k].data_ptr()) for k in names]


def _cut(pu):
    """a sub-range that crosses the joint of the first two sequences"""
    return int(pu.offsets[1]) - 200, int(pu.offsets[1]) + 300


def _intervals(pu):
    """tiles of 250 loci over every sequence, then one interval per sequence that holds all of it but 10 bases at either end"""
    sid, a, b = [], [], []
    for s, n in enumerate(pu.lengths.tolist()):
        for x in range(0, n, 250):
            sid.append(s), a.append(x), b.append(min(x + 250, n))
        sid.append(s), a.append(10), b.append(n - 10)
    strand = ["+-."[k % 3] for k in range(len(sid))]
    return M.Regions(sid, a, b, ["iv%d" % k for k in range(len(sid))], strand).coords(pu.offsets)


def _labels(pu):
    return np.random.default_rng(304).integers(-1, 2, pu.n_loci).astype(np.int8)


reader("loci", "hm_pileup_fetch_loci", load=True)(lambda pu: (pu.loci(),))
reader("loci_sub", "hm_pileup_fetch_loci")(lambda pu: (pu.loci(*_cut(pu)),))
reader("loci_part1", "hm_pileup_fetch_loci", "hm_pileup_partition_planes", load=True)(lambda pu: (pu.loci(partition=1),))
reader("loci_part2", "hm_pileup_fetch_loci", "hm_pileup_partition_planes")(lambda pu: (pu.loci(partition=2),))
reader("loci_caller", "hm_pileup_fetch_loci")(lambda pu: (pu.loci(100, 5000, planes=pu.crafted[:3], plane_base=PLANE_BASE),))
reader("asm", "hm_pileup_fetch_asm", load=True)(lambda pu: (pu.asm(min_cov=ASM_MIN_COV),))
reader("asm_caller", "hm_pileup_fetch_asm")(
    lambda pu: (pu.asm(50, 3000, min_cov=LADDER_MIN_COV, planes=[pu.crafted[k] for k in (3, 4, 5, 6, 2)], plane_base=PLANE_BASE),))


def _asm_table(pu, **kw):
    bins, big = pu.asm_histogram(min_cov=ASM_MIN_COV, **kw)
    tab = pu.asm_bin_pvalues(bins)
    return bins, big, M.asm_qvalues(tab, big)


@reader("asm_q_chain", "hm_pileup_asm_histogram", "hm_pileup_asm_bin_pvalues", "hm_pileup_fetch_asm_q")
def _asm_q_chain(pu):
    bins, big, t = _asm_table(pu)
    nz = np.flatnonzero(bins)
    return nz, bins[nz], big, t.tab, t.big_q, t.m, pu.asm(min_cov=ASM_MIN_COV, table=t)


for _c in range(3):
    reader("asm_regions_%d" % _c, "hm_pileup_fetch_asm_regions")(
        lambda pu, c=_c: pu.asm_regions(c, min_cov=ASM_MIN_COV, max_p=0.5, max_gap=200, min_loci=1))
reader("control_sums", "hm_pileup_control_sums")(lambda pu: (pu.control_sums(int(pu.offsets[1]), int(pu.offsets[2])),))


def _site_table(pu):
    sums = pu.control_sums(int(pu.offsets[2]), int(pu.offsets[3]))
    bins, big = pu.site_histogram()
    return sums, bins, big, M.sites_table(M.rates_from_sums(sums), bins, big)


@reader("sites_chain", "hm_pileup_control_sums", "hm_pileup_site_histogram", "hm_pileup_fetch_sites")
def _sites_chain(pu):
    sums, bins, big, t = _site_table(pu)
    return sums, bins, big, t.m, pu.sites(t)


for _c in range(3):
    reader("domains_%d" % _c, "hm_pileup_fetch_domains", load=_c == 0)(lambda pu, c=_c: pu.domains(c))
    reader("domain_sums_%d" % _c, "hm_pileup_domain_sums")(lambda pu, c=_c: (np.array(pu.domain_sums(c), np.int64),))


@reader("domains_parts", "hm_pileup_fetch_domains_part", "hm_pileup_domain_sums_part")
def _domains_parts(pu):
    """context 0 of the whole reference from three pieces: the summaries, the carries forward, the codes, the carries backward, the
    segments; then the state sums of every piece under the same carries"""
    rule = (*M.domain_scores(*M.DOMAIN_LEVELS[0]), M.DOMAIN_MAX_GAP)
    cuts = [0, int(pu.offsets[1]) - 137, int(pu.offsets[2]) + 61, pu.n_loci]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    part = lambda lo, hi, pass_, carry: pu.domains_part(0, lo, hi, pass_, carry, *rule)  # noqa: E731
    summaries = [part(lo, hi, M.DOMAIN_PASS_SUMMARY, {}) for lo, hi in pieces]
    fwd = M.domain_forward_carries(summaries, rule[2], rule[3])
    codes = [part(lo, hi, M.DOMAIN_PASS_CODES, f) if s["n_rows"] else {} for (lo, hi), s, f in zip(pieces, summaries, fwd)]
    bwd = M.domain_backward_carries(summaries, codes, rule[2], rule[3])
    out = []
    for (lo, hi), s, f, b in zip(pieces, summaries, fwd, bwd):
        seg = part(lo, hi, M.DOMAIN_PASS_SEGMENTS, {**f, **b})["segments"] if s["n_rows"] else np.zeros(0, M.DOMAIN_DTYPE)
        sums = pu.domain_sums(0, lo, hi, *rule, carry={**f, **b}) if s["n_rows"] else (0,) * 6
        out += [seg, np.array(sums, np.int64), np.array([s.get(k, 0) for k in ("n_rows", "first_gpos", "last_gpos", "e_first", "c")], np.int64)]
    return tuple(out)


reader("patterns", "hm_pileup_fetch_patterns")(lambda pu: (pu.patterns(min_reads=1),))
reader("patterns_sub", "hm_pileup_fetch_patterns")(lambda pu: (pu.patterns(*_cut(pu), min_reads=2),))
reader("bedmethyl_0", "hm_pileup_fetch_bedmethyl")(lambda pu: (pu.bedmethyl(min_valid=0),))
reader("bedmethyl_1", "hm_pileup_fetch_bedmethyl")(lambda pu: (pu.bedmethyl(partition=1),))
reader("bedmethyl_2", "hm_pileup_fetch_bedmethyl")(lambda pu: (pu.bedmethyl(*_cut(pu), partition=2),))
reader("linkage", "hm_pileup_fetch_linkage")(lambda pu: (pu.linkage(),))
reader("linkage_all", "hm_pileup_fetch_linkage")(lambda pu: (pu.linkage(min_pairs=0),))
reader("readpos", "hm_pileup_fetch_readpos")(lambda pu: (pu.readpos(),))
reader("readpos_histograms", "hm_pileup_readpos_histograms")(lambda pu: (pu.readpos_histograms(),))
reader("regions", "hm_pileup_fetch_regions", load=True)(lambda pu: (pu.regions(_intervals(pu)["start"], _intervals(pu)["end"]),))
reader("regions_sub_part2", "hm_pileup_fetch_regions", "hm_pileup_partition_planes")(
    lambda pu: (pu.regions(_intervals(pu)["start"], _intervals(pu)["end"], 2, *_cut(pu), partition=2),))
reader("metaplot", "hm_pileup_fetch_metaplot")(lambda pu: pu.metaplot(**_intervals(pu), bins=5, flank=40, flank_bins=2))
reader("context_0", "hm_pileup_fetch_context", load=True)(lambda pu: (pu.context(0),))
reader("context_2", "hm_pileup_fetch_context")(lambda pu: (pu.context(2),))
reader("context_1_part1", "hm_pileup_fetch_context", "hm_pileup_partition_planes", "hm_pileup_planes")(lambda pu: (pu.context(1, partition=1),))
reader("context_0_global", "hm_pileup_fetch_context_path")(lambda pu: (pu.context(0, path=M.CONTEXT_PATH_GLOBAL),))
reader("histograms", "hm_pileup_histograms")(lambda pu: (pu.histograms(),))


@reader("records", "hm_pileup_fetch_records", "hm_pileup_num_records", "hm_pileup_num_pattern_records")
def _records(pu):
    g, p, m, o = pu.records()
    order = np.lexsort((m, p, o, g))                 # the list is unordered
    return g[order], p[order], m[order], o[order], pu.num_records(), pu.num_pattern_records()


reader("label_histograms", "hm_pileup_label_histograms")(lambda pu: (pu.label_histograms(_labels(pu)),))
reader("group_tests_1", "hm_pileup_fetch_groups", load=True, record=False)(lambda pu: (pu.group_tests(min_reps=1),))
reader("group_tests_2", "hm_pileup_fetch_groups", load=True, record=False)(lambda pu: (pu.group_tests(min_reps=2),))
reader("group_tests_sub", "hm_pileup_fetch_groups", load=True, record=False)(lambda pu: (pu.group_tests(*_cut(pu), min_reps=3),))
reader("group_planes", "hm_pileup_group_planes", load=True, record=False)(lambda pu: pu.group_planes(1) + pu.group_planes(2, *_cut(pu)))


# ---- every row fetch once more: only counted, and with a cap one too small -----------------------------------------------------
def _row_calls(pu):
    """name -> (function, row dtype, its arguments between the handle and out, cap) of every fetch with the out / cap rule, over
    the engine's own planes"""
    L, none3, none5 = pu._L, (None,) * 3, (None,) * 5
    N, n_ctx = pu.n_loci, ctypes.c_int64(0)
    rule = (*M.domain_scores(*M.DOMAIN_LEVELS[0]), M.DOMAIN_MAX_GAP)
    flat = np.full(M.SITE_BINS, 0.5)
    calls = {
        "loci": (L.hm_pileup_fetch_loci, M.LOCUS_DTYPE, (*none3, 0, 0, N)),
        "asm": (L.hm_pileup_fetch_asm, M.ASM_DTYPE, (*none5, 0, 0, N, ASM_MIN_COV)),
        "asm_q": (L.hm_pileup_fetch_asm_q, M.ASMQ_DTYPE, (*none5, 0, 0, N, ASM_MIN_COV, None, 0, None, None, 0)),
        "asm_regions": (L.hm_pileup_fetch_asm_regions, M.ASM_REGION_DTYPE, (*none5, 0, 0, N, ASM_MIN_COV, 0, 0.5, 200, 1, 0, ctypes.byref(n_ctx))),
        "sites": (L.hm_pileup_fetch_sites, M.SITE_DTYPE, (*none3, 0, 0, N, 7, _vp(flat), _vp(flat), None, None, None, 0)),
        "domains": (L.hm_pileup_fetch_domains, M.DOMAIN_DTYPE, (*none3, 0, 0, N, 0, *rule, ctypes.byref(n_ctx))),
        "context": (L.hm_pileup_fetch_context, M.REGION_SUM_DTYPE, (*none3, 0, 0, N, 1, 0)),
    }
    if pu.pattern_k:
        calls["patterns"] = (L.hm_pileup_fetch_patterns, M.PATTERN_DTYPE, (0, N, 1))
        calls["bedmethyl"] = (L.hm_pileup_fetch_bedmethyl, M.BEDMETHYL_DTYPE, (0, 0, N, 0))
        calls["linkage"] = (L.hm_pileup_fetch_linkage, M.LINKAGE_DTYPE, (1,))
        calls["readpos"] = (L.hm_pileup_fetch_readpos, M.READPOS_DTYPE, (1,))
    else:
        calls["groups"] = (L.hm_pileup_fetch_groups, M.GROUP_DTYPE, (0, N, 1))
    return calls, flat


def count_only(pu, what):
    calls, _keep = _row_calls(pu)
    fn, _dtype, args = calls[what]
    return (pu._check(fn(pu._h, *args, None, 0)),)


def cap_short(pu, what):
    """the fetch with room for one row less than there are: it returns their number and writes nothing (asserted here)"""
    calls, _keep = _row_calls(pu)
    fn, dtype, args = calls[what]
    n = pu._check(fn(pu._h, *args, None, 0))
    buf = np.full(max(n, 1) * dtype.itemsize, 0x55, np.uint8)
    got = pu._check(fn(pu._h, *args, _vp(buf), max(n - 1, 0)))
    assert got == n and (buf == 0x55).all(), (what, n, got)
    return (got,)


_ROW_EXPORTS = {"loci": "hm_pileup_fetch_loci", "asm": "hm_pileup_fetch_asm", "asm_q": "hm_pileup_fetch_asm_q", "asm_regions": "hm_pileup_fetch_asm_regions",
                "sites": "hm_pileup_fetch_sites", "domains": "hm_pileup_fetch_domains", "context": "hm_pileup_fetch_context",
                "patterns": "hm_pileup_fetch_patterns", "bedmethyl": "hm_pileup_fetch_bedmethyl", "linkage": "hm_pileup_fetch_linkage",
                "readpos": "hm_pileup_fetch_readpos", "groups": "hm_pileup_fetch_groups"}
for _w, _e in _ROW_EXPORTS.items():
    _kw = dict(load=_w in ("loci", "asm", "groups"), record=_w != "groups")
    reader("count_only_" + _w, _e, **_kw)(lambda pu, w=_w: count_only(pu, w))
    reader("cap_short_" + _w, _e, **_kw)(lambda pu, w=_w: cap_short(pu, w))
ROW_FETCHES = tuple(w for w in _ROW_EXPORTS if w != "groups")


# ---- results as bytes ----------------------------------------------------------------------------------------------------------
def blob(result):
    """a reader's result as one bytes object: dtype, shape and bytes of every array, the text of everything else"""
    parts = []
    for x in result:
        if isinstance(x, np.ndarray):
            parts.append(("%s%s|" % (x.dtype.str if x.dtype.names is None else x.dtype.descr, x.shape)).encode() + np.ascontiguousarray(x).tobytes())
        else:
            parts.append(repr(x).encode())
    return b"\0".join(parts)


def evaluate(fn, pu):
    """-> (bytes, result); a HifimethError (a fetch before its count) is a result like any other: its text"""
    try:
        result = fn(pu)
    except M.HifimethError as e:
        return b"error: " + str(e).encode(), None
    return blob(result), result


COUNT_FIELDS = ("n_uu", "n_um", "n_mu", "n_mm", "n_loci", "pcov", "ncov", "ppm", "n_m", "n_u", "sum_ml")


def is_empty_form(name, result):
    """what an engine without a read answers: no rows, zero tables, zero counts (the context fetch counts its table's rows)"""
    for x in result:
        if isinstance(x, np.ndarray) and x.dtype.names:
            counts = [f for f in x.dtype.names if f in COUNT_FIELDS]
            if len(x) and (not counts or any(x[f].any() for f in counts)):
                return False
        elif isinstance(x, np.ndarray):
            if x.size and (x.dtype.kind == "f" or x.any()):       # no table of doubles has a place to be filled from nothing
                return False
        elif x and not (name.endswith("_context") or name == "metaplot"):     # 3 (K + 1) table rows; the intervals that were used
            return False
    return True


# ---- the exports of the header by class ----------------------------------------------------------------------------------------
def _classes():
    out = {}
    for cls, names in (
        ("lifecycle", "hm_pileup_create hm_pileup_destroy hm_pileup_last_error"),
        ("mutator", "hm_pileup_set_option hm_pileup_set_reference hm_pileup_use_planes hm_pileup_use_partition_planes hm_pileup_submit_read "
                    "hm_pileup_submit_read_hp hm_pileup_submit_read_calls hm_pileup_run hm_pileup_count hm_pileup_load_loci hm_pileup_group_sample "
                    "hm_pileup_load_sample_loci hm_pileup_add_readpos"),
        ("host", "hm_asm_qvalues hm_group_qvalues hm_sites_table hm_domain_scores hm_domain_refit"),
        ("reader", "hm_pileup_planes hm_pileup_partition_planes hm_pileup_num_records hm_pileup_histograms hm_pileup_fetch_records "
                   "hm_pileup_label_histograms hm_pileup_fetch_loci hm_pileup_fetch_asm hm_pileup_asm_histogram hm_pileup_asm_bin_pvalues "
                   "hm_pileup_fetch_asm_q hm_pileup_fetch_asm_regions hm_pileup_fetch_groups hm_pileup_group_planes hm_pileup_control_sums "
                   "hm_pileup_site_histogram hm_pileup_fetch_sites hm_pileup_fetch_domains hm_pileup_fetch_domains_part hm_pileup_domain_sums "
                   "hm_pileup_domain_sums_part hm_pileup_num_pattern_records hm_pileup_fetch_patterns hm_pileup_fetch_bedmethyl "
                   "hm_pileup_fetch_linkage hm_pileup_fetch_readpos hm_pileup_readpos_histograms hm_pileup_fetch_regions hm_pileup_fetch_metaplot "
                   "hm_pileup_fetch_context hm_pileup_fetch_context_path"),
    ):
        out.update((n, cls) for n in names.split())
    return out


EXPORTS = _classes()
