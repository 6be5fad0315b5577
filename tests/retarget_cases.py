"""Inputs for the tests of a second hm_pileup_set_reference on one engine (plain module, imported by test_retarget_cases_cpu.py and
test_gpu_pileup_retarget.py; it imports without a GPU).

THE CONTRACT (include/hifimeth_hip.h, hm_pileup_set_reference).  After the call returns HM_OK the engine is what a newly created one
would be on which the same options and caller planes were applied, followed by that one call.  Every case runs job A on an engine to
a stated depth, re-targets the engine and runs job B; a second, freshly created engine runs job B only, and the two agree in every
fetch, byte for byte.

JOBS ON RECORDS.  Four references of three contigs each, a few kilobases together, and one set of alignments per reference made as
sequence_cases.record_input makes them (pileup_cases.make_read: M I M D M with soft clips, both strands, HP 0 / 1 / 2 by turns):

    first     where job A runs
    same      the lengths and the bases of `first`
    changed   the lengths of `first`, other bases, another CpG list
    shorter   shorter contigs, fewer CpGs, other bases

DEPTHS of job A: "a" reads submitted and not run, "b" run and not counted (records and pattern windows resident), "c" one slab run,
counted and fetched, "d" two slabs.

THE RULE.  `changed` and `shorter` are used only where nothing is resident, at the depths "c" and "d".  It is a safety condition: a
library that drops nothing on the second call then still indexes inside the buffers it has allocated (a stale record is counted
into the planes of a reference of its own length, a stale CpG rank is below the n_cpg it was made under), so the cases show wrong
answers on such a library and never a write out of bounds.  RECORD_CASES holds every case; rule_holds() is the rule.

JOBS ON LOADED ROWS (`diff`, `groupdiff`, `samplecorr` / `regiondiff`).  One reference, that of the loader tests (loader_dup_cases.LENGTHS),
re-targeted onto itself: the seen bitmaps of job A and job B then share their words.  Rows are made as the loader tests make theirs:
distinct loci per target, pcov and ncov up to 12 in three kinds of counts.  Half of job B's loci are job A's, half are new.
"""
import dataclasses
import functools

import numpy as np

import loader_dup_cases as D
import pileup_cases as C
import sequence_cases as S
from hifimeth_amd.synth import synth_genome

DEPTHS = ("a", "b", "c", "d")
TARGETS = ("same", "changed", "shorter")
N_READS = 96
N_SLABS = 2
TRIM = S.TRIM
PATTERN_K, PATTERN_SPAN, LINKAGE, PROFILE = 3, 150, 64, 16
FILTER = dict(min_mapq=35, min_pi=99.3)                             # identity in percent

# the option sets of the record families, and the readers of sequence_cases.CATALOGUE each family is held to
COMMON = ("histograms", "loci", "loci_sub", "records", "label_histograms")
PLANE_FNS = ("regions", "metaplot", "context_0", "context_2", "sites_chain", "control_sums", "domains_0", "domains_1", "domains_2", "domain_sums_0")
HP = ("loci_part1", "loci_part2", "asm", "asm_regions_0")
FAMILIES = {
    "plain": (dict(), COMMON),
    "partitions": (dict(partitions=True), COMMON + HP + ("asm_q_chain",)),
    "patterns": (dict(patterns=PATTERN_K, pattern_span=PATTERN_SPAN), COMMON + ("patterns", "patterns_sub")),
    "bedmethyl": (dict(bedmethyl=True), COMMON + ("bedmethyl_0",)),
    "bedmethyl+partitions": (dict(bedmethyl=True, partitions=True), COMMON + ("bedmethyl_0", "bedmethyl_1", "bedmethyl_2")),
    "linkage": (dict(linkage=LINKAGE), COMMON + ("linkage", "linkage_all")),
    "profile+trim": (dict(profile=PROFILE, trim=TRIM), COMMON + ("readpos", "readpos_histograms")),
    "filtered": (dict(**FILTER), COMMON),
    "all": (dict(partitions=True, patterns=PATTERN_K, pattern_span=PATTERN_SPAN, bedmethyl=True, linkage=LINKAGE, profile=PROFILE, trim=TRIM),
            COMMON + HP + PLANE_FNS + ("patterns", "bedmethyl_0", "bedmethyl_1", "linkage", "readpos")),
    "plain, plane functions": (dict(), COMMON + PLANE_FNS),
}
# (family, depth of job A, the reference of job B): every family at every depth onto `same`; the functions of the planes and the
# tables sized by the reference onto `changed` and `shorter`, where nothing is resident
RECORD_CASES = tuple((f, d, "same") for f in FAMILIES if f != "plain, plane functions" for d in DEPTHS) + \
    tuple((f, d, t) for f in ("all", "plain, plane functions") for d in ("c", "d") for t in ("changed", "shorter"))


def rule_holds(depth, target):
    return target == "same" or depth in ("c", "d")


# ---- references and reads ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    """`first`, `same`, `changed` or `shorter` -> [(name, SEQUENCE)] of three contigs"""
    length, seed = {"first": (1500, 501), "same": (1500, 501), "changed": (1500, 502), "shorter": (1100, 503)}[name]
    return synth_genome(n_chr=3, length=length, gc=0.5, seed=seed, n_frac=0.0)


@functools.lru_cache(maxsize=None)
def job(name):
    """"A" (on `first`) or the job B of a target -> (genome, reads): N_READS alignments of 450 .. 900 columns, sorted"""
    ref, seed = {"A": ("first", 511), "same": ("same", 512), "changed": ("changed", 513), "shorter": ("shorter", 514)}[name]
    g = reference(ref)
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(N_READS):
        tid = i % 3
        a, b, c = (int(x) for x in rng.integers(150, 300, 3))
        ni, nd = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        spec = ([("S", int(rng.integers(1, 20)))] if i % 4 == 0 else []) + [("M", a), ("I", ni), ("M", b), ("D", nd), ("M", c)] \
            + ([("S", int(rng.integers(1, 20)))] if i % 5 == 0 else [])
        pos = int(rng.integers(0, len(g[tid][1]) - (a + b + c + nd) + 1))
        r = C.make_read("%s_%d" % (name, i), 16 if (i // 3) % 2 else 0, tid, pos, spec, g, rng, mapq=int(rng.integers(20, 61)))
        reads.append(dataclasses.replace(r, hp=(i // 6) % 3))
    reads.sort(key=lambda r: (r.tid, r.pos))
    return g, reads


def slabs(reads):
    n = (len(reads) + N_SLABS - 1) // N_SLABS
    return [reads[k * n:(k + 1) * n] for k in range(N_SLABS)]


def offsets(genome):
    return np.concatenate([[0], np.cumsum([len(s) for _n, s in genome])]).astype(np.int64)


def cpg_list(genome):
    """the global positions of the reference CpGs: a CG inside one contig"""
    off = offsets(genome)
    return [int(off[s]) + i for s, (_n, seq) in enumerate(genome) for i in range(len(seq) - 1) if seq[i:i + 2].upper() == "CG"]


def run_to(pu, depth, reads, readers=()):
    """job A on the engine up to `depth`; at the depths that count, every reader is asked afterwards"""
    first, second = slabs(reads)
    if depth == "a":
        for r in first:
            pu.add(r)
        return
    S.feed_slab(pu, first, stop="run" if depth == "b" else None)
    if depth == "d":
        S.feed_slab(pu, second)
    if depth in ("c", "d"):
        for fn in readers:
            S.evaluate(fn, pu)


def run_job(pu, reads):
    """a whole job: every slab run and counted at the medians of the histograms so far -> the thresholds per slab"""
    return [S.feed_slab(pu, s) for s in slabs(reads)]


def readers(family):
    cat = dict(S.CATALOGUE)
    return [(n, cat[n]) for n in FAMILIES[family][1]]


# ---- job B by the restatements -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated(target, trim=False, filtered=False):
    """job B of `target` by the restatements (pileup_oracle, bedmethyl_ref, patterns_ref, linkage_ref, readpos_ref), fed as run_job
    feeds it -> dict: bins (3 x 256), thresholds per slab, and per reader of the catalogue the rows as tuples of Python integers"""
    import bedmethyl_ref as BR
    import linkage_ref as LR
    import patterns_ref as PR
    import readpos_ref as RR
    from oracle import pileup_oracle as P
    g, reads = job(target)
    kw = FILTER if filtered else {}
    cut = [S.trimmed(r, TRIM) for r in reads] if trim else reads
    off = offsets(g)
    thrs, seen = [], []
    for slab in slabs(cut):
        seen += [C.as_dict(r) for r in slab]
        thrs.append(S.median_thresholds(P.pileup(seen, g, **kw)["bins"]))
    out = {"histograms": P.pileup(seen, g, **kw)["bins"], "thresholds": thrs}
    cov, parts, bm, win = {}, [{}, {}], [{}, {}, {}], {}
    for slab, thr in zip(slabs(cut), thrs):
        dicts = [C.as_dict(r) for r in slab]
        for sid, soff, p, n, m in P.pileup(dicts, g, thresholds=thr, **kw)["loci"]:
            e = cov.setdefault(int(off[sid]) + soff, [0, 0, m])
            e[0], e[1], e[2] = e[0] + p, e[1] + n, m
        for hp in (1, 2):
            for sid, soff, p, n, _m in P.pileup([d for d, r in zip(dicts, slab) if r.hp == hp], g, thresholds=thr, **kw)["loci"]:
                e = parts[hp - 1].setdefault(int(off[sid]) + soff, [0, 0])
                e[0], e[1] = e[0] + p, e[1] + n
        if filtered:
            continue
        for part, c in enumerate(BR.counters(dicts, g, thr[0], [r.hp for r in slab])):
            for (sid, q), n in c.items():
                e = bm[part].setdefault(int(off[sid]) + q, [0] * 5)
                bm[part][int(off[sid]) + q] = [a + b for a, b in zip(e, n)]
        for key, cnt in PR.windows(dicts, g, PATTERN_K, PATTERN_SPAN, thr[0]).items():
            e = win.setdefault(key, [0] * (1 << PATTERN_K))
            win[key] = [a + b for a, b in zip(e, cnt)]
    out["loci"] = [(q, *cov[q]) for q in sorted(cov)]
    for hp in (1, 2):
        out["loci_part%d" % hp] = [(q, *parts[hp - 1][q], cov[q][2]) for q in sorted(parts[hp - 1])]
    if filtered:
        return out
    out["bedmethyl_0"] = [(q, *n) for q, n in sorted(bm[0].items()) if sum(n) >= 1]
    out["bedmethyl_1"] = [(q, *n) for q, n in sorted(bm[1].items()) if sum(n) >= 1 and n[0] + n[1] >= 1]
    cpgs = PR.reference_cpgs(g)
    out["patterns"] = [(int(off[sid]) + first, int(off[sid]) + cpgs[sid][cpgs[sid].index(first) + PATTERN_K - 1] + 2, *cnt, sum(cnt))
                       for (sid, first), cnt in sorted(win.items())]
    out["linkage"] = LR.rows([C.as_dict(r) for r in cut], g, LINKAGE, thrs[-1][0])
    out["readpos"] = RR.rows([C.as_dict(r) for r in reads], g, PROFILE, thrs[-1], trim=TRIM if trim else (0, 0))
    return out


ROW_FIELDS = {
    "loci": ("gpos", "pcov", "ncov", "motif"), "loci_part1": ("gpos", "pcov", "ncov", "motif"), "loci_part2": ("gpos", "pcov", "ncov", "motif"),
    "bedmethyl_0": ("gpos", "n_mod", "n_canon", "n_nocall", "n_diff", "n_delete"), "bedmethyl_1": ("gpos", "n_mod", "n_canon", "n_nocall", "n_diff", "n_delete"),
    "linkage": ("dist", "n_uu", "n_um", "n_mu", "n_mm"), "readpos": ("motif", "end", "dist", "n_m", "n_u", "sum_ml"),
}


def as_tuples(name, result):
    """a reader's result in the form of restated()[name]"""
    if name == "histograms":
        return np.asarray(result[0])
    rows = result[0]
    if name == "patterns":
        return [(int(r["start"]), int(r["end"]), *(int(x) for x in r["counts"][:1 << PATTERN_K]), int(r["n"])) for r in rows]
    return [tuple(int(r[f]) for f in ROW_FIELDS[name]) for r in rows]


# ---- loaded rows -----------------------------------------------------------------------------------------------------------------------
TOTAL = D.TOTAL
LOAD_MIN_COV = 5
N_ROWS = 3000                                                        # of 9877 loci: some two hundred loci count in three samples of a job
GROUP_SAMPLES = {"A": (1, 1, 2, 2), "B": (1, 2, 2, 1)}               # the group of every sample, in the order they are opened
SAMPLES_OPENED = {"A": 3, "B": 2}
SAMPLES_OPTION = 4


@functools.lru_cache(maxsize=None)
def load_genome():
    rng = np.random.default_rng(521)
    return [("ctg%d" % (s + 1), "".join(rng.choice(list("ACGT"), n))) for s, n in enumerate(D.LENGTHS)]


def _rows(rng, loci):
    """one row per locus in shuffled order: pcov, ncov in 0 .. 12 (a third of the rows each (p, n), (p, 0), (0, n)), motif 0 .. 3"""
    g = rng.permutation(np.asarray(loci, np.int64))
    p, n = D._counts(rng, len(g))
    out = (g, p, n, rng.integers(0, 4, len(g)))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _loci(jobname, k):
    """the loci of row set k of a job: job B's are half job A's of the same k, half loci no row set of job A holds"""
    rng = np.random.default_rng([522, k])
    mine = np.concatenate([D.ENDS[:3], rng.choice(np.setdiff1d(np.arange(TOTAL), D.ENDS), N_ROWS - 3, replace=False)])
    if jobname == "A":
        return mine
    used = np.unique(np.concatenate([_loci("A", j) for j in range(4)]))
    new = np.random.default_rng([523, k]).choice(np.setdiff1d(np.arange(TOTAL), used), N_ROWS // 2, replace=False)
    return np.concatenate([mine[:N_ROWS // 2], new])


@functools.lru_cache(maxsize=None)
def load_rows(jobname, k):
    """row set k (0 .. 3) of job "A" or "B": for `diff` sets 0 and 1 go to parts 1 and 2; for `groupdiff` set k is the k-th sample
    opened, in group GROUP_SAMPLES[job][k]; for `samplecorr` set k is sample k"""
    return _rows(np.random.default_rng([524, "AB".index(jobname), k]), _loci(jobname, k))


def duplicated(rows, k=3):
    """the rows with their first 5 counted rows given k times, the copies put at the end: 5 (k - 1) duplicates whatever the order"""
    g, p, n, m = rows
    i = np.flatnonzero(p + n > 0)[:5]
    return tuple(np.concatenate([x] + [x[i]] * (k - 1)) for x in (g, p, n, m))


def diff_restated(jobname):
    from diff_ref import Loader
    ref = Loader(TOTAL)
    returns = [ref.load(part, *load_rows(jobname, part - 1)) for part in (1, 2)]
    return ref, returns


def groups_restated(jobname):
    from groups_ref import GroupLoader
    ref = GroupLoader(TOTAL, LOAD_MIN_COV)
    indices, returns = [], []
    for k, g in enumerate(GROUP_SAMPLES[jobname]):
        indices.append(ref.begin_sample(g))
        returns.append(ref.load(*load_rows(jobname, k)))
    return ref, indices, returns


def samples_restated(jobname):
    from samples_ref import SampleLoader
    ref = SampleLoader(TOTAL, SAMPLES_OPTION, LOAD_MIN_COV)
    returns = []
    for k in range(SAMPLES_OPENED[jobname]):
        assert ref.open() == k
        returns.append(ref.load(*load_rows(jobname, k)))
    return ref, returns


def load_intervals():
    """tiles of 300 loci over the reference and one interval over all of it, global coordinates -> (start, end)"""
    a = list(range(0, TOTAL, 300)) + [0]
    b = [min(x + 300, TOTAL) for x in a[:-1]] + [TOTAL]
    return np.array(a, np.int64), np.array(b, np.int64)
