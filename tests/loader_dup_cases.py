"""Duplicate loci for the three loaders of `diff`, `groupdiff` and `samplecorr`: seeded row arrays placed in chosen threads, and what
every loader must answer for them, by two routes.  Needs no GPU.

THE RULE (include/hifimeth_hip.h, hm_pileup_load_loci).  A row that passes the checks and carries a count is a duplicate exactly when
an earlier or concurrent row of the same locus was given to the same target -- the partition for `diff`, the open sample for the
other two -- since that target's planes were cleared or opened, across slabs and across calls.  Of k such rows on one locus exactly
k - 1 are duplicates, whatever the launch geometry, the row order or the slab size.  In `diff` a duplicate still adds; in the other
two it adds nothing and which row wins is open.

PLACEMENT.  Row i of a launch is thread i: wavefront i // 64 of workgroup i // 256; a call of n rows with load_slab = s is
ceil(n / s) launches, row i in launch i // s as its row i % s.  Every case says where it puts the rows of a locus (`claim`, with
`partners` or `runs` naming the rows); test_loader_dup_cases_cpu.py holds each case to its claim.

A CASE is a list of calls (target, rows): target 1 or 2, never decreasing.  For `diff` the target is the partition; for `groupdiff`
target t is the t-th sample opened in group 1 (both samples share partition 1 on purpose); for `samplecorr` the t-th sample opened.
Only the last call of a case holds bad rows: the engine is void after it.  Engines and restatements run with minimum coverage 1, so
every winning row adds and the number of rows that add does not depend on which row of a locus wins.

EXPECTED, two routes.  by_counts() works from the multiplicities alone: duplicates = sum over targets and loci of (k - 1), the rows
that add = the counted rows for `diff` and the distinct (target, locus) for the other two, the other bad kinds from the checks in
their order.  by_restatement() feeds the rows in order to diff_ref.Loader, groups_ref.GroupLoader or samples_ref.SampleLoader.  A
call with bad rows returns HM_EDATA, not a number: the rows that added show in the returns of the clean calls, in the planes, and
for the two sample loaders in the restatement's sample counts and levels.  The reference is that of test_gpu_pileup_loaders.py: three
contigs of 9877 bases."""
import functools

import numpy as np

from diff_ref import Loader
from groups_ref import GroupLoader
from samples_ref import SampleLoader

HM_EDATA, HM_ESTATE = -4, -5
LENGTHS = (4099, 3001, 2777)
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)])
TOTAL = int(OFFSETS[-1])
ENDS = [int(x) for s in range(3) for x in (OFFSETS[s], OFFSETS[s + 1] - 1)]      # the first and the last locus of every contig
WAVE, GROUP = 64, 256
MAX_ROWS = 16384
LIMIT = 1 << 20
STRIDE = 257
FOLDS = (3, 8, 64, 65, 256)
LOADERS = ("diff", "groupdiff", "samplecorr")
WHO = {"diff": "hm_pileup_load_loci", "groupdiff": "hm_pileup_load_sample_loci", "samplecorr": "hm_sample_load"}
DUP_TEXT = {"diff": "locus given twice for one part", "groupdiff": "locus given twice in one sample", "samplecorr": "locus given twice in one sample"}
BAD_TEXT = ("gpos outside the reference", "negative count", "count above 2^20 - 1", "motif above 3")
PAIR_KINDS = ("(p, n) + (p, n)", "(p, 0) + (0, n)", "(0, n) + (p, 0)", "(p, 0) + (p, 0)")      # the first of a pair is the row of the lower index
N_ORDERS = 4                                                  # the rows as placed, and three seeded permutations of every call


def message(loader, gpos, negative, big, motif, dup):
    """the engine's text for a call with these bad rows, the kinds in their order and the absent ones left out"""
    parts = [(gpos, BAD_TEXT[0]), (negative, BAD_TEXT[1]), (big, BAD_TEXT[2]), (motif, BAD_TEXT[3]), (dup, DUP_TEXT[loader])]
    return "%s: %d bad rows: %s" % (WHO[loader], sum(n for n, _ in parts), ", ".join("%d %s" % x for x in parts if x[0]))


class Case:
    def __init__(self, name, calls, claim, slab=None, partners=None, kinds=None, runs=None, calls_unlimited=None):
        self.name, self.claim, self.slab = name, claim, slab
        self._calls = {True: calls, False: calls if calls_unlimited is None else calls_unlimited}
        self.partners, self.kinds, self.runs = partners, kinds, runs      # rows of the LAST call: (first, second) per pair; locus -> its rows
        for per in self._calls.values():
            for _t, rows in per:
                for x in rows:
                    x.setflags(write=False)

    def calls(self, loader, order=0):
        """[(target, (gpos, pcov, ncov, motif))]: order 0 as placed, 1 .. 3 every call in a seeded permutation of its own"""
        out = []
        for c, (target, rows) in enumerate(self._calls[loader != "diff"]):
            if order:
                perm = np.random.default_rng([order, c, len(rows[0])]).permutation(len(rows[0]))
                rows = tuple(x[perm] for x in rows)
            out.append((target, rows))
        return out

    def __repr__(self):
        return self.name


def _arrays(g, p, n, m):
    return tuple(np.asarray(x, np.int64).copy() for x in (g, p, n, m))


def _counts(rng, size):
    """size counts of mixed kinds: a third each (p, n), (p, 0) and (0, n), p and n in 1 .. 12"""
    p, n = rng.integers(1, 13, size), rng.integers(1, 13, size)
    kind = rng.integers(0, 3, size)
    p[kind == 2] = 0
    n[kind == 1] = 0
    return p, n


def _pair_counts(rng, kinds):
    """-> (p, n) of the first rows, (p, n) of the second rows of pairs of these kinds"""
    size = len(kinds)
    p1, n1, p2, n2 = (rng.integers(1, 13, size) for _ in range(4))
    n1[(kinds == 1) | (kinds == 3)] = 0
    p1[kinds == 2] = 0
    p2[kinds == 1] = 0
    n2[(kinds == 2) | (kinds == 3)] = 0
    return (p1, n1), (p2, n2)


def _pairs(name, first, second, n_rows, seed, claim, slab=None):
    """one call of n_rows rows: pair j of kind j % 4 on a locus of its own in rows first[j] < second[j], every other row alone on
    its locus; the partners differ in counts and motif"""
    rng = np.random.default_rng(seed)
    first, second = np.asarray(first), np.asarray(second)
    pairs = len(first)
    assert (first < second).all() and len(np.unique(np.concatenate([first, second]))) == 2 * pairs and second.max() < n_rows
    loci = np.concatenate([ENDS, rng.choice(np.setdiff1d(np.arange(TOTAL), ENDS), n_rows - pairs - len(ENDS), replace=False)])
    rng.shuffle(loci)
    kinds = np.arange(pairs) % 4
    (p1, n1), (p2, n2) = _pair_counts(rng, kinds)
    g, p, n = (np.zeros(n_rows, np.int64) for _ in range(3))
    g[first] = g[second] = loci[:pairs]
    p[first], n[first], p[second], n[second] = p1, n1, p2, n2
    rest = np.setdiff1d(np.arange(n_rows), np.concatenate([first, second]))
    g[rest] = loci[pairs:]
    p[rest], n[rest] = _counts(rng, len(rest))
    m = rng.integers(0, 4, n_rows)
    return Case(name, [(1, _arrays(g, p, n, m))], claim, slab=slab, partners=np.stack([first, second], 1), kinds=kinds)


def _pairs_across(name, claim, slab=None):
    return _pairs(name, np.arange(2048), 2048 + np.arange(2048), 4096, 101, claim, slab)


def _folds(name, sets, singles, n_rows, seed, claim, place):
    """one call: `sets` loci of every multiplicity in FOLDS and `singles` rows alone on their loci, the kinds mixed; the rows of a
    locus follow each other in a list whose entry q stands in row place(q)"""
    rng = np.random.default_rng(seed)
    mult = np.array([k for _ in range(sets) for k in FOLDS] + [1] * singles)
    assert mult.sum() == n_rows
    loci = rng.choice(TOTAL, len(mult), replace=False)
    order = np.concatenate([np.arange(singles // 2) + sets * len(FOLDS), np.arange(sets * len(FOLDS)),
                            np.arange(singles // 2, singles) + sets * len(FOLDS)])      # half the single rows before the runs, half behind
    listed = np.repeat(loci[order], mult[order])
    at = place(np.arange(n_rows))
    assert sorted(at.tolist()) == list(range(n_rows))
    g = np.zeros(n_rows, np.int64)
    g[at] = listed
    p, n = _counts(rng, n_rows)
    runs = {int(l): at[listed == l] for l, k in zip(loci, mult) if k > 1}
    return Case(name, [(1, _arrays(g, p, n, rng.integers(0, 4, n_rows)))], claim, runs=runs)


def neighbour_loci():
    """loci whose words the bitmap (32 loci), the byte add (4) and the halfword compare-and-swap (2) share: g and g + 1 for an
    even and an odd g, the 32 loci of one bitmap word, those of the word that holds the end of contig 1 and the start of contig
    2, the loci of the last, partial word, and the first and the last locus of every contig"""
    return np.unique(np.concatenate([[100, 101, 201, 202], np.arange(160, 192), np.arange(4096, 4128), np.arange(TOTAL // 32 * 32, TOTAL), ENDS]))


def _neighbours(name, seed, identical):
    """one call: every locus of neighbour_loci() and 400 others twice, the second rows at least a workgroup behind the first;
    identical: the second row equals the first, and a locus each of 3, 64 and 65 equal rows follows"""
    rng = np.random.default_rng(seed)
    near = neighbour_loci()
    others = rng.choice(np.setdiff1d(np.arange(TOTAL), near), 400 + 300 + 3, replace=False)
    twice, alone, many = np.concatenate([near, others[:400]]), others[400:700], others[700:]
    rng.shuffle(twice)
    pairs = len(twice)
    kinds = np.arange(pairs) % 4
    if identical:
        p1, n1 = _counts(rng, pairs)
        (p2, n2), m1 = (p1, n1), rng.integers(0, 4, pairs)
        m2 = m1
    else:
        (p1, n1), (p2, n2) = _pair_counts(rng, kinds)
        m1, m2 = rng.integers(0, 4, pairs), rng.integers(0, 4, pairs)
    pa, na = _counts(rng, len(alone))
    g = [twice, alone, twice]
    p, n, m = [p1, pa, p2], [n1, na, n2], [m1, rng.integers(0, 4, len(alone)), m2]
    runs = None
    if identical:
        runs = {}
        for locus, k in zip(many, (3, 64, 65)):
            at = sum(len(x) for x in g)
            pk, nk = _counts(rng, 1)
            g.append(np.full(k, locus))
            p.append(np.full(k, pk[0]))
            n.append(np.full(k, nk[0]))
            m.append(np.full(k, rng.integers(0, 4)))
            runs[int(locus)] = at + np.arange(k)
    first = np.arange(pairs)
    return Case(name, [(1, _arrays(*(np.concatenate(x) for x in (g, p, n, m))))], "different workgroups", runs=runs,
                partners=np.stack([first, first + pairs + len(alone)], 1), kinds=None if identical else kinds)


def _across_calls():
    """call 1 gives 600 loci to target 1; call 2 the same loci, other counts, to target 2: not duplicates; call 3 gives target 2
    300 of them again and 100 new ones: 300 duplicates, each counted once"""
    rng = np.random.default_rng(107)
    loci = rng.choice(TOTAL, 700, replace=False)
    calls = []
    for target, g in ((1, loci[:600]), (2, rng.permutation(loci[:600])), (2, rng.permutation(np.concatenate([loci[:600:2], loci[600:]])))):
        p, n = _counts(rng, len(g))
        calls.append((target, _arrays(g, p, n, rng.integers(0, 4, len(g)))))
    return Case("across-calls", calls, "calls")


def _with_other_bad_rows():
    """one call, shuffled: 1500 rows alone on their loci; 40 pairs of the four kinds, a locus of 3 and one of 65 rows; rows of every
    other bad kind, some of them on the duplicated loci, where they add nothing and make nothing a duplicate; rows without a count
    on duplicated, single and fresh loci, one of them with a bad motif (the motif check comes first).  A row that fails two checks
    counts for the first.  `diff` has no count limit and would add the rows above it: its call goes without them."""
    out = {}
    for limited in (True, False):
        rng = np.random.default_rng(108)
        loci = rng.choice(TOTAL, 1500 + 42 + 10, replace=False)
        alone, twice, three, many, fresh = loci[:1500], loci[1500:1540], loci[1540], loci[1541], loci[1542:]
        (p1, n1), (p2, n2) = _pair_counts(rng, np.arange(40) % 4)
        pa, na = _counts(rng, 1500)
        pm, nm = _counts(rng, 68)
        rows = [np.stack([alone, pa, na, rng.integers(0, 4, 1500)], 1), np.stack([twice, p1, n1, rng.integers(0, 4, 40)], 1),
                np.stack([twice, p2, n2, rng.integers(0, 4, 40)], 1),
                np.stack([np.concatenate([np.full(3, three), np.full(65, many)]), pm, nm, rng.integers(0, 4, 68)], 1)]
        d = int(twice[0])
        bad = [(-1, 1, 1, 0), (TOTAL, 1, 1, 0), (1 << 40, 2, 0, 1), (-(1 << 40), 0, 2, 9), (-5, -1, -1, 7),                  # gpos: 5
               (d, -1, 1, 0), (int(alone[0]), 1, -2, 0), (int(fresh[0]), -7, -7, 4), (int(many), -1, 0, 0),                 # negative: 4
               (d, 1, 1, 4), (int(alone[1]), 3, 0, 5), (int(fresh[1]), 0, 2, 255), (int(many), 1, 1, 2 ** 32 - 1),          # motif: 7
               (int(three), 0, 0, 4), (int(fresh[2]), 0, 0, 9), (int(twice[1]), 1, 0, 2 ** 31)]
        big = [(d, LIMIT, 0, 0), (int(alone[2]), 0, LIMIT, 1), (int(fresh[3]), LIMIT - 1, 1, 2), (int(many), 2 ** 31 - 1, 2 ** 31 - 1, 7),
               (int(fresh[4]), 1 << 19, 1 << 19, 3), (int(twice[2]), LIMIT, 5, 4)]                                          # count: 6, two of them with a bad motif too
        none = [(d, 0, 0, 0), (int(twice[3]), 0, 0, 3), (int(alone[3]), 0, 0, 1), (int(fresh[5]), 0, 0, 2), (int(many), 0, 0, 0), (int(three), 0, 0, 1)]
        rows += [np.array(bad, np.int64), np.array(none, np.int64)] + ([np.array(big, np.int64)] if limited else [])
        table = np.concatenate(rows)
        table = table[rng.permutation(len(table))]
        out[limited] = [(1, _arrays(*table.T))]
    return Case("with-other-bad-rows", out[True], "mixed", calls_unlimited=out[False])


@functools.lru_cache(maxsize=None)
def cases():
    lane, wave = np.arange(32), np.arange(32)[:, None]
    block, t = np.arange(8)[:, None], np.arange(128)
    return (
        _pairs_across("pairs-across", "different workgroups"),
        _pairs("pairs-within, adjacent lanes", 2 * np.arange(512), 2 * np.arange(512) + 1, 1024, 102, "adjacent lanes of one wavefront"),
        _pairs("pairs-within, lanes l and 63 - l", (64 * wave + lane).ravel(), (64 * wave + 63 - lane).ravel(), 2048, 103,
               "lanes l and 63 - l of one wavefront"),
        _pairs("pairs-within, two wavefronts", (256 * block + t).ravel(), (256 * block + 128 + t).ravel(), 2048, 104,
               "two wavefronts of one workgroup"),
        _folds("k-fold, contiguous", 2, 200, 2 * sum(FOLDS) + 200, 105, "contiguous", lambda q: q),
        _folds("k-fold, stride 257", 4, 4096 - 4 * sum(FOLDS), 4096, 106, "stride 257", lambda q: STRIDE * q % 4096),
        _neighbours("neighbours", 109, identical=False),
        _pairs_across("across-slabs, partners in two launches", "different launches", slab=2048),
        _pairs_across("across-slabs, partners in one launch", "one launch, different workgroups", slab=4096),
        _pairs_across("across-slabs, slabs of 1000", "slabs of 1000", slab=1000),
        _across_calls(),
        _with_other_bad_rows(),
        _neighbours("identical-duplicates", 110, identical=True),
    )


def case(name):
    return next(c for c in cases() if c.name == name)


# ---- expected, route 1: from the multiplicities -----------------------------------------------------------------------------------
def by_counts(case, loader, order=0):
    """-> dict(returns per call, dup, message of the last call, added: the rows that add over all calls, covered: the loci that
    hold a count afterwards, ascending)"""
    limited = loader != "diff"
    calls = case.calls(loader, order)
    seen, returns, added, bad = {}, [], 0, None
    for target, (g, p, n, m) in calls:
        bad_g = (g < 0) | (g >= TOTAL)
        bad_c = ~bad_g & ((p < 0) | (n < 0))
        bad_b = ~bad_g & ~bad_c & (p + n >= LIMIT) if limited else np.zeros(len(g), bool)
        bad_m = ~bad_g & ~bad_c & ~bad_b & (m > 3)
        counted = ~bad_g & ~bad_c & ~bad_b & ~bad_m & (p + n > 0)
        loci, k = np.unique(g[counted], return_counts=True)
        dup = 0
        for locus, rows_at in zip(loci.tolist(), k.tolist()):
            before = seen.get((target, locus), 0)
            dup += rows_at - (0 if before else 1)               # of k rows in the window k - 1 are duplicates: the first one is not
            seen[target, locus] = before + rows_at
        took = int(counted.sum()) if loader == "diff" else int(counted.sum()) - dup
        added += took
        bad = (int(bad_g.sum()), int(bad_c.sum()), int(bad_b.sum()), int(bad_m.sum()), dup)
        returns.append(HM_EDATA if sum(bad) else took)
    return dict(returns=returns, dup=sum(k - 1 for k in seen.values()), message=message(loader, *bad), added=added,
                covered=np.unique([locus for _t, locus in seen]))


def clean_calls(case, loader):
    """the calls of the case as placed without their bad rows and their duplicates: of every (target, locus) the first counted row.
    Every call of it is clean and returns its number of rows; together they are the rows that add in the two sample loaders"""
    seen, out = set(), []
    for target, (g, p, n, m) in case.calls(loader):
        ok = (g >= 0) & (g < TOTAL) & (p >= 0) & (n >= 0) & (m <= 3) & (p + n > 0) & ((p + n < LIMIT) | (loader == "diff"))
        keep = []
        for i in np.flatnonzero(ok).tolist():
            if (target, int(g[i])) not in seen:
                seen.add((target, int(g[i])))
                keep.append(i)
        out.append((target, tuple(x[keep] for x in (g, p, n, m))))
    return out


# ---- expected, route 2: from the restatements, the rows in order ------------------------------------------------------------------------
def by_restatement(case, loader, order=0, calls=None):
    """-> (the same dict, the restatement after the case, or after `calls` in its place).  `added` is None for `diff`, whose
    restatement does not tell it for a call with bad rows: there the planes hold every added row"""
    ref = Loader(TOTAL) if loader == "diff" else GroupLoader(TOTAL, 1) if loader == "groupdiff" else SampleLoader(TOTAL, 2, 1)
    returns, opened = [], 0
    for target, rows in case.calls(loader, order) if calls is None else calls:
        if loader == "diff":
            returns.append(ref.load(target, *rows))
            continue
        while opened < target:
            assert (ref.begin_sample(1) if loader == "groupdiff" else ref.open()) == opened
            opened += 1
        returns.append(ref.load(*rows))
    b = list(ref.bad.values())
    if loader == "diff":
        b.insert(2, 0)                                       # no count limit
        added = None
    else:
        added = int(ref.samples[1].sum()) if loader == "groupdiff" else int(np.count_nonzero(ref.level))
    return dict(returns=returns, dup=b[4], message=message(loader, *b), added=added, covered=ref.loci()[0]), ref
