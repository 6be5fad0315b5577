"""One pileup engine under shuffled, repeated and interleaved fetches (tests/sequence_cases.py has the inputs and the catalogue).

Every output of the engine runs on shared, mutable device state; every other test file builds an engine, feeds it and asks one family
of fetches once.  Here the expectation of a catalogue entry is its answer on a FRESH engine, fed identically and asked nothing else,
and every comparison is byte equality: the same kernels on the same inputs give the same bits, whatever was asked before.  The fresh
answers themselves are held once to the existing restatements (test_fresh_answers_equal_the_restatements, test_fresh_group_tests_*),
so that the expectation is not merely self-consistent."""
import ctypes

import numpy as np
import pytest

import groups_ref as G
import pileup_cases as C
import sequence_cases as S
from sequence_cases import HM_EINVAL, HM_ESTATE

pytestmark = pytest.mark.gpu
_CACHE = {}
POINTS = [(k, stage) for k in range(S.N_SLABS) for stage in ("run", "count")]     # where an engine can be stopped while it is fed
NAMES = [n for n, _f in S.CATALOGUE]
LOAD_NAMES = [n for n, _f in S.LOAD_CATALOGUE]


# ---- engines -------------------------------------------------------------------------------------------------------------------
def _crafted():
    import torch
    if "crafted" not in _CACHE:
        _CACHE["crafted"] = [torch.from_numpy(x).cuda() for x in S.ladder_planes()]
    return _CACHE["crafted"]


def _new(genome, **options):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(genome, **options)
    pu.crafted = _crafted()
    return pu


def _build(kind, point=None):
    """a fed engine: kind "rec0" / "rec1" (the two record inputs, stopped after POINTS[..] = point if given) or "load" """
    if kind == "load":
        pu = _new(S.load_genome(), **S.LOAD_OPTIONS)
        S.feed_load(pu)
        return pu
    g, reads = S.record_input(int(kind[3]))
    pu = _new(g, **S.RECORD_OPTIONS)
    for k, slab in enumerate(S.slabs(reads)):
        here = point is not None and point[0] == k
        S.feed_slab(pu, slab, stop="run" if here and point[1] == "run" else None)
        if here:
            break
    return pu


def _catalogue(kind):
    return S.LOAD_CATALOGUE if kind == "load" else S.CATALOGUE


def _fresh(kind, point=None, names=None):
    """name -> (bytes, result) of every entry on an engine of its own that is asked nothing else"""
    have = _CACHE.setdefault(("fresh", kind, point), {})
    for name, fn in _catalogue(kind):
        if name not in have and (names is None or name in names):
            pu = _build(kind, point)
            have[name] = S.evaluate(fn, pu)
            pu.close()
    return have


@pytest.fixture(scope="module")
def shared():
    engines = {"rec0": _build("rec0"), "load": _build("load")}
    yield engines
    for pu in engines.values():
        pu.close()


def _shuffle(kind, seed, times=2):
    cat = _catalogue(kind) * times
    return [cat[i] for i in np.random.default_rng(seed).permutation(len(cat))]


# ---- the fresh answers against the restatements ----------------------------------------------------------------------------------
def _tuples(rows, fields):
    return [tuple(int(r[f]) for f in fields) for r in rows]


def test_fresh_answers_equal_the_restatements():
    import bedmethyl_ref as BR
    import context_ref as XR
    import domains_ref as DR
    import linkage_ref as LR
    import patterns_ref as PR
    import readpos_ref as RR
    import regions_ref as GR
    from hifimeth_amd import pileup as M
    from oracle import pileup_oracle as P
    g, reads = S.record_input(0)
    cut = [S.trimmed(r) for r in reads]
    off = np.concatenate([[0], np.cumsum([len(s) for _n, s in g])])
    fresh = {n: r for n, (_b, r) in _fresh("rec0").items()}
    assert all(r is not None for r in fresh.values())
    # the thresholds the feeding used: the medians of the restated histograms so far
    thrs, seen = [], []
    for slab in S.slabs(cut):
        seen += [C.as_dict(r) for r in slab]
        thrs.append(S.median_thresholds(P.pileup(seen, g)["bins"]))
    assert (fresh["histograms"][0] == P.pileup(seen, g)["bins"]).all()
    # loci: the counters of three counts add up; the motif is that of the last record in BAM order
    cov, parts, bm, win = {}, [{}, {}], [{}, {}, {}], {}
    k_pat = S.RECORD_OPTIONS["patterns"]
    for slab_cut, thr in zip(S.slabs(cut), thrs):
        dicts = [C.as_dict(r) for r in slab_cut]
        for sid, soff, p, n, m in P.pileup(dicts, g, thresholds=thr)["loci"]:
            e = cov.setdefault(int(off[sid]) + soff, [0, 0, m])
            e[0], e[1], e[2] = e[0] + p, e[1] + n, m
        for hp in (1, 2):
            for sid, soff, p, n, _m in P.pileup([d for d, r in zip(dicts, slab_cut) if r.hp == hp], g, thresholds=thr)["loci"]:
                e = parts[hp - 1].setdefault(int(off[sid]) + soff, [0, 0])
                e[0], e[1] = e[0] + p, e[1] + n
        for part, c in enumerate(BR.counters(dicts, g, thr[0], [r.hp for r in slab_cut])):
            for (sid, q), n in c.items():
                e = bm[part].setdefault(int(off[sid]) + q, [0] * 5)
                bm[part][int(off[sid]) + q] = [a + b for a, b in zip(e, n)]
        for key, cnt in PR.windows(dicts, g, k_pat, 150, thr[0]).items():
            e = win.setdefault(key, [0] * (1 << k_pat))
            win[key] = [a + b for a, b in zip(e, cnt)]
    assert _tuples(fresh["loci"][0], ("gpos", "pcov", "ncov", "motif")) == [(q, *cov[q]) for q in sorted(cov)]
    for hp in (1, 2):
        assert _tuples(fresh["loci_part%d" % hp][0], ("gpos", "pcov", "ncov", "motif")) == [(q, *parts[hp - 1][q], cov[q][2]) for q in sorted(parts[hp - 1])]
    bm_fields = ("gpos", "n_mod", "n_canon", "n_nocall", "n_diff", "n_delete")
    assert _tuples(fresh["bedmethyl_0"][0], bm_fields) == [(q, *n) for q, n in sorted(bm[0].items()) if sum(n) >= 1]
    assert _tuples(fresh["bedmethyl_1"][0], bm_fields) == [(q, *n) for q, n in sorted(bm[1].items()) if sum(n) >= 1 and n[0] + n[1] >= 1]
    cpgs = PR.reference_cpgs(g)
    want = [(int(off[sid]) + first, int(off[sid]) + cpgs[sid][cpgs[sid].index(first) + k_pat - 1] + 2, *cnt, sum(cnt)) for (sid, first), cnt in sorted(win.items())]
    got = [(int(r["start"]), int(r["end"]), *(int(x) for x in r["counts"][:1 << k_pat]), int(r["n"])) for r in fresh["patterns"][0]]
    assert got == want and len(want) > 20 and not fresh["patterns"][0]["counts"][:, 1 << k_pat:].any()
    everything = [C.as_dict(r) for r in cut]
    assert _tuples(fresh["linkage"][0], ("dist", "n_uu", "n_um", "n_mu", "n_mm")) == LR.rows(everything, g, S.RECORD_OPTIONS["linkage"], thrs[-1][0])
    assert _tuples(fresh["readpos"][0], ("motif", "end", "dist", "n_m", "n_u", "sum_ml")) == \
        RR.rows([C.as_dict(r) for r in reads], g, S.RECORD_OPTIONS["profile"], thrs[-1], trim=S.TRIM)
    # the outputs that are functions of the planes, from the rows just checked
    loci = fresh["loci"][0]
    pc, nc, ky = GR.planes_from_loci(loci, int(off[-1]))
    iv = S._intervals(type("E", (), {"lengths": np.diff(off), "offsets": off}))
    run = GR.Running(pc, nc, ky)
    sums = fresh["regions"][0]
    assert (np.stack([sums[q] for q in GR.QUANTITIES], -1) == GR.region_sums(run, iv["start"], iv["end"])).all() and sums["n_loci"].sum() > 1000
    rows, used = fresh["metaplot"]
    tab, want_used = GR.metaplot(run, iv["start"], iv["end"], iv["seq_start"], iv["seq_end"], iv["strand"], 5, 40, 2)
    assert used == want_used and (np.stack([rows[q] for q in ("n_regions",) + GR.QUANTITIES], -1).reshape(3, 9, 5) == tab).all()
    seqs = [s for _n, s in g]
    for flank in (0, 2):
        assert (fresh["context_%d" % flank][0] == XR.context_table(pc, nc, ky, seqs, flank)).all()
    for ctx in range(3):
        seg, n_rows = DR.domains(loci, ctx, *M.domain_scores(*M.DOMAIN_LEVELS[ctx]), M.DOMAIN_MAX_GAP)
        assert fresh["domains_%d" % ctx][0].tobytes() == seg.tobytes() and fresh["domains_%d" % ctx][1] == n_rows and n_rows > 100


def test_fresh_group_tests_equal_the_restatement_within_its_bound():
    """the selection exactly, the statistic under test_gpu_pileup_groups.py's own bar: 8 x E_ref against mpmath"""
    import test_gpu_pileup_groups as TG
    fresh = {n: r for n, (_b, r) in _fresh("load").items()}
    ref, refs, e_ref = G.dataset_loader(), G.references(), G.e_ref()
    for reps in (1, 2):
        assert TG._tuples(fresh["group_tests_%d" % reps][0]) == ref.tested(reps)
    rows = fresh["group_tests_1"][0]
    worst = TG._check_statistic(rows, lambda r: (ref.sums(int(r["gpos"])), refs["locus %d" % r["gpos"]][1]), e_ref)
    print("%d loci: " % len(rows) + ", ".join("E_gpu(%s) = %.3g = %.3g E_ref" % (k, v, v / e_ref[k]) for k, v in worst.items()))


# ---- 1. ordered pairs ------------------------------------------------------------------------------------------------------------
def _pairs(pu, kind, a):
    fresh, cat = _fresh(kind), dict(_catalogue(kind))
    for b in cat:
        if b != a:
            S.evaluate(cat[a], pu)
            assert S.evaluate(cat[b], pu)[0] == fresh[b][0], "%s after %s" % (b, a)


@pytest.mark.parametrize("a", NAMES)
def test_ordered_pairs(shared, a):
    _pairs(shared["rec0"], "rec0", a)


@pytest.mark.parametrize("a", LOAD_NAMES)
def test_ordered_pairs_on_the_load_engine(shared, a):
    _pairs(shared["load"], "load", a)


# ---- 2. shuffles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", [("rec0", s) for s in range(6)] + [("load", s) for s in (6, 7)])
def test_shuffles(shared, kind, seed):
    fresh = _fresh(kind)
    for i, (name, fn) in enumerate(_shuffle(kind, seed)):
        assert S.evaluate(fn, shared[kind])[0] == fresh[name][0], "seed %d, position %d: %s" % (seed, i, name)


# ---- 3. growth ladders -----------------------------------------------------------------------------------------------------------
def _ladder_tables():
    """the host tables of the q and the site fetches over the whole of the crafted planes (inputs of the ladder, made once)"""
    if "tables" not in _CACHE:
        from hifimeth_amd import pileup as M
        pu = _build("rec0")
        cr = pu.crafted
        bins, big = pu.asm_histogram(0, S.LADDER_N, S.LADDER_MIN_COV, [cr[k] for k in (3, 4, 5, 6, 2)], S.PLANE_BASE)
        asm_t = M.asm_qvalues(pu.asm_bin_pvalues(bins), big)
        sbins, sbig = pu.site_histogram(0, S.LADDER_N, cr[:3], S.PLANE_BASE)
        _CACHE["tables"] = asm_t, M.sites_table([0.3, 0.3, 0.3], sbins, sbig)
        pu.close()
    return _CACHE["tables"]


def _step(pu, what, lo, hi):
    from hifimeth_amd import pileup as M
    cr = pu.crafted
    three, five, base = cr[:3], [cr[k] for k in (3, 4, 5, 6, 2)], S.PLANE_BASE
    asm_t, site_t = _ladder_tables()
    if what == "loci":
        return (pu.loci(lo, hi, three, base),)
    if what == "asm":
        return (pu.asm(lo, hi, S.LADDER_MIN_COV, five, base),)
    if what == "asm_q":
        return (pu.asm(lo, hi, S.LADDER_MIN_COV, five, base, asm_t),)
    if what == "asm_regions":
        return pu.asm_regions(0, lo, hi, S.LADDER_MIN_COV, 0.01, 500, 1, five, base, True)
    if what == "sites":
        return (pu.sites(site_t, lo, hi, three, base),)
    if what == "domains":
        return pu.domains(0, lo, hi, planes=three, plane_base=base)
    if what == "domains_part":
        out = pu.domains_part(0, lo, hi, M.DOMAIN_PASS_SEGMENTS, {}, planes=three, plane_base=base)
        return out["segments"], out["n_rows"], out["d_last"]
    own_lo, own_hi = max(pu.n_loci // 2 - (hi - lo) // 2, 0), min(pu.n_loci // 2 + (hi - lo + 1) // 2, pu.n_loci)
    if what == "patterns":                                    # the engine's own tables: the same widths around its middle
        return (pu.patterns(own_lo, own_hi, 1),)
    return (pu.bedmethyl(own_lo, own_hi, 0, 1),)


@pytest.mark.parametrize("what", ["loci", "asm", "asm_q", "asm_regions", "sites", "domains", "domains_part", "patterns", "bedmethyl"])
def test_growth_ladder(what):
    """a cold engine walks the nested ranges up and down, a fetch of another row type between the steps: every step outgrows the
    staging buffers of the one before, and no step may see the rows, the addresses or the counts of another"""
    crafted = what not in ("patterns", "bedmethyl")
    steps = S.LADDER if crafted else S.LADDER[3::2]
    want = []
    for lo, hi in steps:
        fresh = _build("rec0")
        want.append(S.blob(_step(fresh, what, lo, hi)))
        fresh.close()
    assert len(set(want)) == len(want) or not crafted
    between = _fresh("rec0", names=("linkage", "readpos"))
    pu = _build("rec0")
    for i in list(range(len(steps))) + list(range(len(steps) - 2, -1, -1)):
        assert S.blob(_step(pu, what, *steps[i])) == want[i], (what, steps[i])
        other = "readpos" if what == "loci" or i % 2 else "linkage"
        assert S.evaluate(dict(S.CATALOGUE)[other], pu)[0] == between[other][0], (what, steps[i], other)
    pu.close()


def test_context_flank_and_regions_index_grow_and_shrink():
    fresh, cat = _fresh("rec0", names=("context_0", "context_2", "regions", "regions_sub_part2", "linkage")), dict(S.CATALOGUE)
    pu = _build("rec0")
    for name in ("context_0", "context_2", "context_0", "regions_sub_part2", "regions", "regions_sub_part2"):
        assert S.evaluate(cat[name], pu)[0] == fresh[name][0], name
        assert S.evaluate(cat["linkage"], pu)[0] == fresh["linkage"][0], name
    pu.close()


# ---- 4. readers between slabs ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def between_slabs():
    """engine X is read all over after every run and after every count, engine Y is only fed -> X's answers by point, X, Y"""
    g, reads = S.record_input(0)
    x, y = _new(g, **S.RECORD_OPTIONS), _new(g, **S.RECORD_OPTIONS)
    seen = {}
    for k, slab in enumerate(S.slabs(reads)):
        thr = S.feed_slab(x, slab, stop="run")
        seen[(k, "run")] = [(name, S.evaluate(fn, x)[0]) for name, fn in _shuffle("rec0", 40 + k, times=1)]
        x.count(thr)
        seen[(k, "count")] = [(name, S.evaluate(fn, x)[0]) for name, fn in _shuffle("rec0", 50 + k, times=1)]
        assert S.feed_slab(y, slab) == thr
    yield seen, x, y
    x.close()
    y.close()


@pytest.mark.parametrize("point", POINTS, ids=["%s%d" % (stage, k) for k, stage in POINTS])
def test_readers_between_slabs_equal_an_engine_stopped_there(between_slabs, point):
    seen, _x, _y = between_slabs
    fresh = _fresh("rec0", point)
    assert len(seen[point]) == len(S.CATALOGUE)
    for i, (name, got) in enumerate(seen[point]):
        assert got == fresh[name][0], "position %d: %s" % (i, name)
    if point == (0, "run"):                                   # the state after run: the records are resident, nothing is counted
        assert fresh["records"][1][4] > 500 and fresh["label_histograms"][1][0].any() and fresh["patterns"][1] is None


def test_readers_between_slabs_change_nothing(between_slabs):
    _seen, x, y = between_slabs
    fresh = _fresh("rec0")
    for name, fn in S.CATALOGUE:
        a, b = S.evaluate(fn, x)[0], S.evaluate(fn, y)[0]
        assert a == b == fresh[name][0], name


# ---- 5. failed calls leave nothing behind ----------------------------------------------------------------------------------------
def _failing_calls(pu, off):
    """[(what, call() -> return code, the code it must return, a word of the message or None)]"""
    L, h, o, N = pu._L, pu._h, off._h, pu.n_loci
    n3, n5 = (None,) * 3, (None,) * 5
    row = np.zeros(1, dtype=[("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("motif", "<u4"), ("reserved", "<u4")])
    row["pcov"] = 3
    return [
        ("loci, lo > hi", lambda: L.hm_pileup_fetch_loci(h, *n3, 0, 10, 5, None, 0), HM_EINVAL, b"hm_pileup_fetch_loci"),
        ("patterns off", lambda: L.hm_pileup_fetch_patterns(o, 0, N, 1, None, 0), HM_ESTATE, b"hm_pileup_fetch_patterns"),
        ("patterns, lo > hi", lambda: L.hm_pileup_fetch_patterns(h, 10, 5, 1, None, 0), HM_EINVAL, b"hm_pileup_fetch_patterns"),
        ("bedmethyl off", lambda: L.hm_pileup_fetch_bedmethyl(o, 0, 0, N, 0, None, 0), HM_ESTATE, b"hm_pileup_fetch_bedmethyl"),
        ("load_loci after records", lambda: L.hm_pileup_load_loci(h, 1, row.ctypes.data_as(ctypes.c_void_p), 1), HM_ESTATE, b"staged records"),
        ("bedmethyl, min_valid < 0", lambda: L.hm_pileup_fetch_bedmethyl(h, 0, 0, N, -1, None, 0), HM_EINVAL, b"hm_pileup_fetch_bedmethyl"),
        ("linkage off", lambda: L.hm_pileup_fetch_linkage(o, 1, None, 0), HM_ESTATE, None),
        ("linkage, min_pairs < 0", lambda: L.hm_pileup_fetch_linkage(h, -1, None, 0), HM_EINVAL, None),
        ("readpos off", lambda: L.hm_pileup_fetch_readpos(o, 1, None, 0), HM_ESTATE, None),
        ("asm without partitions", lambda: L.hm_pileup_fetch_asm(o, *n5, 0, 0, N, 2, None, 0), HM_ESTATE, None),
        ("asm, min_cov < 1", lambda: L.hm_pileup_fetch_asm(h, *n5, 0, 0, N, 0, None, 0), HM_EINVAL, None),
        ("groups not on", lambda: L.hm_pileup_fetch_groups(h, 0, N, 1, None, 0), HM_ESTATE, None),
        ("group sample without groups", lambda: L.hm_pileup_group_sample(h, 1), HM_ESTATE, None),
        ("context, flank 4", lambda: L.hm_pileup_fetch_context(h, *n3, 0, 0, N, 1, 4, None, 0), HM_EINVAL, None),
        ("domains, ctx 3", lambda: L.hm_pileup_fetch_domains(h, *n3, 0, 0, N, 3, 100, -100, 10, 1000, None, None, 0), HM_EINVAL, None),
        ("regions, lo > hi", lambda: L.hm_pileup_fetch_regions(h, *n3, 0, 10, 5, 1, None, None, 0, None), HM_EINVAL, None),
    ]


def test_failed_calls_leave_nothing_behind():
    """between the entries of a shuffle: a bad range or argument (HM_EINVAL), a fetch whose option is off on a second engine built
    without options, a load into an engine that staged records (HM_ESTATE), a cap one too small -- each with its code and a
    message, and every entry after it as on a fresh engine"""
    g, reads = S.record_input(0)
    pu, off = _build("rec0"), _new(g)
    S.feed(off, reads)
    off_loci = off.loci().tobytes()
    fresh = _fresh("rec0")
    calls = _failing_calls(pu, off)
    for i, (name, fn) in enumerate(_shuffle("rec0", 60, times=1)):
        what, call, code, word = calls[i % len(calls)]
        assert call() == code, what
        text = pu._L.hm_pileup_last_error(off._h if what.endswith(("off", "without partitions")) else pu._h)
        assert text and (word is None or word in text), (what, text)
        S.cap_short(pu, S.ROW_FETCHES[i % len(S.ROW_FETCHES)])
        assert S.evaluate(fn, pu)[0] == fresh[name][0], "after %s: %s" % (what, name)
    assert i + 1 >= 2 * len(calls) and off.loci().tobytes() == off_loci
    pu.close()
    off.close()


# ---- 6. two engines, one device --------------------------------------------------------------------------------------------------
def test_two_engines_alternate_and_one_is_destroyed_midway():
    half = len(S.CATALOGUE) // 2
    fresh_a, fresh_b = _fresh("rec0"), _fresh("rec1", names=NAMES[:half])
    a, b = _build("rec0"), _build("rec1")
    assert fresh_a["loci"][0] != fresh_b["loci"][0]
    for i, (name, fn) in enumerate(S.CATALOGUE):
        assert S.evaluate(fn, a)[0] == fresh_a[name][0], name
        if i < half:
            assert S.evaluate(fn, b)[0] == fresh_b[name][0], name
        elif i == half:
            b.close()
    a.close()


# ---- 7. an engine without reads, then with them ----------------------------------------------------------------------------------
def test_empty_engine_answers_empty_and_is_then_fed():
    g, reads = S.record_input(0)
    pu = _new(g, **S.RECORD_OPTIONS)
    pu.flush()
    pu.count([128, 128, 128])
    for i, (name, fn) in enumerate(_shuffle("rec0", 70, times=1)):
        if name in ("loci_caller", "asm_caller"):            # the caller's planes are not the engine's: they are not empty
            continue
        _bytes, result = S.evaluate(fn, pu)
        assert result is not None and S.is_empty_form(name, result), "position %d: %s" % (i, name)
    S.feed(pu, reads)                                         # the allocations made on nothing are not trusted afterwards
    fresh = _fresh("rec0")
    for name, fn in S.CATALOGUE:
        assert S.evaluate(fn, pu)[0] == fresh[name][0], name
    pu.close()
