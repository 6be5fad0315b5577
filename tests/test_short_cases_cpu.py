"""The short-read sets of tests/short_cases.py hold what tests/test_gpu_short_reads.py needs, and the bar that test applies sees the
failure it is there for -- on the CPU, in seconds.

The failure: a trunk step or a padding tap that takes a ZERO row where the network's row outside the read is bn0(0) (a constant step
storing zeros, a kept row that is not the constant one, a list entry one tile off).  CNN64(zero_outside=True) computes exactly that
network; on the ladder its error against the true fp64 network must exceed the bar 8 x max(E_oracle, 1e-6) in every context."""
import os

import numpy as np

import short_cases as S
from cnn64 import ALL_STRATA, CNN64, STRATA, bar, reference_sites, site_errors, strata, stratum_of
from conftest import WEIGHTS

NAMES = ("CpG", "CHG", "CHH")


def test_the_ladder_holds_every_length_class():
    reads = S.ladder()
    lengths = [r.l_qseq for r in reads]
    for L in S.LADDER_LENGTHS:
        assert L in lengths, L
    assert set(S.LADDER_LENGTHS) >= {1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 24, 25, 136, 137, 248, 249, 48, 49, 160, 161, 272, 273, 169, 170, 177,
                                     178, 185, 186, 189, 190, 199, 200, 201, 215, 216, 400, 401, 402, 999}
    assert max(lengths) < 1000 and sum(lengths) <= 13000
    rev = np.mean([bool(r.flag & 16) for r in reads])
    wide = np.mean([r.fi.dtype.itemsize == 2 for r in reads])
    assert 0.4 <= rev <= 0.6 and 0.25 <= wide <= 0.42, (rev, wide)
    by_name = {}
    for r in reads:
        by_name.setdefault(r.name.split("_")[0], []).append(r)
    for tag in ("polyC", "polyG", "CG", "CCA"):
        assert sorted(r.l_qseq for r in by_name[tag]) == list(S.DENSE_LENGTHS)
    assert sorted(r.l_qseq for r in by_name["free"]) == list(S.SITE_FREE_LENGTHS)
    assert all(set(r.ascii()) <= set(b"ATN") for r in by_name["free"])
    gc = np.mean([c in b"CG" for r in by_name["rnd"] for c in r.ascii()])
    assert 0.45 < gc < 0.55, gc


def test_the_plan_at_every_boundary():
    for L, (tiles, const) in S.PLAN.items():
        assert S.plan(L)[:2] == (tiles, const), (L, S.plan(L))
        assert S.plan(L)[2] == tiles * 112 + 32
    # the pairs differ in what they are there for
    for a, b in S.LAST_TILE_CONSTANT:
        assert S.plan(a)[0] == S.plan(b)[0] and S.plan(a)[1] == S.plan(b)[1] + 1
    for a, b in S.TILE_COUNT_STEPS:
        assert S.plan(a)[0] + 1 == S.plan(b)[0]
    # reads of 1 .. 24 bases: one computed step between three constant ones; up to 248 bases at least half of the tiles are constant
    assert all(S.plan(L)[:2] == (4, 3) for L in range(1, 25))
    assert all(2 * S.plan(L)[1] >= S.plan(L)[0] for L in range(1, 137)) and all(S.plan(L)[1] >= 2 for L in range(1, 1000))
    # groups: closed on rows, one read per group at group_bases 1, nothing lost
    lens = [r.l_qseq for r in S.crowd()]
    for gb in (1, 4096, 8192, 1 << 30):
        cuts = S.groups(lens, gb)
        assert cuts[0][0] == 0 and cuts[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        rows = [sum(S.plan(L)[2] for L in lens[lo:hi]) for lo, hi in cuts]
        assert all(r >= gb for r in rows[:-1]) and all(r - S.plan(lens[hi - 1])[2] < gb for r, (lo, hi) in zip(rows, cuts))
    assert len(S.groups(lens, 1)) == len(lens) and len(S.groups(lens, 1 << 30)) == 1


def test_the_sets_populate_their_strata(oracle):
    for name, make in S.SETS.items():
        reads = make()
        ref = reference_sites(oracle, reads, {}, min_len=1)
        for c in range(3):
            sizes = {k: int(m.sum()) for k, m in strata(ref[c], c, ALL_STRATA).items()}
            print(name, NAMES[c], len(ref[c]["qoff"]), sizes)
            need = strata(ref[c], c, S.REQUIRED_STRATA[name])
            assert len(need) == len(S.REQUIRED_STRATA[name]) * (2 if c == 2 else 1)
            assert all(m.sum() > 0 for m in need.values()), (name, NAMES[c], sizes)       # CHH: on both strands
            if name == "crowd":
                assert sum(sizes.values()) == sizes.get("both", 0) + sizes.get("both/fwd", 0) + sizes.get("both/rev", 0)
            L = np.array([reads[i].l_qseq for i in ref[c]["rid"]])
            both = (ref[c]["qoff"] < 200) & (ref[c]["qoff"] >= L - 200)
            assert np.array_equal(both, ref[c]["stratum"] == 3) and both.sum() > 0
    n_ladder = sum(len(s["qoff"]) for s in reference_sites(oracle, S.ladder(), {}, min_len=1))
    assert 2000 < n_ladder < 8000, n_ladder


def test_the_three_old_strata_are_unchanged_for_reads_of_401_bases_and_more():
    rng = np.random.default_rng(4)
    for L in (401, 402, 600, 999, 1000, 1025, 70001):
        offs = np.unique(np.concatenate([np.arange(min(L, 450)), np.arange(max(0, L - 450), L), rng.integers(0, L, 500)]))
        old = np.where(offs < 200, 0, np.where(offs >= L - 200, 2, 1)).astype(np.int8)
        new = stratum_of(offs, L)
        assert new.dtype == old.dtype and np.array_equal(new, old), L
    assert (stratum_of(np.arange(399), 399) == 3).sum() == 1 and (stratum_of(np.arange(400), 400) == 3).sum() == 0
    assert (stratum_of(np.arange(200), 200) == 3).all()
    # and strata() without names gives the three masks it always gave
    site = {"stratum": np.array([0, 1, 2, 3, 1], np.int8), "strand": np.array([0, 1, 0, 1, 0], np.uint8)}
    assert list(strata(site, 0)) == list(STRATA) and [m.tolist() for m in strata(site, 0).values()] == \
        [[True, False, False, False, False], [False, True, False, False, True], [False, False, True, False, False]]
    assert list(strata(site, 2)) == [f"{n}/{s}" for n in STRATA for s in ("fwd", "rev")]
    assert strata(site, 2, ("both",))["both/rev"].tolist() == [False, False, False, True, False]


def test_the_crowd_is_rows_not_bases(oracle):
    reads = S.crowd()
    assert len(reads) == 1500 and {r.l_qseq for r in reads} == set(range(1, 65))
    lens = [r.l_qseq for r in reads]
    rows = sum(S.plan(L)[2] for L in lens)
    assert rows / sum(lens) > 10, rows / sum(lens)
    free = [i for i, r in enumerate(reads) if set(r.ascii()) <= set(b"ATN")]
    assert 1 / 8 < len(free) / len(reads) < 1 / 6
    assert 0.4 < np.mean([bool(r.flag & 16) for r in reads]) < 0.6 and 0.25 < np.mean([r.fi.dtype.itemsize == 2 for r in reads]) < 0.42
    cuts = S.groups(lens, 8192)
    assert len(cuts) > 50
    ref = reference_sites(oracle, reads, {}, min_len=1)
    for c in range(3):
        per_group = [int(((ref[c]["rid"] >= lo) & (ref[c]["rid"] < hi)).sum()) for lo, hi in cuts]
        print(NAMES[c], "groups:", len(cuts), "without a site:", sum(n == 0 for n in per_group))
        inner = per_group[1:-1]
        if c < 2:      # an empty launch between groups that do hold sites
            k = per_group.index(0)
            assert 0 < k < len(cuts) - 1 and max(per_group[:k]) > 0 and max(per_group[k + 1:]) > 0, (NAMES[c], per_group)
        else:
            assert min(inner) > 0
    # at one read per group every context has hundreds of groups without a site among groups with sites
    for c in range(3):
        assert 200 < len(reads) - len(np.unique(ref[c]["rid"])) < len(reads) - 200


def test_the_sandwich_alternates(oracle):
    reads = S.sandwich()
    half = len(reads) // 2
    assert len(reads) == 2 * half and all(a is b for a, b in zip(reads[:half], reads[half:][::-1]))
    assert [r.l_qseq for r in reads[1:half:2]] == list(S.SANDWICH_SHORT)
    assert all(2000 <= r.l_qseq <= 3000 for r in reads[0:half:2])


def test_the_bar_sees_a_zero_row_outside_the_read(oracle, oracle_models):
    f64 = [CNN64(os.path.join(WEIGHTS, n + ".hmw")) for n in NAMES]
    zero = [CNN64(os.path.join(WEIGHTS, n + ".hmw"), zero_outside=True) for n in NAMES]
    ref = reference_sites(oracle, S.ladder(), {"o32": oracle_models, "f64": f64, "zero": zero}, min_len=1)
    for c, name in enumerate(NAMES):
        s = ref[c]
        e_o = float(site_errors(s["o32"], s["f64"]).max())
        e_z = site_errors(s["zero"], s["f64"])
        b = bar(e_o)
        by = {k: float(e_z[m].max(initial=0.0)) for k, m in strata(s, c, ALL_STRATA).items()}
        print(f"{name}: n={len(s['qoff'])} E_oracle={e_o:.2e} bar={b:.2e} E_zero_rows={e_z.max():.2e} ({e_z.max() / b:.0f} x the bar) " +
              " ".join(f"{k}={v / b:.0f}x" for k, v in by.items()))
        assert e_z.max() > b, (name, float(e_z.max()), b)
        # every stratum whose windows hang over an end sees it; a window in the middle of a read has no row outside
        for k, v in by.items():
            if not k.startswith("middle"):
                assert v > b, (name, k, v, b)
        mid = s["stratum"] == 1
        assert mid.sum() > 0 and float(e_z[mid].max()) == 0.0
