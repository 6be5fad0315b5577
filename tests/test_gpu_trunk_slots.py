"""The sliding-window trunk's copy-slot tiers (hm_trunk3.hip): a step stores, per layer, only as many list entries of E1 / E2 / E3
rows as its record says are needed -- 16, 32, 48 or all 112.  `slot_counts` mirrors rowlist3_kernel's flag rule on the CPU; the GPU tests
build reads whose steps sit on the tier boundaries (checked through the mirror) and compare the calls of trunk_impl = 3 with the
streaming trunk's (trunk_impl = 1, every row stored) byte for byte, and with the CPU oracle within 1e-4."""
import numpy as np
import pytest

TR_OWN, TR_PAD = 112, 200
SHIFT = (28, 24, 16)          # first new row of E1 / E2 / E3 relative to a step's u
LEFT = -199
# EdgeGeo<K1>: first shared row of the right chain per layer, its step, and whether the chain's last tap is padding (then one row)
GEO = {11: dict(R=(189, 185, 169), PAD=(True, True, False)), 13: dict(R=(185, 177, 169), PAD=(False, False, True))}
STEP = (2, 4, 8)
TIERS = (16, 32, 48)          # list entries the short tiers cover (hm_trunk3.hip: T3_TIER x 8)


def slot_counts(site_pos, L, k1):
    """site_pos: view positions of the sites of one context and strand view of a read of length L.  Returns (u, count, need, computed):
    per tile step (u = -200 + 112 t) and layer the number of flagged new rows, the number of list entries that must be stored (the
    flagged rows, plus the fill row -- the last new row -- unless it is flagged itself), and whether the step is computed (the first
    tile and the tiles behind the read's end are constant steps, which never take a tier)."""
    g = GEO[k1]
    site = np.zeros(L + 2048, bool)     # view positions -1024 .. L + 1024
    sp = np.asarray(site_pos, np.int64)
    assert ((sp >= 0) & (sp < L)).all()
    site[sp + 1024] = True
    sat = lambda y: site[y + 1024]
    ntile = (L + 2 * TR_PAD + TR_OWN - 1) // TR_OWN
    u = -TR_PAD + TR_OWN * np.arange(ntile)
    count = np.zeros((ntile, 3), int)
    need = np.zeros((ntile, 3), int)
    rows = np.arange(TR_OWN)
    for t in range(ntile):
        for l in range(3):
            x = u[t] + SHIFT[l] + rows
            f = sat(x - LEFT) | sat(x - g["R"][l])
            if not g["PAD"][l]:
                f = f | sat(x - g["R"][l] - STEP[l])
            count[t, l] = f.sum()
            need[t, l] = f.sum() + (0 if f[-1] else 1)
    computed = (u != -TR_PAD) & (u < L)
    return u, count, need, computed


def tier_of(need):
    return int(np.searchsorted(TIERS, need))     # the first tier that covers `need` entries; len(TIERS): all 112


# ---- the mirror against hand-worked cases (CPU) ----

def test_mirror_single_site_k11():
    # one site at y = 1000, K1 = 11: left row x = 801 in every layer; right rows E1 1189, E2 1185, E3 1169 and 1177.
    # x lies in step t's window [u + shift, u + shift + 112), u = -200 + 112 t: 801 -> t = 8 (u = 696) for all three shifts;
    # 1189 / 1185 / 1169, 1177 -> t = 12 (u = 1144: windows [1172, 1284), [1168, 1280), [1160, 1272))
    u, count, need, computed = slot_counts([1000], 2000, 11)
    want = np.zeros_like(count)
    want[8] = (1, 1, 1)
    want[12] = (1, 1, 2)
    assert (count == want).all()
    assert (need == want + 1).all()            # the last new row is flagged nowhere: one fill entry everywhere
    assert len(u) == 22 and not computed[0] and computed[1:20].all() and not computed[20:].any()   # u = 2040 >= 2000 from t = 20


def test_mirror_last_row_and_second_right_row_k13():
    # K1 = 13, site at y = 698: its left row x = 499 is row 111 of E1's window of step t = 5 (u = 360: [388, 500)) -- the fill row
    # itself, so nothing is added to `need`; in E2 / E3 (windows [384, 496), [376, 488)) it belongs to step 6 (rows 3 and 11).
    # Right rows: E1 883, 885; E2 875, 879; E3 867 (one row: PAD4) -> step 9 (u = 808: [836, 948), [832, 944), [824, 936))
    u, count, need, _ = slot_counts([698], 1500, 13)
    assert tuple(count[5]) == (1, 0, 0) and tuple(need[5]) == (1, 1, 1)
    assert tuple(count[6]) == (0, 1, 1) and tuple(need[6]) == (1, 2, 2)
    assert tuple(count[9]) == (2, 2, 1) and tuple(need[9]) == (3, 3, 2)
    assert count.sum() == 8


def test_mirror_every_position_a_site():
    _, count, need, computed = slot_counts(np.arange(1200), 1200, 13)
    inner = slice(4, 8)       # windows [u + 16, u + 140) with every source position x + 199, x - 185 - 2 ... inside the read
    assert (count[inner] == TR_OWN).all() and (need[inner] == TR_OWN).all()
    assert [tier_of(n) for n in (0, 16, 17, 32, 33, 48, 49, 112)] == [0, 0, 1, 1, 2, 2, 3, 3]


# ---- reads whose steps sit where the tiers change ----

def _kin(L, rng):
    return [np.clip(np.rint(rng.gamma(2.0, 12.0, L)), 0, 255).astype(np.uint8) for _ in range(4)]


def _chh_read(L, clusters, rng, extra=()):
    """A read of A's with C's at chosen positions: every C followed by two non-G bases is a CHH site of the forward view, and there is
    no other site of any context.  clusters: (t, rows) -> C's at the positions whose LEFT rows are those new E1 rows of step t."""
    from hifimeth_amd.synth import read_from_ascii
    seq = np.full(L, ord("A"), np.uint8)
    for t, rows in clusters:
        y = -TR_PAD + TR_OWN * t + SHIFT[0] - LEFT + np.asarray(rows)
        assert y.min() >= 0 and y.max() < L - 2
        seq[y] = ord("C")
    for y in extra:
        assert 0 <= y < L - 2
        seq[y] = ord("C")
    return read_from_ascii(seq.tobytes(), *_kin(L, rng)), np.nonzero(seq[:L - 2] == ord("C"))[0]


def _cpg_read(L, positions, rng):
    """A read of A / T with CG at chosen positions: CpG sites of the forward view at the C's (and of the reverse view at the G's)."""
    from hifimeth_amd.synth import read_from_ascii
    seq = np.frombuffer(bytes(rng.choice(np.frombuffer(b"AT", np.uint8), L)), np.uint8).copy()
    for y in positions:
        seq[y], seq[y + 1] = ord("C"), ord("G")
    fwd = np.nonzero((seq[:-1] == ord("C")) & (seq[1:] == ord("G")))[0]
    return read_from_ascii(seq.tobytes(), *_kin(L, rng)), fwd, L - 1 - (fwd + 1)


def _boundary_reads():
    """CHH (K1 = 13) reads with runs of n sites whose left rows are the first n new rows of one step: (n, n, n) flagged rows there,
    n + 1 entries to store; n around every tier boundary.  Returns reads and, per read, the mirror's result for the forward CHH view."""
    rng = np.random.default_rng(2024)
    reads, info = [], []
    for L, ns in ((2400, (14, 15, 16, 17)), (2400, (30, 31, 32, 33)), (2300, (46, 47, 48, 49)), (1500, (1, 0, 31, 47))):
        rd, sites = _chh_read(L, [(t + 1, np.arange(n)) for t, n in enumerate(ns) if n], rng)
        reads.append(rd)
        info.append(slot_counts(sites, L, 13))
    # the last new row flagged itself, next to short-tier steps
    rd, sites = _chh_read(1800, [(2, [111]), (3, list(range(15)) + [111]), (4, list(range(47)) + [111])], rng)
    reads.append(rd)
    info.append(slot_counts(sites, 1800, 13))
    return reads, info


THREE_TIER_STEP = 6


def _three_tier_read():
    """A CHH read with one step (t = 6, u = 472) whose three layers take three different tiers.  Eleven sites 6 apart at
    y = u - 140 + 6 k flag, through the right chain, 22 / 22 / 11 rows of E1 / E2 / E3 (x + 185, x + 187; x + 177, x + 181; x + 169: no
    two coincide).  Twelve consecutive sites at y = u + 327 .. u + 338 have their left rows at x = u + 128 .. u + 139: all twelve in
    E1's window [u + 28, u + 140) -- the last new row among them --, eight in E2's [u + 24, u + 136), none in E3's [u + 16, u + 128).
    34 / 30 / 11 flagged rows, 34 / 30 / 12 entries to store: the 48-, the 32- and the 16-entry tier in one step."""
    L, u = 2400, -TR_PAD + TR_OWN * THREE_TIER_STEP
    rng = np.random.default_rng(12)
    rd, sites = _chh_read(L, [], rng, extra=[u - 140 + 6 * k for k in range(11)] + list(range(u + 327, u + 339)))
    return rd, slot_counts(sites, L, 13)


def _two_tier_read():
    """CHH sites every fourth position: the right chain flags two E1 rows per site (x + 185, x + 187: every second row, 56 of 112) but
    E2 rows that coincide with the neighbour's (x + 177, x + 181) and one E3 row: 28 each -- E1 on all 112 entries, E2 and E3 in the
    32-entry tier of the same step."""
    from hifimeth_amd.synth import read_from_ascii
    rng = np.random.default_rng(11)
    L = 1900
    seq = np.full(L, ord("A"), np.uint8)
    seq[0:L - 2:4] = ord("C")
    return read_from_ascii(seq.tobytes(), *_kin(L, rng)), slot_counts(np.arange(0, L - 2, 4), L, 13)


def _assert_three_tier_step(res):
    u, count, need, computed = res
    t = THREE_TIER_STEP
    assert computed[t] and tuple(count[t]) == (34, 30, 11) and tuple(need[t]) == (34, 30, 12)
    assert [tier_of(n) for n in need[t]] == [2, 1, 0]


def _covered(info):
    counts, needs = set(), set()
    for _u, count, need, computed in info:
        counts |= set(count[computed].ravel().tolist())
        needs |= set(need[computed].ravel().tolist())
    return counts, needs


def test_boundary_reads_reach_the_required_counts():
    """(CPU) what the GPU tests below rely on: their reads reach 0 and 1 flagged rows, R - 1, R, R + 1 for every short tier -- as
    flagged rows and as entries to store --, a flagged last row, and a step whose three layers take three different tiers."""
    _reads, info = _boundary_reads()
    counts, needs = _covered(info)
    for R in TIERS:
        assert {R - 1, R, R + 1} <= counts and {R - 1, R, R + 1} <= needs, (R, sorted(counts), sorted(needs))
    assert {0, 1} <= counts
    u, count, need, computed = info[4]
    assert any((need[t] == count[t]).any() and (count[t] > 0).all() for t in np.nonzero(computed)[0])   # last new row flagged
    _assert_three_tier_step(_three_tier_read()[1])
    _rd, (u, count, need, computed) = _two_tier_read()
    assert any(computed[t] and [tier_of(n) for n in need[t]] == [3, 1, 1] for t in range(len(u)))


def _poly_c(L, rng):
    from hifimeth_amd.synth import read_from_ascii
    return read_from_ascii(b"C" * L, *_kin(L, rng))


def _calls(impl, reads, num_cu=0, group_bases=0):
    """The calls of `reads` from a fresh engine that has run an unrelated batch first: the maps are never cleared, so a row that this
    run fails to store holds the other batch's bytes (or another engine's), not by chance the right ones of an earlier run on the same reads."""
    from hifimeth_amd import MethylationCaller
    from hifimeth_amd.synth import synth_reads
    with MethylationCaller(device=0) as m:
        m.set_option("trunk", 1)
        m.set_option("trunk_impl", impl)
        if num_cu:
            m.set_option("num_cu", num_cu)
        if group_bases:
            m.set_option("group_bases", group_bases)
        m.call(synth_reads(len(reads), seed=404, median_len=2400, sigma=0.05, frac_short=0, frac_missing=0))
        return m.call(reads).copy()


def _same(a, b):
    return len(a) == len(b) and all(a[k].tobytes() == b[k].tobytes() for k in ("qoff", "strand", "ctx", "p", "scaled_prob"))


@pytest.fixture(scope="module")
def slot_reads():
    rng = np.random.default_rng(7)
    reads, info = _boundary_reads()
    reads.append(_three_tier_read()[0])
    reads.append(_two_tier_read()[0])
    reads.append(_poly_c(1300, rng))                                   # every position a CHH site: 112 flagged rows
    cpg, fwd, rev = _cpg_read(2000, list(range(300, 364, 2)) + [900, 1500], rng)   # K1 = 11: a run of 32 CpGs, two lone ones
    reads.append(cpg)
    return reads, info, (fwd, rev)


@pytest.fixture(scope="module")
def slot_runs(slot_reads):
    """trunk_impl 3 FIRST, then the reference (trunk_impl 1): nothing of the reference run can be left in memory for the tiered run."""
    got = _calls(3, slot_reads[0])
    return got, _calls(1, slot_reads[0])


@pytest.fixture(scope="module")
def slot_ref(slot_runs):
    return slot_runs[1]


@pytest.mark.gpu
def test_tiered_copy_slots_give_the_streaming_trunks_calls(slot_reads, slot_runs):
    """Steps with 0, 1, R - 1, R, R + 1 (R = 16, 32, 48) and 112 flagged rows, a flagged last row, a step whose three layers take three different tiers, K1 = 11
    and 13, each read's first tile and the constant tiles behind its end beside short-tier steps: byte-identical calls."""
    reads, info, (fwd, rev) = slot_reads
    counts, needs = _covered(info)
    for R in TIERS:
        assert {R - 1, R, R + 1} <= counts and {R - 1, R, R + 1} <= needs
    _u, c11, n11, comp11 = slot_counts(fwd, 2000, 11)
    assert {0, 1} <= set(c11[comp11].ravel().tolist()) and TIERS[0] < n11[comp11].max() <= TIERS[2]   # K1 = 11 in the short tiers
    _u, cp, _np, compp = slot_counts(np.arange(1300), 1300, 13)
    assert (cp[compp] == TR_OWN).any()
    _assert_three_tier_step(_three_tier_read()[1])
    got, ref = slot_runs
    assert len(ref) > 1000 and _same(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("num_cu,group_bases", [(1, 0), (5, 0), (1024, 4096)])
def test_tiered_copy_slots_whatever_the_runs_of_tiles(slot_reads, slot_ref, num_cu, group_bases):
    """Workgroup boundaries inside the reads (1, 5 workgroups; more workgroups than tiles and one read per group): a run's first step is
    a warm-up step on the all-fill record (count 0), the steps behind it take their own tiers."""
    assert _same(_calls(3, slot_reads[0], num_cu, group_bases), slot_ref)


@pytest.mark.gpu
def test_tiered_copy_slots_against_the_oracle(slot_reads, oracle, oracle_models):
    from test_gpu_parity import _check_calls
    reads = slot_reads[0]
    n, _nml, worst = _check_calls(_calls(3, reads), reads, oracle, oracle_models, 7)
    assert n > 1000 and worst <= 1e-4
