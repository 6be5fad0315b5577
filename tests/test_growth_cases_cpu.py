"""(CPU) What test_gpu_engine_growth.py relies on in its slab ladders (growth_cases.py): the sizes that force or forbid a reallocation, the
site densities that fix the kernel path, the probe reads, the repeat slab's bytes, and that the ladders are the same on every machine."""
import numpy as np
import pytest

import growth_cases as G

QUARTER = 1.25                      # head-room DevBuf::reserve adds to every buffer of the CNN engine (hm_host.h: DevBuf::QUARTER)
THRESH = (0.017, 0.017, 0.033)      # trunk_mask_from_sample: sites per base above which a context takes the dense trunk


def _longest(slab):
    return max(r.l_qseq for r in slab if G.staged(r))


def test_ladder_sizes_follow_the_growth_rules():
    """Staged bases as the engine counts them (reads padded to 4; only reads with all four tags and l_qseq >= 1000) hit the targets; every
    growth step is at least twice the largest slab before it -- in bases, in map rows and in the longest read (the largest read group under
    group_bases = 32768) --, the shrink is below half of it, and the last slab exceeds slab 3 but stays inside a quarter of head-room in
    bases and in rows."""
    lad = G.ladder()
    bases = [G.staged_bases(s) for s in lad]
    rows = [G.map_rows(s) for s in lad]
    assert tuple(bases) == G.LADDER_TARGETS
    by_hand = [sum((r.l_qseq + 3) & ~3 for r in s if r.l_qseq >= 1000 and all(getattr(r, k) is not None and len(getattr(r, k)) == r.l_qseq
                                                                             for k in ("fi", "fp", "ri", "rp"))) for s in lad]
    assert by_hand == bases
    for k in G.GROWTH_STEPS:
        assert bases[k] >= 2 * max(bases[:k]) and rows[k] >= 2 * max(rows[:k]) and _longest(lad[k]) >= 2 * max(_longest(s) for s in lad[:k]), k
    k = G.SHRINK_STEP
    assert 2 * bases[k] <= max(bases[:k]) and 2 * rows[k] <= max(rows[:k])
    k = G.HEADROOM_STEP
    assert max(bases[:k]) < bases[k] <= QUARTER * max(bases[:k]) and rows[k] <= QUARTER * max(rows[:k])
    assert sum(r.l_qseq for r in lad[k] if G.staged(r)) > max(sum(r.l_qseq for r in s if G.staged(r)) for s in lad[:k])   # the split tail's slice grows
    assert _longest(lad[k]) <= _longest(lad[3])
    assert any(not G.staged(r) for s in lad for r in s)      # staged_bases() had something to leave out


def test_ladder_holds_the_reads_the_issue_names():
    lad = G.ladder()
    names = [[r.name for r in s] for s in lad]
    L = [[r.l_qseq for r in s if G.staged(r)] for s in lad]
    assert 1000 in L[0] and 1001 in L[0] and any(r.flag & 16 for r in lad[0])
    assert "polyC" in names[1] and "CGrepeat" in names[1]
    assert max(L[2]) >= 70000
    assert sum(1 for x in L[3] if x == 1000) >= 60
    wide = sum(1 for s in lad for r in s if G.staged(r) and r.fi.dtype.itemsize == 2)
    missing = sum(1 for s in lad for r in s if r.l_qseq >= 1000 and not r.has_kinetics())
    short = sum(1 for s in lad for r in s if r.l_qseq < 1000)
    assert wide >= 10 and missing >= 2 and short >= 1, (wide, missing, short)


@pytest.mark.parametrize("which", ["ladder", "ladder_sparse"])
def test_probe_reads_open_and_close_every_slab(which):
    for s in getattr(G, which)():
        for rd in (s[0], s[-1]):
            assert rd.name == "probe" and G.staged(rd) and 1000 <= rd.l_qseq <= 3000
        assert len(s) >= 3


def test_every_slab_is_far_above_the_auto_trunk_thresholds():
    """Per slab and context: a direct count of the sites is at least 1.5 x the threshold, and the engine's own host-side rule
    (hm_trunk_mask_for_reads) says 7 for every slab of LADDER and 4 or 0 -- never CpG or CHG -- for LADDER_SPARSE."""
    from hifimeth_amd.caller import ReadBlock, trunk_mask_for_reads
    for k, s in enumerate(G.ladder() + [G.lead_slab(), G.repeat_unit()]):
        cnt, bases = G.site_counts(s)
        for c in range(3):
            assert cnt[c] >= 1.5 * THRESH[c] * bases, (k, c, cnt, bases)
        assert trunk_mask_for_reads(ReadBlock(s), 7) == 7, k
        assert trunk_mask_for_reads(ReadBlock([r for r in s if G.staged(r)]), 7) == 7, k
    for k, s in enumerate(G.ladder_sparse()):
        cnt, bases = G.site_counts(s)
        assert cnt[0] <= 0.5 * THRESH[0] * bases and cnt[1] <= 0.5 * THRESH[1] * bases, (k, cnt, bases)
        assert trunk_mask_for_reads(ReadBlock(s), 7) & 3 == 0, k


def test_direct_site_count_on_hand_made_sequences():
    from hifimeth_amd.synth import read_from_ascii
    kin = [np.zeros(1000, np.uint8)] * 4
    mk = lambda unit: [read_from_ascii((unit * 1000)[:1000], *kin)]
    assert G.site_counts(mk(b"CG"))[0].tolist() == [500, 0, 0]
    assert G.site_counts(mk(b"C"))[0].tolist() == [0, 0, 998]
    assert G.site_counts(mk(b"G"))[0].tolist() == [0, 0, 998]
    assert G.site_counts(mk(b"CAG"))[0].tolist() == [0, 333, 0]        # C A G: CHG forward; G, then A, C leftwards: C is no D
    assert G.site_counts(mk(b"CAAGTT"))[0].tolist() == [0, 0, 167 + 167]   # C A A forward; G, A, A read leftwards from 3, 9, ..., 999


def test_sparse_ladder_moves_the_launch_window():
    """LADDER_SPARSE: 8 k, 60 k, 4.2 M, 10 k staged bases.  Only the top slab leaves the default window (bases / 48 > 65536), and by enough
    that d_act4 -- sized min(bases, window) sites with a quarter of head-room -- must reallocate at both growth steps; with the default
    window the top slab would take more than 48 launch pairs per context, with its own window it takes 48."""
    bases = [G.staged_bases(s) for s in G.ladder_sparse()]
    assert tuple(bases) == G.SPARSE_TARGETS
    win = [G.launch_window(b) for b in bases]
    assert win[0] == win[1] == win[3] == G.DEFAULT_WINDOW and win[2] == (bases[2] // 48 + 8) // 8 * 8 > G.DEFAULT_WINDOW
    act4 = [min(b, w) for b, w in zip(bases, win)]
    for k in G.SPARSE_GROWTH_STEPS:
        assert bases[k] >= 2 * max(bases[:k]) and act4[k] > QUARTER * max(act4[:k]) + 1, k
    assert G.launch_pairs(bases[2]) == 48 < -(-bases[2] // G.DEFAULT_WINDOW)
    assert [G.launch_pairs(b) for b in (bases[0], bases[1], bases[3])] == [1, 1, 1]


def test_repeat_slab_outgrows_the_pinned_slab_floor():
    unit, slab = G.repeat_unit(), G.repeat_slab()
    assert 18 <= len(unit) <= 22 and len(slab) == G.REPEAT_COUNT * len(unit) and slab[len(unit)] is slab[0]
    assert G.raw_bytes(slab) == G.REPEAT_COUNT * G.raw_bytes(unit) > G.SLAB_FLOOR
    assert G.raw_bytes(G.repeat_slab(G.REPEAT_COUNT - 2)) < G.SLAB_FLOOR < G.raw_bytes(slab)      # no larger than it has to be
    lead = G.lead_slab()
    assert G.staged_bases(lead) == 20_000 and G.raw_bytes(lead) < G.SLAB_FLOOR // 100
    assert G.staged_bases(slab) >= 100 * G.staged_bases(lead)       # every per-slot array regrows behind the lead slab
    assert any(not G.staged(r) for r in unit)


def test_ladders_are_deterministic():
    for make, cached in ((G.make_ladder, G.ladder), (G.make_ladder_sparse, G.ladder_sparse)):
        a, b = make(), cached()
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert len(x) == len(y) and G.slab_bytes(x) == G.slab_bytes(y)
    assert G.slab_bytes(G.repeat_unit()) == G.slab_bytes(G.repeat_unit()) and G.slab_bytes(G.lead_slab()) == G.slab_bytes(G.lead_slab())
