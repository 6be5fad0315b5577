"""Reads shorter than the CNN's window (401) and than a trunk tile (112), for tests/test_gpu_short_reads.py and
tests/test_short_cases_cpu.py: a plain module like scan_cases.py and bigmaps_cases.py.  Front ends take such reads with -l; every
other value test of the CNN kernels stages reads of 1000 bases and more.

The tile plan of a read, restated in numpy (add_read_tiles in hm_engine.cpp, trunk3_kernel's constant-step rule in hm_trunk3.hip):
    tiles of a read      ceil((L + 400) / 112), tile t at view position u0 = -200 + 112 t
    constant tiles       u0 == -200 or u0 >= L: no receptive field of a new row reaches the read
    map rows of a read   tiles * 112 + 32
    groups               a read opens a new group once the current group's rows have reached group_bases
Read sets (seeded generators, stable names; results are cached: the lists are shared and must not be modified):
    ladder()     one or two reads at every length where something changes (LADDER_LENGTHS), dense homopolymers and repeats, site-free reads
    crowd(n)     reads of 1 .. 64 bases: ~15 map rows per base, dozens of reads per equal-cost run, stretches without G / without C
    sandwich()   2 - 3 kb reads with the shortest ladder lengths between them, then the same list backwards
    zero_length_read()   l_qseq = 0 with four empty kinetics arrays
"""
import functools

import numpy as np

from hifimeth_amd.synth import Read, read_from_ascii

TR_OWN, TR_PAD, TR_SLACK = 112, 200, 32        # hm_device.h

# what changes at each length (L: the first length on the far side)
SITE_AND_TAP_EDGES = (1, 2, 3, 4, 5, 10, 11, 12, 13, 14)      # the motifs' 2 and 3 bases; conv1's K1 = 11 / 13 taps
LAST_TILE_CONSTANT = ((24, 25), (136, 137), (248, 249))       # u0 = 24 / 136 / 248 >= L, or computed
TILE_COUNT_STEPS = ((48, 49), (160, 161), (272, 273))         # L + 400 passes a multiple of 112
RIGHT_CHAIN_ROWS = (169, 170, 177, 178, 185, 186, 189, 190)   # off + 169 / 177 / 185 / 189: the right edge chains' first rows
WINDOW_OVERHANG = (199, 200, 201, 215, 216, 400, 401, 402)    # the window hangs over one end or both; E4's first gather row off - 199
BELOW_THE_FLOOR = (999,)                                      # one short of every other suite's shortest read
LADDER_LENGTHS = (SITE_AND_TAP_EDGES + tuple(L for p in LAST_TILE_CONSTANT + TILE_COUNT_STEPS for L in p) + RIGHT_CHAIN_ROWS +
                  WINDOW_OVERHANG + BELOW_THE_FLOOR)
DENSE_LENGTHS = (13, 25, 137)                 # poly-C, poly-G, CG and CCA repeats
SITE_FREE_LENGTHS = (1, 30, 200)              # A / T / N only
SANDWICH_SHORT = (1, 13, 24, 25, 49, 137, 201)
# plan(L) -> (tiles, constant tiles), written out
PLAN = {24: (4, 3), 25: (4, 2), 136: (5, 3), 137: (5, 2), 248: (6, 3), 249: (6, 2), 48: (4, 2), 49: (5, 3), 160: (5, 2), 161: (6, 3),
        272: (6, 2), 273: (7, 3), 1: (4, 3), 999: (13, 3)}

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def plan(L: int):
    """(tiles, constant tiles, map rows) of a read of L bases"""
    tiles = -(-(L + 2 * TR_PAD) // TR_OWN)
    u0 = -TR_PAD + TR_OWN * np.arange(tiles)
    return tiles, int(((u0 == -TR_PAD) | (u0 >= L)).sum()), tiles * TR_OWN + TR_SLACK


def groups(lengths, group_bases: int):
    """[(first read, one past the last)] of the read groups: a group is closed once its map rows reach group_bases"""
    cuts, lo, rows = [], 0, 0
    for i, L in enumerate(lengths):
        if i > lo and rows >= group_bases:
            cuts.append((lo, i))
            lo, rows = i, 0
        rows += plan(int(L))[2]
    if len(lengths) > lo:
        cuts.append((lo, len(lengths)))
    return cuts


def _kin(rng, L, wide):
    if wide:
        return [np.clip(np.rint(rng.gamma(2.0, 30.0, L)), 0, 2000).astype(np.uint16) for _ in range(4)]
    return [np.clip(np.rint(rng.gamma(2.0, 12.0, L)), 0, 255).astype(np.uint8) for _ in range(4)]


def _random(rng, L, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), L)].tobytes()


def _site_free(rng, L):
    return _random(rng, L, b"ATATN")


@functools.lru_cache(maxsize=None)
def ladder():
    """-> reads.  Two reads per length up to 250 bases (one stored forward, one with flag 16), one above; every third read carries u16
    kinetics; random sequence at GC 0.5."""
    rng = np.random.default_rng(20250601)
    reads = []

    def add(seq, tag):
        i = len(reads)
        reads.append(read_from_ascii(seq, *_kin(rng, len(seq), wide=(i % 3 == 1)), flag=16 if i % 2 else 4, name=f"{tag}_{len(seq)}_{i}"))

    for L in LADDER_LENGTHS:
        for _ in range(2 if L <= 250 else 1):
            add(_random(rng, L), "rnd")
    for L in DENSE_LENGTHS:
        for tag, unit in (("polyC", b"C"), ("polyG", b"G"), ("CG", b"CG"), ("CCA", b"CCA")):
            add((unit * L)[:L], tag)
    for L in SITE_FREE_LENGTHS:
        add(_site_free(rng, L), "free")
    assert all(r.l_qseq < 1000 for r in reads) and sum(r.l_qseq for r in reads) < 13000
    return reads


@functools.lru_cache(maxsize=None)
def crowd(n: int = 1500):
    """-> reads of 1 .. 64 bases.  Lengths step by 37 mod 64: neighbours differ, every length occurs.  Every seventh read is site-free;
    reads 400 .. 449 hold no G (no CpG, no CHG, no reverse-strand site) and reads 800 .. 849 no C (reverse-strand CHH only), so that
    whole read groups of a few thousand map rows lack a context between groups that hold it."""
    rng = np.random.default_rng(20250602)
    reads = []
    for i in range(n):
        L = 1 + (37 * i) % 64
        if i % 7 == 3:
            seq, tag = _site_free(rng, L), "free"
        elif 400 <= i < 450:
            seq, tag = _random(rng, L, b"ACCT"), "noG"
        elif 800 <= i < 850:
            seq, tag = _random(rng, L, b"AGGT"), "noC"
        else:
            seq, tag = _random(rng, L), "rnd"
        reads.append(read_from_ascii(seq, *_kin(rng, L, wide=(i % 3 == 0)), flag=16 if i % 2 else 4, name=f"{tag}_{L}_{i}"))
    assert all(a.l_qseq != b.l_qseq for a, b in zip(reads, reads[1:]))
    return reads


@functools.lru_cache(maxsize=None)
def sandwich():
    """-> reads: long, short, long, short, ... long with SANDWICH_SHORT between reads of 2 - 3 kb, then the same reads in reverse order
    (a short read now follows the long read it preceded).  Kept rows of a long read must not reach a short one, nor the other way round."""
    rng = np.random.default_rng(20250603)
    one = []
    for i, L in enumerate(SANDWICH_SHORT):
        long_len = int(rng.integers(2000, 3001))
        one.append(read_from_ascii(_random(rng, long_len), *_kin(rng, long_len, wide=(i % 3 == 2)), flag=16 if i % 2 else 4, name=f"long_{i}"))
        one.append(read_from_ascii(_random(rng, L), *_kin(rng, L, wide=(i % 3 == 0)), flag=4 if i % 2 else 16, name=f"short_{L}"))
    long_len = int(rng.integers(2000, 3001))
    one.append(read_from_ascii(_random(rng, long_len), *_kin(rng, long_len, wide=False), flag=4, name="long_last"))
    return one + one[::-1]


def zero_length_read():
    e = np.empty(0, np.uint8)
    return Read("zero", 0, 4, e, e.copy(), e.copy(), e.copy(), e.copy())


SETS = {"ladder": ladder, "crowd": crowd, "sandwich": sandwich}
# the strata (cnn64.ALL_STRATA) a set must populate in every context -- CHH on both strands.  The ladder's reads of 401, 402 and 999 bases
# also hold a few "middle" sites, which are bounded like the rest where they exist.
REQUIRED_STRATA = {"ladder": ("both", "start", "end"), "crowd": ("both",), "sandwich": ("both", "start", "middle", "end")}
