"""Slab ladders for the engine-growth tests (test_gpu_engine_growth.py): batches of very different sizes through ONE engine, so that every
grow-only buffer (hm_host.h: DevBuf, PinnedArr) is reallocated while the engine is live -- and, in the pipeline, without a wait for the
previous slab.  Everything is seeded; nothing here needs a GPU, and test_growth_cases_cpu.py asserts what the GPU tests rely on.

LADDER          staged bases 6 k, 30 k, 150 k, 330 k, 12 k, 340 k.  Steps 1, 2, 3 at least double the largest slab before them (DevBuf adds
                at most 50 % head-room: every buffer must reallocate), slab 4 is a shrink (stale contents behind the live range), slab 5 fits
                inside the head-room of slab 3 (no reallocation, other reads at every address).  CpG-rich reads (GC 0.5): every context of every
                slab is far above the auto-trunk thresholds, so option trunk = 2 picks the same path whichever slab an engine sees first.
                The longest read doubles from slab to slab as well (1.7 k, 12 k, 70 k, 150 k): with group_bases = 32768 the largest read GROUP grows
                at each step too.
LADDER_SPARSE   CpG-poor reads (GC 0.11) for the per-site path: 8 k, 60 k, 4.2 M, 10 k.  The per-site path's launch window is
                max(sub_batch_sites, bases / 48) (launch_window below mirrors enqueue_run): it leaves the default 65536 only above 3.1 M staged
                bases, and the conv4 hand-off buffer d_act4 (window x 9.6 KB, 25 % head-room) reallocates at the top slab only if the window
                exceeds 1.25 x 60 k -- hence 4.2 M, not 300 k.
repeat_slab     ~20 read objects repeated until the slab's raw bytes exceed the pinned slab's 64 MB floor.

Every slab starts and ends with a "probe" read of at most 3 kb, so that the CPU oracle can check both ends of every buffer cheaply."""
import functools

import numpy as np

from hifimeth_amd.synth import read_from_ascii, synth_reads

# Engine constants mirrored by hand; the GPU tests' group_bytes and launch-pair assertions fail if the main ones drift.
MIN_READ = 1000                   # hm_engine.cpp: hm_engine::min_read_size (check_read)
TR_OWN, TR_PAD, TR_SLACK = 112, 200, 32   # hm_device.h: TR_OWN, TR_PAD, TR_SLACK (hm_engine.cpp: add_read_tiles)
LADDER_TARGETS = (6_000, 30_000, 150_000, 330_000, 12_000, 340_000)
SPARSE_TARGETS = (8_000, 60_000, 4_200_000, 10_000)
GROWTH_STEPS = (1, 2, 3)          # LADDER[k] is at least twice every slab before it
SHRINK_STEP, HEADROOM_STEP = 4, 5
SPARSE_GROWTH_STEPS = (1, 2)
SLAB_FLOOR = 64 << 20             # hm_engine.cpp: stage_read / hm_batch_submit_reads, slab.reserve(max(..., size_t(64) << 20))
REPEAT_COUNT = 24                 # repeats of the ~20 reads of repeat_slab()
DEFAULT_WINDOW = 65536            # hm_engine.cpp: hm_engine::sub_batch (option sub_batch_sites)
TAIL_SITES = 8                    # hm_device.h: TAIL_SITES


def staged(rd):
    """Does the engine stage the read (check_read: all four kinetics tags, l_qseq >= min_read_size)?"""
    return rd.has_kinetics() and rd.l_qseq >= MIN_READ


def staged_bases(slab):
    """total_bases of the batch as the engine counts it: every staged read padded to a multiple of 4."""
    return sum((r.l_qseq + 3) // 4 * 4 for r in slab if staged(r))


def map_rows(slab):
    """Map rows of the slab as one read group (add_read_tiles): whole tiles over [-200, L + 200) plus the slack, per staged read."""
    return sum((r.l_qseq + 2 * TR_PAD + TR_OWN - 1) // TR_OWN * TR_OWN + TR_SLACK for r in slab if staged(r))


def launch_window(bases, sub_batch=DEFAULT_WINDOW):
    """The per-site path's launch window of a batch (hm_engine.cpp, enqueue_run: `sb`, its 48 and its 2^20 cap)."""
    return min(max(sub_batch, (bases // 48 + TAIL_SITES) // TAIL_SITES * TAIL_SITES), 1 << 20)


def launch_pairs(bases, sub_batch=DEFAULT_WINDOW):
    """Front / tail launch pairs per per-site context of a batch: the windows that cover [0, bases)."""
    return -(-bases // launch_window(bases, sub_batch))


def site_counts(slab):
    """Sites per context of the staged reads by a direct count on the ASCII sequence: C followed by G; C, H, G; C, H, H on the forward view,
    and the same motifs of the reverse complement (G preceded by C; G, D, C; G, D, D read leftwards) for CHH, the one context called on both
    views.  Returns ([CpG, CHG, CHH], bases)."""
    cnt, bases = np.zeros(3, np.int64), 0
    for r in slab:
        if not staged(r):
            continue
        s = np.frombuffer(r.ascii(), np.uint8)
        C, G = s == ord("C"), s == ord("G")
        H = (s == ord("A")) | (s == ord("C")) | (s == ord("T"))
        D = (s == ord("A")) | (s == ord("G")) | (s == ord("T"))
        cnt[0] += int((C[:-1] & G[1:]).sum())
        cnt[1] += int((C[:-2] & H[1:-1] & G[2:]).sum())
        cnt[2] += int((C[:-2] & H[1:-1] & H[2:]).sum()) + int((G[2:] & D[1:-1] & D[:-2]).sum())
        bases += r.l_qseq
    return cnt, bases


def _kin(L, rng, wide=False):
    from test_gpu_parity import _kin as kin
    return kin(L, rng, wide)


def _rnd(L, rng, gc=0.5, wide=False, flag=4, name="r"):
    p = [(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.choice(4, L, p=p)].tobytes()
    return read_from_ascii(seq, *_kin(L, rng, wide), flag=flag, name=name)


def _fill(slab, target, last, rng, gc):
    """One more random read so that the slab, with `last` appended, stages exactly `target` bases (targets are multiples of 4)."""
    L = target - staged_bases(slab) - staged_bases([last])
    assert L >= MIN_READ and L % 4 == 0, (target, L)
    slab.append(_rnd(L - 1, rng, gc, name="fill"))      # an odd length: padded by one base
    slab.append(last)
    assert staged_bases(slab) == target
    return slab


def _synth(n, seed, median, gc=0.5, **kw):
    opts = dict(gc=gc, median_len=median, sigma=0.25, min_len=1000, max_len=9000, frac_wide=0.3, frac_short=0.1, frac_missing=0.1)
    opts.update(kw)
    return synth_reads(n, seed=seed, **opts)


def make_ladder():
    """The six slabs of LADDER, built from scratch (ladder() caches one copy)."""
    rng = np.random.default_rng(2026)
    missing = _rnd(1300, rng, name="missing")
    missing.rp = None                                        # passed through uncalled: takes a read_id, no room
    slabs = []
    # 0: ~6 k -- lengths 1000 and 1001, a read stored reversed; every read is checked against the oracle
    s = [_rnd(1203, rng, name="probe"), _rnd(1000, rng, name="len1000"), _rnd(1001, rng, wide=True, flag=16, name="len1001-rev"), missing]
    slabs.append(_fill(s, LADDER_TARGETS[0], _rnd(1102, rng, wide=True, name="probe"), rng, 0.5))
    # 1: ~30 k -- poly-C, a CG repeat
    s = [_rnd(1025, rng, flag=16, name="probe"), read_from_ascii(b"C" * 1300, *_kin(1300, rng), name="polyC"),
         read_from_ascii(b"CG" * 600, *_kin(1200, rng), name="CGrepeat")] + _synth(5, 11, 3000)
    slabs.append(_fill(s, LADDER_TARGETS[1], _rnd(1000, rng, name="probe"), rng, 0.5))
    # 2: ~150 k -- one read of 70 kb
    s = [_rnd(1299, rng, wide=True, name="probe"), _rnd(1025, rng), _rnd(70001, rng, name="long70k")] + _synth(12, 12, 4000)
    slabs.append(_fill(s, LADDER_TARGETS[2], _rnd(1100, rng, flag=16, name="probe"), rng, 0.5))
    # 3: ~330 k -- a crowd of 1000-base reads (1488 map rows each), one read of 150 kb
    s = [_rnd(1001, rng, name="probe")] + [_rnd(1000, rng, wide=(i % 7 == 0), name="crowd") for i in range(60)]
    s += [_rnd(150002, rng, name="long150k")] + _synth(14, 13, 5000)
    slabs.append(_fill(s, LADDER_TARGETS[3], _rnd(1200, rng, name="probe"), rng, 0.5))
    # 4: ~12 k, the shrink -- every read is checked against the oracle
    s = [_rnd(1150, rng, name="probe"), read_from_ascii(b"CCA" * 400, *_kin(1200, rng), flag=16, name="CCA-rev")] + _synth(2, 14, 2500)
    slabs.append(_fill(s, LADDER_TARGETS[4], _rnd(1111, rng, wide=True, flag=16, name="probe"), rng, 0.5))
    # 5: ~340 k inside the head-room of slab 3 -- other reads at every address
    s = [_rnd(1250, rng, name="probe")] + _synth(60, 15, 6000) + [read_from_ascii(b"G" * 1030, *_kin(1030, rng), name="polyG")]
    slabs.append(_fill(s, LADDER_TARGETS[5], _rnd(1003, rng, name="probe"), rng, 0.5))
    return slabs


def make_ladder_sparse():
    rng = np.random.default_rng(2027)
    slabs = []
    for k, (target, n, median) in enumerate(zip(SPARSE_TARGETS, (2, 10, 225, 3), (2500, 5000, 20000, 2500))):
        s = [_rnd(1200 + 101 * k, rng, gc=0.11, wide=(k == 1), name="probe")]
        s += _synth(n, 20 + k, median, gc=0.11, max_len=30000, frac_wide=0.1, sigma=0.2)
        slabs.append(_fill(s, target, _rnd(1000 + 7 * k, rng, gc=0.11, flag=16 if k == 2 else 4, name="probe"), rng, 0.11))
    return slabs


@functools.lru_cache(maxsize=None)
def ladder():
    return make_ladder()


@functools.lru_cache(maxsize=None)
def ladder_sparse():
    return make_ladder_sparse()


def repeat_unit():
    """The ~20 read objects of the repeat slab: mostly B:S kinetics (8.5 raw bytes per base), a short read and a read without a tag among them."""
    rng = np.random.default_rng(2028)
    unit = [_rnd(1201, rng, name="probe")]
    unit += synth_reads(16, seed=31, gc=0.5, median_len=22000, sigma=0.15, min_len=1000, max_len=30000, frac_wide=1.0, frac_short=0, frac_missing=0)
    short = _rnd(700, rng, name="short")
    missing = _rnd(1500, rng, name="missing")
    missing.fi = None
    return unit + [short, missing, _rnd(1002, rng, wide=True, flag=16, name="probe")]


def raw_bytes(slab):
    """Bytes the staged reads take in the pinned slab (place_read: SEQ and the four kinetics arrays, each padded to 16)."""
    a16 = lambda n: (n + 15) // 16 * 16
    return sum(a16((r.l_qseq + 1) // 2) + sum(a16(r.l_qseq * getattr(r, k).dtype.itemsize) for k in ("fi", "fp", "ri", "rp"))
               for r in slab if staged(r))


def repeat_slab(count=REPEAT_COUNT):
    """`count` repeats of repeat_unit() as one list: the same read objects again and again, free to make."""
    return repeat_unit() * count


def lead_slab():
    """The 20 k slab that is in flight while the repeat slab regrows a cold engine's slot arrays."""
    rng = np.random.default_rng(2029)
    s = [_rnd(1300, rng, name="probe")] + _synth(4, 41, 3000)
    return _fill(s, 20_000, _rnd(1009, rng, name="probe"), rng, 0.5)


def slab_bytes(slab):
    """Everything the engine is given of a slab, for the determinism check."""
    out = []
    for r in slab:
        out.append(np.array([r.l_qseq, r.flag], np.int64).tobytes() + r.seq4.tobytes())
        for k in ("fi", "fp", "ri", "rp"):
            a = getattr(r, k)
            out.append(b"-" if a is None else a.dtype.str.encode() + a.tobytes())
    return b"".join(out)
