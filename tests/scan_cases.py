"""Hand-built inputs for the site scanner of the call engine (prep_kernel -> scan_kernel -> emit_kernel -> pack_kernel,
hifimeth_amd/csrc/hm_kernels.hip): a plain module, imported by test_scan_cases_cpu.py, test_gpu_scan_edges.py and
tools/make_golden.py.  Four classes of hifimeth_amd.synth.Read lists that random sequence of a few fixed lengths never produces
on purpose:

    boundary_motifs()   one motif per read, planted in a site-free A/T background so that it straddles a thread (4), wave (256) or
                        chunk (1024) boundary of the kernels' ownership, every motif again with an N inside; forward and flag 16
    tail_lengths()      every l_qseq % 4 behind every other one, reads that begin GGCG and end CCG / CG / C, lengths 1 .. 7
    mixed_widths()      all 16 (u8, u16) combinations over fi, fp, ri, rp, both sides of every threshold of the frame codec
    many_chunks(n)      n scan chunks: one, two, three and four chunks per scan thread, empty trailing threads, a read across a
                        scan thread's range, a last read that fills its chunk

Every function asserts, with the CPU oracle, that its class holds what it is for (conditions, not measurements).  Nothing here
is random beyond a seeded generator; names are stable.  Results are cached: the lists are shared and must not be modified.
"""
import functools

import numpy as np

from hifimeth_amd.synth import Read, read_from_ascii
from oracle import hm_oracle as O

CPG, CHG, CHH = 0, 1, 2
CHUNK = 1024                 # bases per prep / emit workgroup (hm_device.h)
SCAN_THREADS = 1024          # threads of the single scan workgroup (hm_kernels.hip)
BOUNDARIES = (4, 8, 252, 256, 260, 1020, 1024, 1028, 2048, 3072)
GOLDEN_BOUNDARIES = BOUNDARIES[:6]      # tests/golden/scan_edges.json leaves out the four longest (file size), see golden_reads()
BOUNDARY_LEN = 3100          # four chunks
TAIL_LENGTHS = tuple(range(1000, 1004)) + tuple(range(1021, 1028)) + tuple(range(2046, 2052)) + tuple(range(1, 8))
TAIL_ENDS = ("CCG", "CG", "C")
# both sides of every threshold of encode_frames (64, 192, 448, 952), and 195 / 455: the thresholds themselves are where two arms
# agree (448 encodes to 192 by either), 195 and 455 are the last values on which the arm below 192 / 448 and the arm above differ
U16_CYCLE = (0, 63, 64, 65, 191, 192, 193, 195, 447, 448, 449, 455, 951, 952, 953, 2000, 65535)
MANY_CHUNKS = (1023, 1024, 1025, 2047, 2049, 3075)
# chunks per scan thread and scan threads with an empty range, written out: per = ceil(n / 1024), empty = 1024 - ceil(n / per)
SCAN_PARTITION = {1023: (1, 1), 1024: (1, 0), 1025: (2, 511), 2047: (2, 0), 2049: (3, 341), 3075: (4, 255)}

_RC = bytes.maketrans(b"ACGTN", b"TGCAN")
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _kin8(rng, L):
    return [rng.integers(0, 256, L).astype(np.uint8) for _ in range(4)]


def _store(fwd: bytes, kin, flag: int, name: str) -> Read:
    """The record whose FORWARD strand is `fwd`: for flag 16 the stored bytes are the reverse complement (bam_info.cpp:180-192);
    the kinetics arrays are indexed as stored either way."""
    return read_from_ascii(fwd.translate(_RC)[::-1] if flag & 16 else fwd, *kin, flag=flag, name=name)


def site_lists(rd):
    """(fwd, [sorted CpG qoffs, sorted CHG qoffs, sorted CHH qoffs]) of one read, by the oracle."""
    fwd = O.decode(rd)
    return fwd, [np.sort(O.scan(fwd, c)) for c in range(3)]


def background(rng, L: int) -> bytearray:
    """runs of A and T only: no C, no G, hence no site of any context on either strand"""
    out = bytearray()
    base = int(rng.integers(0, 2))
    while len(out) < L:
        out += (b"A", b"T")[base] * int(rng.integers(1, 9))
        base ^= 1
    return out[:L]


def site_free_reads(n_reads: int, L: int = 1000, seed: int = 77):
    """poly-A/T reads: an ordinary input on which the scanner finds nothing"""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n_reads):
        fwd = bytes(background(rng, L))
        if i < 4:
            assert all(len(O.scan(fwd, c)) == 0 for c in range(3))
        reads.append(_store(fwd, _kin8(rng, L), 16 if i % 3 == 0 else 4, f"at_{i}"))
    return reads


# ---- motifs on the ownership boundaries -----------------------------------------------------------------------------
def _plants(B: int):
    """(name, {position: base}, expected [(ctx, qoff, strand)], (first, last) position of the motif) of every motif that
    straddles B, then the same motifs with an N inside (no site).  The neighbours are background (A / T): a lone C is a forward
    CHH site, a lone G a reverse-strand one."""
    out = []
    out.append((f"cpg_c{B - 1}", {B - 1: "C", B: "G"}, [(CPG, B - 1, 0)], (B - 1, B)))
    # C H G: H = A and T give one CHG site; H = C spells CCG, whose second C is a CpG site as well
    out.append((f"chg_a_c{B - 2}", {B - 2: "C", B - 1: "A", B: "G"}, [(CHG, B - 2, 0)], (B - 2, B)))
    out.append((f"chg_c_c{B - 1}", {B - 1: "C", B: "C", B + 1: "G"}, [(CHG, B - 1, 0), (CPG, B, 0)], (B - 1, B + 1)))
    out.append((f"chg_t_c{B - 1}", {B - 1: "C", B: "T", B + 1: "G"}, [(CHG, B - 1, 0)], (B - 1, B + 1)))
    for c0 in (B - 2, B - 1):
        out.append((f"chh_c{c0}", {c0: "C"}, [(CHH, c0, 0)], (c0, c0 + 2)))
    for g in (B, B + 1):
        out.append((f"chh_g{g}", {g: "G"}, [(CHH, g, 1)], (g - 2, g)))
    # an N inside the motif
    out.append((f"cpg_n_c{B - 1}", {B - 1: "C", B: "N"}, [], (B - 1, B)))
    out.append((f"cpg_n_g{B}", {B - 1: "N", B: "G"}, [], (B - 1, B)))
    out.append((f"chg_n_c{B - 2}", {B - 2: "C", B - 1: "N", B: "G"}, [], (B - 2, B)))
    out.append((f"chg_n_c{B - 1}", {B - 1: "C", B: "N", B + 1: "G"}, [], (B - 1, B + 1)))
    out.append((f"chh_n_c{B - 2}", {B - 2: "C", B - 1: "A", B: "N"}, [], (B - 2, B)))
    out.append((f"chh_n_c{B - 1}", {B - 1: "C", B: "N"}, [], (B - 1, B + 1)))
    out.append((f"chh_n_g{B}", {B - 1: "N", B: "G"}, [], (B - 2, B)))
    out.append((f"chh_n_g{B + 1}", {B - 1: "N", B: "T", B + 1: "G"}, [], (B - 1, B + 1)))
    return out


@functools.lru_cache(maxsize=None)
def boundary_motifs():
    """-> (reads, expected, boundary): expected[i] = [(ctx, qoff, strand)] of reads[i] sorted by qoff, written out from the
    construction; boundary[i] = the B the read's motif straddles."""
    rng = np.random.default_rng(20250301)
    bare = bytes(background(rng, BOUNDARY_LEN))
    assert set(bare) == set(b"AT") and all(len(O.scan(bare, c)) == 0 for c in range(3))
    reads, expected, boundary = [], [], []
    for B in BOUNDARIES:
        for name, plant, want, (lo, hi) in _plants(B):
            seq = background(rng, BOUNDARY_LEN)
            for pos, base in plant.items():
                seq[pos] = ord(base)
            fwd = bytes(seq)
            kin = _kin8(rng, BOUNDARY_LEN)
            want = sorted(want, key=lambda t: t[1])
            for flag in (4, 16):
                rd = _store(fwd, kin, flag, f"b{B}_{name}_{'r' if flag & 16 else 'f'}")
                got_fwd, lists = site_lists(rd)
                assert got_fwd == fwd, rd.name
                for c in range(3):
                    assert lists[c].tolist() == [q for k, q, _ in want if k == c], (rd.name, c)
                assert all(fwd[q:q + 1] == (b"G" if s else b"C") for _, q, s in want), rd.name
                assert lo < B <= hi and lo <= min(plant) and max(plant) <= hi, (rd.name, lo, hi)   # bases on both sides of B
                assert ("N" in plant.values()) == (not want) == (b"N" in fwd), rd.name
                reads.append(rd)
                expected.append(want)
                boundary.append(B)
    assert len(reads) == len(BOUNDARIES) * 16 * 2 and sum(len(e) > 0 for e in expected) == len(BOUNDARIES) * 8 * 2
    assert all(len(r.seq4) == (BOUNDARY_LEN + 1) // 2 for r in reads)
    return reads, expected, boundary


# ---- read ends --------------------------------------------------------------------------------------------------------
def _residue_order():
    """TAIL_LENGTHS in an order in which every ordered pair (a, b), a != b, of l_qseq % 4 occurs as neighbours"""
    pools = {r: [L for L in TAIL_LENGTHS if L % 4 == r] for r in range(4)}
    head = [0, 1, 0, 2, 0, 3, 0, 1, 2, 1, 3, 1, 2, 3, 2]
    out = [pools[r].pop(0) for r in head]
    rest = [pools[r] for r in (3, 2, 1, 0)]
    while any(rest):
        for p in rest:
            if p:
                out.append(p.pop(0))
    return out


@functools.lru_cache(maxsize=None)
def tail_lengths():
    """-> reads (to be run with min_read_size 1)"""
    rng = np.random.default_rng(20250302)
    order = _residue_order()
    assert sorted(order) == sorted(TAIL_LENGTHS)
    pairs = {(a % 4, b % 4) for a, b in zip(order, order[1:])}
    assert {(a, b) for a in range(4) for b in range(4) if a != b} <= pairs
    assert {a % 4 for a in order[:-1]} == {0, 1, 2, 3}           # every residue pads the base_off of a successor
    reads = []
    for i, L in enumerate(order):
        end = TAIL_ENDS[i % 3]
        seq = bytearray((b"GGCG" + _ACGT[rng.integers(0, 4, max(0, L - 4))].tobytes())[:L])
        for k in range(min(len(end), L)):
            seq[L - 1 - k] = ord(end[-1 - k])
        fwd = bytes(seq)
        rd = _store(fwd, _kin8(rng, L), 16 if i % 4 == 1 else 4, f"tail_{L}_{end}")
        got_fwd, lists = site_lists(rd)
        assert got_fwd == fwd
        every = set(np.concatenate(lists).tolist())
        if L >= 8:
            assert fwd[:4] == b"GGCG" and fwd.endswith(end.encode())
            assert 0 not in every and 1 not in every and 2 in lists[CPG]   # G at 0 and 1: no two bases in front of them
            assert L - 1 not in every                                         # a C on the last base, or the G of the last CG
            if end == "CCG":
                assert L - 3 in lists[CHG] and L - 2 in lists[CPG]
            elif end == "CG":
                assert L - 2 in lists[CPG]
            else:
                assert fwd[L - 1:] == b"C"      # a C with nothing behind it
        reads.append(rd)
    assert sum(len(np.concatenate(site_lists(r)[1])) for r in reads if r.l_qseq < 8) >= 3   # the tiny reads hold sites too
    return reads


# ---- kinetics width per array -------------------------------------------------------------------------------------------
_U16_CODES = np.array([O.encode_frames(v) for v in U16_CYCLE], np.int64)     # codev1 byte of every value of the cycle


def _codes(a):
    """the codev1 bytes the engine packs for a kinetics array of mixed_widths()"""
    return a.astype(np.int64) if a.dtype.itemsize == 1 else _U16_CODES[np.searchsorted(np.array(U16_CYCLE), a)]


@functools.lru_cache(maxsize=None)
def mixed_widths():
    """-> reads: 16 width combinations x (forward, flag 16).  u16 arrays cycle through U16_CYCLE (every arm of encode_frames,
    both sides of 64 / 192 / 448 / 952), u8 arrays through 0 .. 255, each array at a phase of its own.  Two arrays of one width
    never hold the same value at the same position.  A u8 and a u16 array, whose cycles are 256 and 17 long, meet at a few of the
    1400 positions whatever their phases, and different frame counts share a code (952, 953, 2000 and 65535 all encode to 255):
    asserted instead is that the values of two arrays agree at under 1 % of the positions, and that the CODES of any two arrays
    differ at most positions and agree over 4 in a row at most,
    so that a swapped array changes every window."""
    rng = np.random.default_rng(20250303)
    L = 1400
    enc = [O.encode_frames(v) for v in U16_CYCLE]
    assert enc == [0, 63, 64, 64, 127, 128, 128, 128, 191, 192, 192, 192, 254, 255, 255, 255, 255]
    assert [O.encode_frames(t - 1) != O.encode_frames(t) for t in (64, 192, 448, 952)] == [True] * 4
    j = np.arange(L)
    reads = []
    for combo in range(16):
        gc = 0.16
        fwd = _ACGT[rng.choice(4, L, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])].tobytes()
        kin = []
        for k in range(4):
            if combo >> k & 1:
                kin.append(np.array(U16_CYCLE, np.uint16)[(j + (0, 4, 8, 11)[k] + combo) % len(U16_CYCLE)])
            else:
                kin.append(((j + (0, 67, 131, 199)[k] + combo) % 256).astype(np.uint8))
        for a in range(4):
            for b in range(a + 1, 4):
                raw_same = kin[a].astype(np.int64) == kin[b].astype(np.int64)
                if kin[a].dtype == kin[b].dtype:
                    assert not raw_same.any(), (combo, a, b)
                assert raw_same.mean() < 0.01, (combo, a, b, raw_same.mean())
                # a swapped array changes every window: the CODES differ at most positions and agree over a few in a row at most
                same = np.concatenate([[0], (_codes(kin[a]) == _codes(kin[b])).astype(np.int64), [0]])
                edges = np.flatnonzero(np.diff(same))
                assert same.mean() < 0.4 and (edges[1::2] - edges[0::2]).max(initial=0) <= 4, (combo, a, b, same.mean())
        for k in range(4):
            if combo >> k & 1:
                assert set(kin[k].tolist()) == set(U16_CYCLE)
            else:
                assert set(kin[k].tolist()) == set(range(256))
        for flag in (4, 16):
            rd = _store(fwd, kin, flag, f"w{combo:04b}_{'r' if flag & 16 else 'f'}")
            assert [x.dtype.itemsize for x in (rd.fi, rd.fp, rd.ri, rd.rp)] == [1 + (combo >> k & 1) for k in range(4)]
            reads.append(rd)
    n_sites = sum(len(np.concatenate(site_lists(r)[1])) for r in reads)
    assert 2000 < n_sites < 10000, n_sites
    return reads


# ---- many chunks: the partition of scan_kernel -----------------------------------------------------------------------------
def scan_partition(n_chunks: int):
    """(chunks per scan thread, scan threads whose range is empty) of scan_kernel's partition, from its formula"""
    per = -(-n_chunks // SCAN_THREADS)
    lo = [min(n_chunks, t * per) for t in range(SCAN_THREADS)]
    hi = [min(n_chunks, x + per) for x in lo]
    return per, sum(a == b for a, b in zip(lo, hi))


@functools.lru_cache(maxsize=None)
def many_chunks(n_chunks: int, gc: float = 0.25):
    """-> reads that stage exactly n_chunks chunks: one-chunk reads of 1000 bases, one 5-chunk read that starts two chunks in
    front of a scan thread's range (it lies across three ranges at 2 chunks per thread, two at 3 and 4), and a last read of exactly
    1024 bases whose last 200 are site-free (the totals row is what emit_kernel reads as the chunk behind it)."""
    assert n_chunks in SCAN_PARTITION
    per, empty = scan_partition(n_chunks)
    assert (per, empty) == SCAN_PARTITION[n_chunks]
    rng = np.random.default_rng(20250304 + n_chunks)
    p = [(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]
    k = (n_chunks // 2) // per
    big_at = per * k - 2                  # chunk index = number of one-chunk reads in front
    assert 0 < big_at and big_at + 5 < n_chunks - 1 and (big_at + 2) % per == 0
    lengths = [1000] * big_at + [4 * CHUNK + 417] + [1000] * (n_chunks - 6 - big_at) + [CHUNK]
    assert sum(-(-L // CHUNK) for L in lengths) == n_chunks
    owners = {c // per for c in range(big_at, big_at + 5)}
    assert len(owners) >= 2 and (per > 2 or len(owners) >= 3)
    rev = rng.random(len(lengths)) < 0.4
    reads = []
    for i, L in enumerate(lengths):
        seq = bytearray(_ACGT[rng.choice(4, L, p=p)].tobytes())
        if i == len(lengths) - 1:
            seq[-200:] = background(rng, 200)
        reads.append(_store(bytes(seq), _kin8(rng, L), 16 if rev[i] else 4, f"mc{n_chunks}_{i}"))
    assert 0.3 < rev.mean() < 0.5
    fwd, lists = site_lists(reads[-1])
    every = np.concatenate(lists)
    assert len(every) > 20 and every.max() < CHUNK - 200 and reads[-1].l_qseq == CHUNK
    return reads


# ---- what the device must give ------------------------------------------------------------------------------------------------
def expected_sites(reads, mask: int = 7):
    """Per context the (read, qoff, strand) lists in (read, qoff) order -- what scan_sites(c) returns -- and the call order of
    mod_main.cpp:217-251: per read the forward-strand calls by qoff, then the reverse-strand ones.  -> (lists, order) with
    lists[c] = (rid, qoff, strand) arrays and order = (read_id, strand, qoff, ctx) arrays."""
    per_ctx = [([], [], []) for _ in range(3)]
    o_r, o_s, o_q, o_c = [], [], [], []
    for i, rd in enumerate(reads):
        fwd, lists = site_lists(rd)
        seq = np.frombuffer(fwd, np.uint8)
        qs, cs = [], []
        for c in range(3):
            if not mask >> c & 1:
                continue
            q = lists[c].astype(np.int32)
            per_ctx[c][0].append(np.full(len(q), i, np.int32))
            per_ctx[c][1].append(q)
            per_ctx[c][2].append((seq[q] == ord("G")).astype(np.uint8))
            qs.append(q)
            cs.append(np.full(len(q), c, np.uint8))
        q = np.concatenate(qs) if qs else np.empty(0, np.int32)
        c = np.concatenate(cs) if cs else np.empty(0, np.uint8)
        s = (seq[q] == ord("G")).astype(np.uint8)
        fw, rv = np.flatnonzero(s == 0), np.flatnonzero(s == 1)
        idx = np.concatenate([fw[np.argsort(q[fw], kind="stable")], rv[np.argsort(q[rv], kind="stable")]])
        o_r.append(np.full(len(idx), i, np.int32))
        o_s.append(s[idx])
        o_q.append(q[idx])
        o_c.append(c[idx])
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.empty(0, dt)  # noqa: E731
    lists = [tuple(cat(x, dt) for x, dt in zip(per_ctx[c], (np.int32, np.int32, np.uint8))) for c in range(3)]
    return lists, (cat(o_r, np.int32), cat(o_s, np.uint8), cat(o_q, np.int32), cat(o_c, np.uint8))


GOLDEN_MARGIN = 36           # bases kept behind B in the golden's cut of a boundary read


@functools.lru_cache(maxsize=None)
def golden_reads():
    """The reads of tests/golden/scan_edges.json: of every boundary_motifs() read at GOLDEN_BOUNDARIES the first B + GOLDEN_MARGIN
    forward bases (the rest is site-free background, and the reference's scanner knows no chunks: the fixture pins the motifs, the
    N and the strands, at a fraction of the size), and tail_lengths() whole.  -> (reads, literal) with literal[name] = the
    boundary read's expected [(ctx, qoff, strand)]."""
    rng = np.random.default_rng(20250305)
    reads, expected, boundary = boundary_motifs()
    out, literal = [], {}
    for rd, want, B in zip(reads, expected, boundary):
        if B not in GOLDEN_BOUNDARIES:
            continue
        L = B + GOLDEN_MARGIN
        fwd = O.decode(rd)[:L]
        assert all(q + 2 < L for _, q, _ in want) and set(O.decode(rd)[L:]) <= set(b"AT")
        cut = _store(fwd, _kin8(rng, L), rd.flag, rd.name)
        assert [[q for k, q, _ in want if k == c] for c in range(3)] == [x.tolist() for x in site_lists(cut)[1]], rd.name
        out.append(cut)
        literal[rd.name] = want
    return out + tail_lengths(), literal


def golden_records():
    """(name, flag, SEQ as stored) of golden_reads()"""
    return [(r.name, r.flag, r.ascii().decode()) for r in golden_reads()[0]]
