"""Read groups whose trunk maps cross 2^31 and 2^32 bytes (tests/test_gpu_bigmaps.py, tests/test_bigmaps_cases_cpu.py).

Pure numpy: a restatement of the engine's group plan (add_read_tiles in hm_engine.cpp)
    rows of a read      ceil((L + 400) / 112) * 112 + 32
    map_off of a read   the running sum of the rows of the reads before it in the group
    map row of view position x of view v      v * view_rows + map_off + 200 + x      (view_rows: the group's total rows)
and of what a site reads from the maps
    E4 gather rows      site row - 215 + 16 s, s = 1 .. 23          (site row - 199 .. site row + 153)
    edge chains         E1 .. E3 rows from site row - 199 to site row + 189 (K1 = 13; + 185 for K1 = 11)
A map row is 512 B in E1 .. E3 and 384 B in E4, so byte offsets pass a threshold T at row ceil(T / stride): the first row whose
offset no longer fits.  A case is one read list that the engine puts into ONE group (group_bases >= its rows): filler reads, and
around every crossing a short PROBE read placed so that the crossing row lies at least `margin` rows inside the probe's own map
region in the crossing's view -- sites of the probe then gather from both sides of the crossing and across it.

The thresholds are parameters: divided by 256 the same plan holds at ~22 k and ~44 k rows and is checked on the CPU in
milliseconds; at full scale the two cases hold 5.8 M and 11.3 M rows (one group each: 37 GB and 73 GB of group buffers)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from hifimeth_amd.synth import Read, pack_codes, synth_slab, unpack_codes

TR_OWN, TR_PAD, TR_SLACK = 112, 200, 32        # hm_device.h
STRIDE = {"E1..E3": 512, "E4": 384}            # bytes per map row (either precision: 2 x 128 fp16 or 128 fp32; 2 x 96 / 96)
GATHER_LO, GATHER_HI = -199, 153               # E4 rows of a site relative to its own row: -215 + 16 s, s = 1 .. 23
CHAIN_HI = 189                                 # last E1 .. E3 row an edge chain reads (K1 = 13)
T31, T32 = 1 << 31, 1 << 32
GROUP_BYTES_PER_ROW = 6440                     # GROUP_BYTES_PER_BASE of hm_engine.cpp: what a group's buffers take per map row
MAX_GROUP_ROWS_X2 = 1 << 27                    # add_read_tiles: 2 * rows < 2^27


def read_rows(L: int) -> int:
    return -(-(L + 2 * TR_PAD) // TR_OWN) * TR_OWN + TR_SLACK


def crossing_row(threshold: int, stride: int) -> int:
    """The first map row whose byte offset is >= threshold."""
    return -(-threshold // stride)


@dataclass
class Crossing:
    buffer: str        # "E1..E3" or "E4"
    threshold: int     # bytes
    view: int
    row: int           # the crossing row in the buffer (views back to back: view * view_rows + row in the view)
    read: int = -1     # index of the probe read
    rel: int = -1      # the crossing row relative to the first row of the probe's region in `view`

    def label(self) -> str:
        return f"{self.buffer} >= {self.threshold} B in view {self.view} (row {self.row})"


@dataclass
class Case:
    name: str
    ctx_mask: int
    n_views: int
    view_rows: int
    lens: np.ndarray                 # l_qseq per read
    map_off: np.ndarray              # first map row of each read's region (view 0)
    crossings: List[Crossing]
    probe_fwd: dict = field(default_factory=dict)   # probe read index -> forward-strand codes (A0 C1 G2 T3)
    reads: Optional[List[Read]] = None

    @property
    def contexts(self) -> str:
        return ",".join(n for c, n in enumerate(("cpg", "chg", "chh")) if self.ctx_mask >> c & 1)

    @property
    def probes(self) -> List[int]:
        return sorted(self.probe_fwd)

    @property
    def group_bytes_needed(self) -> int:
        return GROUP_BYTES_PER_ROW * self.view_rows

    # -- sites of a probe, as the engine orders a read's calls: (strand, qoff) ---------------------------------------
    def probe_sites(self, read: int):
        """(qoff, strand, ctx) of the probe's sites in the case's contexts: CpG / CHG / CHH on a forward C, CHH on a G whose two
        preceding bases are no C (the reverse strand's C H H)."""
        s = self.probe_fwd[read].astype(np.int64)
        L = len(s)
        n1 = np.concatenate([s[1:], [-1]])
        n2 = np.concatenate([s[2:], [-1, -1]])
        p1 = np.concatenate([[-1], s[:-1]])
        p2 = np.concatenate([[-1, -1], s[:-2]])
        isc = s == 1
        ctx = np.full(L, 3, np.int64)
        ctx[isc & (n1 == 2)] = 0
        ctx[isc & (n1 >= 0) & (n1 != 2) & (n2 == 2)] = 1
        ctx[isc & (n1 >= 0) & (n1 != 2) & (n2 >= 0) & (n2 != 2)] = 2
        strand = np.zeros(L, np.int64)
        rev = (s == 2) & (p1 >= 0) & (p1 != 1) & (p2 >= 0) & (p2 != 1)
        ctx[rev] = 2
        strand[rev] = 1
        keep = (ctx < 3) & ((self.ctx_mask >> np.minimum(ctx, 2) & 1) == 1)
        q = np.nonzero(keep)[0]
        order = np.lexsort((q, strand[q]))
        q = q[order]
        return q.astype(np.int32), strand[q].astype(np.uint8), ctx[q].astype(np.uint8)

    def site_rows(self, read, strand, qoff) -> np.ndarray:
        """Map row (views back to back) of the sites (read, strand, qoff): arrays or scalars."""
        read, strand, qoff = np.asarray(read, np.int64), np.asarray(strand, np.int64), np.asarray(qoff, np.int64)
        off = np.where(strand == 1, self.lens[read] - 1 - qoff, qoff)
        return strand * self.view_rows + self.map_off[read] + TR_PAD + off

    def sides(self, x: Crossing):
        """The probe's sites in the crossing's view by the rows they read from the crossing's buffer: (all below, all above,
        some on either side).  E4: the 23 gather rows; E1 .. E3: the rows of the edge chains."""
        q, strand, _ = self.probe_sites(x.read)
        q = q[strand == x.view]
        row = self.site_rows(x.read, x.view, q)
        lo, hi = row + GATHER_LO, row + (GATHER_HI if x.buffer == "E4" else CHAIN_HI)
        below, above = int((hi < x.row).sum()), int((lo >= x.row).sum())
        return below, above, len(q) - below - above

    def where(self, read: int, strand: int, qoff: int) -> str:
        """A call's place in the plan, for a failing comparison: read, view, map row and the nearest crossing."""
        row = int(self.site_rows(read, strand, qoff))
        near = min(self.crossings, key=lambda x: abs(row - x.row))
        kind = "probe" if read in self.probe_fwd else "filler"
        return (f"read {read} ({kind}, {int(self.lens[read])} bases, map_off {int(self.map_off[read])}) qoff {qoff} view {strand}: map row {row}, "
                f"{row - near.row:+d} rows from the crossing {near.label()}")


# ---- the plan ------------------------------------------------------------------------------------------------------------
def _tiles(L: int) -> int:
    return -(-(L + 2 * TR_PAD) // TR_OWN)


def _fill(gap_lo, gap_hi, kmin, kmax, rng):
    """Tile counts of filler reads whose rows sum into [gap_lo, gap_hi] (m reads of k tiles: 112 sum(k) + 32 m), or None."""
    if gap_hi < 0:
        return None
    gap_lo = max(gap_lo, 0)
    if gap_lo == 0:
        return []
    mean = TR_OWN * (kmin + kmax) / 2 + TR_SLACK
    m_pref = max(1, int(round((gap_lo + gap_hi) / 2 / mean)))
    m_max = gap_hi // (TR_OWN * kmin + TR_SLACK)
    for m in sorted(range(1, m_max + 1), key=lambda m: abs(m - m_pref)):
        K_lo = max(m * kmin, -(-(gap_lo - TR_SLACK * m) // TR_OWN))
        K_hi = min(m * kmax, (gap_hi - TR_SLACK * m) // TR_OWN)
        if K_lo > K_hi:
            continue
        ks = rng.integers(kmin, kmax + 1, m)
        K = int(min(max(int(ks.sum()), K_lo), K_hi))
        i = 0
        while int(ks.sum()) != K:            # nudge the draw onto the sum, one tile at a time, round robin
            d = 1 if ks.sum() < K else -1
            if kmin <= ks[i % m] + d <= kmax:
                ks[i % m] += d
            i += 1
        return [int(k) for k in ks]
    return None


def _plan(spec, R, probe_lens, fill, margin, rng):
    """(lens, is_probe, crossings) of a read list with exactly R rows, or None.  spec: (buffer, threshold, view) per crossing."""
    kmin, kmax = _tiles(fill[0]), _tiles(fill[1])
    xs = [Crossing(b, t, v, crossing_row(t, STRIDE[b])) for b, t, v in spec]
    order = sorted(range(len(xs)), key=lambda i: xs[i].row - xs[i].view * R)
    lens, probe_at, cur = [], [], 0

    def add_fillers(ks):
        nonlocal cur
        for k in ks:
            L = min(max(TR_OWN * k - 2 * TR_PAD - int(rng.integers(0, TR_OWN)), fill[0]), fill[1])
            assert _tiles(L) == k
            lens.append(L)
            cur += read_rows(L)

    for n, i in enumerate(order):
        x = xs[i]
        local = x.row - x.view * R
        Lp = probe_lens[n % len(probe_lens)]
        rp = read_rows(Lp)
        if local < margin or local > R - margin:
            return None
        ks = _fill(local - rp + margin - cur, local - margin - cur, kmin, kmax, rng)
        if ks is None:
            return None
        add_fillers(ks)
        x.read, x.rel = len(lens), local - cur
        assert margin <= x.rel <= rp - margin
        probe_at.append(len(lens))
        lens.append(Lp)
        cur += rp
    ks = _fill(R - cur, R - cur, kmin, kmax, rng)
    if ks is None:
        return None
    add_fillers(ks)
    assert cur == R
    return np.array(lens, np.int64), probe_at, xs


def _probe_read(L, rng, wide, reverse, name):
    fwd = rng.choice(4, L, p=[0.32, 0.18, 0.18, 0.32]).astype(np.uint8)
    if wide:
        kin = [np.clip(np.rint(rng.gamma(2.0, 30.0, L)), 0, 2000).astype(np.uint16) for _ in range(4)]
    else:
        kin = [np.clip(np.rint(rng.gamma(2.0, 12.0, L)), 0, 255).astype(np.uint8) for _ in range(4)]
    stored = np.ascontiguousarray((3 - fwd)[::-1]) if reverse else fwd      # flag 0x10: SEQ holds the reverse complement
    return fwd, Read(name, L, 16 if reverse else 0, pack_codes(stored), *kin)


def build_case(name: str, spec, ctx_mask: int, n_views: int, view_rows_min: int, fill=(15000, 25000), probe_lens=(3000, 2600, 2200, 2900),
               margin: int = 1000, seed: int = 1, pool: int = 64, synth: bool = True) -> Case:
    """The smallest plan with view_rows >= view_rows_min (a multiple of 16: every read's rows are) that places a probe around
    every crossing of `spec` and fills the group exactly.  synth = False: the plan only, no reads.
    Probe 0 carries B:S (wide) kinetics, probe 1 is stored reverse (flag 0x10); the fillers cycle `pool` distinct reads cut to length."""
    assert margin >= 400
    R0 = -(-view_rows_min // 16) * 16
    for R in range(R0, R0 + 16 * 256, 16):
        got = _plan(spec, R, probe_lens, fill, margin, np.random.default_rng(seed))
        if got is not None:
            break
    else:
        raise ValueError(f"{name}: no plan with {R0} .. {R0 + 16 * 256} rows")
    lens, probe_at, xs = got
    rows = np.array([read_rows(int(L)) for L in lens], np.int64)
    case = Case(name, ctx_mask, n_views, R, lens, np.concatenate([[0], np.cumsum(rows)[:-1]]), xs)
    assert int(rows.sum()) == R
    rng = np.random.default_rng(seed + 1000)
    probes = {}
    for n, i in enumerate(probe_at):
        fwd, rd = _probe_read(int(lens[i]), rng, wide=(n == 0), reverse=(n == 1), name=f"{name}/probe{n}")
        case.probe_fwd[i] = fwd
        probes[i] = rd
    if synth:
        n_fill = len(lens) - len(probe_at)
        src = synth_slab(max(1, min(pool, n_fill)), seed=seed + 2000, median_len=fill[1], sigma=0.0, min_len=fill[1], max_len=fill[1],
                         frac_wide=0.05, frac_short=0, frac_missing=0, genome_len=max(4 * fill[1], 1_000_000))
        codes = [unpack_codes(r.seq4, r.l_qseq) for r in src]
        case.reads, k = [], 0
        for i, L in enumerate(lens):
            if i in probes:
                case.reads.append(probes[i])
                continue
            s, L = src[k % len(src)], int(L)
            case.reads.append(Read(f"{name}/fill{k}", L, 4, pack_codes(codes[k % len(src)][:L]), s.fi[:L], s.fp[:L], s.ri[:L], s.rp[:L]))
            k += 1
    return case


def case_a(scale: int = 1, synth: bool = True, view_rows_min: Optional[int] = None) -> Case:
    """Two views, all contexts: E1 .. E3 and E4 pass 2^31 B in view 0 and 2^32 B in view 1."""
    t31, t32 = T31 // scale, T32 // scale
    spec = [("E1..E3", t31, 0), ("E4", t31, 0), ("E1..E3", t32, 1), ("E4", t32, 1)]
    if scale == 1:
        return build_case("A", spec, 7, 2, view_rows_min or 5_750_000, seed=11, synth=synth)
    # scaled down the four crossings lie within a few thousand rows of each other in their views: short fillers, and a view size
    # that keeps them a probe apart (view 1's rows are 2^32 B / stride - view_rows: see test_bigmaps_cases_cpu.py)
    return build_case("a", spec, 7, 2, view_rows_min or 31_000 * 256 // scale, fill=(1000, 1600), seed=11, synth=synth)


def case_b(scale: int = 1, synth: bool = True, view_rows_min: Optional[int] = None) -> Case:
    """One view, CpG and CHG: E1 .. E3 and E4 pass 2^32 B in view 0."""
    t32 = T32 // scale
    spec = [("E1..E3", t32, 0), ("E4", t32, 0)]
    if scale == 1:
        return build_case("B", spec, 3, 1, view_rows_min or 11_300_000, seed=12, synth=synth)
    return build_case("b", spec, 3, 1, view_rows_min or 46_000 * 256 // scale, fill=(1000, 1600), seed=12, synth=synth)
