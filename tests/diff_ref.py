"""`diff` in numpy: what hm_pileup_load_loci does to the planes, and what the command reads from a *.cov.bed file.

A restatement of include/hifimeth_hip.h's rules for the tests, sharing no code with hifimeth_amd/pileup.py.

THE LOADER.  Seven planes over the concatenated reference: pcov, ncov, key (the pooled sample) and pcov1, ncov1, pcov2, ncov2.
A row (gpos, pcov, ncov, motif) for `part` is checked in this order and the first failure names it:
    gpos outside [0, total)  ->  bad "gpos";   pcov < 0 or ncov < 0  ->  bad "count";   motif > 3  ->  bad "motif".
A bad row adds nothing.  A row with pcov + ncov == 0 is ignored.  Every other row adds its counts to the planes of its part and to
the pooled ones and raises key[gpos] to max(key, motif); it is bad "dup" -- and still adds -- when the locus held a count of the
same part before it.  In whatever order k such rows of one part reach one locus, k - 1 of them find a count there, and all k when
an earlier call left one: the number of duplicates does not depend on the order.
A call with a bad row returns HM_EDATA and voids the engine: every later load returns HM_ESTATE.

THE PARSER.  Lines end at \\n (a \\r before it is dropped); empty lines are skipped; a row needs six tab-separated columns: name,
start, end, a column nobody reads, pcov, ncov; more columns are ignored.  A number is 1 .. 18 decimal digits and nothing else."""
import gzip
import re

import numpy as np

HM_EDATA, HM_ESTATE = -4, -5
PLANES = ("pcov", "ncov", "key", "pcov1", "ncov1", "pcov2", "ncov2")
KINDS = ("gpos", "count", "motif", "dup")


class Loader:
    def __init__(self, total):
        self.total = int(total)
        self.planes = {k: np.zeros(self.total, np.int64) for k in PLANES}
        self.failed = False
        self.bad = dict.fromkeys(KINDS, 0)                    # of the last call

    def load(self, part, gpos, pcov, ncov, motif):
        """-> rows that added a count, or HM_EDATA / HM_ESTATE"""
        assert part in (1, 2)
        if self.failed:
            return HM_ESTATE
        g, p, n = (np.asarray(x, np.int64).reshape(-1) for x in (gpos, pcov, ncov))
        m = np.broadcast_to(np.asarray(motif, np.int64), g.shape)
        self.bad = dict.fromkeys(KINDS, 0)
        bad_g = (g < 0) | (g >= self.total)
        bad_c = ~bad_g & ((p < 0) | (n < 0))
        bad_m = ~bad_g & ~bad_c & (m > 3)
        self.bad.update(gpos=int(bad_g.sum()), count=int(bad_c.sum()), motif=int(bad_m.sum()))
        add = ~bad_g & ~bad_c & ~bad_m & (p + n > 0)
        g, p, n, m = g[add], p[add], n[add], m[add]
        P, N = self.planes["pcov%d" % part], self.planes["ncov%d" % part]
        loci, rows_at = np.unique(g, return_counts=True)
        held = (P[loci] != 0) | (N[loci] != 0)
        self.bad["dup"] = int((rows_at - 1 + held).sum())
        for plane, v in ((P, p), (N, n), (self.planes["pcov"], p), (self.planes["ncov"], n)):
            np.add.at(plane, g, v)
        np.maximum.at(self.planes["key"], g, m)
        if sum(self.bad.values()):
            self.failed = True
            return HM_EDATA
        return int(add.sum())

    def loci(self, part=0):
        """the covered loci of the pooled sample (part 0) or of a part: (gpos, pcov, ncov, key & 3) arrays, ascending"""
        tag = "" if part == 0 else str(part)
        P, N = self.planes["pcov" + tag], self.planes["ncov" + tag]
        g = np.nonzero(P + N > 0)[0]
        return g, P[g], N[g], self.planes["key"][g] & 3

    def tested(self, min_cov):
        """the loci where each part holds at least min_cov counts: (gpos, pcov1, ncov1, pcov2, ncov2, context 0..2), ascending"""
        q = self.planes
        g = np.nonzero((q["pcov1"] + q["ncov1"] >= min_cov) & (q["pcov2"] + q["ncov2"] >= min_cov))[0]
        return [(int(i), int(q["pcov1"][i]), int(q["ncov1"][i]), int(q["pcov2"][i]), int(q["ncov2"][i]), min(int(q["key"][i]) & 3, 2))
                for i in g]


_NUMBER = re.compile(rb"[0-9]{1,18}\Z")


def parse_cov_bed(path, names, lengths, motif):
    """-> (gpos, pcov, ncov, motif) int64 arrays; ValueError("<path>:<line>: ...") for a line the command rejects"""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    start_of, length_of = {}, {}
    at = 0
    for name, length in zip(names, lengths):
        start_of[name.encode()], length_of[name.encode()] = at, int(length)
        at += int(length)
    rows = []
    lines = raw.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                           # the text behind the last newline is a line only if there is some
    for no, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        col = line.split(b"\t")

        def reject(why):
            return ValueError("%s:%d: %s" % (path, no, why))
        if len(col) < 6:
            raise reject("columns")
        if col[0] not in start_of:
            raise reject("sequence")
        if not _NUMBER.match(col[1]) or int(col[1]) >= length_of[col[0]]:
            raise reject("start")
        if not _NUMBER.match(col[2]) or int(col[2]) != int(col[1]) + 1:
            raise reject("end")
        if not _NUMBER.match(col[4]) or not _NUMBER.match(col[5]) or int(col[4]) >= 1 << 31 or int(col[5]) >= 1 << 31:
            raise reject("counts")
        rows.append((start_of[col[0]] + int(col[1]), int(col[4]), int(col[5]), motif))
    out = np.array(rows, np.int64).reshape(-1, 4)
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]
