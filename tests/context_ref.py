"""Plain restatement of `pileup -S` (include/hifimeth_hip.h: methylation by the k-mer around each cytosine): from three host plane
arrays and the list of sequences to the table [3, 4^k + 1, 4].  Plain module, imported by test_pileup_context_cpu.py and
test_gpu_pileup_context.py.  Nothing here is shared with the library: the definition in the header is the specification, and a
window is a slice of its own sequence's text, reverse-complemented as text, and looked up by name.
"""
import itertools

import numpy as np

CTX = ("CpG", "CHG", "CHH")
COMPLEMENT = str.maketrans("ACGT", "TGCA")


def kmer_rows(k):
    """{k-mer: row}: A < C < G < T, the first base most significant"""
    return {"".join(t): i for i, t in enumerate(itertools.product("ACGT", repeat=k))}


def reverse_complement(text):
    return text.translate(COMPLEMENT)[::-1]


def window(seq, pos, flank):
    """the k bases around the cytosine called at `pos` of `seq`, read on its strand, or None for `other`"""
    if seq[pos] == "C":
        a, b = pos - flank, pos + 3 + flank
    elif seq[pos] == "G":
        a, b = pos - 2 - flank, pos + 1 + flank
    else:
        return None
    if a < 0 or b > len(seq):
        return None
    w = seq[a:b] if seq[pos] == "C" else reverse_complement(seq[a:b])
    return w if set(w) <= set("ACGT") else None


def context_table(pcov, ncov, key, seqs, flank, min_cov=1, base=0, lo=0, hi=None):
    """planes whose element 0 is locus `base` of the concatenated `seqs`, of which [lo, hi) is looked at -> int64 [3, 4^k + 1, 4]:
    context, row (the last: `other`), (n_loci, pcov, ncov, ppm)"""
    k = 3 + 2 * flank
    rows = kmer_rows(k)
    other = 4 ** k
    hi = len(pcov) if hi is None else hi
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    pc, nc = np.asarray(pcov).astype(np.int64), np.asarray(ncov).astype(np.int64)
    ctx = np.asarray(key).astype(np.int64) & 3
    tab = np.zeros((3, other + 1, 4), np.int64)
    counted = np.flatnonzero(pc[lo:hi] + nc[lo:hi] >= min_cov) + lo
    holder = np.searchsorted(off, base + counted, side="right") - 1               # the sequence that holds g (an empty one holds none)
    for i, sid in zip(counted.tolist(), holder.tolist()):
        p, n, c = int(pc[i]), int(nc[i]), int(ctx[i])
        if c > 2:
            continue
        w = window(seqs[sid], base + i - int(off[sid]), flank)
        cov = p + n
        tab[c, other if w is None else rows[w]] += (1, p, n, (2000000 * p + cov) // (2 * cov))
    return tab


def near_ends(pcov, ncov, seqs, flank, min_cov=1):
    """(a counted locus lies within flank + 2 bases of a sequence's start, ... of a sequence's end), planes from locus 0"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    g = np.flatnonzero(np.asarray(pcov).astype(np.int64) + np.asarray(ncov).astype(np.int64) >= min_cov)
    sid = np.searchsorted(off, g, side="right") - 1
    return bool((g - off[sid] < flank + 2).any()), bool((off[sid + 1] - 1 - g < flank + 2).any())
