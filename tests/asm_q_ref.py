"""What the tests of `pileup -H -A -Q` share: the dense tuple space restated, Benjamini-Hochberg in numpy by the definition of
hm_asm_qvalues, and the hand-made inputs of the host-only test (also written to a file for the stand-alone checker
tools/asm_qvalues_check.cpp: `python tests/asm_q_ref.py FILE`)."""
import sys

import numpy as np

DBL_MIN = 2.2250738585072014e-308
ASM_T, ASM_PAIRS = 64, 2080
ASM_BINS = 3 * ASM_PAIRS * ASM_PAIRS
BIN_DTYPE = np.dtype([("bin", "<u4"), ("reserved", "<u4"), ("count", "<u8"), ("pvalue", "<f8"), ("qvalue", "<f8")])
ASM_DTYPE = np.dtype([("gpos", "<i8"), ("pcov1", "<i4"), ("ncov1", "<i4"), ("pcov2", "<i4"), ("ncov2", "<i4"), ("motif", "<u4"),
                      ("reserved", "<u4"), ("diff", "<f8"), ("pvalue", "<f8")])


def pair(p, n):
    t = p + n
    return t * (t + 1) // 2 + p


def bin_index(ctx, p1, n1, p2, n2):
    """of a tested locus with both haplotype totals < 64 (int or numpy arrays)"""
    return (ctx * ASM_PAIRS + pair(p1, n1)) * ASM_PAIRS + pair(p2, n2)


def bh_numpy(p: np.ndarray) -> np.ndarray:
    """R's p.adjust(method = "BH"), one p per locus: over the distinct p (bit-equal values grouped) ascending, R = the number of
    loci with p <= it, q = the minimum over it and all larger p of min(1.0, p * m / R), evaluated left to right in fp64"""
    p = np.asarray(p, np.float64)
    if len(p) == 0:
        return p.copy()
    u, cnt = np.unique(p, return_counts=True)
    q = np.minimum(1.0, u * float(len(p)) / np.cumsum(cnt).astype(np.float64))
    q = np.minimum.accumulate(q[::-1])[::-1]
    return q[np.searchsorted(u, p)]


def make_tab(entries) -> np.ndarray:
    """[(ctx, p1, n1, p2, n2, count, pvalue)] -> hm_asm_bin_t rows ascending in bin, qvalue NaN"""
    tab = np.zeros(len(entries), BIN_DTYPE)
    for i, (c, p1, n1, p2, n2, count, pv) in enumerate(entries):
        tab[i] = (bin_index(c, p1, n1, p2, n2), 0, count, pv, np.nan)
    tab = tab[np.argsort(tab["bin"], kind="stable")]
    return tab


def make_big(rows) -> np.ndarray:
    """[(p1, n1, p2, n2, motif, pvalue)] -> hm_asm_t rows with ascending gpos"""
    big = np.zeros(len(rows), ASM_DTYPE)
    for i, (p1, n1, p2, n2, motif, pv) in enumerate(rows):
        big[i] = (500 + 7 * i, p1, n1, p2, n2, motif, 0, 100.0 * p1 / (p1 + n1) - 100.0 * p2 / (p2 + n2), pv)
    return big


def expected(tab, big):
    """-> (tab q, big q, m) by bh_numpy over the expanded multiset of p of every context"""
    tq, bq, m = np.full(len(tab), np.nan), np.full(len(big), np.nan), np.zeros(3, np.uint64)
    tc = (tab["bin"] // (ASM_PAIRS * ASM_PAIRS)).astype(np.int64)
    bc = np.minimum(big["motif"], 2).astype(np.int64)
    for c in range(3):
        ti, bi = np.nonzero(tc == c)[0], np.nonzero(bc == c)[0]
        p = np.concatenate([np.repeat(tab["pvalue"][ti], tab["count"][ti].astype(np.int64)), big["pvalue"][bi]])
        m[c] = len(p)
        q = bh_numpy(p)
        first = np.concatenate([[0], np.cumsum(tab["count"][ti].astype(np.int64))])[:-1]
        tq[ti] = q[first] if len(ti) else []
        bq[bi] = q[len(p) - len(bi):]
    return tq, bq, m


def cases():
    """name -> (tab, big): tie groups, weights > 1, all p = 1.0, p = DBL_MIN, an empty context, one locus only, big rows mixed in"""
    rng = np.random.default_rng(77)
    out = {}
    # CpG: ties across bins (0.03 three times, with weights), DBL_MIN, 1.0; CHG empty; CHH (from motif 2 and 3): big rows tie with a bin
    out["mixed"] = (
        make_tab([(0, 5, 0, 0, 5, 1, 0.03), (0, 6, 1, 1, 6, 40, 0.03), (0, 2, 3, 3, 2, 7, 1.0), (0, 10, 0, 0, 10, 1, DBL_MIN),
                  (0, 9, 0, 0, 9, 3, 1e-5), (0, 7, 7, 0, 14, 2, 0.03), (0, 1, 4, 4, 1, 1000, 0.5), (0, 63, 0, 0, 63, 1, 1e-300),
                  (2, 5, 0, 0, 5, 2, 0.004), (2, 3, 3, 3, 3, 9, 1.0), (2, 8, 1, 2, 7, 5, 0.02)]),
        make_big([(64, 0, 0, 5, 2, 0.004), (30, 40, 5, 5, 3, 0.6), (10, 10, 100, 0, 0, 1e-12), (0, 65, 65, 0, 3, DBL_MIN),
                  (62, 2, 1, 5, 2, 0.02), (1, 5, 32, 32, 0, 0.03)]))
    out["all_one"] = (make_tab([(1, 3, 3, 3, 3, 4, 1.0), (1, 2, 2, 2, 2, 1, 1.0), (0, 1, 1, 1, 1, 6, 1.0)]),
                      make_big([(40, 40, 40, 40, 1, 1.0)]))
    out["one_bin_locus"] = (make_tab([(2, 5, 0, 0, 5, 1, 0.0079)]), make_big([]))
    out["one_big_locus"] = (make_tab([]), make_big([(70, 0, 0, 70, 0, 1e-40)]))
    out["dbl_min_only"] = (make_tab([(0, 60, 0, 0, 60, 3, DBL_MIN), (0, 61, 0, 0, 61, 1, DBL_MIN)]), make_big([]))
    out["empty"] = (make_tab([]), make_big([]))
    # many random tuples: p rounded to two digits makes ties, weights up to 1000 push m far beyond the entries
    n = 3000
    t1, t2 = rng.integers(1, 64, n), rng.integers(1, 64, n)
    p1, p2 = (rng.random(n) * (t1 + 1)).astype(np.int64), (rng.random(n) * (t2 + 1)).astype(np.int64)
    ent = {}
    for c, a, b, x, y in zip(rng.integers(0, 3, n), p1, t1 - p1, p2, t2 - p2):
        ent[(int(c), int(a), int(b), int(x), int(y))] = (int(rng.choice([1, 2, 17, 1000])), max(float(np.round(rng.random() ** 6, 2)), 0.01))
    tab = make_tab([(*k, w, pv) for k, (w, pv) in ent.items()])
    big = make_big([(int(rng.integers(64, 500)), int(rng.integers(0, 9)), int(rng.integers(0, 70)), int(rng.integers(1, 9)),
                     int(rng.integers(0, 4)), max(float(np.round(rng.random() ** 4, 2)), 0.01)) for _ in range(200)])
    out["random"] = (tab, big)
    return out


if __name__ == "__main__":                                  # the cases and their expected q, for tools/asm_qvalues_check.cpp
    with open(sys.argv[1], "wb") as f:
        for name, (tab, big) in cases().items():
            tq, bq, m = expected(tab, big)
            f.write(np.array([len(tab), len(big)], "<i8").tobytes() + tab.tobytes() + big.tobytes())
            f.write(tq.astype("<f8").tobytes() + bq.astype("<f8").tobytes() + m.astype("<u8").tobytes())
