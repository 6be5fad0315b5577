"""The fit of the two levels of `pileup -D` (`-D -Y`), restated from include/hifimeth_hip.h over domains_ref.py's textbook Viterbi:
what hm_pileup_domain_sums must return and what the iteration must do with it.  The sums are Python ints.  Every (A, B) and every
refitted level comes from the C library's host-only hm_domain_scores / hm_domain_refit through ctypes -- a last-ulp difference in
`log` would move a weight -- while refit_py is the plain division and clamp those levels are tested against."""
import ctypes

import numpy as np

from domains_ref import ctx_rows, emissions, switch_costs, viterbi

LOCUS_DTYPE = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("motif", "<u4"), ("reserved", "<u4")])
EPS = 1e-6
HM_OK, HM_EINVAL, HM_EDATA = 0, -1, -4


def lib_scores(lo, hi, penalty):
    """hm_domain_scores -> (A, B, S), or None where it fails"""
    from hifimeth_amd._lib import lib
    A, B, S = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib().hm_domain_scores(lo, hi, penalty, ctypes.byref(A), ctypes.byref(B), ctypes.byref(S))
    return (int(A.value), int(B.value), int(S.value)) if rc == HM_OK else None


def lib_refit(sums, penalty):
    """hm_domain_refit -> (return code, lo, hi); the levels start as NaN, so `untouched` shows"""
    from hifimeth_amd._lib import lib
    lo, hi = ctypes.c_double(float("nan")), ctypes.c_double(float("nan"))
    rc = lib().hm_domain_refit((ctypes.c_int64 * 6)(*sums), penalty, ctypes.byref(lo), ctypes.byref(hi))
    return rc, float(lo.value), float(hi.value)


def refit_py(sums):
    """step 3 without the check of the scores: None for an empty state, else (l', h') -- Python's int / int is the correctly
    rounded quotient, as is the C division of the two converted ints while they are below 2^53"""
    P0, N0, R0, P1, N1, R1 = sums
    if R0 == 0 or R1 == 0:
        return None
    assert max(P0 + N0, P1 + N1) < 1 << 53
    return min(max(P0 / (P0 + N0), EPS), 1 - EPS), min(max(P1 / (P1 + N1), EPS), 1 - EPS)


def state_sums(chains, ctx, A, B, S, max_gap):
    """(P0, N0, R0, P1, N1, R1) over the rows of context ctx in all chains (each hm_locus_t-like rows of one sequence): every
    chain is segmented on its own"""
    out = [0] * 6
    for loci in chains:
        r = ctx_rows(loci, ctx)
        z = viterbi(emissions(r["pcov"], r["ncov"], A, B), switch_costs([int(g) for g in r["gpos"]], S, max_gap))
        for p, n, s in zip(r["pcov"], r["ncov"], z):
            out[3 * s] += int(p)
            out[3 * s + 1] += int(n)
            out[3 * s + 2] += 1
    return tuple(out)


def fit(sums_of, lo, hi, penalty, max_iter):
    """sums_of(A, B, S) -> the six sums.  -> (lo, hi, status, history), history rows (i, l_i, h_i, A_i, B_i, sums)"""
    assert max_iter >= 1
    history = []
    scores = lib_scores(lo, hi, penalty)
    assert scores is not None, "the start levels are the caller's error"
    i = 0
    while True:
        A, B, S = scores
        sums = tuple(int(x) for x in sums_of(A, B, S))
        history.append((i, lo, hi, A, B, sums))
        rc, l2, h2 = lib_refit(sums, penalty)
        assert rc in (HM_OK, HM_EDATA)
        if sums[2] == 0 or sums[5] == 0:
            assert rc == HM_EDATA
            return lo, hi, "one_state", history
        if rc == HM_EDATA:
            return lo, hi, "degenerate", history
        new = lib_scores(l2, h2, penalty)
        assert new is not None
        if new[:2] == (A, B):
            return lo, hi, "converged", history
        for j in range(i):
            if history[j][3:5] == new[:2]:
                # the cycle is the iterations j .. i; j is taken with the levels that closed it
                members = [(new[:2], (l2, h2))] + [(h[3:5], (h[1], h[2])) for h in history[j + 1:]]
                best = min(members, key=lambda m: m[0])
                return best[1][0], best[1][1], "cycle", history
        if i + 1 == max_iter:
            return l2, h2, "max_iter", history
        lo, hi, scores, i = l2, h2, new, i + 1


def fit_chains(chains, ctx, lo, hi, penalty, max_gap, max_iter):
    return fit(lambda A, B, S: state_sums(chains, ctx, A, B, S, max_gap), lo, hi, penalty, max_iter)


def fit_tsv(fits, names=("CpG", "CHG", "CHH")):
    """<prefix>.domains.fit.tsv from per context None or fit()'s result"""
    text = ""
    for c, f in enumerate(fits):
        if f is None:
            continue
        for i, l, h, A, B, sums in f[3]:
            text += "\t".join([names[c], str(i), "%.17g" % l, "%.17g" % h, str(A), str(B)] + [str(x) for x in sums]) + "\n"
        text += "\t".join([names[c], f[2], "%.17g" % f[0], "%.17g" % f[1]]) + "\n"
    return text


# ---- the synthetic two-level track ---------------------------------------------------------------------------------------------------
TRACK_LEVELS = (0.05, 0.85)
TRACK_SEED = 20240


def synthetic_track(seed=TRACK_SEED, n_chains=3, rows_per_chain=8000):
    """-> (chains, lengths): per sequence hm_locus_t-like rows in the concatenated reference's coordinates, and the sequences'
    lengths.  CpG rows 1 .. 6 loci apart in alternating stretches of 200 .. 500 rows drawn at 0.05 and at 0.85, coverage
    Poisson(20) (at least 1); one locus in ten of another context between them; one gap of 3000 loci per chain (a break)."""
    rng = np.random.default_rng(seed)
    chains, lengths, base = [], [], 0
    for _ in range(n_chains):
        state = int(rng.integers(0, 2))
        levels = []
        while len(levels) < rows_per_chain:
            levels += [TRACK_LEVELS[state]] * int(rng.integers(200, 501))
            state ^= 1
        R = len(levels)
        step = rng.integers(1, 7, R)
        step[R // 2] = 3000
        gpos = base + np.cumsum(step)
        cov = np.maximum(rng.poisson(20, R), 1)
        p = rng.binomial(cov, np.array(levels))
        rows = np.zeros(R, LOCUS_DTYPE)
        rows["gpos"], rows["pcov"], rows["ncov"] = gpos, p, cov - p
        rows["motif"] = np.where(rng.random(R) < 0.1, rng.integers(1, 3, R), 0)
        length = int(gpos[-1] - base) + 1 + int(rng.integers(0, 50))
        chains.append(rows)
        lengths.append(length)
        base += length
    return chains, lengths
