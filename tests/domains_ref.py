"""Methylation domains (`pileup -D`), restated in plain numpy / Python ints from include/hifimeth_hip.h: what
hm_pileup_fetch_domains must return, given the hm_locus_t rows of the range.

Per context c and range: ROWS = the loci with pcov >= 0, ncov >= 0, pcov + ncov > 0 and min(motif, 2) == c, ascending.  Two states,
0 = low and 1 = high.  Row t scores e_t = min(pcov, 2^20 - 1) * A + min(ncov, 2^20 - 1) * B in state 1 and 0 in state 0; a change
of state between rows t-1 and t costs S_t = S when gpos_t - gpos_{t-1} <= max_gap and 0 (a break) otherwise.  The path is the one
of textbook Viterbi with both delta kept (this file never forms their difference, which is how the device computes it) and
back-pointers that move only on a strict gain.  A SEGMENT is a maximal run of rows with one state and no break inside."""
import numpy as np

DOMAIN_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("pcov", "<i8"), ("ncov", "<i8"), ("n_loci", "<i4"), ("state", "<u4"),
                         ("motif", "<u4"), ("flags", "<u4"), ("level", "<f8"), ("score", "<f8")])
AFTER_BREAK, BEFORE_BREAK = 1, 2
COV_CLAMP = (1 << 20) - 1
W_MAX = 1 << 24


def ctx_rows(loci, ctx):
    """the rows of context ctx among hm_locus_t rows (a row whose counter is negative is none)"""
    p, n = loci["pcov"].astype(np.int64), loci["ncov"].astype(np.int64)
    return loci[(p >= 0) & (n >= 0) & (p + n > 0) & (np.minimum(loci["motif"], 2) == ctx)]


def emissions(pcov, ncov, A, B):
    return [min(int(p), COV_CLAMP) * A + min(int(n), COV_CLAMP) * B for p, n in zip(pcov, ncov)]


def switch_costs(gpos, S, max_gap):
    """S_t for every row; S_0 = 0"""
    return [0] + [S if int(gpos[t]) - int(gpos[t - 1]) <= max_gap else 0 for t in range(1, len(gpos))]


def path_score(z, e, cost):
    return sum(e[t] for t in range(len(z)) if z[t]) - sum(cost[t] for t in range(1, len(z)) if z[t] != z[t - 1])


def viterbi(e, cost):
    """-> the states z_0 .. z_{R-1}: sequential Viterbi from delta_{-1} = (0, 0), Python ints"""
    R = len(e)
    if R == 0:
        return []
    d0, d1 = 0, 0
    back = []                                                 # back[t] = (previous state into 0, previous state into 1)
    for t in range(R):
        into0 = 1 if d1 - cost[t] > d0 else 0
        into1 = 0 if d0 - cost[t] > d1 else 1
        back.append((into0, into1))
        n0 = d1 - cost[t] if into0 else d0
        n1 = (d0 - cost[t] if into1 == 0 else d1) + e[t]
        d0, d1 = n0, n1
    z = [0] * R
    z[R - 1] = 1 if d1 > d0 else 0
    for t in range(R - 1, 0, -1):
        z[t - 1] = back[t][z[t]]
    return z


def pooled(P, N, A, B):
    """level and score as the host computes them: every operation rounded once in fp64"""
    P, N = np.float64(int(P)), np.float64(int(N))
    return np.float64(100.0) * P / (P + N), (P * np.float64(A) + N * np.float64(B)) / np.float64(65536.0)


def domains(loci, ctx, A, B, S, max_gap):
    """-> (segments as DOMAIN_DTYPE, R) for hm_locus_t-like rows (fields gpos, pcov, ncov, motif) of one range"""
    assert 0 < A <= W_MAX and -W_MAX <= B < 0 and 0 <= S <= W_MAX and max_gap >= 1 and ctx in (0, 1, 2)
    r = ctx_rows(loci, ctx)
    R = len(r)
    gpos = [int(g) for g in r["gpos"]]
    cost = switch_costs(gpos, S, max_gap)
    z = viterbi(emissions(r["pcov"], r["ncov"], A, B), cost)
    brk = [True] + [gpos[t] - gpos[t - 1] > max_gap for t in range(1, R)] + [True]   # brk[t]: a break before row t; brk[R] ends the rows
    out = []
    i = 0
    while i < R:
        j = i
        while j + 1 < R and z[j + 1] == z[i] and not brk[j + 1]:
            j += 1
        g = np.zeros((), DOMAIN_DTYPE)
        P, N = int(r["pcov"][i:j + 1].astype(np.int64).sum()), int(r["ncov"][i:j + 1].astype(np.int64).sum())
        g["start"], g["end"], g["pcov"], g["ncov"] = gpos[i], gpos[j] + 1, P, N
        g["n_loci"], g["state"], g["motif"] = j - i + 1, z[i], ctx
        g["flags"] = (AFTER_BREAK if brk[i] else 0) | (BEFORE_BREAK if brk[j + 1] else 0)
        g["level"], g["score"] = pooled(P, N, A, B)
        out.append(g)
        i = j + 1
    return (np.array(out, DOMAIN_DTYPE) if out else np.zeros(0, DOMAIN_DTYPE)), R
