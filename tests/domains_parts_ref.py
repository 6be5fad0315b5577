"""The three passes of hm_pileup_fetch_domains_part over one piece, restated sequentially in Python ints from include/hifimeth_hip.h:
a stand-in for the device in tests of the host chaining (hifimeth_amd.pileup.chain_domain_parts, stitch_domains).

A piece is the list of its rows (gpos, pcov, ncov), all of one context, ascending.  `piece(rows, ctx)` is the callable
chain_domain_parts takes.  Nothing here scans: d and the states are walked row by row, and the composite of pass S is folded from
the left with the rule of DESIGN.md section 10 (exact in c, or constant -- lo == hi -- once |c| >= 2^48)."""
import numpy as np

from domains_ref import AFTER_BREAK, BEFORE_BREAK, COV_CLAMP, DOMAIN_DTYPE, pooled

SUMMARY, CODES, SEGMENTS, KEEP = 0, 1, 2, 2
INF, CSAT, D_MAX = 1 << 62, 1 << 48, 1 << 46


def clamp(x, lo, hi):
    return min(max(x, lo), hi)


def compose(f, g):
    """g after f, both (c, lo, hi)"""
    c = f[0] + g[0]
    lo, hi = clamp(f[1] + g[0], g[1], g[2]), clamp(f[2] + g[0], g[1], g[2])
    if c >= CSAT:
        c, lo = CSAT, hi
    elif c <= -CSAT:
        c, hi = -CSAT, lo
    return c, lo, hi


def _forward(rows, carry, A, B, S, max_gap):
    """-> (d per row, S_t per row) from the carry-in"""
    e = [min(p, COV_CLAMP) * A + min(n, COV_CLAMP) * B for _g, p, n in rows]
    cost = [S if carry.get("has_prev") and rows[0][0] - carry["prev_gpos"] <= max_gap else 0]
    cost += [S if rows[t][0] - rows[t - 1][0] <= max_gap else 0 for t in range(1, len(rows))]
    d, x = [], carry["prev_d"] if carry.get("has_prev") else 0
    for t in range(len(rows)):
        x = clamp(x, -cost[t], cost[t]) + e[t]
        assert abs(x) <= D_MAX
        d.append(x)
    return d, cost, e


def run(rows, ctx, pass_, carry, A, B, S, max_gap):
    R = len(rows)
    if R == 0:
        return {"n_rows": 0, **({"segments": np.zeros(0, DOMAIN_DTYPE)} if pass_ == SEGMENTS else {})}
    out = {"n_rows": R, "first_gpos": rows[0][0], "last_gpos": rows[-1][0],
           "e_first": min(rows[0][1], COV_CLAMP) * A + min(rows[0][2], COV_CLAMP) * B}
    if pass_ == SUMMARY:
        f = (0, -INF, INF)
        for t in range(1, R):
            e = min(rows[t][1], COV_CLAMP) * A + min(rows[t][2], COV_CLAMP) * B
            s = S if rows[t][0] - rows[t - 1][0] <= max_gap else 0
            f = compose(f, (e, e - s, e + s))
        out["c"], out["lo"], out["hi"] = f
        return out
    if carry.get("has_prev"):
        assert abs(carry["prev_d"]) <= D_MAX and carry["prev_gpos"] < rows[0][0]
    d, cost, _e = _forward(rows, carry, A, B, S, max_gap)
    out["d_last"] = d[-1]
    code = [1 if d[t] > cost[t + 1] else 0 if d[t] < -cost[t + 1] else KEEP for t in range(R - 1)]   # from row t + 1 to row t
    if pass_ == CODES:
        out["back"] = next((c for c in code if c != KEEP), KEEP)
        return out
    z = [0] * R
    z[-1] = carry["last_state"] if carry.get("has_next") else 1 if d[-1] > 0 else 0
    assert z[-1] in (0, 1)
    for t in range(R - 2, -1, -1):
        z[t] = z[t + 1] if code[t] == KEEP else code[t]
    brk = [not carry.get("has_prev") or rows[0][0] - carry["prev_gpos"] > max_gap]
    brk += [rows[t][0] - rows[t - 1][0] > max_gap for t in range(1, R)]
    brk += [not carry.get("has_next") or carry["next_gpos"] - rows[-1][0] > max_gap]
    segs, i = [], 0
    while i < R:
        j = i
        while j + 1 < R and z[j + 1] == z[i] and not brk[j + 1]:
            j += 1
        g = np.zeros((), DOMAIN_DTYPE)
        P, N = sum(r[1] for r in rows[i:j + 1]), sum(r[2] for r in rows[i:j + 1])
        g["start"], g["end"], g["pcov"], g["ncov"] = rows[i][0], rows[j][0] + 1, P, N
        g["n_loci"], g["state"], g["motif"] = j - i + 1, z[i], ctx
        g["flags"] = (AFTER_BREAK if brk[i] else 0) | (BEFORE_BREAK if brk[j + 1] else 0)
        g["level"], g["score"] = pooled(P, N, A, B)
        segs.append(g)
        i = j + 1
    out["segments"] = np.array(segs, DOMAIN_DTYPE)
    return out


def piece(rows, ctx):
    rows = [(int(g), int(p), int(n)) for g, p, n in rows]
    return lambda pass_, carry, A, B, S, max_gap: run(rows, ctx, pass_, carry, A, B, S, max_gap)
