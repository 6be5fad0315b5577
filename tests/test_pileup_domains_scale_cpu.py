"""The planes of domains_scale_cases.py at a small scan unit, without a GPU: from domains_ref alone, that they hold what the
builder claims, and the shortcut test_gpu_pileup_domains_scale.py relies on -- the reference over the whole range W, cut at the
breaks, IS the reference over each break-delimited range, so one reference pass serves all of them on the device."""
import numpy as np
import pytest

from domains_fit_ref import LOCUS_DTYPE, state_sums
from domains_ref import AFTER_BREAK, BEFORE_BREAK, ctx_rows, domains, emissions, switch_costs
from domains_scale_cases import BIG, TIE, build, slice_edges

S = TIE[2]


def _loci(host, lo, hi):
    """the hm_locus_t rows of the covered loci of [lo, hi)"""
    p, n, key = (x[lo:hi] for x in host)
    on = np.nonzero((p | n) != 0)[0]
    rows = np.zeros(len(on), LOCUS_DTYPE)
    rows["gpos"], rows["pcov"], rows["ncov"], rows["motif"] = on + lo, p[on], n[on], key[on] & 3
    return rows


def _d(rows, A, B, S, max_gap):
    """-> (d_t, S_t) per row: delta_t(1) - delta_t(0) by its recurrence (as in test_gpu_pileup_domains.py)"""
    e, cost = emissions(rows["pcov"], rows["ncov"], A, B), switch_costs(rows["gpos"], S, max_gap)
    d, x = [], 0
    for t in range(len(e)):
        x = min(max(x, -cost[t]), cost[t]) + e[t]
        d.append(x)
    return d, cost


@pytest.fixture(scope="module", params=[16, 32])
def case(request):
    host, info = build(request.param)
    loci = _loci(host, 0, info["n"])
    segs, R = domains(loci, 0, *TIE)
    rows = ctx_rows(loci, 0)
    z = np.repeat(segs["state"], segs["n_loci"]).astype(np.int64)
    d, cost = _d(rows, *TIE)
    return host, info, loci, segs, R, rows, z, d, cost


def test_row_counts_and_carry_geometry(case):
    host, info, loci, _segs, R, rows, _z, _d_, _cost = case
    u, rng = info["u"], info["ranges"]
    assert R == info["R"] == 2 * u * u + 3 * u + 5 == len(rows) and np.array_equal(rows["gpos"], info["row_locus"])
    want = {"A": u * u, "B": u * u + 1, "C": u * u + 3 * u + 4, "W": R}
    for name, (lo, hi, first, n) in rng.items():
        assert n == want[name] == len(ctx_rows(_loci(host, lo, hi), 0)), name
        assert int(info["row_locus"][first]) >= lo and (first == 0 or int(info["row_locus"][first - 1]) < lo)
    nagg = {name: -(-n // u) for name, (_lo, _hi, _f, n) in rng.items()}
    per = {name: -(-a // u) for name, a in nagg.items()}
    assert nagg == {"A": u, "B": u + 1, "C": u + 4, "W": 2 * u + 4} and per == {"A": 1, "B": 2, "C": 2, "W": 3}
    assert -(-(nagg["A"] + 1) // u) == 2                      # the reduce-only passes' extra slot: a slice of its own, in thread u / 2
    assert rng["B"][3] - (nagg["B"] - 1) * u == 1 and (nagg["B"] - 1) // 2 == u // 2    # B: the last workgroup one row, thread u / 2 one aggregate
    assert (nagg["W"] - 1) // 3 == (2 * u + 3) // 3 < u - 1   # W: the last aggregates' thread; later threads hold none
    assert rng["C"][0] % 4 == 1 and rng["C"][0] % 4096 != 0
    # row, locus and CHG row counts all differ; the other context has no break
    chg = ctx_rows(loci, 1)
    assert len(chg) == R + 4 and set(np.diff(chg["gpos"]).tolist()) == {4} and len(ctx_rows(loci, 2)) == 0
    assert len(loci) == 2 * R + 4 + 1 and info["n"] == 4 * (R + 4)


def test_two_breaks_and_the_one_row_segment(case):
    _host, info, _loci_, segs, _R, rows, _z, d, cost = case
    u, g = info["u"], info["row_locus"]
    gaps = np.diff(g)
    assert set(gaps.tolist()) == {4, 12} and np.flatnonzero(gaps == 12).tolist() == [u * u - 1, u * u] and TIE[3] < 12
    assert cost[u * u] == 0 and cost[u * u + 1] == 0 and sum(1 for c in cost if c == 0) == 3
    one = segs[segs["start"] == g[u * u]]
    assert len(one) == 1 and int(one[0]["n_loci"]) == 1 and int(one[0]["flags"]) == AFTER_BREAK | BEFORE_BREAK and int(one[0]["state"]) == 0
    assert (segs["flags"] != 0).sum() == 5                    # W's first and last segment, the one-row segment and its two neighbours
    # neither break is passed with a tie: the rows in front of them do not take their state from behind the break
    assert d[u * u - 1] > 0 and d[u * u] < 0
    assert len(segs) > info["R"] // 200 and {int(s) for s in segs["state"]} == {0, 1}


def test_no_clamp_stretches(case):
    _host, info, _loci_, segs, _R, rows, z, d, cost = case
    u, g = info["u"], info["row_locus"]
    assert [name for _a, _b, name, _d_in in info["stretches"]] == ["A", "A", "C", "C"]
    behind, inside = set(), set()
    for a, b, name, d_in in info["stretches"]:
        lo, hi, first, n = info["ranges"][name]
        assert b - a + 1 >= 7 * u and first <= a - 4 and b + 5 < first + n
        e = emissions(rows["pcov"][a:b + 1], rows["ncov"][a:b + 1], *TIE[:2])
        assert set(e) == {4, -4} and sum(1 for x, y in zip(e, e[1:]) if x == y) > len(e) // 20      # alternating, some signs repeated
        assert d[a - 1] == d_in and all(abs(d[t - 1]) <= cost[t] == S for t in range(a, b + 2))      # no clamp acts, up to the row behind
        assert len({d[t] for t in range(a + u, b, u)}) > 1    # d differs between workgroup edges
        assert sum(1 for s in segs if s["start"] <= g[a] and s["end"] > g[b]) == 1
        # the row behind the stretch decides its state, by d = +-(S + 4) exactly, against the rows that follow
        assert d[b + 1] == (S + 4 if d_in else -S - 4)
        assert set(z[a:b + 2].tolist()) == {1 if d_in else 0} and set(z[b + 2:b + 6].tolist()) == {0 if d_in else 1}
        inside.add(int(z[a]))
        behind.add(int(z[b + 2]))
        # carry slices: forward from the range's first row, backward from its end; per = 2 in A under the reduce-only passes, in B
        # and in C, per = 3 in W
        R = info["R"]
        origins = [(first, 2 * u), (first + n, 2 * u), (0, 3 * u), (R, 3 * u)] + ([(u * u + 1, 2 * u)] if name == "A" else [])
        for origin, width in origins:
            edges = slice_edges(a, b, origin, width)
            assert len(edges) >= 2 and len([x for x in edges if a < x <= b]) >= 2, (a, b, origin, width)
    assert inside == {0, 1} and behind == {0, 1}
    assert {d_in for _a, _b, _n, d_in in info["stretches"]} == {0, 4}


def test_counters_beyond_the_clamp_and_the_negative_one(case):
    host, info, _loci_, segs, _R, rows, _z, _d_, _cost = case
    p, n, _key = host
    assert int(p.max()) == BIG and int(n.max()) == 2 * BIG and (p < 0).sum() == 1 and (n < 0).sum() == 0
    hi_seg = segs[(segs["start"] <= info["negative"]) & (segs["end"] > info["negative"])]
    assert len(hi_seg) == 1 and int(hi_seg[0]["state"]) == 1 and int(hi_seg[0]["pcov"]) > BIG and int(hi_seg[0]["n_loci"]) >= 7
    assert int(p[info["negative"]]) == -1 and info["negative"] % 4 == 2
    lo_seg = segs[segs["ncov"] > 2 * BIG]
    assert len(lo_seg) == 1 and int(lo_seg[0]["state"]) == 0 and int(lo_seg[0]["n_loci"]) >= 7


def _sums(rows, z):
    out = [0] * 6
    for s in (0, 1):
        m = z == s
        out[3 * s:3 * s + 3] = int(rows["pcov"][m].astype(np.int64).sum()), int(rows["ncov"][m].astype(np.int64).sum()), int(m.sum())
    return tuple(out)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_reference_of_a_range_is_a_slice_of_the_whole(case, name):
    host, info, _loci_, segs, _R, rows, z, _d_, _cost = case
    lo, hi, first, n = info["ranges"][name]
    alone, R = domains(_loci(host, lo, hi), 0, *TIE)
    part = segs[(segs["start"] >= lo) & (segs["end"] <= hi)]
    assert R == n and len(alone) == len(part) > 3 and alone.tobytes() == part.tobytes()
    assert int(part["n_loci"].sum()) == n                     # no segment of W lies across the range's ends
    want = state_sums([_loci(host, lo, hi)], 0, *TIE)
    assert _sums(rows[first:first + n], z[first:first + n]) == want and want[2] > 0 and want[5] > 0
