"""tests/bigmaps_cases.py, the case builder of tests/test_gpu_bigmaps.py, checked without a GPU: the plan's arithmetic at a stride
scaled down by 256 (crossings at ~22 k and ~44 k rows instead of 5.6 M and 11.2 M), the probes counted, the full-scale plans without
their reads, and the builder's site lists against the oracle's."""
import numpy as np
import pytest

import bigmaps_cases as BM

SCALE = 256


@pytest.fixture(scope="module", params=["a", "b"])
def small(request):
    return BM.case_a(SCALE) if request.param == "a" else BM.case_b(SCALE)


def _check_plan(case, thresholds):
    # rows and map_off as add_read_tiles counts them, from the lengths alone
    off = 0
    for i, L in enumerate(case.lens):
        assert case.map_off[i] == off
        off += (int(L) + 400 + 111) // 112 * 112 + 32
    assert off == case.view_rows and case.view_rows % 16 == 0
    assert sorted(x.threshold for x in case.crossings) == sorted(thresholds)
    for x in case.crossings:
        stride = BM.STRIDE[x.buffer]
        assert (x.row - 1) * stride < x.threshold <= x.row * stride          # the first row whose offset no longer fits below the threshold
        assert x.view < case.n_views and x.view * case.view_rows <= x.row < (x.view + 1) * case.view_rows
        # the crossing lies >= 400 rows inside the probe's own region in that view
        first = x.view * case.view_rows + int(case.map_off[x.read])
        assert x.read in case.probe_fwd and x.rel == x.row - first
        assert 400 <= x.rel <= BM.read_rows(int(case.lens[x.read])) - 400
        # view position 0 of the probe is row first + 200: the crossing is a view position of the probe or of its pads
        assert x.row == x.view * case.view_rows + case.map_off[x.read] + 200 + (x.rel - 200)
    assert len({x.read for x in case.crossings}) == len(case.crossings)      # a probe of its own each


def test_scaled_plan_arithmetic(small):
    t31, t32 = BM.T31 // SCALE, BM.T32 // SCALE
    _check_plan(small, [t31, t31, t32, t32] if small.name == "a" else [t32, t32])
    assert len(small.reads) == len(small.lens) and all(r.l_qseq == L for r, L in zip(small.reads, small.lens))
    assert all(r.has_kinetics() and r.l_qseq >= 1000 for r in small.reads)
    assert min(small.lens[i] for i in small.probes) >= 2000 and max(small.lens[i] for i in small.probes) <= 3000
    probes = [small.reads[i] for i in small.probes]
    assert sum(r.fi.dtype == np.uint16 for r in probes) == 1 and sum(r.flag & 16 != 0 for r in probes) == 1


def test_every_crossing_has_sites_on_both_sides_and_across(small):
    for x in small.crossings:
        below, above, across = small.sides(x)
        assert below >= 20 and above >= 20 and across >= 5, (x.label(), below, above, across)
        # counted again the long way for the E4 buffer: the 23 gather rows of every site of the crossing's view
        if x.buffer == "E4":
            q, strand, _ = small.probe_sites(x.read)
            L = int(small.lens[x.read])
            n = [0, 0, 0]
            for qq in q[strand == x.view]:
                offv = L - 1 - int(qq) if x.view else int(qq)
                rows = [x.view * small.view_rows + int(small.map_off[x.read]) + 200 + offv - 215 + 16 * s for s in range(1, 24)]
                n[0 if rows[-1] < x.row else 1 if rows[0] >= x.row else 2] += 1
            assert n == [below, above, across]


def test_full_scale_plans():
    """The plans the GPU test stages, without their reads: the six crossings, the engine's 2^27-row cap, map_off in int32."""
    a, b = BM.case_a(synth=False), BM.case_b(synth=False)
    assert a.reads is None and b.reads is None
    _check_plan(a, [BM.T31, BM.T31, BM.T32, BM.T32])
    _check_plan(b, [BM.T32, BM.T32])
    assert sorted((x.buffer, x.threshold, x.view, x.row) for x in a.crossings) == [
        ("E1..E3", BM.T31, 0, 4_194_304), ("E1..E3", BM.T32, 1, 8_388_608), ("E4", BM.T31, 0, 5_592_406), ("E4", BM.T32, 1, 11_184_811)]
    assert sorted((x.buffer, x.threshold, x.view, x.row) for x in b.crossings) == [("E1..E3", BM.T32, 0, 8_388_608), ("E4", BM.T32, 0, 11_184_811)]
    assert 5_750_000 <= a.view_rows < 5_760_000 and 11_300_000 <= b.view_rows < 11_310_000
    assert (a.ctx_mask, a.n_views, b.ctx_mask, b.n_views) == (7, 2, 3, 1)
    for c in (a, b):
        assert 2 * c.view_rows < BM.MAX_GROUP_ROWS_X2
        assert int(c.map_off.max()) + 2 * c.view_rows < 2 ** 31          # map_off, and every row number built on it, fits int32
        fill = np.delete(c.lens, c.probes)
        assert fill.min() >= 15000 and fill.max() <= 25000
        for x in c.crossings:
            below, above, across = c.sides(x)
            assert below >= 20 and above >= 20 and across >= 5, (c.name, x.label(), below, above, across)
    # at least one read of margin behind the last crossing of either view
    assert 2 * a.view_rows - 11_184_811 > 25_400 and a.view_rows - 5_592_406 > 25_400 and b.view_rows - 11_184_811 > 25_400


def test_probe_sites_are_the_oracles(small, oracle, oracle_models):
    """oracle.call_read on a probe returns the sites the builder counted, in the engine's (strand, qoff) order once sorted so."""
    for i in small.probes:
        rd = small.reads[i]
        assert oracle.decode(rd) == bytes(np.frombuffer(b"ACGT", np.uint8)[small.probe_fwd[i]])
        if i != small.probes[0]:
            continue                           # the CNN of one probe per case is enough: the others' lists are checked by the scanner
        want = oracle.call_read(oracle_models, small.ctx_mask, rd)
        order = np.lexsort((want["qoff"], want["strand"]))
        q, strand, ctx = small.probe_sites(i)
        assert len(q) > 100
        assert np.array_equal(q, want["qoff"][order]) and np.array_equal(strand, want["strand"][order]) and np.array_equal(ctx, want["ctx"][order])
    for i in small.probes[1:]:
        fwd = oracle.decode(small.reads[i])
        q, strand, ctx = small.probe_sites(i)
        for c in range(3):
            if small.ctx_mask >> c & 1:
                assert np.array_equal(np.sort(q[ctx == c]), np.sort(oracle.scan(fwd, c))), (i, c)


def test_where_names_the_nearest_crossing(small):
    x = small.crossings[0]
    q, strand, _ = small.probe_sites(x.read)
    q = q[strand == x.view]
    row = small.site_rows(x.read, x.view, q)
    k = int(np.argmin(np.abs(row - x.row)))
    text = small.where(x.read, x.view, int(q[k]))
    assert f"read {x.read} (probe" in text and f"view {x.view}" in text and f"map row {int(row[k])}" in text
    assert f"{int(row[k]) - x.row:+d} rows from the crossing {x.label()}" in text
