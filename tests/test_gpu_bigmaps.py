"""The dense-trunk path on read groups whose maps cross 2^31 and 2^32 bytes (tests/bigmaps_cases.py).

trunk*_kernel -> edge*_kernel -> the tail kernels hand E1 .. E4 between them by map ROW number, and each turns a row into a byte
address with arithmetic of its own (RInfo.map_off and e4row are int32, edge2_kernel's LDS-DMA source is a 32-bit product widened
afterwards, the strip tail carries its keys as int32, ...).  Rows are 512 B (E1 .. E3) and 384 B (E4): a production-sized group -- up
to 16 Mi rows, CHH with a second view behind the first -- passes 2^31 B at rows 4 194 304 / 5 592 406 and 2^32 B at rows 8 388 608 /
11 184 811, and every other GPU test stays below a few hundred thousand rows.  Here two read lists are staged as ONE group each:
    A   5.75 M rows, two views, all contexts: both buffers pass 2^31 B in view 0 and 2^32 B in view 1   (37 GB of group buffers)
    B   11.3 M rows, one view, CpG + CHG:     both buffers pass 2^32 B in view 0                        (73 GB)
with a short probe read around every crossing (sites that gather from below it, from above it and across it).
Checks, per kernel variant: the calls and the logits are byte-identical to the same reads run in groups of 32 Ki rows (a configuration
test_gpu_logits.py holds against fp64), and the probes' calls hold the usual bar against the CPU oracle -- byte-identity alone would
pass if both runs were wrong in the same way.  A failing comparison names the first differing call's read, view, map row and its
distance to the nearest crossing, so that it points at a kernel."""
import time

import numpy as np
import pytest

import bigmaps_cases as BM
from test_gpu_parity import DP_TOL, _check_calls

pytestmark = pytest.mark.gpu

SMALL_GROUP = 32768          # rows per group of the reference runs
MAP_BYTES_PER_ROW = 3 * 2 * 512 + 2 * 384    # what run_trunk_path reserves per row of the largest group: E1 .. E3 and E4, two views each

# (id, precision, options on top of the defaults, cases)
CONFIGS = [
    ("default", 1, {}, "AB"),
    ("trunk_impl0", 1, {"trunk_impl": 0}, "AB"),
    ("trunk_impl1", 1, {"trunk_impl": 1}, "AB"),
    ("edge_impl0", 1, {"edge_impl": 0}, "AB"),
    ("tail_impl0", 1, {"tail_impl": 0}, "AB"),
    ("tail_impl1", 1, {"tail_impl": 1}, "AB"),
    ("tail_impl2", 1, {"tail_impl": 2}, "AB"),
    ("tail_impl3", 1, {"tail_impl": 3}, "A"),       # the strip tail is CHH's: case B has no CHH
    ("num_cu1", 1, {"num_cu": 1}, "AB"),            # workgroup runs that start and end on either side of a crossing
    ("num_cu7", 1, {"num_cu": 7}, "AB"),
    ("precision0", 0, {}, "AB"),                    # trunk_kernel_f32, edge_kernel_f32, tail_kernel
    ("precision2", 2, {}, "AB"),
]
PAIRS = [pytest.param(c, cfg[0], id=f"{c}-{cfg[0]}") for c in "AB" for cfg in CONFIGS if c in cfg[3]]
ORACLE_CHECKED = {"default": DP_TOL, "precision0": DP_TOL, "precision2": 1e-3}   # precision 2: the bar of its own test (test_gpu_parity.py)

_CASES, _REF, _ORACLE = {}, {}, {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = BM.case_a() if name == "A" else BM.case_b()
    return _CASES[name]


def _run(m, reads):
    """test_gpu_parity._run with the logits kept per context: (calls, [logits of CpG, CHG, CHH] in scan order)."""
    m.clear()
    assert m.submit_all(reads) == len(reads)
    m.upload()
    m.run()
    calls = m.fetch().copy()
    logits = [m.site_logits(c).copy() for c in range(3)]
    m.clear()
    return calls, logits


def _overwrite_the_maps(m, case):
    """The same reads in reverse order through the default kernels: every E4 row, and the E1 .. E3 rows that run's chains read, then hold
    another read's values.  The configurations share one engine and all compute the same maps: without this a kernel that stored a row
    to a wrong address would find the right one still filled in by the configuration before it."""
    m.clear()
    m.submit_all(case.reads[::-1])
    m.upload()
    m.run()
    m.sync()
    m.clear()


def _defaults():
    import torch
    return {"precision": 1, "trunk_impl": 3, "edge_impl": 1, "tail_impl": 3, "num_cu": torch.cuda.get_device_properties(0).multi_processor_count}


def _configure(m, precision, opts):
    for k, v in _defaults().items():     # precision first: tail_impl 0 / 2 are refused under precision 2
        m.set_option(k, v)
    for k, v in opts.items():
        m.set_option(k, v)
    m.set_option("precision", precision)


@pytest.fixture(scope="module")
def big(request):
    """One engine per case, shared by the case's configurations (options are switched between calls; the parametrisation gives the
    case module scope): a group's buffers are allocated once.  Never two large engines at once: pytest finishes case A's engine before
    it makes case B's."""
    import torch
    from hifimeth_amd import MethylationCaller
    case = _case(request.param)
    free, total = torch.cuda.mem_get_info(0)
    need = case.group_bytes_needed
    print(f"\ncase {case.name}: {len(case.reads)} reads, {case.view_rows} rows per view, group buffers {need / 1e9:.1f} GB; "
          f"device memory free {free / 1e9:.1f} GB of {total / 1e9:.1f} GB")
    if free < 1.5 * need:
        pytest.skip(f"case {case.name} needs {need / 1e9:.1f} GB of group buffers; {free / 1e9:.1f} GB free is below 1.5 x that")
    m = MethylationCaller(contexts=case.contexts, device=0, timing=True)
    m.set_option("trunk", 1)
    m.set_option("group_bases", case.view_rows)      # a group is closed once it HOLDS this many rows: the whole list is one group
    yield case, m
    m.close()


def _reference(case, precision):
    """The same reads in groups of 32 Ki rows, default kernels, per precision: computed once, never modified."""
    key = (case.name, precision)
    if key not in _REF:
        from hifimeth_amd import MethylationCaller
        with MethylationCaller(contexts=case.contexts, device=0, timing=True) as m:
            m.set_option("trunk", 1)
            m.set_option("precision", precision)
            m.set_option("group_bases", SMALL_GROUP)
            calls, logits = _run(m, case.reads)
            t = m.timing()
        assert min(t["trunk_launches"][c] for c in range(3) if case.ctx_mask >> c & 1) > case.view_rows // (2 * SMALL_GROUP)
        assert len(calls) > 0.04 * case.lens.sum()
        for a in [calls] + logits:
            a.setflags(write=False)
        _REF[key] = (calls, logits)
    return _REF[key]


def _first_difference(case, got, ref, got_lg, ref_lg):
    """None, or where the first differing call / logit lies in the plan."""
    if len(got) != len(ref):
        return f"{len(got)} calls for {len(ref)}"
    a, b = got.view(np.uint8).reshape(-1, got.dtype.itemsize), ref.view(np.uint8).reshape(-1, ref.dtype.itemsize)
    bad = np.nonzero((a != b).any(axis=1))[0]
    if len(bad):
        g, r = got[bad[0]], ref[bad[0]]
        rows = case.site_rows(ref["read_id"][bad], ref["strand"][bad], ref["qoff"][bad])
        return (f"{len(bad)} of {len(ref)} calls differ, map rows {int(rows.min())} .. {int(rows.max())}; the first: call {int(bad[0])} ctx {int(r['ctx'])} "
                f"p {float(g['p'])!r} for {float(r['p'])!r}: " + case.where(int(r["read_id"]), int(r["strand"]), int(r["qoff"])))
    for c in range(3):
        if got_lg[c].shape != ref_lg[c].shape:
            return f"context {c}: logits of {got_lg[c].shape} for {ref_lg[c].shape}"
        bad = np.nonzero((got_lg[c].view(np.uint32) != ref_lg[c].view(np.uint32)).any(axis=1))[0]
        if len(bad):
            sel = ref[ref["ctx"] == c]
            sel = sel[np.lexsort((sel["qoff"], sel["read_id"]))]      # scan order: (read, qoff)
            r = sel[bad[0]]
            return (f"context {c}: {len(bad)} of {len(sel)} sites' logits differ; the first: {got_lg[c][bad[0]].tolist()} for {ref_lg[c][bad[0]].tolist()}: "
                    + case.where(int(r["read_id"]), int(r["strand"]), int(r["qoff"])))
    return None


class _OracleOnce:
    """oracle.call_read with the probes' results kept: three precisions check the same reads."""

    def __init__(self, oracle):
        self._o = oracle

    def call_read(self, models, mask, rd):
        key = (id(rd), mask)
        if key not in _ORACLE:
            _ORACLE[key] = self._o.call_read(models, mask, rd)
        return _ORACLE[key]


def _probe_calls(case, calls):
    """The probes' calls, renumbered 0 .. for _check_calls."""
    reads, parts = [], []
    for k, i in enumerate(case.probes):
        sub = calls[calls["read_id"] == i].copy()
        sub["read_id"] = k
        parts.append(sub)
        reads.append(case.reads[i])
    return np.concatenate(parts), reads


def _check_probes(case, calls, oracle, oracle_models, tol):
    sub, reads = _probe_calls(case, calls)
    once = _OracleOnce(oracle)
    for k, i in enumerate(case.probes):        # the builder's own site lists first: a wrong count below would say nothing about the kernels
        q, strand, ctx = case.probe_sites(i)
        g = sub[sub["read_id"] == k]
        assert np.array_equal(g["qoff"], q) and np.array_equal(g["strand"], strand) and np.array_equal(g["ctx"], ctx), f"probe read {i}: site list"
    if tol == DP_TOL:
        n, nml, worst = _check_calls(sub, reads, once, oracle_models, case.ctx_mask)
    else:                                      # test_fp16_weight_mode_holds_its_bar...: same lists and order, |dp| <= 1e-3, ML bytes within 1
        n, worst = 0, 0.0
        for k, rd in enumerate(reads):
            want = once.call_read(oracle_models, case.ctx_mask, rd)
            g = sub[sub["read_id"] == k]
            order = np.lexsort((want["qoff"], want["strand"]))
            assert len(g) == len(order) and np.array_equal(g["qoff"], want["qoff"][order]) and np.array_equal(g["strand"], want["strand"][order])
            assert np.array_equal(g["ctx"], want["ctx"][order])
            dp = np.abs(g["p"] - want["p"][order])
            at = int(np.argmax(dp)) if len(dp) else 0
            assert float(dp.max(initial=0)) <= tol, (float(dp.max()), case.where(case.probes[k], int(g["strand"][at]), int(g["qoff"][at])))
            assert int(np.abs(g["scaled_prob"].astype(int) - want["ml"][order].astype(int)).max(initial=0)) <= 1
            worst, n = max(worst, float(dp.max(initial=0))), n + len(g)
    assert n == len(sub) > 300 * len(reads) * (1 if case.ctx_mask & 4 else 0.3)
    return n, worst


@pytest.mark.parametrize("big,cfg", PAIRS, indirect=["big"], scope="module")
def test_one_big_group_gives_the_calls_of_many_small_ones(big, cfg, oracle, oracle_models):
    case, m = big
    _, precision, opts, _ = next(c for c in CONFIGS if c[0] == cfg)
    t0 = time.perf_counter()
    ref, ref_lg = _reference(case, precision)
    t1 = time.perf_counter()
    _overwrite_the_maps(m, case)
    _configure(m, precision, opts)
    m.timing(reset=True)
    try:
        got, got_lg = _run(m, case.reads)
        t = m.timing(reset=True)
    finally:
        _configure(m, 1, {})
    t2 = time.perf_counter()
    # one group: one trunk launch per context, over every row of the plan; the buffers hold at least the plan's maps
    ctxs = [c for c in range(3) if case.ctx_mask >> c & 1]
    assert list(t["trunk_launches"]) == [1 if c in ctxs else 0 for c in range(3)], t["trunk_launches"]
    assert t["group_bases"] == case.view_rows
    tile_rows = case.view_rows - BM.TR_SLACK * len(case.reads)
    assert list(t["trunk_positions"]) == [tile_rows * (2 if c == 2 else 1) if c in ctxs else 0 for c in range(3)], (t["trunk_positions"], tile_rows)
    assert t["group_bytes"] >= MAP_BYTES_PER_ROW * case.view_rows, (t["group_bytes"], case.view_rows)
    for x in case.crossings:                   # the buffers really are that large: the crossing's byte offset lies inside its buffer
        assert x.row * BM.STRIDE[x.buffer] >= x.threshold and (x.row + 400) * BM.STRIDE[x.buffer] < 2 * case.view_rows * BM.STRIDE[x.buffer]
    diff = _first_difference(case, got, ref, got_lg, ref_lg)
    assert diff is None, f"case {case.name}, {cfg}: {diff}"
    assert sum(len(lg) for lg in got_lg) == len(got) and all(np.isfinite(lg).all() for lg in got_lg)
    note = ""
    if cfg in ORACLE_CHECKED:
        n, worst = _check_probes(case, got, oracle, oracle_models, ORACLE_CHECKED[cfg])
        note = f"; {len(case.probes)} probes, {n} sites against the oracle: max|dp| = {worst:.2e}"
    print(f"\ncase {case.name} {cfg}: {len(got)} calls, reference {t1 - t0:.2f} s, big group {t2 - t1:.2f} s, group_bytes {t['group_bytes'] / 1e9:.1f} GB{note}")
