"""A cold engine on batches that outgrow its grow-only buffers (growth_cases.py): every slab of a ladder through ONE fresh engine -- pipelined,
synchronously, from three threads, with options changed in between -- must give, byte for byte, what a fresh engine that sees only that slab
gives (`cold`); the CPU oracle and the fp64 reference check a part of the same results independently.

What is observed of the growth: hm_get_timing's group_bytes (the read group's scratch: maps, edge rows, tail hand-off buffers) for the dense
trunk, and for the per-site path the number of front / tail launch pairs per context, ceil(bases / window): the window is not reported itself
(the timing field window_sites counts the sites of the hm_windows seam, not the launch window), but a 4.2 Mbase slab takes 48 pairs per context
with its own window and 65 with the default one."""
import os
import threading

import numpy as np
import pytest

import growth_cases as G
from cnn64 import CNN64, bar, reference_sites, site_errors, strata
from conftest import WEIGHTS
from test_gpu_parity import DP_TOL

pytestmark = pytest.mark.gpu

NAMES = ("CpG", "CHG", "CHH")
TAIL_SLICE_BOUND = 2 ** 63 - 1      # "tail_slice" has a lower bound (16) only: the largest value the ABI's int64 carries
LADDERS = {"dense": G.ladder, "dense4": lambda: G.ladder()[:4], "sparse": G.ladder_sparse}
CONFIGS = {
    "default": {},
    "trunk1": {"trunk": 1},
    "trunk3-groups": {"trunk": 1, "trunk_impl": 3, "group_bases": 32768, "num_cu": 7},
    "tail2-wide": {"trunk": 1, "tail_impl": 2, "tail_slice": TAIL_SLICE_BOUND},
    "p0-trunk1": {"precision": 0, "trunk": 1},
    "p1-trunk0": {"precision": 1, "trunk": 0},
    "p0-trunk0": {"precision": 0, "trunk": 0},
    # cold references of test_options_changed_between_batches only
    "trunk3-groups-allcu": {"trunk": 1, "trunk_impl": 3, "group_bases": 32768},
    "trunk3-cu1": {"trunk": 1, "trunk_impl": 3, "num_cu": 1},
}
CASES = [("default", "dense"), ("trunk1", "dense"), ("trunk3-groups", "dense"), ("tail2-wide", "dense"), ("p0-trunk1", "dense"),
         ("p1-trunk0", "sparse"), ("p1-trunk0", "dense4"), ("p0-trunk0", "sparse")]
CASE_IDS = [f"{c}-{l}" for c, l in CASES]


def _engine(cfg, cold=False):
    """A fresh engine with a configuration's options.  `default` sets none -- but its COLD engines get slab 0's trunk_mask, so that the
    reference does not depend on which slab an engine saw first (growth_cases: every slab gives the same mask anyway)."""
    from hifimeth_amd import MethylationCaller
    from hifimeth_amd.caller import ReadBlock, trunk_mask_for_reads
    m = MethylationCaller(device=0, timing=True)
    for k, v in CONFIGS[cfg].items():
        m.set_option(k, v)
    if cfg == "default" and cold:
        m.set_option("trunk_mask", trunk_mask_for_reads(ReadBlock(G.ladder()[0]), 7))
    return m


def _pairs(t):
    """Front / tail launch pairs of the timed per-site launches: a pair whose window of the site list turned out empty counts twice in
    empty_launches (collect_timing)."""
    assert t["empty_launches"] % 2 == 0
    return sum(t["front_launches"]) + t["empty_launches"] // 2


def _run(m, slab, scan=False):
    """One slab through the synchronous calls: calls, per-context logits (hm_site_logits) and, on request, the site lists."""
    m.clear()
    m.submit_all(slab)
    m.upload()
    m.run()
    out = {"calls": m.fetch().copy(), "logits": [m.site_logits(c).copy() for c in range(3)]}
    if scan:
        out["scan"] = [m.scan_sites(c) for c in range(3)]
    m.clear()
    t = m.timing(reset=True)
    out["group_bytes"], out["pairs"] = t["group_bytes"], _pairs(t)
    return out


_COLD, _PIPED, _SYNC = {}, {}, {}


def cold(cfg, lad, k):
    """want[k]: calls and site_logits of a fresh engine that sees only slab k of the ladder, then closes.  Memoised per (config, slab) --
    dense4 is a prefix of dense."""
    lad = "dense" if lad == "dense4" else lad
    key = (cfg, lad, k)
    if key not in _COLD:
        m = _engine(cfg, cold=True)
        try:
            _COLD[key] = _run(m, LADDERS[lad]()[k])
        finally:
            m.close()
    return _COLD[key]


def _counts(calls):
    return [int((calls["ctx"] == c).sum()) for c in range(3)]


def piped(cfg, lad):
    """The ladder through m.stream() on one fresh engine: per slab the calls and the batch's per-context site counts; the timing after it."""
    if (cfg, lad) not in _PIPED:
        got = []
        m = _engine(cfg)
        try:
            total = m.stream(LADDERS[lad](), on_batch=lambda k, b, calls: got.append((calls.copy(), [b.num_sites(c) for c in range(4)])))
            t = m.timing()
        finally:
            m.close()
        assert total == sum(len(c) for c, _ in got)
        _PIPED[(cfg, lad)] = (got, t)
    return _PIPED[(cfg, lad)]


def synced(cfg, lad):
    """The ladder slab by slab through the synchronous calls of one fresh engine (slot 0, nothing overlaps)."""
    if (cfg, lad) not in _SYNC:
        m = _engine(cfg)
        try:
            _SYNC[(cfg, lad)] = [_run(m, slab, scan=(cfg == "default")) for slab in LADDERS[lad]()]
        finally:
            m.close()
    return _SYNC[(cfg, lad)]


def _same_calls(got, want, what):
    assert len(want) > 0 and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():     # locate it: which field, which context, how far into the list
        for f in got.dtype.names:
            bad = np.nonzero(got[f] != want[f])[0]
            if len(bad):
                raise AssertionError(f"{what}: {len(bad)} of {len(got)} calls differ in '{f}', first at {bad[0]}, last at {bad[-1]}, contexts "
                                     f"{np.unique(want['ctx'][bad]).tolist()}, max |dp| {np.abs(got['p'] - want['p']).max():.3e}")
        raise AssertionError(f"{what}: calls differ in padding bytes only")


@pytest.mark.parametrize("cfg,lad", CASES, ids=CASE_IDS)
def test_pipeline_on_a_cold_engine_matches_cold_engines(cfg, lad):
    """m.stream(ladder) on a fresh engine: slab k + 1 is staged, uploaded and queued -- its larger group scratch reserved -- without a wait
    for slab k (whether slab k is really still running then depends on host timing; the test does not force it).  Every slab's calls and per-context site counts are the cold engine's, and the group scratch (dense trunk) or the launch window
    (per-site path) really grew."""
    slabs = LADDERS[lad]()
    got, t = piped(cfg, lad)
    assert len(got) == len(slabs)
    for k, (calls, ns) in enumerate(got):
        want = cold(cfg, lad, k)["calls"]
        _same_calls(calls, want, f"{cfg} {lad} slab {k}")
        assert ns[3] == len(want) and ns[:3] == _counts(want), (k, ns)
    print(f"\n{cfg} {lad}: piped group_bytes {t['group_bytes']}, cold slab 0 {cold(cfg, lad, 0)['group_bytes']}, launch pairs {_pairs(t)}")
    if CONFIGS[cfg].get("trunk") == 0:
        assert t["group_bytes"] == 0 and sum(t["trunk_launches"]) == 0
        assert _pairs(t) == 3 * sum(G.launch_pairs(G.staged_bases(s)) for s in slabs)
    else:
        assert sum(t["front_launches"]) == 0 and all(n > 0 for n in t["trunk_launches"])
        assert t["group_bytes"] > cold(cfg, lad, 0)["group_bytes"] > 0


@pytest.mark.parametrize("cfg,lad", CASES, ids=CASE_IDS)
def test_synchronous_ladder_grows_step_by_step(cfg, lad):
    """m.call(slab) up the ladder on one fresh engine: calls and site_logits(c) are the cold engine's byte for byte.  Dense trunk: group_bytes
    rises strictly at each growth step and stays across the shrink and the step inside the head-room.  Per-site path: each slab takes
    3 x ceil(bases / window) launch pairs, the window being the batch's own (48 pairs per context for the top slab of the sparse ladder;
    the default window would need 65)."""
    slabs = LADDERS[lad]()
    runs = synced(cfg, lad)
    for k, r in enumerate(runs):
        want = cold(cfg, lad, k)
        _same_calls(r["calls"], want["calls"], f"{cfg} {lad} slab {k}")
        for c in range(3):
            assert r["logits"][c].shape == (_counts(want["calls"])[c], 2)
            assert r["logits"][c].tobytes() == want["logits"][c].tobytes(), (cfg, lad, k, NAMES[c])
    gb = [r["group_bytes"] for r in runs]
    pairs = [r["pairs"] for r in runs]
    print(f"\n{cfg} {lad}: group_bytes {gb} launch pairs {pairs}")
    if CONFIGS[cfg].get("trunk") == 0:
        assert gb == [0] * len(runs)
        assert pairs == [3 * G.launch_pairs(G.staged_bases(s)) for s in slabs]
        if lad == "sparse":
            assert pairs[2] == 3 * 48 and G.launch_window(G.staged_bases(slabs[2])) > G.DEFAULT_WINDOW
    else:
        assert pairs == [0] * len(runs) and gb[0] > 0
        for k in range(1, len(runs)):
            assert (gb[k] > gb[k - 1]) if k in G.GROWTH_STEPS else (gb[k] == gb[k - 1]), (k, gb)
        assert gb[0] == cold(cfg, lad, 0)["group_bytes"]


_ORACLE = {}


def _oracle_calls(oracle, oracle_models, lad, k, i):
    lad = "dense" if lad == "dense4" else lad
    if (lad, k, i) not in _ORACLE:
        want = oracle.call_read(oracle_models, 7, LADDERS[lad]()[k][i])
        order = np.lexsort((want["qoff"], want["strand"]))     # (strand, qoff): FWD calls then REV calls
        _ORACLE[(lad, k, i)] = {f: want[f][order] for f in ("qoff", "strand", "ctx", "p", "ml")}
    return _ORACLE[(lad, k, i)]


def _check_reads(calls, lad, k, ids, oracle, oracle_models):
    """test_gpu_parity._check_calls read by read, for the reads `ids` of a slab: identical site lists, |dML| <= 1; returns sites, worst |dp|."""
    slab = LADDERS[lad]()[k]
    n, worst = 0, 0.0
    for i in ids:
        got = calls[calls["read_id"] == i]
        if not G.staged(slab[i]):
            assert len(got) == 0
            continue
        want = _oracle_calls(oracle, oracle_models, lad, k, i)
        assert len(got) == len(want["qoff"]) > 0, (lad, k, i)
        for f in ("qoff", "strand", "ctx"):
            assert np.array_equal(got[f], want[f]), (lad, k, i, f)
        assert np.abs(got["scaled_prob"].astype(int) - want["ml"].astype(int)).max() <= 1
        worst = max(worst, float(np.abs(got["p"] - want["p"]).max()))
        n += len(got)
    return n, worst


ORACLE_CASES = [(cfg, lad, k) for cfg, lad in (("default", "dense"), ("tail2-wide", "dense"), ("p1-trunk0", "sparse"), ("p1-trunk0", "dense4"))
                for k in range({"dense": 6, "dense4": 4, "sparse": 4}[lad])]


@pytest.mark.parametrize("cfg,lad,k", ORACLE_CASES, ids=[f"{c}-{l}-slab{k}" for c, l, k in ORACLE_CASES])
def test_growth_ladder_against_the_oracle(oracle, oracle_models, cfg, lad, k):
    """The independent reference: the PIPELINED results of default, tail2-wide and p1-trunk0 against the CPU oracle -- every read of the slabs
    of at most 16 k bases (the 6 k slab and the 12 k shrink; 8 k and 10 k of the sparse ladder), the first and the last read of every other
    slab: |dp| <= 1e-4, |dML| <= 1, identical site lists.  One case per slab; the oracle's calls of a read are computed once per module."""
    got, _t = piped(cfg, lad)
    slab = LADDERS[lad]()[k]
    ids = range(len(slab)) if G.staged_bases(slab) <= 16000 else (0, len(slab) - 1)
    n, worst = _check_reads(got[k][0], lad, k, ids, oracle, oracle_models)
    print(f"\n{cfg} {lad} slab {k}: {n} sites against the oracle, worst |dp| {worst:.2e}")
    assert n > 100, (cfg, lad, k, n)
    assert worst <= DP_TOL, (cfg, lad, k, worst)


def test_growth_ladder_probe_logits_against_fp64(oracle, oracle_models):
    """The second half of the independent reference: the logits of every slab's first and last read under the default options (from the
    synchronous ladder, which test_synchronous_ladder_grows_step_by_step holds byte-identical to the cold engines) against the fp64 bar
    of test_gpu_logits: 8 x the fp32 oracle's own error on the same sites, per context and stratum."""
    slabs = G.ladder()
    probes = [(k, i) for k, s in enumerate(slabs) for i in (0, len(s) - 1)]
    f64 = [CNN64(os.path.join(WEIGHTS, n + ".hmw")) for n in NAMES]
    sites = reference_sites(oracle, [slabs[k][i] for k, i in probes], {"o32": oracle_models, "f64": f64})
    runs = synced("default", "dense")
    worst_ratio = 0.0
    for c in range(3):
        s = sites[c]
        lg, rid, qoff, strand = [], [], [], []
        for j, (k, i) in enumerate(probes):
            r, q, st = runs[k]["scan"][c]
            lg.append(runs[k]["logits"][c][r == i])
            rid.append(np.full(int((r == i).sum()), j, np.int32))
            qoff.append(q[r == i])
            strand.append(st[r == i])
        lg, rid, qoff, strand = (np.concatenate(x) for x in (lg, rid, qoff, strand))
        assert len(qoff) > 100 and np.array_equal(rid, s["rid"]) and np.array_equal(qoff, s["qoff"]) and np.array_equal(strand, s["strand"]), NAMES[c]
        e_oracle = float(site_errors(s["o32"], s["f64"]).max())
        e = site_errors(lg, s["f64"])
        print(f"\ndefault probes {NAMES[c]}: n={len(e)} E_gpu={e.max():.2e} E_oracle={e_oracle:.2e} ratio={e.max() / e_oracle:.2f} bar={bar(e_oracle):.2e}")
        worst_ratio = max(worst_ratio, float(e.max()) / e_oracle)
        for name, mask in strata(s, c).items():
            assert mask.sum() > 0 and e[mask].max() <= bar(e_oracle), (NAMES[c], name, float(e[mask].max()), bar(e_oracle))
    print(f"worst logit error / E_oracle {worst_ratio:.2f}")


def test_options_changed_between_batches():
    """hm_set_option refuses none of num_cu, group_bases and tail_slice after a run (it refuses only out-of-range values and the precision 2 /
    tail_impl pairs), so there is no refusal to assert: the options are changed on a live engine and the next slabs must come out as on cold
    engines that had the final options from the start.  Sliding-window trunk: slab 1 on ONE workgroup and one group; then num_cu = 7 and
    group_bases = 32768, slab 2; then num_cu at the device's count, slab 3.  d_dump holds one block of conv4 rows per workgroup
    (trunk3_dump_bytes: 43 KB each) and is grow-only, so each raise of num_cu is a real reallocation under a larger grid, whose workgroups
    address it by blockIdx -- a buffer reserved on first use only would be overrun.  That it regrew is read off group_bytes: slabs 2 and 3
    also outgrow every other group buffer (a 70 kb and a 150 kb read group), so after each the live engine must hold exactly what the cold
    engine with the final options holds; with d_dump left at its earlier size it would hold less.  Split tail: slab 1 in slices of 64
    sites, then tail_slice at its bound: the hand-off buffer is laid out anew for slabs 2 and 3."""
    import torch
    slabs = G.ladder()
    all_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert all_cu >= 2 * 7
    m = _engine("trunk3-cu1")
    try:
        _same_calls(_run(m, slabs[1])["calls"], cold("trunk3-cu1", "dense", 1)["calls"], "trunk3 slab 1, num_cu 1")
        m.set_option("num_cu", 7)
        m.set_option("group_bases", 32768)
        r, want = _run(m, slabs[2]), cold("trunk3-groups", "dense", 2)
        _same_calls(r["calls"], want["calls"], "trunk3 slab 2, num_cu 7")
        assert r["group_bytes"] == want["group_bytes"], (r["group_bytes"], want["group_bytes"])
        m.set_option("num_cu", all_cu)
        r3, want = _run(m, slabs[3]), cold("trunk3-groups-allcu", "dense", 3)
        _same_calls(r3["calls"], want["calls"], "trunk3 slab 3, all CUs")
        assert all(r3["logits"][c].tobytes() == want["logits"][c].tobytes() for c in range(3))
        assert r3["group_bytes"] == want["group_bytes"], (r3["group_bytes"], want["group_bytes"])
        # the dump buffer's share of that figure: the cold engines differ in num_cu alone
        assert want["group_bytes"] > cold("trunk3-groups", "dense", 3)["group_bytes"]
    finally:
        m.close()
    m = _engine("trunk1")
    try:
        m.set_option("tail_impl", 2)
        m.set_option("tail_slice", 64)
        _same_calls(_run(m, slabs[1])["calls"], cold("tail2-wide", "dense", 1)["calls"], "tail2 slab 1, slices of 64")
        m.set_option("tail_slice", TAIL_SLICE_BOUND)
        for k in (2, 3):
            r, want = _run(m, slabs[k]), cold("tail2-wide", "dense", k)
            _same_calls(r["calls"], want["calls"], f"tail2 slab {k}, one slice")
            assert all(r["logits"][c].tobytes() == want["logits"][c].tobytes() for c in range(3))
    finally:
        m.close()


def test_cold_engine_staged_from_three_threads():
    """LADDER dealt round-robin to three threads that stage, queue and collect on one fresh default engine, all starting behind a barrier:
    whichever slab comes first decides the kernel path (the same for every slab) and whichever order the scratch grows in, each result is
    the cold engine's.  One run."""
    slabs = G.ladder()
    got, errs = [None] * len(slabs), []
    gate = threading.Barrier(3)
    m = _engine("default")

    def worker(ids):
        try:
            gate.wait()
            for i in ids:
                b = m.begin_batch()
                b.submit_all(slabs[i])
                b.enqueue()
                got[i] = b.wait().copy()
                b.release()
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)

    try:
        ts = [threading.Thread(target=worker, args=(range(k, len(slabs), 3),)) for k in range(3)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        grown = m.timing()["group_bytes"]
    finally:
        m.close()
    assert not errs, errs
    for k in range(len(slabs)):
        _same_calls(got[k], cold("default", "dense", k)["calls"], f"threads slab {k}")
    assert grown > cold("default", "dense", 0)["group_bytes"]


def test_repeat_slab_regrows_the_slot_and_the_pinned_slab():
    """growth_cases.repeat_slab: REPEAT_COUNT = 24 repeats of 20 read objects, 66.5 MiB of raw bytes -- above the pinned slab's 64 MiB floor --
    and 8.6 M bases against 20 k: through ReadBlock / submit_block into the slot that has just held the 20 k lead slab, while a second lead
    slab is queued (not waited for) in the next slot.  The pinned slab, every per-slot array and the pinned h_calls regrow; group_bases = 262144 keeps the
    group scratch small.  Byte-identical to a cold engine, and repeat i of the unit gives repeat 0's calls with read_id shifted."""
    from hifimeth_amd import MethylationCaller
    from hifimeth_amd.caller import ReadBlock
    unit, slab, lead = G.repeat_unit(), G.repeat_slab(), G.lead_slab()
    opts = {"trunk": 1, "group_bases": 262144}
    res = {}
    for who in ("cold", "live"):
        m = MethylationCaller(device=0)
        try:
            for k, v in opts.items():
                m.set_option(k, v)
            if who == "live":
                b0, b1 = m.begin_batch(), m.begin_batch()
                for b in (b0, b1):
                    b.submit_block(ReadBlock(lead), 2)
                    b.enqueue()
                res["lead"] = b0.wait().copy()
                b0.release()                     # slot 1 is free again, sized for 20 k bases; b1 is queued in slot 2
            b = m.begin_batch()
            assert b.submit_block(ReadBlock(slab), 4) == G.REPEAT_COUNT * sum(1 for r in unit if G.staged(r))
            assert b.staged_bases() == G.staged_bases(slab)
            b.enqueue()
            res[who] = b.wait().copy()
            b.release()
            if who == "live":
                res["lead2"] = b1.wait().copy()
                b1.release()
        finally:
            m.close()
    _same_calls(res["live"], res["cold"], "repeat slab")
    assert res["lead"].tobytes() == res["lead2"].tobytes() and len(res["lead"]) > 5000
    got = res["live"]
    assert len(got) % G.REPEAT_COUNT == 0
    rep = got.reshape(G.REPEAT_COUNT, -1)
    assert rep.shape[1] > 100000
    for f in ("qoff", "strand", "ctx", "scaled_prob", "reserved", "p"):
        assert (rep[f].view(np.uint8 if rep[f].dtype.itemsize == 1 else np.uint32) == rep[f][0].view(np.uint8 if rep[f].dtype.itemsize == 1 else np.uint32)).all(), f
    assert (rep["read_id"] - rep["read_id"][0] == (np.arange(G.REPEAT_COUNT) * len(unit))[:, None]).all()
