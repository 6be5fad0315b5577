"""The feature-extraction front of the call engine (prep_kernel -> scan_kernel -> emit_kernel -> pack_kernel, window_kernel) on
the hand-built inputs of tests/scan_cases.py: motifs across the thread / wave / chunk boundaries of the kernels' ownership, every
read-tail length behind every other, kinetics widths per array, and batches of one to four chunks per scan thread.  Runs on the GPU
box only:  python -m pytest tests/test_gpu_scan_edges.py -m gpu -q
Everything here is integer or bit-exact work: every comparison is equality, against the CPU oracle, against site lists written
out from the construction, and against the reference's own scanner (tests/golden/scan_edges.json).  The engine runs in its default
mode (the arithmetic mode does not touch the scanner); one test repeats the call order on the per-site path."""
import json
import os

import numpy as np
import pytest

import scan_cases as S
from conftest import GOLDEN
from hifimeth_amd.synth import read_from_ascii

pytestmark = pytest.mark.gpu

MASKS = ["cpg", "chg", "chh", "cpg,chg", "cpg,chh", "chg,chh", "cpg,chg,chh"]


def _reads(case):
    if case == "boundary":
        return S.boundary_motifs()[0]
    if case == "tails":
        return S.tail_lengths()
    if case == "widths":
        return S.mixed_widths()
    if case == "edges":
        return S.boundary_motifs()[0] + S.tail_lengths()
    return S.many_chunks(int(case[2:]))


ALL_CASES = ["boundary", "tails", "widths"] + [f"mc{n}" for n in S.MANY_CHUNKS]
_want = {}


def _expected(case, mask=7):
    """oracle lists and call order of a case, computed once and shared"""
    if (case, mask) not in _want:
        _want[case, mask] = S.expected_sites(_reads(case), mask)
    return _want[case, mask]


def _stage(m, reads):
    m.clear()
    assert m.submit_all(reads) == len(reads)
    m.upload()
    m.run()


@pytest.fixture(scope="module")
def eng():
    from hifimeth_amd import MethylationCaller
    m = MethylationCaller(device=0, min_read_size=1)      # the tail reads go down to one base
    # By default the engine picks the dense trunk or the per-site kernels once, from the site density of its first batch: which
    # tests are selected would decide the CNN path of all the others.  The dense trunk, what ordinary reads take, is set instead.
    m.set_option("trunk", 1)
    yield m
    m.close()


@pytest.fixture(scope="module")
def device(eng):
    """case -> what the device gave for it (site lists, counts, calls): every batch runs once"""
    done = {}

    def get(case):
        if case not in done:
            _stage(eng, _reads(case))
            done[case] = dict(sites=[eng.scan_sites(c) for c in range(3)], nums=[eng.num_sites(c) for c in range(4)],
                              calls=eng.fetch().copy())
            eng.clear()
        return done[case]
    return get


def _assert_lists(got_sites, got_nums, lists, tag):
    for c in range(3):
        rid, qoff, strand = got_sites[c]
        assert np.array_equal(rid, lists[c][0]) and np.array_equal(qoff, lists[c][1]) and np.array_equal(strand, lists[c][2]), (tag, c)
        assert got_nums[c] == len(lists[c][0]), (tag, c)
    assert got_nums[3] == sum(len(x[0]) for x in lists), tag


def _assert_order(calls, order, tag):
    o_r, o_s, o_q, o_c = order
    assert len(calls) == len(o_r), (tag, len(calls), len(o_r))
    for f, want in (("read_id", o_r), ("strand", o_s), ("qoff", o_q), ("ctx", o_c)):
        assert np.array_equal(calls[f], want), (tag, f)


@pytest.mark.parametrize("case", ALL_CASES)
def test_site_lists_equal_the_oracle(device, case):
    """scan_sites(c) in (read, qoff, strand) and num_sites(0..3), on all four classes; many_chunks with one to four chunks per scan
    thread: the running prefix inside a thread's range, empty ranges, a read across ranges, the totals row behind the last read"""
    lists, order = _expected(case)
    got = device(case)
    _assert_lists(got["sites"], got["nums"], lists, case)
    assert got["nums"][3] > (0 if case == "tails" else 100)
    if case == "boundary":      # and the lists written out from the construction
        _reads_, expected, _b = S.boundary_motifs()
        for c in range(3):
            rid, qoff, strand = got["sites"][c]
            lit = [(i, q, s) for i, want in enumerate(expected) for k, q, s in want if k == c]
            assert lit == list(zip(rid.tolist(), qoff.tolist(), strand.tolist())), c


@pytest.mark.parametrize("case", ["boundary", "tails"] + [f"mc{n}" for n in S.MANY_CHUNKS])
def test_calls_come_in_the_reference_order(device, case):
    """fetch(): read_id, strand, qoff, ctx in the order of mod_main.cpp:217-251 -- per read the forward-strand calls by qoff, then
    the reverse-strand ones -- built from the oracle's lists; the whole arrays (p is the CNN's business, not compared here)"""
    _lists, order = _expected(case)
    calls = device(case)["calls"]
    _assert_order(calls, order, case)
    assert np.isfinite(calls["p"]).all()


def test_calls_come_in_the_reference_order_on_the_per_site_path():
    from hifimeth_amd import MethylationCaller
    with MethylationCaller(device=0, min_read_size=1) as m:
        m.set_option("trunk", 0)
        calls = m.call(_reads("edges"))
    _assert_order(calls, _expected("edges")[1], "edges, trunk 0")


@pytest.mark.parametrize("n_chunks", [2049, 3075])
def test_calls_do_not_depend_on_the_scan_partition(eng, device, n_chunks):
    """three and four chunks per scan thread against the same reads in batches of at most 1000 chunks (one chunk per scan thread:
    the path the small oracle-checked tests take): the same bytes, p included"""
    reads = S.many_chunks(n_chunks)
    big = device(f"mc{n_chunks}")["calls"]
    parts, first, n_batches = [], 0, 0
    while first < len(reads):
        last, chunks = first, 0
        while last < len(reads) and chunks + -(-reads[last].l_qseq // S.CHUNK) <= 1000:
            chunks += -(-reads[last].l_qseq // S.CHUNK)
            last += 1
        parts.append(eng.call(reads[first:last], first_id=first).copy())
        first = last
        n_batches += 1
    assert n_batches == -(-n_chunks // 1000)
    assert np.concatenate(parts).tobytes() == big.tobytes() and len(big) > 100_000


def _assert_windows(m, reads, oracle, keep):
    """windows of the staged batch against oracle.window, bit for bit, at the sites keep(read index, qoff) selects"""
    n = 0
    for c in range(3):
        rid, qoff, strand = m.scan_sites(c)
        got = m.windows(c)
        assert got.shape == (len(qoff), 401, 8)
        for i in np.unique(rid):
            sel = np.flatnonzero(rid == i)
            sel = sel[np.array([keep(int(i), int(q)) for q in qoff[sel]], bool)]
            if len(sel) == 0:
                continue
            rd = reads[i]
            want, want_s = oracle.windows(rd, oracle.decode(rd), qoff[sel])
            assert np.array_equal(want_s, strand[sel]), (c, rd.name)
            same = (got[sel] == want).reshape(len(sel), -1).all(1)
            assert same.all(), (c, rd.name, qoff[sel][~same][:5].tolist())
            n += len(sel)
    return n


def test_windows_with_a_width_per_kinetics_array(eng, oracle):
    """every site of mixed_widths(): all 16 (u8, u16) combinations over fi, fp, ri, rp, the u16 arrays on both sides of every
    threshold of encode_frames, the arrays out of phase -- pins kin_code's width and stride per array and jr = len - 1 - j"""
    reads = S.mixed_widths()
    _stage(eng, reads)
    n = _assert_windows(eng, reads, oracle, lambda i, q: True)
    eng.clear()
    assert n == sum(len(x[0]) for x in _expected("widths")[0]) > 2000


def test_windows_at_read_ends_and_ownership_boundaries(eng, oracle):
    """every site of boundary_motifs() and tail_lengths() whose window touches a read end or that lies within 2 positions of a
    boundary B: the halo, the scalar store tail of prep_kernel and the padded base_off of the next read"""
    reads = _reads("edges")

    def keep(i, q):
        L = reads[i].l_qseq
        return q < 200 or q + 200 >= L or any(abs(q - B) <= 2 for B in S.BOUNDARIES)

    _stage(eng, reads)
    n = _assert_windows(eng, reads, oracle, keep)
    eng.clear()
    lists = _expected("edges")[0]
    assert n == sum(keep(int(i), int(q)) for c in range(3) for i, q in zip(lists[c][0], lists[c][1])) > 2000


@pytest.mark.parametrize("spec", MASKS)
def test_context_masks_give_the_masked_lists_and_order(spec):
    from hifimeth_amd import MethylationCaller
    from hifimeth_amd.caller import parse_contexts
    mask = parse_contexts(spec)
    assert mask == sum(1 << ("cpg", "chg", "chh").index(t) for t in spec.split(","))
    reads = _reads("edges")
    lists, order = _expected("edges", mask)
    with MethylationCaller(contexts=spec, device=0, min_read_size=1) as m:
        _stage(m, reads)
        _assert_lists([m.scan_sites(c) for c in range(3)], [m.num_sites(c) for c in range(4)], lists, spec)
        _assert_order(m.fetch(), order, spec)
    for c in range(3):
        assert (len(lists[c][0]) > 0) == bool(mask >> c & 1)


def test_a_batch_without_sites(eng):
    """1025 chunks of poly-A/T reads: an ordinary input with no site of any context"""
    reads = S.site_free_reads(1025)
    assert sum(-(-r.l_qseq // S.CHUNK) for r in reads) == 1025
    _stage(eng, reads)
    eng.sync()
    assert [eng.num_sites(c) for c in range(4)] == [0, 0, 0, 0]
    assert len(eng.fetch()) == 0
    assert all(len(eng.scan_sites(c)[0]) == 0 for c in range(3))
    eng.clear()
    assert len(eng.call(S.tail_lengths())) == len(_expected("tails")[1][0])     # and the engine goes on working


def test_reference_scanner_lists(eng):
    """the device against the lists the reference's own C++ scanner printed for the boundary and tail reads
    (tests/golden/scan_edges.json)"""
    recs = json.load(open(os.path.join(GOLDEN, "scan_edges.json")))
    rng = np.random.default_rng(3)
    reads = [read_from_ascii(r["seq"].encode(), *[rng.integers(0, 256, len(r["seq"])).astype(np.uint8) for _ in range(4)],
                             flag=r["flag"], name=r["name"]) for r in recs]
    _stage(eng, reads)
    n = 0
    for c, key in enumerate(("cpg", "chg", "chh")):
        rid, qoff, _ = eng.scan_sites(c)
        cut = np.searchsorted(rid, np.arange(len(recs) + 1))
        for i, r in enumerate(recs):
            assert qoff[cut[i]:cut[i + 1]].tolist() == sorted(r[key]), (key, r["name"])
            n += len(r[key])
    assert n == eng.num_sites(3) > 5000
    eng.clear()
