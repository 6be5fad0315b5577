"""The edge kernel that computes its own E1 rows (engine option edge_impl = 2, the default; hm_edge2.hip, E1C) against the edge kernel
that gathers them from the trunk's E1 map (edge_impl = 1), through the C ABI.

With edge_impl = 2 the sliding-window trunk stores no E1 row and the E1 map is not allocated; the edge kernel runs conv1 over the feature
rows of its three E1 positions per site (off - 199; off + 189 for K1 = 11; off + 185 and off + 187 for K1 = 13) with the trunk's weights,
bias, k-block order and split.  Nothing downstream changes arithmetic, so everything must agree BYTE FOR BYTE: the edge rows
(hm_debug_edge_rows: the rows of the last group and context run -- read with one context in one group, where that is all of them), the
logits of every site and the calls.  Both kernels run on ONE engine, the new one first (on a fresh engine: no E1 map exists yet, so it
cannot pass by reading rows an earlier run left behind), then the gathering one, which makes the engine allocate and fill the map.

K1 = 11 is CpG and CHG, K1 = 13 is CHH (both strand views).  The only tolerance here is the whole-path comparison against the CPU
oracle, which takes DP_TOL from tests/test_gpu_parity.py."""
import numpy as np
import pytest

from hifimeth_amd.synth import read_from_ascii, synth_reads
from test_gpu_parity import DP_TOL, _check_calls

pytestmark = pytest.mark.gpu

SPECS = ["cpg", "chg", "chh"]
CTX = {"cpg": 0, "chg": 1, "chh": 2}


def _kin(L, rng, values=None):
    if values is not None:
        return [rng.choice(np.array(values, np.uint8), L) for _ in range(4)]
    return [np.clip(np.rint(rng.gamma(2.0, 12.0, L)), 0, 255).astype(np.uint8) for _ in range(4)]


def _random_read(L, rng, flag=4, values=None, frac_n=0.0):
    codes = rng.choice(4, L)
    seq = np.frombuffer(b"ACGT", np.uint8)[codes].copy()
    if frac_n:
        seq[rng.random(L) < frac_n] = ord("N")
    return read_from_ascii(seq.tobytes(), *_kin(L, rng, values), flag=flag)


def _both(spec, reads, group_bases=0, rows=True):
    """{edge_impl: (calls, logits bytes, edge rows or None, sites per context)} for edge_impl 2 and then 1 on one engine."""
    from hifimeth_amd import MethylationCaller
    out = {}
    with MethylationCaller(contexts=spec, device=0, timing=True) as m:
        m.set_option("trunk", 1)
        if group_bases:
            m.set_option("group_bases", group_bases)
        for impl in (2, 1):
            m.set_option("edge_impl", impl)
            m.clear()
            assert m.submit_all(reads) == len(reads)
            m.upload()
            m.run()
            calls = m.fetch().copy()
            n = [m.num_sites(c) for c in range(3)]
            logits = b"".join(m.site_logits(c).tobytes() for c in range(3))
            er = m.edge_rows(sum(n)).copy() if rows else None
            t = m.timing()
            m.clear()
            out[impl] = (calls, logits, er, n, t["group_bytes"])
    return out


def _assert_same(out, what):
    new, old = out[2], out[1]
    assert new[3] == old[3], (what, new[3], old[3])
    if new[2] is not None:
        bad = np.nonzero((new[2] != old[2]).any(axis=(1, 2)))[0]
        assert len(bad) == 0, (what, f"{len(bad)} of {len(new[2])} sites differ in their edge rows, first {bad[:8].tolist()}")
    assert new[1] == old[1], (what, "logits differ")
    assert new[0].tobytes() == old[0].tobytes(), (what, "calls differ")
    return sum(new[3])


@pytest.mark.parametrize("spec", SPECS)
def test_sites_whose_e1_rows_lie_outside_the_read(spec):
    """Reads of 1000, 1001 and 1203 bases, stored forward and reversed: every site of the first and last 200 positions has off - 199 or
    off + 18x outside the read -- rows that are wholly (the trunk's constant row) or partly (the read's first / last K1 - 1 positions)
    made of zero feature rows.  One group, one context: the edge rows of all sites are compared."""
    rng = np.random.default_rng(101)
    reads = [_random_read(L, rng, flag) for L in (1000, 1001, 1203) for flag in (4, 20)]
    out = _both(spec, reads)
    n = _assert_same(out, spec)
    assert n > (30 if spec != "chh" else 1000), n
    # the engine holds no E1 map until the gathering kernel asks for one: 2 views x 512 B per map row, and the head-room of a reserve
    assert out[1][4] - out[2][4] >= 1024 * sum(r.l_qseq for r in reads), (out[2][4], out[1][4])


@pytest.mark.parametrize("spec", SPECS)
def test_tile_boundaries_and_group_cuts(spec):
    """Reads of a few thousand bases: a site's three E1 positions lie in up to three different 112-row tiles of the trunk, and with
    groups of 4096 rows the reads fall into several groups (whose buffers are reused).  Calls and logits of all groups are compared; the
    same reads once more in one group for the edge rows."""
    rng = np.random.default_rng(102)
    reads = [_random_read(L, rng, flag) for L, flag in ((3500, 4), (2917, 20), (4099, 4), (1500, 4))]
    n = _assert_same(_both(spec, reads, group_bases=4096, rows=False), spec)
    assert n > (100 if spec != "chh" else 2000), n
    assert _assert_same(_both(spec, reads), spec) == n


def _sparse_read(n_sites, motif, L, rng):
    """A read of A and T with n_sites copies of `motif` ("CG": one CpG site each; "CAA": one CHH site each; "CAG": one CHG site), some
    of them in the first and last 200 positions."""
    seq = np.frombuffer(b"AT", np.uint8)[rng.choice(2, L)].copy()
    at = np.linspace(5, L - 10, n_sites).astype(int) if n_sites > 1 else np.array([L // 2])
    for p in at:
        seq[p:p + len(motif)] = np.frombuffer(motif, np.uint8)
    return read_from_ascii(seq.tobytes(), *_kin(L, rng))


@pytest.mark.parametrize("n_sites", [1, 31, 32, 33])
@pytest.mark.parametrize("spec,motif", [("cpg", b"CG"), ("chh", b"CAA")])
def test_ragged_last_pass(spec, motif, n_sites):
    """1, 31, 32 and 33 sites in the context's list: a pass of 32 site slots with nvalid < 32, exactly full, and one site over."""
    rng = np.random.default_rng(103 + n_sites)
    out = _both(spec, [_sparse_read(n_sites, motif, 1300, rng)])
    assert out[2][3][CTX[spec]] == n_sites, out[2][3]
    assert _assert_same(out, (spec, n_sites)) == n_sites


@pytest.mark.parametrize("spec", SPECS)
def test_extreme_kinetics_and_n_bases(spec):
    """Kinetics bytes 0, 63, 64 and 255 (both ends of the two lowest and the highest exponent of the frame code) and 3 % N bases
    (all-zero one-hot) in the feature spans of the E1 rows, on short reads so that the spans of most sites reach the read's ends too."""
    rng = np.random.default_rng(104)
    reads = [_random_read(L, rng, flag, values=(0, 63, 64, 255), frac_n=0.03) for L, flag in ((1100, 4), (1417, 20))]
    reads.append(_random_read(1250, rng, 4, values=(255,)))
    reads.append(_random_read(1250, rng, 4, values=(0,)))
    n = _assert_same(_both(spec, reads), spec)
    assert n > (20 if spec != "chh" else 500), n


def test_whole_path_against_the_oracle(oracle, oracle_models):
    """The default engine (edge_impl = 2, no E1 map) against the CPU oracle: |dp| <= DP_TOL, ML bytes within 1, as the path tests of
    tests/test_gpu_parity.py ask of every kernel set."""
    from hifimeth_amd import MethylationCaller
    rng = np.random.default_rng(105)
    reads = synth_reads(3, seed=105, median_len=2200, sigma=0.3, frac_wide=0.3, frac_short=0, frac_missing=0, frac_n=0.003)
    reads += [_random_read(1000, rng), _random_read(1201, rng, 20, values=(0, 63, 64, 255), frac_n=0.02)]
    with MethylationCaller(device=0) as m:
        m.set_option("trunk", 1)
        calls = m.call(reads).copy()
    n, nml, worst = _check_calls(calls, reads, oracle, oracle_models, 7)
    assert n > 1500, n
    print(f"edge_impl 2 whole path: {n} sites, max|dp| = {worst:.2e}, ML bytes off by one: {nml}")
