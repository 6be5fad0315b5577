"""Every kernel path's logits against the fp64 CPU reference of the CNN (tests/cnn64.py).

The calls' |dp| <= 1e-4 bar (test_gpu_parity.py) is weak wherever the network is confident: p saturates, and a logit error
hundreds of times what fp32 arithmetic makes passes unseen.  Here each engine configuration stages a read set, and the
logits of every site (hm_site_logits, in scan order) are compared with fp64 logits of the oracle's windows of the same sites:
    e = max_k |l_k - l64_k| / (1 + max_k |l64_k|) per site,  E = max over a context's sites,
    bar = 8 x max(E_oracle, 1e-6), E_oracle: the fp32 oracle's own E on the same sites.
f16x3 keeps 22 of fp32's 24 significand bits per operand; simulated on the CPU it stays within ~1.2 x E_oracle
(test_cnn64_cpu.py); the rest of the factor 8 covers the MFMA accumulation order.  The same simulation with one product
term dropped in one or two layers sits > 100 x above E_oracle, and so do the engine's real modes that drop it
(test_the_bar_sees_one_dropped_product_term)."""
import os

import numpy as np
import pytest

from cnn64 import CNN64, STRATA, bar, reference_sites, site_errors, strata
from conftest import WEIGHTS
from hifimeth_amd.synth import read_from_ascii, synth_slab
from test_gpu_parity import _extreme_reads, _kin, _mixed_reads

pytestmark = pytest.mark.gpu

NAMES = ("CpG", "CHG", "CHH")


def _tile_reads():
    """Reads whose L + 400 is 0, 1 and 111 mod 112: the dense trunk's last tile of a read view is full, holds one position,
    or all but one."""
    rng = np.random.default_rng(112)
    reads = []
    for k in (13, 30):
        for r in (0, 1, 111):
            L = 112 * k - 400 + r
            reads.append(read_from_ascii("".join("ACGT"[i] for i in rng.choice(4, L)).encode(), *_kin(L, rng, wide=(r == 1)),
                                         flag=16 if r == 111 else 0))
    return reads


SETS = {
    "mixed": _mixed_reads,
    "extreme": _extreme_reads,
    "tiles": _tile_reads,
    "gc70": lambda: synth_slab(6, seed=700, gc=0.7, cpg_oe=1.0, median_len=6000, sigma=0.5, frac_wide=0.2),
    "human": lambda: synth_slab(10, seed=97, gc=0.41, cpg_oe=0.24, median_len=6000, sigma=0.4, frac_wide=0.2),
}

CONFIGS = {
    "p1-trunk0": {"precision": 1, "trunk": 0},
    "trunk1": {"trunk": 1},
    "trunk_impl0": {"trunk": 1, "trunk_impl": 0},
    "trunk_impl1": {"trunk": 1, "trunk_impl": 1},
    "trunk_impl2": {"trunk": 1, "trunk_impl": 2},
    "edge_impl0": {"trunk": 1, "edge_impl": 0},
    "tail_impl0": {"trunk": 1, "tail_impl": 0},
    "tail_impl1": {"trunk": 1, "tail_impl": 1},
    "tail_impl2": {"trunk": 1, "tail_impl": 2, "tail_slice": 64},
    "trunk3-cu1-groups": {"trunk": 1, "trunk_impl": 3, "num_cu": 1, "group_bases": 32768},
    "trunk3-cu7-groups": {"trunk": 1, "trunk_impl": 3, "num_cu": 7, "group_bases": 32768},
    "p0-trunk0-w4": {"precision": 0, "trunk": 0, "front_waves": 4},
    "p0-trunk0-w8": {"precision": 0, "trunk": 0, "front_waves": 8},
    "p0-trunk1": {"precision": 0, "trunk": 1},
}

# real modes that drop the w_lo * x_hi product in some layers: each must exceed precision 1's bar in every context
BLIND_IF_WITHIN = {
    "precision2-tail1": {"trunk": 1, "tail_impl": 1, "precision": 2},
    "precision2-tail3": {"trunk": 1, "tail_impl": 3, "precision": 2},
    "conv3_w16-trunk3": {"trunk": 1, "trunk_impl": 3, "conv3_w16": 1},
}

_REF = {}


def _ref(name, oracle, oracle_models):
    """fp64 and fp32-oracle logits of a read set's sites, computed once per module."""
    if name not in _REF:
        reads = SETS[name]()
        f64 = [CNN64(os.path.join(WEIGHTS, n + ".hmw")) for n in NAMES]
        sites = reference_sites(oracle, reads, {"o32": oracle_models, "f64": f64})
        for c, s in enumerate(sites):
            s["e_oracle"] = float(site_errors(s["o32"], s["f64"]).max(initial=0.0))
            sizes = {k: int(m.sum()) for k, m in strata(s, c).items()}
            assert min(sizes.values()) > 0, (name, NAMES[c], sizes)   # every stratum is exercised
        _REF[name] = (reads, sites)
    return _REF[name]


def _stage(m, reads):
    m.clear()
    m.submit_all(reads)
    m.upload()
    m.run()


def _errors(m, reads, sites, perm=None, names=STRATA):
    """E per context (and per stratum of `names`) of the engine's staged batch; checks that its site lists are the oracle's."""
    out = []
    for c in range(3):
        s = sites[c]
        idx = np.arange(len(s["qoff"])) if perm is None else perm[c]
        rid, qoff, strand = m.scan_sites(c)
        want_rid = s["rid"][idx] if perm is None else len(reads) - 1 - s["rid"][idx]
        assert np.array_equal(rid, want_rid) and np.array_equal(qoff, s["qoff"][idx]) and np.array_equal(strand, s["strand"][idx]), c
        lg = m.site_logits(c)
        assert lg.shape == (len(idx), 2) and np.isfinite(lg).all()
        e = np.empty(len(idx))
        e[idx] = site_errors(lg, s["f64"][idx])
        by = {k: float(e[mk].max()) for k, mk in strata(s, c, names).items()}
        out.append((float(e.max(initial=0.0)), by))
    return out


def _report(set_name, cfg, sites, errs):
    rows = []
    for c in range(3):
        E, by = errs[c]
        eo = sites[c]["e_oracle"]
        worst = max(by, key=by.get)
        rows.append(f"{set_name:8s} {cfg:18s} {NAMES[c]:4s} n={len(sites[c]['qoff']):6d} E_gpu={E:.2e} E_oracle={eo:.2e} "
                    f"ratio={E / eo:6.2f} bar={bar(eo):.2e} worst={worst}:{by[worst]:.2e}")
    print("\n" + "\n".join(rows))


def _check(set_name, cfg, sites, errs):
    _report(set_name, cfg, sites, errs)
    for c in range(3):
        b = bar(sites[c]["e_oracle"])
        for k, v in errs[c][1].items():
            assert v <= b, (set_name, cfg, NAMES[c], k, v, b)


def _engine(opts):
    from hifimeth_amd import MethylationCaller
    m = MethylationCaller(device=0)
    for k, v in opts.items():
        m.set_option(k, v)
    return m


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("set_name", [s for s in SETS if s != "human"])
def test_logits_within_the_bar(oracle, oracle_models, set_name, cfg):
    reads, sites = _ref(set_name, oracle, oracle_models)
    m = _engine(CONFIGS[cfg])
    try:
        _stage(m, reads)
        _check(set_name, cfg, sites, _errors(m, reads, sites))
    finally:
        m.close()


@pytest.mark.parametrize("cfg", ["trunk3-cu1-groups", "trunk3-cu7-groups"])
def test_second_different_batch_through_the_sliding_window_trunk(oracle, oracle_models, cfg):
    """Runs cut inside reads and many groups, then another batch (the mixed set in reverse order: other reads at every
    group and run boundary) and the first again through the same engine: kept rows of an earlier batch must not leak."""
    reads, sites = _ref("mixed", oracle, oracle_models)
    perm = [np.lexsort((s["qoff"], len(reads) - 1 - s["rid"])) for s in sites]
    m = _engine(CONFIGS[cfg])
    try:
        _stage(m, reads)
        _check("mixed", cfg, sites, _errors(m, reads, sites))
        _stage(m, reads[::-1])
        _check("mixed-rev", cfg, sites, _errors(m, reads[::-1], sites, perm))
        _stage(m, reads)
        _check("mixed", cfg, sites, _errors(m, reads, sites))
    finally:
        m.close()


@pytest.mark.parametrize("cfg", list(CONFIGS) + ["default"])
def test_logits_within_the_bar_on_human_like_reads(oracle, oracle_models, cfg):
    """GC 0.41, CpG depleted: with the default options (trunk 2) CpG takes the per-site kernels and CHG / CHH the trunk in
    one batch."""
    reads, sites = _ref("human", oracle, oracle_models)
    from hifimeth_amd import MethylationCaller
    m = _engine(CONFIGS.get(cfg, {})) if cfg != "default" else MethylationCaller(device=0, timing=True)
    try:
        _stage(m, reads)
        if cfg == "default":
            m.sync()
            t = m.timing()
            assert t["front_launches"][0] > 0 and t["trunk_launches"][0] == 0 and t["trunk_launches"][1] > 0 and t["trunk_launches"][2] > 0
        _check("human", cfg, sites, _errors(m, reads, sites))
    finally:
        m.close()


@pytest.mark.parametrize("mode", list(BLIND_IF_WITHIN))
def test_the_bar_sees_one_dropped_product_term(oracle, oracle_models, mode):
    """Real engine modes with plain fp16 weights in conv8 + fc1 (precision 2, on either tail) or in conv3 (conv3_w16) must
    exceed precision 1's bar in every context: otherwise the check above would be blind to an error of that size."""
    reads, sites = _ref("mixed", oracle, oracle_models)
    m = _engine(BLIND_IF_WITHIN[mode])
    try:
        _stage(m, reads)
        errs = _errors(m, reads, sites)
    finally:
        m.close()
    _report("mixed", mode, sites, errs)
    for c in range(3):
        E, b = errs[c][0], bar(sites[c]["e_oracle"])
        assert E > b, (mode, NAMES[c], E, b)
