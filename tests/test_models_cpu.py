"""The model directories of tests/models.py and the references that test_gpu_models.py holds the kernels to, on the CPU.

The fp32 oracle and the fp64 model agree on models they were never run on (other k1 per slot, random weights, negative bn0
gammas, an all-zero bias); the power-of-two rescaling leaves the fp64 logits bit-identical, so one fp64 reference serves every
scaled directory; the random model is a live network (no layer dead or saturated, logits that vary, a permuted channel seen);
and the simulated split-half arithmetic meets the bar the GPU tests assert, so that bar can be met."""
import os

import numpy as np
import pytest
import torch

import models
from cnn64 import CNN64, bar, reference_sites, site_errors, strata
from models import NAMES

_REF = {}


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("models")
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = models.make(kind, os.path.join(root, kind))
        return made[kind]
    return get


def _cnn(d, **kw):
    return [CNN64(os.path.join(d, n + ".hmw"), **kw) for n in NAMES]


def _ref(kind, dirs, oracle):
    """Per context the read set's sites with the fp32 oracle's, the fp64 and the simulated split-half logits of directory `kind`."""
    if kind not in _REF:
        d = dirs(kind)
        variants = {"o32": [oracle.Model(os.path.join(d, n + ".hmw")) for n in NAMES], "f64": _cnn(d), "f16x3": _cnn(d, split=True)}
        _REF[kind] = reference_sites(oracle, models.model_reads(), variants)
    return _REF[kind]


def test_read_set_populates_every_stratum(oracle):
    reads = models.model_reads()
    assert sum(r.l_qseq for r in reads) == 8544
    ref = reference_sites(oracle, reads, {})
    for c, name in enumerate(NAMES):
        sizes = {k: int(m.sum()) for k, m in strata(ref[c], c).items()}
        print(name, sizes)
        assert len(sizes) == (6 if c == 2 else 3) and min(sizes.values()) > 0, (name, sizes)


def test_model_directories_are_what_they_say(dirs):
    from hifimeth_amd.onnx_weights import load_hmw
    sw = {n: load_hmw(os.path.join(dirs("swapped"), n + ".hmw")) for n in NAMES}
    assert [sw[n].k1 for n in NAMES] == [13, 13, 11]
    assert np.array_equal(sw["CHH"].conv_w[0], models.shipped("CpG").conv_w[0]) and np.array_equal(sw["CpG"].fc1_w, models.shipped("CHH").fc1_w)
    rnd = {n: load_hmw(os.path.join(dirs("random"), n + ".hmw")) for n in NAMES}
    assert [rnd[n].k1 for n in NAMES] == [13, 11, 11]
    for n in NAMES:
        w = rnd[n]
        assert int((w.bn_gamma < 0).sum()) >= 3 and 0.5 <= float(np.abs(w.bn_gamma).min()) and float(np.abs(w.bn_gamma).max()) <= 2.0
        assert not w.conv_b[5].any() and w.conv_b[4].any() and w.conv_b[6].any()
        assert (w.bn_var[4:] >= 1e-4).all() and (w.bn_var[4:] <= 2e-3).all()
        assert open(os.path.join(dirs("random"), n + ".hmw"), "rb").read() != open(os.path.join(dirs("random"), NAMES[(NAMES.index(n) + 1) % 3] + ".hmw"), "rb").read()
    # the same seeds give the same bytes
    again = models.random_model("CHG")
    assert all(np.array_equal(a, b) for a, b in zip(again.conv_w, rnd["CHG"].conv_w)) and np.array_equal(again.bn_gamma, rnd["CHG"].bn_gamma)


@pytest.mark.parametrize("kind", ["swapped", "random"])
def test_oracle_and_fp64_model_agree(dirs, oracle, kind):
    """The bound of test_oracle_golden.py::test_cnn_matches_reference_torchscript: max |logit difference| < 2e-5."""
    ref = _ref(kind, dirs, oracle)
    for c, name in enumerate(NAMES):
        err = float(np.abs(ref[c]["o32"] - ref[c]["f64"]).max())
        print(f"{kind} {name}: n={len(ref[c]['qoff'])} max |l_oracle - l64| = {err:.2e}")
        assert len(ref[c]["qoff"]) > 100 and err < 2e-5, (kind, name, err)


@pytest.mark.parametrize("k", [6, -6, 10, -10])
def test_scaling_leaves_the_fp64_logits_bit_identical(dirs, oracle, k):
    rng = np.random.default_rng(64)
    sites = reference_sites(oracle, models.model_reads(), {})
    reads = models.model_reads()
    base, scaled = _cnn(models.WEIGHTS), _cnn(dirs(f"scaled{k:+d}"))
    for c, name in enumerate(NAMES):
        # 40 sites of every read: windows over both read ends, homopolymers, wide kinetics
        wins = []
        for rid in np.unique(sites[c]["rid"]):
            offs = sites[c]["qoff"][sites[c]["rid"] == rid]
            pick = np.unique(np.concatenate([offs[:5], offs[-5:], rng.choice(offs, min(30, len(offs)), replace=False)]))
            wins.append(oracle.windows(reads[rid], oracle.decode(reads[rid]), pick)[0])
        wins = np.concatenate(wins)
        a, b = base[c].logits(wins), scaled[c].logits(wins)
        assert len(wins) > 100 and np.isfinite(a).all() and np.array_equal(a, b), (k, name)
        assert not np.array_equal(base[c].layers[1][0], scaled[c].layers[1][0])


def _activations(m, windows):
    """Post-ReLU outputs of conv1 .. conv8 and fc1 of an fp64 CNN64 (the loop of CNN64.logits)."""
    mean, scale, beta = m.bn
    out = []
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(windows, np.float64)).transpose(1, 2)
        x = (x - mean[:, None]) * scale[:, None] + beta[:, None]
        for i in range(8):
            x = m._layer(i, x)
            out.append(x.numpy())
        out.append(m._layer(8, x.reshape(x.shape[0], -1)).numpy())
    return out


def test_random_model_is_not_a_dead_network(dirs, oracle):
    ref = _ref("random", dirs, oracle)
    reads = models.model_reads()
    d = dirs("random")
    rng = np.random.default_rng(3)
    for c, name in enumerate(NAMES):
        s = ref[c]
        m = CNN64(os.path.join(d, name + ".hmw"))
        # windows of 200 of the context's sites, spread over the reads
        wins = []
        for rid in np.unique(s["rid"]):
            offs = s["qoff"][s["rid"] == rid]
            pick = np.sort(rng.choice(offs, min(40, len(offs)), replace=False))
            wins.append(oracle.windows(reads[rid], oracle.decode(reads[rid]), pick)[0])
        wins = np.concatenate(wins)
        share = [float((a > 0).mean()) for a in _activations(m, wins)]
        std = float(s["f64"].std(axis=0).min())
        print(f"random {name}: active share per layer {' '.join(f'{v:.2f}' for v in share)}; logit std {std:.2f}")
        assert all(0.2 <= v <= 0.8 for v in share), (name, share)
        assert std >= 0.2, (name, std)
        # one conv3 output channel's weights permuted: a packing error of that size must not hide under the bar
        p = CNN64(os.path.join(d, name + ".hmw"))
        w3 = p.layers[2][0]
        w3[5] = w3[5].reshape(-1)[torch.from_numpy(np.random.default_rng(9).permutation(w3[5].numel()))].reshape(w3[5].shape)
        e_perm = float(site_errors(p.logits(wins), m.logits(wins)).max())
        b = bar(float(site_errors(s["o32"], s["f64"]).max()))
        print(f"random {name}: permuted conv3 channel E={e_perm:.2e} bar={b:.2e}")
        assert e_perm > b, (name, e_perm, b)


@pytest.mark.parametrize("kind", ["swapped", "random"])
def test_simulated_split_half_meets_the_bar(dirs, oracle, kind):
    ref = _ref(kind, dirs, oracle)
    for c, name in enumerate(NAMES):
        s = ref[c]
        eo = float(site_errors(s["o32"], s["f64"]).max())
        es = float(site_errors(s["f16x3"], s["f64"]).max())
        print(f"{kind} {name}: n={len(s['qoff'])} E_oracle={eo:.2e} E_f16x3={es:.2e} ({es / eo:.1f}x) bar={bar(eo):.2e}")
        assert es <= bar(eo), (kind, name, es, eo)
