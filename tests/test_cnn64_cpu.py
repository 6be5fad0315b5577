"""The fp64 CNN reference of the logit tests (tests/cnn64.py) and the bar it sets, on the CPU.

test_gpu_logits.py bounds each kernel path's logits by 8 x the fp32 oracle's own error against fp64.  Here: the fp64 model is
the reference's network, and that bar admits the split-half arithmetic the kernels implement while it rejects the same
arithmetic with ONE product term dropped in one or two layers -- so a GPU path that passes it has no such error."""
import os

import numpy as np
import pytest

from cnn64 import CNN64, bar, reference_sites, site_errors, strata
from conftest import GOLDEN, WEIGHTS
from test_gpu_parity import _extreme_reads, _mixed_reads

NAMES = ("CpG", "CHG", "CHH")


def _models(**kw):
    return [CNN64(os.path.join(WEIGHTS, n + ".hmw"), **kw) for n in NAMES]


@pytest.mark.parametrize("ctx,name", [(0, "CpG"), (1, "CHG"), (2, "CHH")])
def test_fp64_model_matches_the_reference_torchscript(ctx, name):
    z = np.load(os.path.join(GOLDEN, f"cnn_{name}.npz"))
    got = CNN64(os.path.join(WEIGHTS, name + ".hmw")).logits(z["windows"])
    err = float(np.abs(got - z["logits"]).max())
    print(f"{name}: max |l64 - l_torchscript| = {err:.2e}")
    assert err <= 1e-5


def test_chunks_do_not_change_the_result(monkeypatch):
    import cnn64
    z = np.load(os.path.join(GOLDEN, "cnn_CHH.npz"))
    m = CNN64(os.path.join(WEIGHTS, "CHH.hmw"), split=True)
    whole = m.logits(z["windows"])
    monkeypatch.setattr(cnn64, "CHUNK", 7)
    assert np.array_equal(m.logits(z["windows"]), whole)


def test_the_bar_separates_one_dropped_product_term(oracle, oracle_models):
    """On the mixed read set: simulated f16x3 stays within 8 x E_oracle in every context; the same with w_lo dropped in conv8 +
    fc1 (engine option precision 2) or in conv3 (conv3_w16) exceeds it in every context."""
    variants = {"o32": oracle_models, "f64": _models(), "f16x3": _models(split=True),
                "precision2": _models(split=True, drop_wlo=("conv8", "fc1")), "conv3_w16": _models(split=True, drop_wlo=("conv3",))}
    ref = reference_sites(oracle, _mixed_reads(), variants)
    for c, name in enumerate(NAMES):
        s = ref[c]
        assert len(s["qoff"]) > 100
        e = {k: float(site_errors(s[k], s["f64"]).max()) for k in variants if k != "f64"}
        b = bar(e["o32"])
        print(f"{name}: n={len(s['qoff'])} E_oracle={e['o32']:.2e} bar={b:.2e} " +
              " ".join(f"{k}={e[k]:.2e} ({e[k] / e['o32']:.1f}x)" for k in ("f16x3", "precision2", "conv3_w16")))
        assert e["f16x3"] <= b, (name, e)
        assert e["precision2"] > b and e["conv3_w16"] > b, (name, e)


@pytest.mark.parametrize("which", ["mixed", "extreme"])
def test_read_sets_populate_every_stratum(oracle, which):
    reads = _mixed_reads() if which == "mixed" else _extreme_reads()
    ref = reference_sites(oracle, reads, {})
    for c, name in enumerate(NAMES):
        sizes = {k: int(m.sum()) for k, m in strata(ref[c], c).items()}
        print(which, name, sizes)
        assert len(sizes) == (6 if c == 2 else 3) and min(sizes.values()) > 0, (name, sizes)
