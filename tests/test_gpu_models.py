"""The CNN kernels on model directories other than the shipped one (tests/models.py), against the fp64 reference.

Every other CNN test loads hifimeth_amd/weights: K1 = 13 has only run in the CHH slot, the strip tail only on a K1 = 13 model,
pack_model only on three weight sets whose bn0 gammas are all near +1.2, and the byte identities between kernel variants were
seen for those three only.  Here the same bars hold on
    swapped    the shipped models in each other's slots (K1 = 13 in CpG / CHG on the resident tail, K1 = 11 in CHH on the strip tail),
    random     He-initialised weights, negative bn0 gammas, an all-zero conv6 bias, K1 = 13 in the CpG slot,
    scaled(k)  the shipped models with three layer pairs rescaled by 2^k -- the same function, other layer scales:
               strict fp32 must not notice (byte for byte), split-half must follow its CPU simulation.
test_models_cpu.py shows that the references used here are sound and that the bars can be met."""
import os
import subprocess

import numpy as np
import pytest

import bamutil
import models
from cnn64 import CNN64, bar, reference_sites, site_errors, strata
from conftest import ROOT, WEIGHTS
from models import NAMES
from test_gpu_logits import _errors, _report, _stage
from test_gpu_parity import _run

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")

CONFIGS = {
    "default": {},
    "trunk1": {"trunk": 1},
    "p1-trunk0": {"precision": 1, "trunk": 0},
    "p0-trunk1": {"precision": 0, "trunk": 1},
    "p0-trunk0": {"precision": 0, "trunk": 0},
    "trunk_impl0": {"trunk": 1, "trunk_impl": 0},
    "edge_impl0": {"trunk": 1, "edge_impl": 0},
    "tail_impl0": {"trunk": 1, "tail_impl": 0},
    "tail_impl2": {"trunk": 1, "tail_impl": 2, "tail_slice": 64},
    "trunk3-cu1-groups": {"trunk": 1, "trunk_impl": 3, "num_cu": 1, "group_bases": 32768},
}

_REF = {}
_READS = []


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("models")
    made = {"shipped": WEIGHTS}

    def get(kind):
        if kind not in made:
            made[kind] = models.make(kind, os.path.join(root, kind))
        return made[kind]
    return get


def _reads():
    if not _READS:
        _READS.extend(models.model_reads())
    return _READS


def _ref(kind, dirs, oracle):
    """Per context the read set's sites with the fp64 and the fp32-oracle logits of model directory `kind`, and for the scaled
    directories the simulated split-half logits too; computed once per module.  A scaled directory's fp64 logits ARE the shipped
    models' (test_models_cpu.py::test_scaling_leaves_the_fp64_logits_bit_identical): they are shared, not computed again."""
    if kind not in _REF:
        d = dirs(kind)
        variants = {"o32": [oracle.Model(os.path.join(d, n + ".hmw")) for n in NAMES]}
        if kind.startswith("scaled"):
            variants["f16x3"] = [CNN64(os.path.join(d, n + ".hmw"), split=True) for n in NAMES]
        else:
            variants["f64"] = [CNN64(os.path.join(d, n + ".hmw")) for n in NAMES]
        sites = reference_sites(oracle, _reads(), variants)
        for c, s in enumerate(sites):
            if kind.startswith("scaled"):
                s["f64"] = _ref("shipped", dirs, oracle)[c]["f64"]
                s["e_sim"] = float(site_errors(s["f16x3"], s["f64"]).max(initial=0.0))
            s["e_oracle"] = float(site_errors(s["o32"], s["f64"]).max(initial=0.0))
            sizes = {k: int(m.sum()) for k, m in strata(s, c).items()}
            assert min(sizes.values()) > 0, (kind, NAMES[c], sizes)   # every stratum is exercised
        _REF[kind] = sites
    return _REF[kind]


def _engine(model_dir, opts, timing=False):
    from hifimeth_amd import MethylationCaller
    m = MethylationCaller(model_dir=model_dir, device=0, timing=timing)
    for k, v in opts.items():
        m.set_option(k, v)
    return m


def _check(kind, cfg, sites, errs):
    _report(kind, cfg, sites, errs)
    for c in range(3):
        b = bar(sites[c]["e_oracle"])
        for k, v in errs[c][1].items():
            assert v <= b, (kind, cfg, NAMES[c], k, v, b)


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("kind", ["swapped", "random"])
def test_logits_within_the_bar(dirs, oracle, kind, cfg):
    """Per stratum E_gpu <= 8 x max(E_oracle, 1e-6), E_oracle measured with the fp32 oracle on the same model.  With the default options
    every context of this read set is dense enough for the trunk (CpG 11 %, CHG 2.8 %, CHH 39 % of the bases are sites; the thresholds
    are 1.7 % and, for CHH's two views, 3.3 %), and the CHH slot -- a K1 = 11 model in both directories -- takes the strip tail."""
    reads, sites = _reads(), _ref(kind, dirs, oracle)
    m = _engine(dirs(kind), CONFIGS[cfg], timing=(cfg == "default"))
    try:
        _stage(m, reads)
        if cfg == "default":
            m.sync()
            t = m.timing()
            bases = sum(r.l_qseq for r in reads)
            assert all(len(sites[c]["qoff"]) >= 1.5 * (0.033 if c == 2 else 0.017) * bases for c in range(3))
            assert list(t["front_launches"]) == [0, 0, 0] and all(n > 0 for n in t["trunk_launches"]), t
            assert t["tail_strip_passes"] > 0, t
        _check(kind, cfg, sites, _errors(m, reads, sites))
    finally:
        m.close()


def _const_steps(reads):
    """The tile plan's constant steps: per read and strand view the first tile + the tiles at u >= len."""
    want = 0
    for rd in reads:
        ntile = (rd.l_qseq + 400 + 111) // 112
        want += 1 + sum(1 for t in range(ntile) if -200 + 112 * t >= rd.l_qseq)
    return want


@pytest.mark.parametrize("option,values", [("trunk_impl", (0, 1, 2, 3)), ("edge_impl", (0, 1)), ("tail_impl", (0, 1, 2, 3))])
@pytest.mark.parametrize("kind", ["swapped", "random"])
def test_kernel_variants_are_byte_identical(dirs, kind, option, values):
    """"Every accumulator keeps its order", "the skipped blocks were exact zeros", "a constant row equals a computed step's": calls and
    logits are equal byte for byte across the trunk, edge and tail kernels on these weights too, for a second batch (the reads
    reversed) through the same engine as well; the sliding-window trunk's count of constant steps is the tile plan's."""
    reads = _reads()
    got = []
    for v in values:
        m = _engine(dirs(kind), {"trunk": 1, option: v}, timing=True)
        try:
            a = _run(m, reads)
            if option == "trunk_impl" and v == 3:
                want = _const_steps(reads)
                assert list(m.timing()["trunk_const_steps"]) == [want, want, 2 * want]
            b = _run(m, reads[::-1])
        finally:
            m.close()
        got.append((a[0].tobytes(), a[1], b[0].tobytes(), b[1]))
        assert len(a[0]) == len(b[0]) > 4000 and len(a[1]) == 8 * len(a[0])
    for v, g in zip(values[1:], got[1:]):
        for part, x, y in zip(("calls", "logits", "calls of batch 2", "logits of batch 2"), got[0], g):
            assert x == y, (kind, option, v, part)


@pytest.mark.parametrize("ctx", [0, 1, 2])
def test_cnn_layers_vs_oracle(dirs, oracle, ctx):
    """debug_layer 1 .. 8 of the random model in every slot against the oracle's layers, on a window that hangs over a read's start and
    one from the middle of a read, split-half and fp32: the bound of test_gpu_parity.py::test_cnn_layers_vs_oracle.  A failure
    of the logit test above is localised here."""
    reads, s = _reads(), _ref("random", dirs, oracle)[ctx]
    om = oracle.Model(os.path.join(dirs("random"), NAMES[ctx] + ".hmw"))
    picks = [int(np.flatnonzero(s["stratum"] == 0)[0]), int(np.flatnonzero(s["stratum"] == 1)[-1])]
    wins = [oracle.windows(reads[s["rid"][i]], oracle.decode(reads[s["rid"][i]]), s["qoff"][i:i + 1])[0][0] for i in picks]
    assert not (wins[0][0].any() and wins[0][400].any()) and wins[1][0].any() and wins[1][400].any()   # (a reverse-strand window is flipped)
    for precision in (1, 0):
        m = _engine(dirs("random"), {"precision": precision})
        try:
            for wi, w in enumerate(wins):
                for layer in range(1, 9):
                    want = om.layer(w, layer)
                    got = m.debug_layer(ctx, w, layer)
                    assert got.shape == want.shape, (layer, got.shape, want.shape)
                    err = float(np.abs(got - want).max())
                    assert err <= 1e-4 * max(1.0, float(np.abs(want).max())), (NAMES[ctx], precision, wi, layer, err)
        finally:
            m.close()


def test_the_bar_sees_one_dropped_product_term(dirs, oracle):
    """Precision 2 (plain fp16 weights in conv8 + fc1) on the random model must exceed precision 1's bar in every context: otherwise
    the checks above would be blind to an error of that size on these weights."""
    reads, sites = _reads(), _ref("random", dirs, oracle)
    m = _engine(dirs("random"), {"trunk": 1, "precision": 2})
    try:
        _stage(m, reads)
        errs = _errors(m, reads, sites)
    finally:
        m.close()
    _report("random", "precision2", sites, errs)
    for c in range(3):
        E, b = errs[c][0], bar(sites[c]["e_oracle"])
        assert E > b, (NAMES[c], E, b)


@pytest.mark.parametrize("trunk", [1, 0])
def test_strict_fp32_is_scale_free(dirs, trunk):
    """Precision 0: a power-of-two rescaling of adjacent layers commutes with every fp32 multiply, add and FMA far from the exponent
    limits, and conv1 / bn0 are untouched -- so the calls and logits on scaled(+10) and scaled(-10) are the shipped models', byte for
    byte.  A difference means some stage of the "fp32" path is not fp32."""
    reads = _reads()
    got = {}
    for kind in ("shipped", "scaled+10", "scaled-10"):
        m = _engine(dirs(kind), {"precision": 0, "trunk": trunk})
        try:
            calls, logits = _run(m, reads)
        finally:
            m.close()
        got[kind] = (calls.tobytes(), logits)
    assert len(got["shipped"][0]) > 4000 * 16
    for kind in ("scaled+10", "scaled-10"):
        assert got[kind][1] == got["shipped"][1], (kind, "logits")
        assert got[kind][0] == got["shipped"][0], (kind, "calls")


@pytest.mark.parametrize("cfg", ["trunk1", "p1-trunk0"])
@pytest.mark.parametrize("k", [6, -6, 10, -10])
def test_split_half_follows_its_simulation(dirs, oracle, k, cfg):
    """Precision 1's accuracy depends on the layer scales (the fp16 halves of an activation 2^k times larger or smaller keep fewer
    significant bits of the sum).  What it must do is follow its CPU simulation: per context E_gpu <= 8 x max(E_sim, 1e-6), E_sim the
    error of CNN64(split=True) on the same sites against the shared fp64 reference, 8 the allowance for the MFMA accumulation order.
    Asserted at k = +-6; k = +-10 is printed only (the table in DESIGN.md, "Models other than the shipped ones")."""
    kind = f"scaled{k:+d}"
    reads, sites = _reads(), _ref(kind, dirs, oracle)
    m = _engine(dirs(kind), CONFIGS[cfg])
    try:
        _stage(m, reads)
        lg = [m.site_logits(c) for c in range(3)]
    finally:
        m.close()
    rows, E = [], []
    for c in range(3):
        s = sites[c]
        assert lg[c].shape == s["f64"].shape
        finite = bool(np.isfinite(lg[c]).all())
        E.append(float(site_errors(lg[c], s["f64"]).max()) if finite else float("inf"))
        rows.append(f"scaled k={k:+3d} {cfg:10s} {NAMES[c]:4s} n={len(s['qoff']):5d} E_gpu={E[c]:.2e} E_sim={s['e_sim']:.2e} "
                    f"E_oracle={s['e_oracle']:.2e} E_gpu/E_sim={E[c] / s['e_sim']:5.2f}")
    print("\n" + "\n".join(rows))
    if abs(k) == 6:
        for c in range(3):
            assert np.isfinite(E[c]) and E[c] <= 8.0 * max(sites[c]["e_sim"], 1e-6), (k, cfg, NAMES[c], E[c], sites[c]["e_sim"])


def test_onnx_directory_through_the_cli(dirs, tmp_path):
    """`hifimeth-hip call -m <dir>` with the random models as .onnx -- CpG / CHG in the initializer + Gemm dialect, CHH in the Constant +
    MatMul / Add dialect, conv6's bias input left out of all three (the reader must supply zeros) -- writes the same BAM, byte for
    byte, as with the .hmw directory; a directory holding both forms takes the .hmw.  Every run has its own working directory and the
    same relative arguments: the @PG line records the command line."""
    from test_abi import _write_onnx
    rnd, swp = models.random_models(), models.swapped_models()
    runs = {"hmw": {}, "onnx": {}, "both": {}}
    for tag in runs:
        d = tmp_path / tag / "m"
        d.mkdir(parents=True)
        for n in NAMES:
            dialect = "constants" if n == "CHH" else "initializers"
            if tag != "onnx":
                models.save_hmw(rnd[n], str(d / (n + ".hmw")))
            if tag == "onnx":
                _write_onnx(rnd[n], str(d / (n + ".onnx")), dialect, omit_bias=(5,))
            if tag == "both":      # other weights in the .onnx: taking it would show
                _write_onnx(swp[n], str(d / (n + ".onnx")), dialect)
        bamutil.reads_to_bam(str(tmp_path / tag / "in.bam"), _reads())
        subprocess.run([CLI, "call", "-m", "m", "-t", "4", "in.bam", "out.bam"], cwd=str(tmp_path / tag), check=True, timeout=120,
                       stderr=subprocess.DEVNULL)
        runs[tag] = open(tmp_path / tag / "out.bam", "rb").read()
    _, recs = bamutil.read_bam(str(tmp_path / "hmw" / "out.bam"))
    assert sum(1 for r in recs if b"MM" in r["aux"]) == len(_reads())
    assert runs["onnx"] == runs["hmw"] and runs["both"] == runs["hmw"]
    # and the output does depend on the weights: the shipped models give another file
    (tmp_path / "shipped").mkdir()
    os.symlink(WEIGHTS, str(tmp_path / "shipped" / "m"))
    bamutil.reads_to_bam(str(tmp_path / "shipped" / "in.bam"), _reads())
    subprocess.run([CLI, "call", "-m", "m", "-t", "4", "in.bam", "out.bam"], cwd=str(tmp_path / "shipped"), check=True, timeout=120,
                   stderr=subprocess.DEVNULL)
    assert open(tmp_path / "shipped" / "out.bam", "rb").read() != runs["hmw"]


def test_weights_the_split_cannot_hold_are_refused(tmp_path):
    """pack_model keeps every conv and fc1 weight as fp16 hi + lo halves: a weight of 65520 or more would become an fp16 infinity (and
    NaN logits) without a word.  hm_create refuses such a model, a non-finite parameter, and a conv1 weight whose product with bn0's
    folded slope overflows, naming the context and the layer; the same weight at 6e4 loads and runs."""
    from hifimeth_amd import HifimethError, MethylationCaller

    def directory(tag, ctx, edit):
        ms = models.random_models()
        edit(ms[ctx])
        return models.write_dir(str(tmp_path / tag), ms)

    def conv5(v):
        def edit(w):
            w.conv_w[4][17, 33, 1] = v
        return edit

    with pytest.raises(HifimethError, match=r"CHG.*conv5"):
        MethylationCaller(model_dir=directory("a", "CHG", conv5(7e4)), device=0)
    with pytest.raises(HifimethError, match=r"CHG.*conv5"):
        MethylationCaller(model_dir=directory("b", "CHG", conv5(-np.inf)), device=0)
    with pytest.raises(HifimethError, match=r"CHH.*fc2 bias"):
        MethylationCaller(model_dir=directory("c", "CHH", lambda w: w.fc2_b.__setitem__(1, np.nan)), device=0)
    # CpG is context 0: the CHG model of the same directory is never read when only CpG is asked for
    with MethylationCaller(model_dir=directory("d", "CHG", conv5(7e4)), contexts="cpg", device=0) as m:
        assert len(m.call(_reads()[:1])) > 0
    # conv1 x slope: 6e4 is a finite fp16 itself, times a one-hot slope gamma / sd > 1.1 it is not
    w = models.random_model("CpG")
    slope = np.abs(w.bn_gamma[:4]) / np.sqrt(w.bn_var[:4] + w.bn_eps)
    ch = int(np.argmax(slope))
    assert slope[ch] > 1.2
    with pytest.raises(HifimethError, match=r"CpG.*conv1 folded"):
        MethylationCaller(model_dir=directory("e", "CpG", lambda w: w.conv_w[0].__setitem__((3, ch, 2), 6e4)), device=0)
    with MethylationCaller(model_dir=directory("f", "CHG", conv5(6e4)), device=0) as m:
        assert m.debug_layer(1, np.zeros((401, 8), np.float32), 1).shape == (197, 128)   # K1 = 11: (401 + 2 - 11) // 2 + 1 rows
