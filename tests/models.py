"""Model directories other than the shipped one, made at test time, and the read set the model tests run on.

The engine takes any directory of {CpG,CHG,CHH}.hmw / .onnx with the right geometry; these are the directories the tests give it
besides hifimeth_amd/weights.  Everything is seeded, nothing is committed as a binary.

    swapped     CpG.hmw and CHG.hmw are the shipped CHH model (k1 = 13), CHH.hmw is the shipped CpG model (k1 = 11): whatever the
                engine keys on the context slot instead of the model shows.
    random      k1 = 13 for CpG, 11 for CHG and CHH.  Conv and fc weights N(0, variance 2 / fan_in) (He), biases N(0, sd 0.1),
                bn0 gamma in +-[0.5, 2] with three or four negative, beta N(0, sd 0.3), mean and var drawn from the shipped ranges
                of the channel group (one-hot: mean 0.17 .. 0.33, var 0.14 .. 0.22; kinetics: mean 0.02 .. 0.032, var 1e-4 .. 2e-3,
                log-uniform), conv6's bias all zero (the ONNX form leaves that input out).
    scaled(k)   the shipped three with conv2, conv4 and conv7 (weights and bias) times 2^k and conv3, conv5 and conv8 (weights) times
                2^-k.  ReLU is positively homogeneous and the scaling is exact, so the function the model computes is unchanged.
"""
import os

import numpy as np

from conftest import WEIGHTS
from hifimeth_amd.onnx_weights import CHANNELS, FC1_OUT, N_CLASSES, ModelWeights, load_hmw, save_hmw
from hifimeth_amd.synth import read_from_ascii

NAMES = ("CpG", "CHG", "CHH")
RANDOM_K1 = {"CpG": 13, "CHG": 11, "CHH": 11}
RANDOM_SEED = {"CpG": 1301, "CHG": 1102, "CHH": 1103}
SCALED_UP, SCALED_DOWN = (1, 3, 6), (2, 4, 7)     # conv2, conv4, conv7 | conv3, conv5, conv8 (0-based)


def shipped(name):
    return load_hmw(os.path.join(WEIGHTS, name + ".hmw"))


def write_dir(path, models):
    """{context name: ModelWeights} -> path/<name>.hmw; returns path."""
    os.makedirs(path, exist_ok=True)
    for name, w in models.items():
        save_hmw(w, os.path.join(path, name + ".hmw"))
    return str(path)


def swapped_models():
    return {"CpG": shipped("CHH"), "CHG": shipped("CHH"), "CHH": shipped("CpG")}


def random_model(name):
    rng = np.random.default_rng(RANDOM_SEED[name])
    k1 = RANDOM_K1[name]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    he = lambda shape, fan_in: f32(rng.normal(0.0, np.sqrt(2.0 / fan_in), shape))
    gamma = rng.uniform(0.5, 2.0, 8)
    neg = [int(rng.integers(0, 4)), int(rng.integers(4, 8))]          # one one-hot and one kinetics channel at least
    neg += [int(c) for c in rng.choice([c for c in range(8) if c not in neg], int(rng.integers(1, 3)), replace=False)]
    gamma[neg] *= -1.0
    mean = np.concatenate([rng.uniform(0.17, 0.33, 4), rng.uniform(0.02, 0.032, 4)])
    var = np.concatenate([rng.uniform(0.14, 0.22, 4), np.exp(rng.uniform(np.log(1e-4), np.log(2e-3), 4))])
    conv_w, conv_b = [], []
    for i in range(8):
        k = k1 if i == 0 else 3
        conv_w.append(he((CHANNELS[i + 1], CHANNELS[i], k), CHANNELS[i] * k))
        conv_b.append(f32(rng.normal(0.0, 0.1, CHANNELS[i + 1])))
    conv_b[5][:] = 0.0
    w = ModelWeights(k1, float(np.float32(1e-5)), f32(gamma), f32(rng.normal(0.0, 0.3, 8)), f32(mean), f32(var), conv_w, conv_b,
                     he((FC1_OUT, 128), 128), f32(rng.normal(0.0, 0.1, FC1_OUT)),
                     he((N_CLASSES, FC1_OUT), FC1_OUT), f32(rng.normal(0.0, 0.1, N_CLASSES)))
    assert int((w.bn_gamma < 0).sum()) >= 3 and (np.abs(w.bn_gamma) >= 0.5).all() and (np.abs(w.bn_gamma) <= 2.0).all()
    return w


def random_models():
    return {n: random_model(n) for n in NAMES}


def scale_pairs(w, k):
    """`w` with the three layer pairs rescaled by 2^k (in place; returns w)."""
    up, down = np.float32(2.0) ** k, np.float32(2.0) ** -k
    for i in SCALED_UP:
        w.conv_w[i] = w.conv_w[i] * up
        w.conv_b[i] = w.conv_b[i] * up
    for i in SCALED_DOWN:
        w.conv_w[i] = w.conv_w[i] * down
    return w


def scaled_models(k):
    return {n: scale_pairs(shipped(n), k) for n in NAMES}


def make(kind, path):
    """kind: "swapped", "random" or "scaled<k>" (k signed, e.g. "scaled-6") -> the directory written at `path`."""
    if kind == "swapped":
        return write_dir(path, swapped_models())
    if kind == "random":
        return write_dir(path, random_models())
    assert kind.startswith("scaled"), kind
    return write_dir(path, scaled_models(int(kind[len("scaled"):])))


def model_reads():
    """8544 bases: the exact minimum length stored unmapped, a chunk-boundary length stored reversed with wide kinetics, a
    length just over two chunks, a CG repeat, both homopolymers and an N-laden repeat (tests/test_gpu_parity.py:_mixed_reads)."""
    from test_gpu_parity import _kin
    rng = np.random.default_rng(2718)
    reads = []
    for L, flag in ((1000, 4), (1025, 16), (2049, 0)):
        seq = "".join("ACGT"[i] for i in rng.choice(4, L))
        reads.append(read_from_ascii(seq.encode(), *_kin(L, rng, wide=(L == 1025)), flag=flag))
    reads.append(read_from_ascii(b"CG" * 600, *_kin(1200, rng)))
    reads.append(read_from_ascii(b"C" * 1100, *_kin(1100, rng)))
    reads.append(read_from_ascii(b"G" * 1030, *_kin(1030, rng)))
    reads.append(read_from_ascii((b"ACGTNCGNNCCGCANGCTGGGNAAGNTTGCNAACCNGG" * 30), *_kin(38 * 30, rng)))
    return reads
