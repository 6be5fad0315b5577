"""Plain fp64 CPU reference of the CNN (torch, float64), for the logit tests.

bn0 -> 8 x (Conv1d stride 2, padding 1, + bias, ReLU) -> channels-first flatten -> fc1 + ReLU -> fc2, from the .hmw weights.
`zero_outside=True` (tests only) is a WRONG network on purpose: window rows outside the read become zeros BEHIND bn0 instead of bn0(0) --
what a trunk step or a padding tap that took a zero row for the constant one would compute; the short-read tests show that their bar
rejects it.  `split=True` simulates the device's split-half ("f16x3") arithmetic instead: both operands of every layer are split into
fp16 hi + lo halves, the layer sums w_hi*x_hi + w_hi*x_lo + w_lo*x_hi (exactly, in fp64) and its output is rounded to fp32.
Layers named in `drop_wlo` ("conv1" .. "conv8", "fc1", "fc2") lose their w_lo*x_hi term (plain fp16 weights).
"""
import numpy as np
import torch
import torch.nn.functional as F

from hifimeth_amd.onnx_weights import load_hmw

CHUNK = 2048    # windows per pass: conv1 of 2048 windows already holds 2048 x 128 x 201 doubles
LAYERS = tuple(f"conv{i}" for i in range(1, 9)) + ("fc1", "fc2")


def _halves(t):
    hi = t.to(torch.float16).to(torch.float64)
    return hi, (t - hi).to(torch.float16).to(torch.float64)


class CNN64:
    def __init__(self, hmw_path, split=False, drop_wlo=(), zero_outside=False):
        w = load_hmw(hmw_path)
        d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        self.bn = (d(w.bn_mean), d(w.bn_gamma) / torch.sqrt(d(w.bn_var) + float(w.bn_eps)), d(w.bn_beta))
        self.layers = [(d(cw), d(cb)) for cw, cb in zip(w.conv_w, w.conv_b)] + [(d(w.fc1_w), d(w.fc1_b)), (d(w.fc2_w), d(w.fc2_b))]
        self.split = split
        self.zero_outside = zero_outside
        assert set(drop_wlo) <= set(LAYERS), drop_wlo
        self.drop = set(drop_wlo)

    def _layer(self, i, x):
        w, b = self.layers[i]
        op = (lambda a, k: F.conv1d(a, k, stride=2, padding=1)) if i < 8 else (lambda a, k: a @ k.T)
        if not self.split:
            y = op(x, w)
        else:
            x = x.to(torch.float32).to(torch.float64)          # the layer's input as the device holds it (fp32)
            xh, xl = _halves(x)
            wh, wl = _halves(w)
            y = op(xh, wh if LAYERS[i] in self.drop else wh + wl) + op(xl, wh)
        y = y + (b[:, None] if i < 8 else b)
        if i < 9:
            y = torch.relu(y)
        return y.to(torch.float32).to(torch.float64) if self.split else y

    def logits(self, windows):
        """windows [n, 401, 8] -> logits [n, 2] float64."""
        windows = np.asarray(windows, np.float32).reshape(-1, 401, 8)
        out = np.empty((len(windows), 2), np.float64)
        mean, scale, beta = self.bn
        with torch.no_grad():
            for a in range(0, len(windows), CHUNK):
                x = torch.from_numpy(windows[a:a + CHUNK].astype(np.float64)).transpose(1, 2)   # [n, 8, 401]
                # rows outside the read are the rows the window builder leaves all zero (inside a read an N with four zero kinetics codes
                # would look the same)
                outside = (x == 0).all(dim=1, keepdim=True)
                x = (x - mean[:, None]) * scale[:, None] + beta[:, None]
                if self.zero_outside:
                    x = torch.where(outside, torch.zeros_like(x), x)
                for i in range(8):
                    x = self._layer(i, x)
                x = x.reshape(x.shape[0], -1)             # [n, 64, 2] -> c * 2 + l
                for i in (8, 9):
                    x = self._layer(i, x)
                out[a:a + CHUNK] = x.numpy()
        return out


def reference_sites(oracle, reads, models, min_len=1000):
    """Every context's sites of the reads the engine calls, in its (read, qoff) order, with the logits of the oracle's
    windows under each of `models` ({name: [CpG, CHG, CHH] objects with .logits(windows)}).  Per context a dict of
    rid, qoff, strand, stratum (0: the window hangs over the read's start, qoff < 200; 2: over its end, qoff >= L - 200;
    1: neither; 3: over both, which takes a read of at most 399 bases) and one [n, 2] array per model name."""
    out = []
    for c in range(3):
        cols = {k: [] for k in ("rid", "qoff", "strand", "stratum")}
        lg = {k: [] for k in models}
        pend = []

        def flush():
            if pend:
                w = np.concatenate(pend)
                for k, ms in models.items():
                    lg[k].append(np.asarray(ms[c].logits(w)))
                pend.clear()
        for i, rd in enumerate(reads):
            if not rd.has_kinetics() or rd.l_qseq < min_len:
                continue
            fwd = oracle.decode(rd)
            offs = np.sort(oracle.scan(fwd, c))
            if len(offs) == 0:
                continue
            w, s = oracle.windows(rd, fwd, offs)
            pend.append(w)
            if sum(len(p) for p in pend) >= CHUNK:
                flush()
            cols["rid"].append(np.full(len(offs), i, np.int32))
            cols["qoff"].append(offs.astype(np.int32))
            cols["strand"].append(s)
            cols["stratum"].append(stratum_of(offs, rd.l_qseq))
        flush()
        d = {k: np.concatenate(v) if v else np.empty(0, np.int32) for k, v in cols.items()}
        d.update({k: np.concatenate(v) if v else np.empty((0, 2)) for k, v in lg.items()})
        out.append(d)
    return out


STRATA = ("start", "middle", "end")
ALL_STRATA = STRATA + ("both",)      # "both": a short read's site whose window hangs over the read's start AND its end


def stratum_of(offs, L):
    """0 start / 1 middle / 2 end as ever (for L >= 400 no site is both), 3 where qoff < 200 and qoff >= L - 200."""
    offs = np.asarray(offs)
    st = np.where(offs < 200, 0, np.where(offs >= L - 200, 2, 1))
    return np.where((offs < 200) & (offs >= L - 200), 3, st).astype(np.int8)


def strata(site, ctx, names=STRATA):
    """{name: boolean mask} of the strata a context's errors are bounded in: read start / middle / end, and for CHH also
    by strand.  `names`: the strata asked for -- sets of reads of 1000 bases and more have the three of STRATA, a set with reads
    under 400 bases also "both" (ALL_STRATA), a set of nothing but such reads only that one."""
    st = site["stratum"]
    ks = [ALL_STRATA.index(n) for n in names]
    if ctx < 2:
        return {ALL_STRATA[k]: st == k for k in ks}
    return {f"{ALL_STRATA[k]}/{'fwd' if s == 0 else 'rev'}": (st == k) & (site["strand"] == s) for k in ks for s in (0, 1)}


def site_errors(got, ref):
    """Per site: max_k |l_k - l64_k| / (1 + max_k |l64_k|)."""
    got = np.asarray(got, np.float64).reshape(-1, 2)
    ref = np.asarray(ref, np.float64).reshape(-1, 2)
    return np.abs(got - ref).max(axis=1) / (1.0 + np.abs(ref).max(axis=1))


def bar(e_oracle):
    """The bar for a context: 8 x the fp32 oracle's own error against fp64 (floor 1e-6)."""
    return 8.0 * max(float(e_oracle), 1e-6)
