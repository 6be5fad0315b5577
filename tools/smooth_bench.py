#!/usr/bin/env python3
"""Time `smooth` on the card: hm_smooth_fetch over synthetic planes of 2^LOG2 positions at CHH density, for the half-widths
16, 500 and 16384, next to the floor -- hm_pileup_fetch_loci over the same range, which also writes one compacted row per locus
(24 B against 40 B).  Two times per leg: the whole call (count, write, the rows' copy to the host), and the call that only counts
(out NULL), which for the smoother is the running sums plus one evaluated window per locus (min_loci 2) and no copy.  The legs
alternate, so that a drift of the machine falls on all of them.  One JSON line.

usage: python tools/smooth_bench.py [--log2 30] [--density 0.25] [--repeat 3] [--check]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

HALF_WIDTHS = (16, 500, 16384)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="positions of the planes: 2^LOG2 (30: 1 Gbase, 12 GB of planes + 43 GB of running sums)")
    ap.add_argument("--density", type=float, default=0.25, help="share of the positions that carry a CHH locus")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="compare 20 000 loci around the middle with tests/smooth_ref.py")
    a = ap.parse_args()
    import torch
    from hifimeth_amd.pileup import LOCUS_DTYPE, SMOOTH_DTYPE, MethylationPileup
    n = 1 << a.log2
    gen = torch.Generator(device="cuda").manual_seed(9)
    on = torch.rand(n, device="cuda", generator=gen) < a.density
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    pc = torch.where(on, torch.randint(0, 8, (n,), dtype=torch.int32, device="cuda", generator=gen), zero)
    nc = torch.where(on, torch.randint(1, 8, (n,), dtype=torch.int32, device="cuda", generator=gen), zero)
    ky = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    del on, zero
    torch.cuda.synchronize()
    pu = MethylationPileup([("chr1", n)], bases=np.full(n, ord("N"), np.uint8), planes=(pc, nc, ky))
    L = pu._L
    n_rows = L.hm_pileup_fetch_loci(pu._h, None, None, None, 0, 0, n, None, 0)
    rows = np.zeros(n_rows, SMOOTH_DTYPE)                     # one host buffer for every leg: the loci rows are shorter
    ptr = rows.ctypes.data
    legs = {"loci": lambda: L.hm_pileup_fetch_loci(pu._h, None, None, None, 0, 0, n, ptr, n_rows),
            "loci_count": lambda: L.hm_pileup_fetch_loci(pu._h, None, None, None, 0, 0, n, None, 0)}
    for h in HALF_WIDTHS:
        legs[f"smooth_h{h}"] = lambda h=h: L.hm_smooth_fetch(pu._h, 0, 2, 0, n, h, 1, 1, ptr, n_rows)
        legs[f"smooth_h{h}_count"] = lambda h=h: L.hm_smooth_fetch(pu._h, 0, 2, 0, n, h, 1, 2, None, 0)
    times = {k: [] for k in legs}
    for k, leg in legs.items():                               # warm-up: the buffers, the code objects
        got = leg()
        assert got == n_rows or (k.endswith("_count") and 0 < got <= n_rows), (k, got, n_rows)
    for _ in range(a.repeat):
        for k, leg in legs.items():
            t0 = time.perf_counter()
            leg()
            times[k].append(time.perf_counter() - t0)
    best = {k: min(v) for k, v in times.items()}
    out = dict(smooth_positions=n, smooth_loci=int(n_rows), smooth_call_s={k: [round(x, 4) for x in v] for k, v in times.items()},
               smooth_best_s={k: round(v, 4) for k, v in best.items()},
               smooth_ratio_to_loci={f"h{h}": round(best[f"smooth_h{h}"] / best["loci"], 3) for h in HALF_WIDTHS},
               smooth_ratio_h16384_to_h16=round(best["smooth_h16384"] / best["smooth_h16"], 3),
               smooth_count_ratio_h16384_to_h16=round(best["smooth_h16384_count"] / best["smooth_h16_count"], 3))
    if a.check:
        sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests")))
        import smooth_ref as S
        lo, hi = n // 2 - 40000, n // 2 + 40000
        loci = np.zeros(hi - lo, LOCUS_DTYPE)
        m = L.hm_pileup_fetch_loci(pu._h, None, None, None, 0, lo, hi, loci.ctypes.data, hi - lo)
        same = True
        for h in HALF_WIDTHS:
            got = pu.fetch_smooth(2, lo + 17000, hi - 17000, half_width=h)
            same = same and got.tobytes() == S.smooth_prefix(loci[:m], [0, n], 2, h, lo=lo + 17000, hi=hi - 17000).tobytes() and len(got) > 0
        out["check_smooth_equals_reference"] = bool(same)
    pu.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
