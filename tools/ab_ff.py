#!/usr/bin/env python
"""Gate of the fused feed-forward launch (kernels.ff_fused_ln) against today's pair of launches on the level-0 shapes of cfg2, bf16,
LayerNorm-folded form: kernels.linear_geglu_ln, then kernels.conv2d of the [M, 1, 1, 1280] view with bias and residual (what
layers.gemm_linear issues).  The two alternate round by round in one process; minimum and median per variant over the rounds, and
whether the outputs have the same bits (else their relative L2 distance).
    python tools/ab_ff.py [--rounds R] [--iters N] [--m 655360,262144]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagine360_amd import kernels as K  # noqa: E402
from tools.bench_kernels import timeit  # noqa: E402

C, INNER = K.FF_FUSED_SHAPE


def operands(M, dt=torch.bfloat16, seed=0, dev="cuda"):
    """x (rows with a non-zero mean), its row statistics, the LayerNorm-folded packed operands of both GEMMs and a residual."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    x = (rn(M, C) + 0.3).to(dt).to(dev)
    w1, b1 = (rn(2 * INNER, C) * C ** -0.5).to(dt).to(dev), (rn(2 * INNER) * 0.1).to(dt).to(dev)
    w2, b2 = (rn(C, INNER) * INNER ** -0.5).to(dt).to(dev), (rn(C) * 0.1).to(dt).to(dev)
    gamma, beta = (1.0 + 0.1 * rn(C)).to(dt).to(dev), (0.1 * rn(C)).to(dt).to(dev)
    xs = x.float().reshape(M, C // K.ROW_SLICE, K.ROW_SLICE)
    stats = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).contiguous()
    wg, c1, c2 = K.fold_layer_norm(w1, b1, gamma, beta)
    wp, c1p = K.pack_geglu(wg, c1)
    c2p = K.interleave_geglu(wg, c2)[1].contiguous()
    w2p = K.pack_conv_weight(w2.reshape(C, INNER, 1, 1))
    return dict(x=x, stats=stats, wp=wp, c1p=c1p.contiguous(), c2p=c2p, w2p=w2p, b2=b2, eps=1e-5)


def pair(o, res):
    M = o["x"].shape[0]
    h = K.linear_geglu_ln(o["x"], o["wp"], o["c1p"], o["c2p"], o["stats"], o["eps"], INNER)
    return K.conv2d(h.reshape(M, 1, 1, INNER), o["w2p"], C, bias=o["b2"], res=res.reshape(M, 1, 1, C)).reshape(M, C)


def fused(o, res):
    return K.ff_fused_ln(o["x"], o["wp"], o["c1p"], o["c2p"], o["stats"], o["eps"], o["w2p"], o["b2"], res)


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 10
    ms = [int(v) for v in sys.argv[sys.argv.index("--m") + 1].split(",")] if "--m" in sys.argv else [655360, 262144]
    K.lib()
    print(f"device {torch.cuda.get_device_name(0)}  rounds {rounds} x {iters} launches, variants alternated", flush=True)
    for M in ms:
        o = operands(M)
        res = o["x"]                                  # the production call: the residual is x itself
        yp, yf = pair(o, res), fused(o, res)
        torch.cuda.synchronize()
        same = torch.equal(yp, yf)
        rel = float((yf.float() - yp.float()).norm() / yp.float().norm())
        tp, tf = [], []
        for _ in range(rounds):
            tp.append(timeit(lambda: pair(o, res), iters) * 1e3)
            tf.append(timeit(lambda: fused(o, res), iters) * 1e3)
        fl = 2.0 * M * C * 2 * INNER + 2.0 * M * INNER * C
        for name, t in (("pair", tp), ("fused", tf)):
            print(f"M {M:7d}  {name:5s} min {min(t):7.3f} ms  median {statistics.median(t):7.3f} ms  {fl / min(t) / 1e9:6.0f} TF/s", flush=True)
        print(f"M {M:7d}  fused / pair (min) {min(tf) / min(tp):.3f}  gain {100.0 * (1.0 - min(tf) / min(tp)):5.1f} %  "
              f"{'bit-identical' if same else f'bits differ: rel L2 {rel:.3e}'}", flush=True)
        del o, yp, yf


if __name__ == "__main__":
    main()
