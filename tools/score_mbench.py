#!/usr/bin/env python3
"""The LM-head stage of caption scoring, fused against the route the package had before it.

    fused : zs_lmhead_nll + zs_nll_finalize            (hidden rows -> per-token log-prob)
    parent: zs_gemm to full f32 logits [M, 50257] (ZsGPT2LMHeadModel.forward's vocab GEMM) +
            torch.log_softmax + gather

on the same bf16 rows, M = 1280 (64 clips x 20 scored tokens) and M = 64, V = 50257, K = 768.
Times are device events around REPS back-to-back calls after a warm-up of every shape, the two
routes alternating over ROUNDS rounds (min / median / max of the per-call time per route), so a
drift of the shared machine shows as spread, not as a difference.  Algorithmic bytes are computed
from the shapes.  Both routes' log-probs are compared on the same inputs first.

    python tools/score_mbench.py [out.txt]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zero-shot-aac_amd"))

V, K = 50257, 768
REPS, ROUNDS = 200, 7


def algorithmic_bytes(M):
    """(fused, parent) bytes the two routes must move: W and A once each; the fused route's
    partials ([M][nblk] x (2 stats + value + index), written and read once); the parent's f32
    logits written by the GEMM, read and written by log_softmax, gathered."""
    nblk = -(-V // 128)
    base = V * K * 2 + M * K * 2
    fused = base + 2 * M * nblk * 16 + M * 24
    parent = base + M * V * 4 * 3 + M * 12
    return fused, parent


def main(out_path=None):
    from zsaac import ops
    assert torch.cuda.is_available(), "score_mbench needs the GPU (no fallback)"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    w = (torch.randn(V, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    nblk = ops.lmhead_nblk(V)
    lines = [f"score_mbench: LM-head stage of scoring, bf16, V {V}, K {K}; {REPS} calls per "
             f"window, {ROUNDS} alternating rounds; per-call time in us (min / median / max)"]
    for M in (1280, 64):
        a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
        tgt = torch.randint(0, V, (M,), generator=g).to(torch.int32).to(dev)
        ps = torch.empty(M, nblk, 2, device=dev)
        pv = torch.empty(M, nblk, device=dev)
        pi = torch.empty(M, nblk, device=dev, dtype=torch.int32)
        tl = torch.zeros(M, device=dev)
        lp, am = torch.zeros(M, device=dev), torch.zeros(M, device=dev, dtype=torch.int32)
        sm, cnt = torch.zeros(1, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
        logits = torch.empty(M, V, device=dev)
        idx = tgt.long()[:, None]

        def fused():
            ops.lmhead_nll(a, w, tgt, ps, pv, pi, tl)
            ops.nll_finalize(ps, pv, pi, tgt, tl, V, 1, M, lp, am, sm, cnt)
            return lp

        def parent():
            ops.gemm(a, w, logits, split_k=1)
            return torch.log_softmax(logits, -1).gather(1, idx)[:, 0]

        diff = float((fused() - parent()).abs().max())

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / REPS

        for fn in (fused, parent):
            window(fn)                                   # warm-up of every shape
        tf, tp = [], []
        for _ in range(ROUNDS):
            tf.append(window(fused))
            tp.append(window(parent))
        bf, bp = algorithmic_bytes(M)
        mf, mp = statistics.median(tf), statistics.median(tp)
        lines.append(f"M {M:5d}  fused  {min(tf):8.1f} / {mf:8.1f} / {max(tf):8.1f} us   "
                     f"{bf / 1e6:7.1f} MB algorithmic -> {bf / mf / 1e6:6.2f} TB/s")
        lines.append(f"M {M:5d}  parent {min(tp):8.1f} / {mp:8.1f} / {max(tp):8.1f} us   "
                     f"{bp / 1e6:7.1f} MB algorithmic -> {bp / mp / 1e6:6.2f} TB/s")
        verdict = "fused faster" if max(tf) < min(tp) else (
            "FUSED SLOWER" if min(tf) > max(tp) else "within the spread")
        lines.append(f"M {M:5d}  parent / fused (medians) {mp / mf:5.2f}x: {verdict}; "
                     f"max |logprob fused - parent| {diff:.2e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
