#!/usr/bin/env python3
"""Sampling a token per row: the fused kernel against what torch offers on the same logits, and
a sampled decode step against the stepwise greedy step.

    fused : zs_sample_rows                       (f32 logits [R, 50257] -> token, log-prob)
    torch : softmax, sort, cumsum, the nucleus mask, multinomial    (top_p 0.8)
            softmax, multinomial                                    (unfiltered)
    step  : one decode step of the bf16 stepwise decoder at R rows: sampled (layers, ln_f, LM-head
            GEMM to f32 logits, zs_sample_rows, zs_greedy_step) against the parent's stepwise
            greedy step (layers, ln_f, zs_lmhead_topk, zs_greedy_step; ZSAAC_GRID_DECODE=0)

Times are device events around REPS back-to-back calls after a warm-up of every shape, the
routes alternating over ROUNDS rounds (min / median / max of the per-call time per route), so a
drift of the shared machine shows as spread, not as a difference.

    python tools/sample_mbench.py [out.txt]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zero-shot-aac_amd"))
os.environ.setdefault("ZSAAC_GRID_DECODE", "0")      # the stepwise greedy step is the comparison

V = 50257
REPS, ROUNDS = 50, 7


def window(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def compare(lines, tag, routes):
    """routes: [(name, fn)], the first is the fused one."""
    for _, fn in routes:
        window(fn, 5)
    times = {name: [] for name, _ in routes}
    for _ in range(ROUNDS):
        for name, fn in routes:
            times[name].append(window(fn))
    med = {}
    for name, _ in routes:
        t = times[name]
        med[name] = statistics.median(t)
        lines.append(f"{tag}  {name:14s} {min(t):9.1f} / {med[name]:9.1f} / {max(t):9.1f} us")
    (a, _), (b, _) = routes[0], routes[1]
    verdict = ("first faster" if max(times[a]) < min(times[b]) else
               "FIRST SLOWER" if min(times[a]) > max(times[b]) else "within the spread")
    lines.append(f"{tag}  {b} / {a} (medians) {med[b] / med[a]:6.2f}x: {verdict}")


def main(out_path=None):
    from zsaac import ops
    from zsaac import synthetic as S
    from zsaac.decoder import Gpt2Decoder, Gpt2Weights
    assert torch.cuda.is_available(), "sample_mbench needs the GPU (no fallback)"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    lines = [f"sample_mbench: V {V}; {REPS} calls per window, {ROUNDS} alternating rounds; "
             f"per-call time in us (min / median / max)"]
    Vp = -(-V // 4) * 4
    for R in (64, 256):
        logits = torch.empty(R, Vp, device=dev)[:, :V]
        logits.copy_((torch.randn(R, V, generator=g) * 4.0).to(dev))
        ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        pv, pi = torch.empty(R, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
        lp = torch.empty(R, device=dev)

        def fused(p):
            return lambda: ops.sample_rows(logits, ctr, 1, pv, pi, top_p=p, logprob=lp)

        def torch_top_p():
            pr = torch.softmax(logits, -1)
            sp, si = torch.sort(pr, -1, descending=True)
            before = torch.cumsum(sp, -1) - sp
            sp = torch.where(before <= 0.8, sp, torch.zeros((), device=dev))
            return si.gather(1, torch.multinomial(sp, 1))

        def torch_plain():
            return torch.multinomial(torch.softmax(logits, -1), 1)

        compare(lines, f"R {R:3d} top_p 0.8 ", [("fused", fused(0.8)), ("torch", torch_top_p)])
        compare(lines, f"R {R:3d} unfiltered", [("fused", fused(1.0)), ("torch", torch_plain)])

    # one decode step at R rows, bf16, stepwise
    sd = S.gpt2_state_dict(seed=0, std=0.1, emb_std=0.1, stop_boost=2.0)
    w = Gpt2Weights(sd, dev, torch.bfloat16)
    for R in (64,):
        dec = Gpt2Decoder(w, R, 32, 67, use_graph=False, persist=False)
        assert not dec.grid_decode
        dec.plen.fill_(20)
        for t in dec.kc + dec.vc:
            t.zero_()
        ops.greedy_init(R, dec.plen, dec.pos, dec.done, dec.out_len, dec.out_ids, dec.max_steps,
                        dec.step_ctr, dec.all_done)
        b, _ = dec._sample_buffers(R, False)
        rows = torch.arange(R, device=dev, dtype=torch.int32)
        dec.kvrow[:R].copy_(rows[:, None].expand(R, dec.Lmax))

        def rearm():
            dec.step_ctr.zero_(), dec.done.zero_(), dec.pos.fill_(19)

        def sampled():
            rearm()
            dec._decode_forward(R, kvrow=dec.kvrow[:R])
            ops.gemm(dec.hf[:R], w.wte, b["logits"][:R], split_k=1)
            ops.sample_rows(b["logits"][:R], dec.step_ctr, 1, b["pv"], b["pi"], top_p=0.8,
                            logprob=b["lp"])
            ops.greedy_step(b["pv"], b["pi"], R, 1, dec.step_ctr, dec.max_steps, -1, -1,
                            dec.out_ids, dec.out_len, dec.done, dec.pos, dec.next_tok, dec.all_done)

        def greedy():
            rearm()
            dec._greedy_step_body(R)

        compare(lines, f"step R {R:3d} bf16", [("sampled", sampled), ("greedy", greedy)])
        t_head = window(lambda: ops.gemm(dec.hf[:R], w.wte, b["logits"][:R], split_k=1))
        t_topk = window(lambda: ops.lmhead_topk(dec.hf[:R], w.wte, 1, None, dec.pval1, dec.pidx1))
        lines.append(f"step R {R:3d} bf16  of which: LM-head GEMM to f32 logits {t_head:8.1f} us "
                     f"(greedy's fused LM-head argmax {t_topk:8.1f} us)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
