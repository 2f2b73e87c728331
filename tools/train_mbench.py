#!/usr/bin/env python3
"""One training step of the MLP mapper (GPT-2 frozen), this project's kernels against torch autograd.

    zsaac : MapperTrainer.step -- forward, backward (zs_attention_bwd, zs_layernorm_bwd,
            zs_gelu_tanh_bwd, zs_gemm on transposed weights, the LM-head gradient without logits),
            zs_adamw
    torch : the same step by autograd over the oracle's code (oracle/caption.py: mlp_mapper,
            gpt2_logits) on the same device, the mapper's four tensors the only parameters,
            torch.optim.AdamW.  bf16: f32 master parameters cast to bf16 in the forward, every
            other weight bf16.

The reference's batch of 40 clips, captions of 25 tokens, synthetic weights.  The hard prompts
are given and of one length (11 ids), so the torch route runs all 40 sequences as one batch (the
ragged layout would cost it a Python loop over clips; zsaac takes ragged prompts either way).

Times are device events around REPS back-to-back steps after a warm-up, the two routes
alternating over ROUNDS rounds (min / median / max of the per-step time per route), so a drift of
the shared machine shows as spread, not as a difference.  The first step's loss of both routes
is printed beside each other.

    python tools/train_mbench.py [out.txt [bf16,f32]]
    python tools/train_mbench.py --steps N bf16|f32     # zsaac steps only (for a kernel trace)
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zero-shot-aac_amd"), ROOT):
    sys.path.insert(0, p)

B, T, H = 40, 25, 11
ROUNDS, REPS = 5, 3
LR, WD = 1e-5, 0.01
KEYS = ("clap_project.model.0.weight", "clap_project.model.0.bias",
        "clap_project.model.2.weight", "clap_project.model.2.bias")


def setup(dtype, dev):
    from zsaac import synthetic as S
    from zsaac.pipeline import CaptionConfig, CaptionPipeline
    from zsaac.train import MapperTrainer
    sd = S.gpt2_state_dict()
    sd.update(S.mlp_mapper_state_dict(1))
    pipe = CaptionPipeline(sd, None, S.label_table(), S.label_token_table(),
                           CaptionConfig(dtype=dtype, batch=B), device=dev)
    g = torch.Generator().manual_seed(0)
    emb = S.synthetic_clap_embeddings(B).to(dev)
    caps = torch.randint(0, 50257, (B, T), generator=g, dtype=torch.int32)
    hard = torch.randint(0, 50257, (B, H), generator=g, dtype=torch.int32).to(dev)
    hlen = torch.full((B,), H, dtype=torch.int32, device=dev)
    tr = MapperTrainer(pipe, sd, lr=LR, weight_decay=WD, max_caption_tokens=T)
    cap_dev = (caps.to(dev), torch.full((B,), T, dtype=torch.int32, device=dev))
    return sd, tr, emb, caps, cap_dev, (hard, hlen)


def torch_route(sd, dtype, dev, emb, caps, hard):
    from oracle import caption as OC
    sdt = {k: (v.to(device=dev, dtype=dtype) if v.is_floating_point() else v.to(dev))
           for k, v in sd.items()}
    params = [sd[k].to(device=dev, dtype=torch.float32).clone().requires_grad_(True) for k in KEYS]
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD, betas=(0.9, 0.999), eps=1e-8)
    wte = sdt["gpt.transformer.wte.weight"]
    prefix = torch.nn.functional.normalize(emb, dim=-1).to(dtype)
    ids, hl = caps.to(dev).long(), hard.long()
    P = H + 10

    def step():
        opt.zero_grad(set_to_none=True)
        for k, p in zip(KEYS, params):
            sdt[k] = p.to(dtype)
        soft = OC.mlp_mapper(prefix, sdt).reshape(B, 10, -1)
        x = torch.cat((wte[hl], soft, wte[ids[:, :-1]]), dim=1)
        with torch.device(dev):                 # the oracle builds its causal mask where torch puts it
            logits = OC.gpt2_logits(x, sdt)[0][:, P - 1:]
        loss = torch.nn.functional.cross_entropy(logits.reshape(B * T, -1).float(), ids.reshape(-1))
        loss.backward()
        opt.step()
        return loss.detach()
    return step


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main(out_path=None, only=None):
    assert torch.cuda.is_available(), "train_mbench needs the GPU (no fallback)"
    dev = torch.device("cuda", 0)
    lines = [f"train_mbench: one training step, batch {B}, captions of {T} tokens, hard prompts of "
             f"{H} ids; {ROUNDS} alternating rounds of {REPS} steps; per-step time in ms "
             "(min / median / max)"]
    for dn, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        if only and dn not in only.split(","):
            continue
        sd, tr, emb, caps, cap_dev, hard = setup(dtype, dev)
        ours = lambda: tr.step(emb, cap_dev, hard=hard)
        theirs = torch_route(sd, dtype, dev, emb, caps, hard[0])
        l0, l1 = float(ours()), float(theirs())               # the first step of both, also warm-up
        window(ours, 1), window(theirs, 1)
        to, tt = [], []
        for _ in range(ROUNDS):
            to.append(window(ours, REPS))
            tt.append(window(theirs, REPS))
        tr.check()
        mo, mt = statistics.median(to), statistics.median(tt)
        for name, ts, md in (("zsaac", to, mo), ("torch", tt, mt)):
            lines.append(f"{dn:4s} {name} {min(ts):8.2f} / {md:8.2f} / {max(ts):8.2f} ms per step")
        lines.append(f"{dn:4s} torch / zsaac (medians) {mt / mo:5.2f}x; first-step loss zsaac {l0:.4f} "
                     f"torch {l1:.4f}")
        del tr, theirs, sd
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def steps_only(n, dn):
    dev = torch.device("cuda", 0)
    sd, tr, emb, caps, cap_dev, hard = setup(torch.bfloat16 if dn == "bf16" else torch.float32, dev)
    for _ in range(n):
        tr.step(emb, cap_dev, hard=hard)
    torch.cuda.synchronize()
    tr.check()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--steps":
        steps_only(int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else "bf16")
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None, sys.argv[2] if len(sys.argv) > 2 else None)
