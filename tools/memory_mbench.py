#!/usr/bin/env python3
"""Projection onto a text memory bank, fused against the route torch offers.

    fused : zs_memory_project + zs_memory_merge          (one pass over the bank, no [M][N] array)
    torch : ((q @ T.T) * 100).softmax(-1) @ T in the same dtype on the same device, the bank in
            chunks where the [M][N] logits would not fit CHUNK_BYTES (chunks combined by their
            log-sum-exp)

M = 64 queries, K = 1024, banks of N = 65 536 and 1 048 576 rows, bf16 and f32.

Times are device events around REPS back-to-back calls after a warm-up of every shape, the two
routes alternating over ROUNDS rounds (min / median / max of the per-call time per route), so a
drift of the shared machine shows as spread, not as a difference.  Per size: the achieved bytes/s
over the algorithmic N * K * sizeof (the bank read once) beside the 6.29 TB/s a device copy
measures on this part, and TF/s over the 4 M N K flops of the two products.  The fused result is
compared first with the torch route's in f32.

    python tools/memory_mbench.py [out.txt [bf16-65536,bf16-1048576,f32-65536,f32-1048576]]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zero-shot-aac_amd"))

M, K = 64, 1024
SCALE = 100.0
ROUNDS = 5
CHUNK_BYTES = 1 << 30
COPY_TBS = 6.29


def unit_rows(n, gen, dtype, dev):
    out = torch.empty(n, K, dtype=dtype, device=dev)
    for r0 in range(0, n, 1 << 16):                      # a 4 GiB bank in pieces, made on the device
        x = torch.randn(min(1 << 16, n - r0), K, generator=gen, device=dev)
        out[r0:r0 + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).to(dtype)
    return out


def main(out_path=None, only=None):
    from zsaac import ops
    assert torch.cuda.is_available(), "memory_mbench needs the GPU (no fallback)"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"memory_mbench: softmax({SCALE:g} q T^T) T, M {M}, K {K}; {ROUNDS} alternating rounds; "
             f"per-call time in ms (min / median / max); device copy rate {COPY_TBS} TB/s"]
    sizes = [(torch.bfloat16, 1 << 16, 20), (torch.bfloat16, 1 << 20, 4),
             (torch.float32, 1 << 16, 10), (torch.float32, 1 << 20, 2)]
    for dtype, N, reps in sizes:
        dn = "bf16" if dtype == torch.bfloat16 else "f32"
        if only and f"{dn}-{N}" not in only.split(","):
            continue
        q, bank = unit_rows(M, gen, dtype, dev), unit_rows(N, gen, dtype, dev)
        ns = ops.memory_nsplit(N, K, dtype)
        pm = torch.empty(M, ns, K, device=dev)
        pl = torch.empty(M, ns, 2, device=dev)
        out = torch.empty(M, K, device=dev)
        rows = max(1, min(N, CHUNK_BYTES // (M * 4)))

        def fused():
            ops.memory_project(q, bank, SCALE, ns, pm, pl)
            ops.memory_merge(pm, pl, M, ns, K, out, False, None)
            return out

        def torch_route():
            if rows >= N:
                return ((q @ bank.T) * SCALE).softmax(dim=-1) @ bank
            acc, lse = None, None
            for n0 in range(0, N, rows):
                t = bank[n0:n0 + rows]
                z = (q @ t.T).float() * SCALE
                l = torch.logsumexp(z, dim=-1, keepdim=True)
                part = ((z - l).exp().to(dtype) @ t).float()
                if acc is None:
                    acc, lse = part, l
                else:
                    new = torch.logaddexp(lse, l)
                    acc = acc * (lse - new).exp() + part * (l - new).exp()
                    lse = new
            return acc

        a, b = fused().float(), torch_route().float()
        differ = f"max |fused - torch| {float((a - b).abs().max()):.2e} (max |torch| {float(b.abs().max()):.2e})"

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

        for fn in (fused, torch_route):
            window(fn)                                   # warm-up of every shape
        tf, tt = [], []
        for _ in range(ROUNDS):
            tf.append(window(fused))
            tt.append(window(torch_route))
        nbytes, flops = float(N) * K * q.element_size(), 4.0 * M * N * K
        mf, mt = statistics.median(tf), statistics.median(tt)
        tag = f"{dn:4s} N {N:7d} nsplit {ns:3d}"
        for name, ts, md in (("fused", tf, mf), ("torch", tt, mt)):
            lines.append(f"{tag}  {name} {min(ts):8.3f} / {md:8.3f} / {max(ts):8.3f} ms  "
                         f"{nbytes / md / 1e9:6.2f} TB/s of the bank ({nbytes / md / 1e9 / COPY_TBS:5.1%} of "
                         f"copy)  {flops / md / 1e9:7.1f} TF/s   ({reps} calls per window)")
        cond = "fused min < torch median: holds" if min(tf) < mt else "fused min < torch median: FAILS"
        lines.append(f"{tag}  torch / fused (medians) {mt / mf:5.2f}x; {cond}; {differ}")
        del q, bank, pm
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, sys.argv[2] if len(sys.argv) > 2 else None)
