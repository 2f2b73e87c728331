#!/usr/bin/env python3
"""Ranks of given gallery items, fused against the route available without the kernel.

    fused : zs_sim_rank                                   (no [M][N] matrix anywhere)
    torch : S = Q @ G.T in the same dtype, tsim = S.gather(tgt), then (S > tsim[:, t, None]).sum(1)
            per target, chunked over the queries where S would not fit CHUNK_BYTES

at two sizes:

    clotho : Clotho-eval t2a, M 5225 queries x N 1045 gallery, K 1024, T 1, bf16 and f32
    bank   : a caption bank against itself, M = N = 65536, K 1024, T 5, bf16; targets once the
             query's own group of 5 consecutive rows (a bank of 5 captions per clip: the first pass
             visits the diagonal tiles only) and once uniformly random (its worst case)

Times are device events around REPS back-to-back calls after a warm-up of every shape, the two
routes alternating over ROUNDS rounds (min / median / max of the per-call time per route), so a
drift of the shared machine shows as spread, not as a difference.  TF/s counts the 2 M N K flops
of ONE product per call, whatever the route spends.  The fused ranks of the first 256 queries are
compared first with strict counts over an f32 product of the same operands (near-ties may differ
by the accumulation order; the timed torch route itself rounds S to its dtype).

    python tools/retrieval_mbench.py [out.txt [clotho-bf16,clotho-f32,bank-group,bank-random]]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zero-shot-aac_amd"))

K = 1024
ROUNDS = 5
CHUNK_BYTES = 2 << 30


def unit_rows(n, gen, dtype, dev):
    x = torch.randn(n, K, generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).to(dtype).to(dev)


def main(out_path=None, only=None):
    from zsaac import ops
    assert torch.cuda.is_available(), "retrieval_mbench needs the GPU (no fallback)"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(0)
    lines = [f"retrieval_mbench: rank of T given gallery items per query, K {K}; {ROUNDS} "
             f"alternating rounds; per-call time in ms (min / median / max)"]
    sizes = [("clotho", 5225, 1045, 1, torch.bfloat16, "group", 20),
             ("clotho", 5225, 1045, 1, torch.float32, "group", 20),
             ("bank", 65536, 65536, 5, torch.bfloat16, "group", 2),
             ("bank", 65536, 65536, 5, torch.bfloat16, "random", 2)]
    for name, M, N, T, dtype, layout, reps in sizes:
        dn = "bf16" if dtype == torch.bfloat16 else "f32"
        if only and f"{name}-{dn if name == 'clotho' else layout}" not in only.split(","):
            continue
        q, g = unit_rows(M, gen, dtype, dev), unit_rows(N, gen, dtype, dev)
        if name == "clotho":                         # caption j's clip is j // 5
            tgt = (torch.arange(M) // 5)[:, None]
        elif layout == "group":
            # (the last group starts at N - T: M is no multiple of T and every target stays a row)
            tgt = torch.clamp(torch.arange(M) // T * T, max=N - T)[:, None] + torch.arange(T)[None, :]
        else:
            tgt = torch.randint(0, N, (M, T), generator=gen)
        # torch.gather checks its indices on the device and traps on one outside the row
        assert 0 <= int(tgt.min()) and int(tgt.max()) < N, "targets outside the gallery"
        tgt = tgt.to(torch.int32).to(dev).contiguous()
        idx = tgt.long()
        rank = torch.empty(M, T, dtype=torch.int32, device=dev)
        sim = torch.empty(M, T, device=dev)
        rows = max(1, min(M, CHUNK_BYTES // (N * q.element_size())))
        out = torch.empty(M, T, dtype=torch.int64, device=dev)

        def fused():
            ops.sim_rank(q, g, tgt, sim, rank)
            return rank

        def torch_route():
            for m0 in range(0, M, rows):
                s = q[m0:m0 + rows] @ g.t()
                ts = s.gather(1, idx[m0:m0 + rows])
                for t in range(T):
                    out[m0:m0 + rows, t] = (s > ts[:, t, None]).sum(1)
            return out

        # cross-check on the first rows against an f32 product of the same operands (the timed
        # torch route rounds S to its dtype: in bf16 its counts are those of the rounded values)
        nchk = min(M, 256)
        s32 = q[:nchk].float() @ g.float().t()
        r32 = torch.stack([(s32 > s32.gather(1, idx[:nchk])[:, t, None]).sum(1) for t in range(T)], 1)
        d = (fused()[:nchk].long() - r32).abs()
        differ = f"{int((d != 0).sum())} of {nchk * T} ranks differ from an f32 product's (max {int(d.max())})"
        torch_route()
        del s32

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
        flops = 2.0 * M * N * K
        mf, mt = statistics.median(tf), statistics.median(tt)
        tag = f"{name:6s} {dn:4s} M {M:5d} N {N:5d} T {T} targets {layout:6s}"
        lines.append(f"{tag}  fused {min(tf):8.3f} / {mf:8.3f} / {max(tf):8.3f} ms  "
                     f"{flops / mf / 1e9:7.1f} TF/s   ({reps} calls per window)")
        lines.append(f"{tag}  torch {min(tt):8.3f} / {mt:8.3f} / {max(tt):8.3f} ms  "
                     f"{flops / mt / 1e9:7.1f} TF/s   (S in chunks of {rows} rows)")
        cond = "fused min <= torch median: holds" if min(tf) <= mt else \
            "fused min <= torch median: FAILS"
        lines.append(f"{tag}  torch / fused (medians) {mt / mf:5.2f}x; {cond}; "
                     f"{differ}")
        del q, g, out
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, sys.argv[2] if len(sys.argv) > 2 else None)
