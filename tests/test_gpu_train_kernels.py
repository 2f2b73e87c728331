"""The training kernels of csrc/train.hip, op by op, against tests/train_ref.py.

Tolerance, the project's rule (train_ref.tolerance = attn_ref.tolerance): error <= 4 x yardstick
+ 1e-6, the yardstick being the same formula in CPU float32 against float64 on the operands as
stored; a bf16 output is compared with the reference rounded by ``round_to`` and allowed one bf16
step of it (a value next to a rounding boundary may land on either side).  Copies, casts and the
variance-0 path are exact (torch.equal)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_ref as R  # noqa: E402
from gpu_helpers import Out  # noqa: E402

pytestmark = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAN = float("nan")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, got, ref64, ref32, bf16=False):
    yard, tol = R.tolerance(ref64, ref32, bf16)
    err = (got.double() - ref64).abs()
    print(f"{name}: max err {float(err.max()):.3e} yardstick {yard:.3e} "
          f"ratio {float(err.max()) / max(yard, 1e-30):.2f}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= tol).all()), f"{name}: {float((err - tol).max()):.3e} over the tolerance"


# ------------------------------------------------------------------ attention
ATT = [(2, 1), (2, 2), (2, 33), (2, 65), (2, 130), (12, 33)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("heads,L", ATT)
def test_attention_bwd(cuda, heads, L, dtype):
    from zsaac import ops
    B = 3
    lens = [1, L, max(1, L // 2)]
    g = _g(100 * heads + L)
    qkv = torch.randn(B * L, 3 * heads * 64, generator=g).to(dtype)
    do = (0.5 * torch.randn(B * L, heads * 64, generator=g)).to(dtype)
    qp, dp = qkv.clone().view(B, L, -1), do.clone().view(B, L, -1)
    for b in range(B):
        qp[b, lens[b]:] = NAN
        dp[b, lens[b]:] = NAN
    rt = BF16 if dtype == BF16 else None
    ref64 = R.attention_bwd(qkv, do, B, L, lens, heads, F64, rt)
    ref32 = R.attention_bwd(qkv, do, B, L, lens, heads, F32, rt)
    out = Out(cuda, (B * L, 3 * heads * 64), dtype, 7.0)
    ln = torch.tensor(lens, dtype=torch.int32, device=cuda)
    ops.attention_bwd(qp.view(B * L, -1).to(cuda), dp.view(B * L, -1).to(cuda), B, L, heads, out.t,
                      lens=ln)
    got = out.cpu()
    _check(f"attention_bwd h{heads} L{L}", got, ref64, ref32, dtype == BF16)
    for b in range(B):
        assert bool((got.view(B, L, -1)[b, lens[b]:] == 0).all())
    out2 = Out(cuda, (B * L, 3 * heads * 64), dtype, 7.0)
    ops.attention_bwd(qp.view(B * L, -1).to(cuda), dp.view(B * L, -1).to(cuda), B, L, heads, out2.t,
                      lens=ln)
    assert torch.equal(out2.cpu(), got)


def test_attention_bwd_without_lens(cuda):
    from zsaac import ops
    B, L, heads = 2, 5, 2
    g = _g(1)
    qkv, do = torch.randn(B * L, 384, generator=g), torch.randn(B * L, 128, generator=g)
    out = Out(cuda, (B * L, 384), F32, 7.0)
    ops.attention_bwd(qkv.to(cuda), do.to(cuda), B, L, heads, out.t)
    _check("attention_bwd no lens", out.cpu(), R.attention_bwd(qkv, do, B, L, None, heads),
           R.attention_bwd(qkv, do, B, L, None, heads, F32))


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", [32, 768])
@pytest.mark.parametrize("M", [1, 3, 70])
@pytest.mark.parametrize("gain,res", [(False, False), (True, False), (True, True)])
def test_layernorm_bwd(cuda, C, M, gain, res):
    from zsaac import ops
    g = _g(C + M)
    x = torch.randn(M, C, generator=g) * 2 + 0.3
    if M >= 3:
        x[1] = 0.75                                          # a constant row
    dy = torch.randn(M, C, generator=g)
    w = (1 + 0.1 * torch.randn(C, generator=g)) if gain else None
    r = torch.randn(M, C, generator=g) if res else None
    ref64, ref32 = (R.layernorm_bwd(x, dy, w, r, dtype=d) for d in (F64, F32))
    if res:      # in place on the residual, as the trainer runs it
        out = Out(cuda, (M, C), F32, 7.0, init=r)
        ops.layernorm_bwd(x.to(cuda), dy.to(cuda), out.t, g=w.to(cuda), residual=out.t)
    else:
        out = Out(cuda, (M, C), F32, 7.0)
        ops.layernorm_bwd(x.to(cuda), dy.to(cuda), out.t, g=None if w is None else w.to(cuda))
    _check(f"layernorm_bwd C{C} M{M}", out.cpu(), ref64, ref32)


@pytest.mark.parametrize("C", [32, 768])
@pytest.mark.parametrize("M", [1, 3, 70])
def test_layernorm_bwd_rows(cuda, C, M):
    from zsaac import ops
    g = _g(7 * C + M)
    n = 2 * M + 3
    x = torch.randn(n, C, generator=g)
    rows = torch.randperm(n, generator=g)[:M]
    dy = torch.randn(M, C, generator=g)
    w = 1 + 0.1 * torch.randn(C, generator=g)
    ref64, ref32 = (R.layernorm_bwd(x, dy, w, rows=rows, dtype=d) for d in (F64, F32))
    out = Out(cuda, (n, C), F32, 7.0, init=torch.zeros(n, C))
    ops.layernorm_bwd(x.to(cuda), dy.to(cuda), out.t, g=w.to(cuda),
                      rows=rows.to(device=cuda, dtype=torch.int32))
    got = out.cpu()
    _check(f"layernorm_bwd rows C{C} M{M}", got, ref64, ref32)
    rest = torch.ones(n, dtype=torch.bool)
    rest[rows] = False
    assert bool((got[rest] == 0).all())


# ------------------------------------------------------------------ activations
def _acts(n, seed):
    u = 3 * torch.randn(n, generator=_g(seed))
    u[0] = 30.0
    if n > 1:
        u[1], u[2] = -30.0, 0.0
    return u, torch.randn(n, generator=_g(seed + 1))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_gelu_tanh_bwd(cuda, n, dtype):
    from zsaac import ops
    u, dh = _acts(n, n)
    u = u.to(dtype)
    rt = BF16 if dtype == BF16 else None
    out = Out(cuda, (n,), dtype, 7.0)
    ops.gelu_tanh_bwd(u.to(cuda), dh.to(cuda), out.t)
    _check(f"gelu_tanh_bwd n{n}", out.cpu(), R.gelu_tanh_bwd(u, dh, F64, rt),
           R.gelu_tanh_bwd(u, dh, F32, rt), dtype == BF16)


@pytest.mark.parametrize("n", [1, 5, 4099])
def test_tanh_bwd(cuda, n):
    from zsaac import ops
    u, dh = _acts(n, n + 50)
    h = torch.tanh(u)
    assert abs(float(h[0])) == 1.0
    out = Out(cuda, (n,), F32, 7.0)
    ops.tanh_bwd(h.to(cuda), dh.to(cuda), out.t)
    _check(f"tanh_bwd n{n}", out.cpu(), R.tanh_bwd(h, dh), R.tanh_bwd(h, dh, F32))


# ------------------------------------------------------------------ LM-head gradient
def _nll_case(M, seed, dtype):
    g = _g(seed)
    V, K = 1000, 64
    wte = (0.3 * torch.randn(V, K, generator=g)).to(dtype)
    hf = torch.randn(M, K, generator=g).to(dtype)
    tgt = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    if M > 1:
        tgt[1::7] = -1
        tgt[-1] = V - 1
    valid = int((tgt >= 0).sum())
    cnt = torch.tensor([valid - valid // 2, 0, valid // 2], dtype=torch.int32)
    return V, K, wte, hf, tgt, cnt


@pytest.mark.parametrize("M", [1, 70])
def test_nll_grad_rows_with_the_mix_f32(cuda, M):
    """memory_project + memory_merge over the bank wte (scale 1, not normalised) feeding
    nll_grad_rows: the LM-head gradient without logits in memory."""
    from zsaac import ops
    V, K, wte, hf, tgt, cnt = _nll_case(M, M, F32)
    ref64, ref32 = (R.nll_grad_rows(R.softmax_mix(hf, wte, d), wte, tgt, cnt, d) for d in (F64, F32))
    ns = ops.memory_nsplit(V, K, F32)
    pm = torch.zeros(M, ns, K, device=cuda)
    pl = torch.zeros(M, ns, 2, device=cuda)
    mix = torch.zeros(M, K, device=cuda)
    wd, out = wte.to(cuda), Out(cuda, (M, K), F32, 7.0)
    ops.memory_project(hf.to(cuda), wd, 1.0, ns, pm, pl)
    ops.memory_merge(pm, pl, M, ns, K, mix, normalize=False)
    ops.nll_grad_rows(mix, wd, tgt.to(cuda), cnt.to(cuda), out.t)
    got = out.cpu()
    _check(f"nll_grad_rows mix M{M}", got, ref64, ref32)
    assert bool((got[tgt < 0] == 0).all())


@pytest.mark.parametrize("M", [1, 70])
def test_nll_grad_rows_bf16_table(cuda, M):
    from zsaac import ops
    V, K, wte, hf, tgt, cnt = _nll_case(M, M + 9, BF16)
    mix = R.softmax_mix(hf, wte, F64).float()
    ref64, ref32 = (R.nll_grad_rows(mix, wte, tgt, cnt, d) for d in (F64, F32))
    out = Out(cuda, (M, K), F32, 7.0)
    ops.nll_grad_rows(mix.to(cuda), wte.to(cuda), tgt.to(cuda), cnt.to(cuda), out.t)
    _check(f"nll_grad_rows bf16 M{M}", out.cpu(), ref64, ref32)


def test_nll_loss_and_soft_grad_rows(cuda):
    from zsaac import ops
    s = torch.tensor([-20.5, -3.25, 0.0, -7.0])
    c = torch.tensor([5, 1, 0, 2], dtype=torch.int32)
    loss = Out(cuda, (1,), F32, 7.0)
    ops.nll_loss(s.to(cuda), c.to(cuda), loss.t)
    assert abs(float(loss.cpu()[0]) - 30.75 / 8) <= 1e-6
    B, S, D, n, h_cap = 3, 9, 32, 2, 4
    dx = torch.randn(B * S, D, generator=_g(4))
    hl = torch.tensor([0, 4, 9], dtype=torch.int32)            # 9 is cut to h_cap
    out = Out(cuda, (B, n * D), F32, 7.0)
    ops.soft_grad_rows(dx.to(cuda), hl.to(cuda), h_cap, n, B, S, out.t)
    want = torch.stack([dx.view(B, S, D)[b, H:H + n].reshape(-1) for b, H in enumerate((0, 4, 4))])
    assert torch.equal(out.cpu(), want)


# ------------------------------------------------------------------ column sums, transposes
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("N", [5, 7680])
def test_colsum(cuda, B, N):
    from zsaac import ops
    x = torch.randn(B, N, generator=_g(B + N))
    out = Out(cuda, (N,), F32, 7.0)
    ops.colsum(x.to(cuda), out.t)
    _check(f"colsum B{B} N{N}", out.cpu(), R.colsum(x), R.colsum(x, F32))
    out2 = Out(cuda, (N,), F32, 7.0)
    ops.colsum(x.to(cuda), out2.t)
    assert torch.equal(out.cpu(), out2.cpu())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R_,C", [(1, 5), (3, 70), (33, 3840), (64, 7680)])
def test_transpose_cast(cuda, R_, C, dtype):
    from zsaac import ops
    x = torch.randn(R_, C, generator=_g(R_ + C))
    Rp = -(-R_ // 32) * 32
    out = Out(cuda, (C, Rp), dtype, 7.0)
    ops.transpose_cast(x.to(cuda), out.t)
    want = R.transpose_cast(x, BF16 if dtype == BF16 else None)
    assert torch.equal(out.cpu().double(), want)
    # a strided source (a column slice) reads the same values
    wide = torch.randn(R_, C + 8, generator=_g(1))
    out = Out(cuda, (C, Rp), dtype, 7.0)
    ops.transpose_cast(wide.to(cuda)[:, 8:], out.t)
    assert torch.equal(out.cpu().double(), R.transpose_cast(wide[:, 8:], BF16 if dtype == BF16 else None))


# ------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("n", [1, 1023, 4099])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw(cuda, n, step, wd):
    from zsaac import ops
    g = _g(n + step)
    p, grad = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    m = torch.zeros(n) if step == 1 else 0.05 * torch.randn(n, generator=g)
    v = torch.zeros(n) if step == 1 else 0.01 * torch.rand(n, generator=g)
    lr = 1e-3
    r64, r32 = (R.adamw(p, grad, m, v, step, lr, weight_decay=wd, dtype=d) for d in (F64, F32))
    pd, md, vd = (Out(cuda, (n,), F32, 7.0, init=t) for t in (p, m, v))
    op = Out(cuda, (n,), BF16, 7.0)
    ctr = torch.zeros(1, dtype=torch.int32, device=cuda)
    ops.adamw(pd.t, grad.to(cuda), md.t, vd.t, step, lr, weight_decay=wd, operand=op.t, step_ctr=ctr)
    for name, got, a, b in zip("pmv", (pd, md, vd), r64, r32):
        _check(f"adamw {name} n{n} step{step}", got.cpu(), a, b)
    assert torch.equal(op.cpu(), pd.cpu().to(BF16)) and int(ctr.item()) == step
    # without an operand copy or a step word; an f32 operand is a bit-exact copy
    p2, m2, v2 = (Out(cuda, (n,), F32, 7.0, init=t) for t in (p, m, v))
    o32 = Out(cuda, (n,), F32, 7.0)
    ops.adamw(p2.t, grad.to(cuda), m2.t, v2.t, step, lr, weight_decay=wd, operand=o32.t)
    assert torch.equal(p2.cpu(), pd.cpu()) and torch.equal(o32.cpu(), pd.cpu())


# ------------------------------------------------------------------ noise
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("D", [32, 1024])
def test_noise_inject(cuda, B, D):
    from zsaac import ops
    x = torch.randn(B, D, generator=_g(B + D)) * 2
    xd = x.to(cuda)
    out = Out(cuda, (B, D), F32, 7.0)
    ops.noise_inject(xd, out.t, 0.0, seed=5)
    assert torch.equal(out.cpu(), x)                         # variance 0: a bit-exact copy
    step = torch.tensor([3], dtype=torch.int32, device=cuda)
    out = Out(cuda, (B, D), F32, 7.0)
    ops.noise_inject(xd, out.t, 0.016, seed=5, step_ctr=step)
    got = out.cpu()
    ref64, ref32 = (R.noise_inject(x, 0.016, 5, 3, dtype=d) for d in (F64, F32))
    _check(f"noise_inject B{B} D{D}", got, ref64, ref32)
    # in place, and another step / seed draw other noise
    ip = Out(cuda, (B, D), F32, 7.0, init=x)
    ops.noise_inject(ip.t, ip.t, 0.016, seed=5, step_ctr=step)
    assert torch.equal(ip.cpu(), got)
    for kw in (dict(seed=6, step_ctr=step), dict(seed=5)):
        o = Out(cuda, (B, D), F32, 7.0)
        ops.noise_inject(xd, o.t, 0.016, **kw)
        assert not torch.equal(o.cpu(), got)


def test_noise_inject_row_identity_and_moments(cuda):
    from zsaac import ops
    x = torch.randn(3, 1024, generator=_g(8))
    ids = torch.tensor([40, 41, 42], dtype=torch.int32, device=cuda)
    three = Out(cuda, (3, 1024), F32, 7.0)
    ops.noise_inject(x.to(cuda), three.t, 0.016, seed=2, row_id=ids)
    alone = Out(cuda, (1, 1024), F32, 7.0)
    ops.noise_inject(x[2:3].to(cuda), alone.t, 0.016, seed=2, row_id=ids[2:])
    assert torch.equal(alone.cpu()[0], three.cpu()[2])       # a row alone = itself as row 2 of 3
    # the draws themselves: with x = 0 and variance 1 the un-normalised sum is n; recover it from
    # the output direction and the reference's norm of the same draws
    B, D = 70, 1024
    out = Out(cuda, (B, D), F32, 7.0)
    ops.noise_inject(torch.zeros(B, D, device=cuda), out.t, 1.0, seed=1)
    n64 = R.normals(1, np.arange(B), 0, D)
    draws = out.cpu().double().numpy() * np.linalg.norm(n64, axis=1, keepdims=True)
    assert float(np.abs(draws - n64).max()) <= 1e-4
    k = draws.size
    assert abs(draws.mean()) <= 5 / math.sqrt(k)
    assert abs(draws.var() - 1) <= 5 * math.sqrt(2 / k)


# ------------------------------------------------------------------ refusals (before any launch)
def test_entries_refuse_bad_arguments(cuda):
    from zsaac import ops
    from zsaac._lib import ZsError, call
    z = torch.zeros(257 * 192, device=cuda)
    with pytest.raises(ZsError, match="L <= 256"):
        ops.attention_bwd(z, z[:257 * 64], 1, 257, 1, torch.zeros_like(z))
    with pytest.raises(ZsError, match="alias"):
        call("zs_attention_bwd", z.data_ptr(), z.data_ptr() + 4096, 1, 4, None, 1, z.data_ptr(), 0, None)
    with pytest.raises(ZsError, match="16-byte"):
        call("zs_attention_bwd", z.data_ptr() + 4, z.data_ptr() + 4096, 1, 4, None, 1,
             z.data_ptr() + 8192, 0, None)
    with pytest.raises(ZsError, match="null"):
        call("zs_layernorm_bwd", None, 1, 32, 32, None, z.data_ptr(), 32, None, 1e-5, None, 0,
             z.data_ptr(), 32, None)
    with pytest.raises(ZsError, match="Rp"):
        call("zs_transpose_cast", z.data_ptr(), 3, 5, 5, z.data_ptr() + 4096, 3, 0, None)
    with pytest.raises(ZsError, match="step >= 1"):
        ops.adamw(z[:4], z[4:8], z[8:12], z[12:16], 0, 1e-3)
    with pytest.raises(ZsError, match="variance"):
        ops.noise_inject(z[:64].view(2, 32), z[64:128].view(2, 32), -1.0)
    with pytest.raises(ZsError):
        ops.colsum(torch.zeros(2, 4), torch.zeros(4))        # host tensors
