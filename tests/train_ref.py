"""Plain CPU restatements of the training kernels of csrc/train.hip, one function per op, written
as formulas (no autograd), and the float64 training oracle the end-to-end tests compare with.

Pure torch / numpy on the CPU; every float is computed in ``dtype``: float64 is the reference,
float32 the yardstick (the same formula in the kernel's precision).  ``round_to`` rounds to the
storage type where a kernel stores its output.  tests/test_train_ref.py ties each formula to
torch.autograd on the forward formula (and AdamW to torch.optim.AdamW, the Philox words to
tests/sample_ref.py's known answers); tests/test_gpu_train_kernels.py compares the kernels with
them.  Nothing here reads a golden or the original project.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import sample_ref

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
KEYS = ("clap_project.model.0.weight", "clap_project.model.0.bias",
        "clap_project.model.2.weight", "clap_project.model.2.bias")


def _round(v, round_to):
    return v if round_to is None else v.to(round_to).to(v.dtype)


def tolerance(ref64, ref32, bf16=False):
    """The project's rule (attn_ref.tolerance): yardstick = the float32 formula's largest
    deviation from float64 on this data, tolerance 4 x yardstick + 1e-6; a bf16 output adds one
    bf16 step of the reference elementwise.  -> (yardstick, tolerance tensor)."""
    yard = float((ref32.double() - ref64).abs().max())
    tol = torch.full_like(ref64, 4.0 * yard + 1e-6)
    if bf16:
        tol = tol + ref64.abs() * 2.0 ** -8
    return yard, tol


# ------------------------------------------------------------------ the ops
def attention_fwd(qkv, B, L, lens, heads, dtype=F64):
    """The forward whose backward attention_bwd states: causal softmax(q k^T / 8) v over the
    keys j <= i, j < lens[b], head dim 64, on the packed [B*L, 3*heads*64] layout; rows
    i >= lens[b] give zeros.  Differentiable (test_train_ref ties attention_bwd to it)."""
    E = heads * 64
    x = qkv.to(dtype).reshape(B, L, 3, heads, 64)
    out = []
    for b in range(B):
        n = L if lens is None else int(lens[b])
        q, k, v = (x[b, :n, i].transpose(0, 1) for i in range(3))            # [H, n, 64]
        sc = (q @ k.transpose(-1, -2)) / 8.0
        mask = torch.ones(n, n, dtype=torch.bool).tril()
        p = torch.softmax(sc.masked_fill(~mask, -float("inf")), -1)
        o = (p @ v).transpose(0, 1).reshape(n, E)
        out.append(torch.cat((o, torch.zeros(L - n, E, dtype=dtype))))
    return torch.cat(out)


def attention_bwd(qkv, d_out, B, L, lens, heads, dtype=F64, round_to=None):
    """P = softmax(Q K^T / 8) (causal), dP = dO V^T, D_i = sum_j P_ij dP_ij, dV = P^T dO,
    dS = P o (dP - D), dQ = dS K / 8, dK = dS^T Q / 8; rows i >= lens[b] are not read (they may
    hold NaN) and get zeros.  -> dqkv [B*L, 3*heads*64]."""
    E = heads * 64
    x = qkv.reshape(B, L, 3, heads, 64)
    do = d_out.reshape(B, L, heads, 64)
    out = torch.zeros(B, L, 3, heads, 64, dtype=dtype)
    for b in range(B):
        n = L if lens is None else int(lens[b])
        q, k, v = (x[b, :n, i].to(dtype).transpose(0, 1) for i in range(3))   # [H, n, 64]
        g = do[b, :n].to(dtype).transpose(0, 1)
        sc = (q @ k.transpose(-1, -2)) / 8.0
        mask = torch.ones(n, n, dtype=torch.bool).tril()
        sc = sc.masked_fill(~mask, -float("inf"))
        p = torch.exp(sc - torch.logsumexp(sc, -1, keepdim=True))
        dp = g @ v.transpose(-1, -2)
        dd = (p * dp).sum(-1, keepdim=True)
        ds = p * (dp - dd)
        out[b, :n, 0] = ((ds @ k) / 8.0).transpose(0, 1)
        out[b, :n, 1] = ((ds.transpose(-1, -2) @ q) / 8.0).transpose(0, 1)
        out[b, :n, 2] = (p.transpose(-1, -2) @ g).transpose(0, 1)
    return _round(out.reshape(B * L, 3 * E), round_to)


def layernorm_bwd(x, dy, g=None, res=None, eps=1e-5, rows=None, dtype=F64):
    """dx of LayerNorm(x) g + b: a = dy g, dx = rstd (a - mean(a) - xhat mean(a xhat)) + res.
    ``rows``: dy row m belongs to row rows[m]; -> a zero buffer shaped like x with those rows."""
    x, dy = x.to(dtype), dy.to(dtype)
    idx = torch.arange(dy.shape[0]) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    xr = x[idx]
    mean = xr.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xr - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (xr - mean) * rstd
    a = dy if g is None else dy * g.to(dtype)
    dx = rstd * (a - a.mean(-1, keepdim=True) - xhat * (a * xhat).mean(-1, keepdim=True))
    if res is not None:
        dx = dx + res.to(dtype)[idx]
    if rows is None:
        return dx
    out = torch.zeros_like(x)
    out[idx] = dx
    return out


def gelu_new(u):
    return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))


def gelu_tanh_bwd(u, dh, dtype=F64, round_to=None):
    """du = gelu_new'(u) dh,  gelu_new'(u) = (1 + t)/2 + u (1 - t^2) c (1 + 3 a u^2) / 2,
    t = tanh(c (u + a u^3)), c = sqrt(2/pi), a = 0.044715."""
    u, dh = u.to(dtype), dh.to(dtype)
    c, a = math.sqrt(2.0 / math.pi), 0.044715
    t = torch.tanh(c * (u + a * u ** 3))
    return _round((0.5 * (1 + t) + 0.5 * u * (1 - t * t) * c * (1 + 3 * a * u * u)) * dh, round_to)


def tanh_bwd(h, dh, dtype=F64):
    h, dh = h.to(dtype), dh.to(dtype)
    return (1 - h * h) * dh


def softmax_mix(hf, wte, dtype=F64):
    """mix[m] = sum_v softmax(hf[m] . wte^T)_v wte[v] (what zs_memory_project + _merge compute)."""
    hf, wte = hf.to(dtype), wte.to(dtype)
    return torch.softmax(hf @ wte.t(), -1) @ wte


def nll_grad_rows(mix, wte, tgt, cnt, dtype=F64):
    """dhf[m] = (mix[m] - wte[tgt[m]]) / sum(cnt); zeros for tgt[m] < 0."""
    mix, wte = mix.to(dtype), wte.to(dtype)
    t = torch.as_tensor(tgt, dtype=torch.long)
    on = t >= 0
    out = torch.zeros_like(mix)
    out[on] = (mix[on] - wte[t[on]]) / float(int(torch.as_tensor(cnt).sum()))
    return out


def colsum(x, dtype=F64):
    return x.to(dtype).sum(0)


def transpose_cast(x, round_to=None, dtype=F64):
    """[R, C] -> [C, R rounded up to 32], zero-filled."""
    R, C = x.shape
    out = torch.zeros(C, -(-R // 32) * 32, dtype=dtype)
    out[:, :R] = _round(x.to(dtype), round_to).t()
    return out


def adamw(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, dtype=F64):
    """One torch.optim.AdamW update, written out.  -> (p, m, v)."""
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    p = p * (1 - lr * weight_decay)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def normals(seed, row_ids, step, D, dtype=np.float64):
    """n [len(row_ids), D]: columns 4c .. 4c+3 of row r from Philox4x32-10(key = seed, counter =
    (r, step, c, 0)), words (0, 1) and (2, 3) through Box-Muller on 24-bit uniforms."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rid = np.asarray(row_ids, dtype=np.int64).reshape(-1, 1) & sample_ref.MASK
    nc = -(-D // 4)
    c = np.arange(nc, dtype=np.int64).reshape(1, -1)
    z = np.zeros((rid.shape[0], nc), dtype=np.int64)
    w = sample_ref.philox4x32_10((rid + z, z + (int(step) & sample_ref.MASK), c + z, z),
                                 (z + (seed & sample_ref.MASK), z + (seed >> 32)))
    out = np.zeros((rid.shape[0], nc, 4), dtype=dtype)
    for i in (0, 2):
        u1 = ((w[i] >> np.uint64(8)).astype(dtype) + dtype(1)) * dtype(2.0 ** -24)
        u2 = (w[i + 1] >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)
        r, th = np.sqrt(dtype(-2) * np.log(u1)), dtype(2 * math.pi) * u2
        out[:, :, i], out[:, :, i + 1] = r * np.cos(th), r * np.sin(th)
    return out.reshape(rid.shape[0], nc * 4)[:, :D]


def noise_inject(x, variance, seed=0, step=0, row_ids=None, dtype=F64):
    """noise_injection: x if variance == 0, else normalize(normalize(x) + sqrt(variance) n)."""
    if variance == 0:
        return x.clone()
    nd = np.float64 if dtype == F64 else np.float32
    rid = np.arange(x.shape[0]) if row_ids is None else row_ids
    n = torch.from_numpy(normals(seed, rid, step, x.shape[1], nd)).to(dtype)
    x = x.to(dtype)
    y = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) + math.sqrt(variance) * n
    return y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def linear_schedule(step, warmup, total):
    return step / max(1, warmup) if step < warmup else max(0.0, (total - step) / max(1, total - warmup))


# ------------------------------------------------------------------ the training oracle
def cast_sd(sd, dtype, round_to=None):
    return {k: (_round(v.float(), round_to).to(dtype) if v.is_floating_point() else v)
            for k, v in sd.items()}


def oracle_loss(sd, prefix, hards, caps):
    """The batch's mean token cross-entropy through the oracle (tests/test_gpu_score.py::_oracle's
    recipe, differentiable): per clip [wte(hard) ; mapper(prefix) ; wte(cap[:-1])] ->
    OC.gpt2_logits -> log-softmax at the scored rows.  ``prefix`` [B, 1024] is the mapper's
    input (normalised, noised).  Everything runs in sd's dtype.
    -> (loss, soft [B, 7680], max |logit| of the scored rows)."""
    from oracle import caption as OC
    wte = sd["gpt.transformer.wte.weight"]
    soft = OC.mlp_mapper(prefix, sd)
    tot, n, mx = 0.0, 0, 0.0
    for b, (hard, ids) in enumerate(zip(hards, caps)):
        emb_h = wte[torch.as_tensor(hard, dtype=torch.long)]
        pe = torch.cat((emb_h, soft[b].reshape(-1, wte.shape[1])))
        tail = wte[torch.as_tensor(ids[:-1], dtype=torch.long)]
        logits = OC.gpt2_logits(torch.cat((pe, tail))[None], sd)[0][0][pe.shape[0] - 1:]
        ls = torch.log_softmax(logits, -1)
        tot = tot - ls.gather(1, torch.as_tensor(ids, dtype=torch.long)[:, None]).sum()
        n += len(ids)
        mx = max(mx, float(logits.detach().abs().max()))
    return tot / n, soft, mx


def oracle_grads(sd, prefix, hards, caps):
    """-> (loss, d_soft [B, 7680], {key: grad}, max |logit|) by autograd through oracle_loss."""
    sd = dict(sd)
    for k in KEYS:
        sd[k] = sd[k].detach().clone().requires_grad_(True)
    loss, soft, mx = oracle_loss(sd, prefix, hards, caps)
    soft.retain_grad()
    loss.backward()
    return loss.detach(), soft.grad.detach(), {k: sd[k].grad.detach() for k in KEYS}, mx


def oracle_train(sd, prefix, hards, caps, steps, lr, weight_decay):
    """``steps`` steps of torch.optim.AdamW on the four mapper tensors -> the loss before each
    update and the final tensors."""
    sd = dict(sd)
    params = [sd[k].detach().clone().requires_grad_(True) for k in KEYS]
    for k, p in zip(KEYS, params):
        sd[k] = p
    opt = torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, betas=(0.9, 0.999), eps=1e-8)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = oracle_loss(sd, prefix, hards, caps)[0]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: p.detach() for k, p in zip(KEYS, params)}
