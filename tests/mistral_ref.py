"""Plain CPU references of the Mistral decoder's non-GEMM kernels (csrc/mistral.hip), one function
per op.

Pure torch on the CPU; every float is computed in ``dtype``: float64 is the reference, float32
the yardstick (the same formula in the kernel's precision; its distance from the float64 run on a
case's own data is what plain float32 arithmetic costs there).  ``round_to`` rounds to the
storage type at the points where a kernel stores (or, in the fused decode step, re-reads) a bf16
value.  Nothing here reads a golden or the original project.  tests/test_mistral_ref.py ties these
functions to oracle/mistral.py and asserts the input conditions of the GPU cases;
tests/test_gpu_mistral_kernels.py compares the kernels with them.

The functions work on the kernels' own layouts: split-K slabs as a flat f32 buffer, slab s at
``s * ss``; caches [seq][KVH][Lmax][128]; rotary tables [Lmax][64]; gate|up columns
glu-interleaved (zsaac/mistral.py glu_interleave).

``mut`` names one deliberate, in-bounds arithmetic error of a kernel (MUTANTS).  It is only ever
set by tests/test_mistral_ref.py, which shows on the CPU that the inputs of the GPU cases tell
each of them from the reference by more than twice the case's tolerance.

The second half builds the inputs both test files share.
"""
from __future__ import annotations

import math

import torch

HD, HALF = 128, 64
LMAX = 72
EPS = 1e-5
I32 = torch.int32
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAN = float("nan")

MUTANTS = ("kvh_mod", "scale8", "strict", "sin_sign", "seq_m", "no_tail", "skip_pass2", "up8",
           "p_all")


def _round(v, round_to):
    return v if round_to is None else v.to(round_to).to(v.dtype)


def tolerance(ref64, ref32, bf16=False):
    """The project's rule (test_gpu_magic_kernels.py::_check): yardstick = the float32 formula's
    largest deviation from float64 on this data, tolerance 4 x yardstick + 1e-6; a bf16 output
    adds one bf16 step of the reference elementwise (2^-8 |ref|: the float64 and the f32 rounding
    may fall on opposite sides of a tie).  -> (yardstick, tolerance tensor like ref64)."""
    yard = float((ref32.double() - ref64).abs().max())
    tol = torch.full_like(ref64, 4.0 * yard + 1e-6)
    if bf16:
        tol = tol + ref64.abs() * 2.0 ** -8
    return yard, tol


# ------------------------------------------------------------------ the ops
def slab_sum(y, nsplit, ss, n, dtype=F64, mut=""):
    """sum_s y[s * ss : s * ss + n], slab 0 first, then 1, 2, ... (the kernels' order)."""
    last = 1 + 4 * ((nsplit - 1) // 4) if mut == "no_tail" else nsplit
    v = y[:n].to(dtype).clone()
    for s in range(1, last):
        v = v + y[s * ss:s * ss + n].to(dtype)
    return v


def add_rmsnorm(x, y, nsplit, ss, M, D, eps, w, dtype=F64, round_to=None, mut=""):
    """x[m] += sum_s y[s][m] (y None: x unchanged), h[m] = w * (x[m] * rsqrt(mean(x[m]^2) + eps))
    (w None: no weight).  -> (x afterwards [M, D], h [M, D])."""
    xn = x.to(dtype).reshape(M, D)
    if y is not None:
        xn = xn + slab_sum(y, nsplit, ss, M * D, dtype, mut).view(M, D)
    sq = xn * xn
    if mut == "skip_pass2":
        sq = sq.clone()
        sq[:, 4096:8192] = 0.0
    h = xn * torch.rsqrt(sq.sum(-1, keepdim=True) / D + eps)
    if w is not None:
        h = h * w.to(dtype)
    return xn, _round(h, round_to)


def add_ss(x, y, nsplit, ss, M, D, dtype=F64, mut=""):
    """x[m] += sum_s y[s][m]; rss[c][m] = the sum of x[m]^2 over columns 512 c .. 512 c + 511.
    The bf16 copy xb is the f32 x rounded once.  -> (x afterwards [M, D], rss [D / 512, M])."""
    xn = x.to(dtype).reshape(M, D)
    if y is not None:
        xn = xn + slab_sum(y, nsplit, ss, M * D, dtype, mut).view(M, D)
    return xn, (xn * xn).view(M, D // 512, 512).sum(-1).t().contiguous()


def embed(hard, soft, tail, tok, emb):
    """Prefill rows per sequence [emb[hard[b]] ; soft[b] ; emb[tail]] (absent parts None), or the
    decode rows emb[tok].  A copy: no arithmetic, so no ``dtype``.  -> f32 [M, D]."""
    e = emb.to(F32)
    if tok is not None:
        return e[tok.long()]
    B = hard.shape[0] if hard is not None else soft.shape[0]
    parts = []
    if hard is not None:
        parts.append(e[hard.long()])
    if soft is not None:
        parts.append(soft.to(F32))
    if tail is not None:
        parts.append(e[tail.long()][None].expand(B, -1, -1))
    return torch.cat(parts, dim=1).reshape(-1, e.shape[1])


def rope_kv(qkv, nsplit, ss, M, H, KVH, pos, rows_per_seq, cos, sin, kc, vc, dtype=F64,
            round_to=None, mut=""):
    """q|k|v slabs [nsplit][M][(H + 2 KVH) * 128]: the q and k heads rotated by position pos[m]
    (pair (i, i + 64): lo = a cos - b sin, hi = b cos + a sin; HF's rotate_half), k and v written
    to row pos[m] of sequence m // rows_per_seq.  -> (q [M, H * 128], kc, vc afterwards)."""
    s = slab_sum(qkv, nsplit, ss, M * (H + 2 * KVH) * HD, dtype, mut).view(M, H + 2 * KVH, HD)
    p = pos.long()
    c, sn = cos.to(dtype)[p][:, None], sin.to(dtype)[p][:, None]
    a, b = s[:, :H + KVH, :HALF], s[:, :H + KVH, HALF:]
    hi = b * c - a * sn if mut == "sin_sign" else b * c + a * sn
    rot = _round(torch.cat((a * c - b * sn, hi), dim=-1), round_to)
    kc, vc = kc.to(dtype).clone(), vc.to(dtype).clone()
    seq = torch.arange(M) if mut == "seq_m" else torch.arange(M) // rows_per_seq
    kc[seq, :, p] = rot[:, H:]
    vc[seq, :, p] = _round(s[:, H + KVH:], round_to)
    return rot[:, :H].reshape(M, H * HD), kc, vc


def attention(q, M, H, KVH, pos, rows_per_seq, kc, vc, dtype=F64, round_to=None, mut=""):
    """Causal grouped-query attention: query row m, head h against keys 0..pos[m] of sequence
    m // rows_per_seq, kv head h // (H / KVH): softmax((q k^T) / sqrt(128)) v.  -> [M, H * 128]."""
    q = q.to(dtype).view(M, H, HD)
    kc, vc = kc.to(dtype), vc.to(dtype)
    scale = 0.125 if mut == "scale8" else HD ** -0.5
    hh = torch.arange(H)
    kvh = hh % KVH if mut == "kvh_mod" else hh // (H // KVH)
    out = torch.empty(M, H, HD, dtype=dtype)
    for m in range(M):
        p = int(pos[m])
        seq = m if mut == "seq_m" else m // rows_per_seq
        n = p if mut == "strict" else p + 1
        k, v = kc[seq, kvh, :n], vc[seq, kvh, :n]                      # [H, n, 128]
        sc = torch.einsum("hd,hnd->hn", q[m], k) * scale
        if mut == "p_all":                     # key p counted by all 8 key groups
            sc[:, p] += math.log(8.0)
        out[m] = torch.einsum("hn,hnd->hd", sc.softmax(-1), v)
    return _round(out.reshape(M, H * HD), round_to)


def decode_attention(qkv, nsplit, ss, M, H, KVH, pos, cos, sin, kc, vc, dtype=F64,
                     cache_round=None, out_round=None, mut=""):
    """One decode step, row m = sequence m: rope_kv (rows_per_seq 1) then attention over keys
    0..pos[m].  ``cache_round`` (bf16 caches): q and the new k / v are rounded to the cache type
    before the scores, where the kernel rounds them -- in the float64 reference too.
    -> (out [M, H * 128], kc, vc afterwards)."""
    q, kc, vc = rope_kv(qkv, nsplit, ss, M, H, KVH, pos, 1, cos, sin, kc, vc, dtype, cache_round,
                        mut)
    return attention(q, M, H, KVH, pos, 1, kc, vc, dtype, out_round, mut), kc, vc


def glu_cols(F):
    """Columns of gate f and up f in a glu-interleaved gate|up row of 2F: gate f at
    16 (f / 8) + 8 (f / 4 % 2) + f % 4, up f four columns after it."""
    f = torch.arange(F)
    g = 16 * (f // 8) + 8 * ((f // 4) % 2) + f % 4
    return g, g + 4


def silu_mul(gu, nsplit, ss, M, F, dtype=F64, round_to=None, mut=""):
    """act[m][f] = silu(gate f) * up f from gate|up slabs [nsplit][M][2F], silu(g) =
    g / (1 + exp(-g)).  -> [M, F]."""
    s = slab_sum(gu, nsplit, ss, M * 2 * F, dtype, mut).view(M, 2 * F)
    g, u = glu_cols(F)
    if mut == "up8":
        u = (g + 8).clamp(max=2 * F - 1)
    gt, up = s[:, g], s[:, u]
    return _round(gt / (1.0 + torch.exp(-gt)) * up, round_to)


def scale_cols(x, M, N, ld, scale, dtype=F64):
    """x[m][n] *= scale[n] for n < N of an [M][ld] matrix; columns N.. untouched."""
    out = x.to(dtype).clone().view(M, ld)
    out[:, :N] = out[:, :N] * scale.to(dtype)
    return out


# ------------------------------------------------------------------ shared inputs
HEADS = [(8, 2), (4, 4), (6, 1)]
NORM_D = [4, 1024, 4096, 4100, 8192, 16384]
NORM_M = [1, 3]
NORM_NSPLIT = [1, 4, 5, 6, 9]
ADD_SS_NSPLIT = [5, 6, 9]
ADD_SS_SHAPES = [(32, 512), (32, 4096), (5, 4096)]
SILU_NSPLIT = [1, 5, 6]
SILU_SHAPES = [(1, 8), (5, 8), (1, 1032), (5, 1032)]
SILU_GATES = [100.0, -100.0, 20.0, -20.0, 81.0, -81.0]
ROPE_NSPLIT = [1, 3]
ROPE_POS = [0, 1, 31, 32, 71]
ATT_POS = [0, 7, 8, 31, 32, 33, 63, 64, 71]
ATT_FORMS = ["ragged9", "ragged3", "prefill5", "prefill33"]
DEC_POS = [0, 1, 8, 31, 32, 33, 64, 71]
DEC_NSPLIT = [1, 5, 6]
EMBED_FORMS = [(3, 2, 2), (3, 0, 2), (3, 2, 0), (0, 2, 1)]
EMBED_V, EMBED_PAD = 50, 2
ONLINE_KEY, ONLINE_POS = 36, [71, 40]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rope_tables(L=LMAX, theta=10000.0):
    """cos / sin [L][64] f32, as zsaac/mistral.py builds them (HF's inv_freq)."""
    inv = 1.0 / (theta ** (torch.arange(0, HD, 2, dtype=torch.int64).float() / HD))
    fr = torch.arange(L, dtype=F32)[:, None] * inv[None]
    return fr.cos().contiguous(), fr.sin().contiguous()


def slab_layout(vals, ss, fill=NAN):
    """vals [nsplit, n] -> the flat f32 buffer with slab s at s * ss; what lies between the slabs
    (ss > n) holds ``fill``."""
    nsplit, n = vals.shape
    buf = torch.full(((nsplit - 1) * ss + n,), fill, dtype=F32)
    for s in range(nsplit):
        buf[s * ss:s * ss + n] = vals[s]
    return buf


def residual_case(M, D, nsplit, pad, seed=0):
    """x [M, D], the slabs y (None at nsplit 0, then ss = 0 as the decoder's first norm passes
    it; else ss = M D + pad with NaN in the padding) and a weight w.  With more than one row, row
    1 has magnitude 1e-4 in x and in every slab (eps decides its norm).  -> dict."""
    g = gen(1000 * seed + 7 * D + 3 * M + nsplit + pad)
    x = torch.randn(M, D, generator=g) * 3
    yv = torch.randn(max(nsplit, 1), M, D, generator=g)
    if M > 1:
        x[1] *= 1e-4 / 3
        yv[:, 1] *= 1e-4
    w = torch.randn(D, generator=g) * 0.5 + 1.0
    ss = M * D + pad if nsplit else 0
    y = slab_layout(yv.view(max(nsplit, 1), -1), ss) if nsplit else None
    return dict(x=x, y=y, ss=ss, w=w, nsplit=nsplit)


def qkv_case(M, H, KVH, nsplit, seed=0):
    """q|k|v slabs for M rows, ss padded by 8 (NaN) when there is more than one."""
    n = M * (H + 2 * KVH) * HD
    g = gen(seed + 31 * H + nsplit)
    ss = n + 8 if nsplit > 1 else n
    return slab_layout(torch.randn(nsplit, n, generator=g), ss), ss


def rope_case(H, KVH, form):
    """(M, pos, rows_per_seq, sequences): ragged = one row per sequence at ROPE_POS; prefill =
    2 sequences of 5 rows at positions 0..4."""
    if form == "ragged":
        return len(ROPE_POS), torch.tensor(ROPE_POS, dtype=I32), 1, len(ROPE_POS)
    return 10, torch.arange(5, dtype=I32).repeat(2), 5, 2


def att_case(H, KVH, form, dt):
    """q [M, H * 128] and caches in ``dt`` (exact inputs), pos, rows_per_seq.  Cache positions
    past each sequence's largest pos hold NaN.  Forms: ragged9 (ATT_POS, one row per sequence),
    ragged3 (pos 0 / 33 / 71: with 6 heads the last block has two live waves), prefill5 /
    prefill33 (two sequences of P rows at 0..P-1), online (H == KVH; key ONLINE_KEY of each
    sequence is 3 q of its row, so the running maximum jumps when the second 32-key step reaches
    it).  -> dict."""
    g = gen(17 * H + KVH + len(form))
    if form.startswith("prefill"):
        P = int(form[7:])
        pos, rps, S = torch.arange(P, dtype=I32).repeat(2), P, 2
    else:
        p = {"ragged9": ATT_POS, "ragged3": [0, 33, 71], "online": ONLINE_POS}[form]
        pos, rps, S = torch.tensor(p, dtype=I32), 1, len(p)
    M = pos.numel()
    q = torch.randn(M, H * HD, generator=g).to(dt)
    kc = torch.randn(S, KVH, LMAX, HD, generator=g).to(dt)
    vc = torch.randn(S, KVH, LMAX, HD, generator=g).to(dt)
    if form == "online":
        assert H == KVH
        kc[:, :, ONLINE_KEY] = (3.0 * q.float().view(M, H, HD)).to(dt)
    for s in range(S):
        last = int(pos[s * rps:(s + 1) * rps].max())
        kc[s, :, last + 1:] = NAN
        vc[s, :, last + 1:] = NAN
    return dict(q=q, kc=kc, vc=vc, pos=pos, rps=rps, M=M)


def dec_case(H, KVH, nsplit, dt):
    """A decode step for the 8 sequences at DEC_POS: q|k|v slabs, caches in ``dt`` that hold NaN
    at every position >= pos[m].  -> dict."""
    M = len(DEC_POS)
    g = gen(5 * H + KVH + nsplit)
    qkv, ss = qkv_case(M, H, KVH, nsplit, seed=3)
    kc = torch.randn(M, KVH, LMAX, HD, generator=g).to(dt)
    vc = torch.randn(M, KVH, LMAX, HD, generator=g).to(dt)
    for m, p in enumerate(DEC_POS):
        kc[m, :, p:] = NAN
        vc[m, :, p:] = NAN
    return dict(qkv=qkv, ss=ss, kc=kc, vc=vc, pos=torch.tensor(DEC_POS, dtype=I32), M=M)


def silu_case(M, F, nsplit):
    """Glu-interleaved gate|up slabs (ss padded by 8 with NaN when nsplit > 1) whose summed gates
    of the first SILU_GATES columns of row 0 are exactly those values (slab 0 holds the value,
    the other slabs zero there)."""
    g = gen(M + F + nsplit)
    vals = torch.randn(nsplit, M, 2 * F, generator=g) * 2
    gc, _ = glu_cols(F)
    for i, v in enumerate(SILU_GATES[:F]):
        vals[:, 0, gc[i]] = 0.0
        vals[0, 0, gc[i]] = v
    n = M * 2 * F
    ss = n + 8 if nsplit > 1 else n
    return slab_layout(vals.view(nsplit, -1), ss), ss


def embed_case(form, D, table_dt, B=2):
    """(hard [B, H] | None, soft [B, ns, D] | None, tail [nt] | None, table [V, D]): ids include
    0, V - 1 and the pad id."""
    H, ns, nt = form
    g = gen(H + 10 * ns + 100 * nt + D)
    emb = torch.randn(EMBED_V, D, generator=g).to(table_dt)
    hard = soft = tail = None
    if H:
        hard = torch.randint(3, EMBED_V - 1, (B, H), generator=g, dtype=I32)
        hard[0, 0], hard[1, H - 1], hard[1, 0] = 0, EMBED_V - 1, EMBED_PAD
    if ns:
        soft = torch.randn(B, ns, D, generator=g)
    if nt:
        tail = torch.tensor([EMBED_V - 1, 0][:nt], dtype=I32)
    return hard, soft, tail, emb


def step_max_jump(q, kc, pos, H, KVH):
    """Per (row, head) of a rows_per_seq 1 case: the largest rise of the running maximum of the
    scaled scores from one 8-key step of the attention loop to a later one (float64)."""
    M = pos.numel()
    qd, kd = q.double().view(M, H, HD), kc.double()
    out = torch.empty(M, H, dtype=F64)
    for m in range(M):
        p = int(pos[m])
        for h in range(H):
            sc = (kd[m, h // (H // KVH), :p + 1] @ qd[m, h]) * HD ** -0.5
            run = torch.stack([sc[j:j + 8].max() for j in range(0, p + 1, 8)]).cummax(0).values
            out[m, h] = (run[1:] - run[:-1]).max() if run.numel() > 1 else 0.0
    return out
