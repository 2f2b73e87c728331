"""Plain CPU references of the GEMM family (csrc/gemm.hip, lmhead.hip, gemm_fast.h, gemm_core.h,
gemm_rows.hip, gemm_skinny.hip): zs_gemm, zs_gemm_ln, zs_gemm_ln_f32 and zs_lmhead_topk(_t), one
function per entry point, and the strided cases the GPU tests run.

Pure torch on the CPU; every float is computed in ``dtype``: float64 is the reference, float32
the yardstick (the same formula in the kernels' accumulation precision; its distance from the
float64 run on a case's own data is what plain float32 arithmetic costs there).  The rule is
mistral_ref.tolerance: 4 x yardstick + 1e-6, a bf16 output adds 2^-8 |ref| elementwise.  Operands
are taken in their storage type (bf16 or f32) and widened, so a product of two bf16 operands is
exact in either precision; the float32 run accumulates k in chunks of 16 so that it does not depend
on a BLAS blocking.  Nothing here reads a golden or the original project.  tests/test_gemm_ref.py
ties these functions to torch's own linear / gelu / layer_norm / topk / logsumexp and asserts the
input conditions of the GPU cases; tests/test_gpu_gemm_kernels.py compares the kernels with them.

``mut`` names one deliberate, in-bounds arithmetic error of a kernel (MUTANTS).  It is only ever
set by tests/test_gemm_ref.py, which shows on the CPU that the inputs of the GPU cases tell each
of them from the reference by more than twice the case's tolerance.

The second half builds the strided problems both test files share: A inside an [M + 1][lda]
buffer, W inside [N + 1][ldw], NaN in every padding column and in the extra row.
"""
from __future__ import annotations

import math

import torch

from mistral_ref import tolerance  # noqa: F401  (the one rule, re-exported)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAN = float("nan")
INF = float("inf")
LM_BN = 128                  # lmhead.hip LM_BN: vocabulary columns per partial block
PAD_IDX = 0x7fffffff         # index of a padding entry of a short block (value -inf)
ACTS = ("none", "gelu_erf", "gelu_tanh", "relu", "tanh")     # = ACT_NONE .. ACT_TANH (0 .. 4)

MUTANTS = ("gelu_swap", "bias_shift_tail", "drop_k8", "ldr_is_n", "split_last", "no_ln_round",
           "ln_affine_skipped", "tie_high", "temp_mul", "norm_sq", "lse_block_max")


def _round(v, round_to):
    return v if round_to is None else v.to(round_to).to(v.dtype)


# ------------------------------------------------------------------ the ops
def act_apply(x, act):
    """The five epilogue activations written out from their definitions."""
    if act == "gelu_erf":
        return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    if act == "gelu_tanh":       # HF gelu_new
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))
    if act == "relu":
        return torch.clamp_min(x, 0.0)
    if act == "tanh":
        return torch.tanh(x)
    assert act == "none", act
    return x


def matmul(a, w, dtype=F64):
    """a w^T with both operands widened from their storage type to ``dtype``.  float64: one
    product; float32: k accumulated in chunks of 16 (no dependence on a BLAS blocking)."""
    a, w = a.to(dtype), w.to(dtype)
    if dtype == F64:
        return a @ w.t()
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=dtype)
    for k in range(0, a.shape[1], 16):
        acc = acc + a[:, k:k + 16] @ w[:, k:k + 16].t()
    return acc


def gemm(a, w, bias=None, residual=None, act="none", out_dtype=F32, dtype=F64, mut="",
         k_per_split=None, tile_m=64):
    """act(a w^T + bias) + residual, rounded to ``out_dtype`` last.  a [M, K], w [N, K] in their
    storage type (views of the strided buffers are fine), bias [N] f32, residual [M, N] f32.
    ``k_per_split`` / ``tile_m`` only place the split_last / drop_k8 mutants."""
    M, K = a.shape
    N = w.shape[0]
    a = a.to(dtype)
    if mut == "drop_k8":                 # the last 8 k of the last row of the first row tile
        a = a.clone()
        a[min(M, tile_m) - 1, K - 8:] = 0.0
    if mut == "split_last" and k_per_split:      # the last split-K slab is not added
        a = a.clone()
        a[:, (math.ceil(K / k_per_split) - 1) * k_per_split:] = 0.0
    v = matmul(a, w, dtype)
    if bias is not None:
        b = bias.to(dtype)
        if mut == "bias_shift_tail" and N % 8:   # index + 1 in the nv < 8 column tail
            t = N - N % 8
            b = b.clone()
            b[t:] = bias.to(dtype)[torch.clamp(torch.arange(t, N) + 1, max=N - 1)]
        v = v + b
    if mut == "gelu_swap":
        act = {"gelu_erf": "gelu_tanh", "gelu_tanh": "gelu_erf"}.get(act, act)
    v = act_apply(v, act)
    if residual is not None:
        r = residual
        if mut == "ldr_is_n":            # the residual read as if its rows were N apart
            r = torch.as_strided(residual, (M, N), (N, 1), residual.storage_offset())
        v = v + r.to(dtype)
    return _round(v, out_dtype if out_dtype == BF16 else None)


def layernorm(x, ln_w, ln_b, eps, dtype=F64, mut=""):
    """LayerNorm over the last axis (biased variance); ln_w = ln_b = None: normalise only."""
    x = x.to(dtype)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    h = d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    if ln_w is not None and mut != "ln_affine_skipped":
        h = h * ln_w.to(dtype) + ln_b.to(dtype)
    return h


def gemm_ln(x, ln_w, ln_b, eps, w, bias=None, residual=None, act="none", out_dtype=F32, dtype=F64,
            round_ln=BF16, mut=""):
    """gemm(LayerNorm(x), w, ...).  round_ln = bf16 where zs_gemm_ln rounds the normalised rows
    (its MFMA A operand); None for zs_gemm_ln_f32, which keeps them in f32.  ln_w = ln_b = None:
    normalise only (zs_gemm_ln; zs_gemm_ln_f32 without LN parameters is plain ``gemm``)."""
    h = layernorm(x, ln_w, ln_b, eps, dtype, mut)
    h = _round(h, None if mut == "no_ln_round" else round_ln)
    return gemm(h, w, bias, residual, act, out_dtype, dtype, mut)


def topk_sorted(v, idx, k):
    """The k best of (value, index) pairs along the last axis: value descending, then index
    ascending (a stable sort of values that are already in index order).  Short rows are padded
    with (-inf, PAD_IDX)."""
    n = v.shape[-1]
    if n < k:
        v = torch.cat([v, torch.full(v.shape[:-1] + (k - n,), -INF, dtype=v.dtype)], -1)
        idx = torch.cat([idx, torch.full(idx.shape[:-1] + (k - n,), PAD_IDX, dtype=idx.dtype)], -1)
    order = torch.sort(v, dim=-1, descending=True, stable=True)[1][..., :k]
    return torch.gather(v, -1, order), torch.gather(idx, -1, order)


def lmhead(a, w, topk, row_norm=False, temperature=1.0, dtype=F64, mut=""):
    """logits = a w^T (row_norm: / max(||a||, 1e-12); then / temperature, a true division), and per
    block of 128 columns: the max, sum(exp(logit - max)) and the top-``topk`` (value, index) ordered
    by value descending then index ascending; a partial last block is padded with
    (-inf, PAD_IDX).  -> dict(logits [M, V], stat [M, nblk, 2], val / idx [M, nblk, topk],
    lse [M], gval / gidx [M, topk])."""
    M, K = a.shape
    V = w.shape[0]
    nblk = (V + LM_BN - 1) // LM_BN
    logits = matmul(a, w, dtype)
    if row_norm:
        n2 = (a.to(dtype) ** 2).sum(-1, keepdim=True)
        nrm = n2 if mut == "norm_sq" else torch.sqrt(n2)
        logits = logits * (1.0 / torch.clamp_min(nrm, 1e-12))
    if temperature != 1.0:
        t = torch.tensor(temperature, dtype=F32).to(dtype)       # the kernel's float argument
        logits = logits * t if mut == "temp_mul" else logits / t
    stat = torch.zeros(M, nblk, 2, dtype=dtype)
    val = torch.zeros(M, nblk, topk, dtype=dtype)
    idx = torch.zeros(M, nblk, topk, dtype=torch.int64)
    cols = torch.arange(V).expand(M, V)
    for b in range(nblk):
        lo, hi = b * LM_BN, min(V, (b + 1) * LM_BN)
        blk = logits[:, lo:hi]
        mx = blk.max(-1, keepdim=True)[0]
        if mut == "lse_block_max" and hi - lo > 64:
            # two-half merge with each half's sum-exp rescaled by the OTHER half's max
            m0, m1 = blk[:, :64].max(-1, keepdim=True)[0], blk[:, 64:].max(-1, keepdim=True)[0]
            s0, s1 = torch.exp(blk[:, :64] - m0).sum(-1), torch.exp(blk[:, 64:] - m1).sum(-1)
            se = s0 * torch.exp(m1 - mx)[:, 0] + s1 * torch.exp(m0 - mx)[:, 0]
        else:
            se = torch.exp(blk - mx).sum(-1)
        stat[:, b, 0], stat[:, b, 1] = mx[:, 0], se
        bv, bi = blk, cols[:, lo:hi]
        if mut == "tie_high":            # ties -> the higher index: sort the reversed columns
            bv, bi = bv.flip(-1), bi.flip(-1)
        val[:, b], idx[:, b] = topk_sorted(bv, bi, topk)
    g = stat[:, :, 0].max(-1)[0]
    lse = g + torch.log((stat[:, :, 1] * torch.exp(stat[:, :, 0] - g[:, None])).sum(-1))
    gval, gidx = topk_sorted(logits, cols, topk)
    return dict(logits=logits, stat=stat, val=val, idx=idx, lse=lse, gval=gval, gidx=gidx)


def bubble_insert(vals, k, fixed):
    """CPU emulation of topk_insert (csrc/lmhead.hip), the select-only register insertion of one
    lane: ``vals`` in increasing index order.  fixed=False is the loop before the tie-order fix (a bubble whose
    displaced entry is compared with strict > against its successor); True is the kernel's loop:
    lt[q] = cv > tv[q] on the old list, slot q takes cv where lt[q] and not lt[q - 1] and its upper
    neighbour where both hold.  -> [(value, index)] of length k."""
    tv, ti = [-INF] * k, [PAD_IDX] * k
    for n, v in enumerate(vals):
        cv, ci = float(v), n
        if not cv > tv[k - 1]:
            continue
        if fixed:
            lt = [cv > tv[q] for q in range(k)]
            for q in range(k - 1, 0, -1):
                if lt[q]:
                    tv[q], ti[q] = (tv[q - 1], ti[q - 1]) if lt[q - 1] else (cv, ci)
            if lt[0]:
                tv[0], ti[0] = cv, ci
        else:
            for q in range(k):
                if cv > tv[q]:
                    tv[q], ti[q], cv, ci = cv, ci, tv[q], ti[q]
    return list(zip(tv, ti))


# ------------------------------------------------------------------ shared case builders
def strided(t, ld, fill=NAN):
    """``t`` [R, C] inside an [R + 1][ld] buffer of its dtype, ``fill`` in every padding column and
    in the extra row.  -> (buffer, view [R, C])."""
    R, C = t.shape
    assert ld >= C
    buf = torch.full((R + 1, ld), fill, dtype=t.dtype)
    buf[:R, :C] = t
    return buf, buf[:R, :C]


def operands(M, N, K, dt, seed, lda=None, ldw=None, kind="randn"):
    """Seeded A [M, K] and W [N, K] of storage type ``dt`` in NaN-padded strided buffers.
    kind: "randn" (A ~ N(0,1), W ~ N(0,1/K)), "ints" (integers in [-3, 3]: every partial sum is
    exact in f32) or "grid" (multiples of 1/8 in [-2, 2]: products multiples of 1/64, sums exact)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "ints":
        a = torch.randint(-3, 4, (M, K), generator=g).to(F32)
        w = torch.randint(-3, 4, (N, K), generator=g).to(F32)
    elif kind == "grid":
        a = torch.randint(-16, 17, (M, K), generator=g).to(F32) / 8
        w = torch.randint(-16, 17, (N, K), generator=g).to(F32) / 8
    else:
        a = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
    abuf, av = strided(a.to(dt), lda or K)
    wbuf, wv = strided(w.to(dt), ldw or K)
    return dict(abuf=abuf, a=av, wbuf=wbuf, w=wv, gen=g)


# The common table of epilogues: (bias, residual, out dtype, out layout, activation).
#   bias      "none" | "al" (16-byte aligned) | "off" (4 bytes past a 16-byte boundary)
#   residual  "none" | "pad4" (ldr = N + 4, aligned) | "pad1" (ldr = N + 1) | "alias" (= out)
#   layout    "n" (ldo = N) | "n8" (ldo = N + 8) | "n3" (ldo = N + 3) | "off" (ldo = N + 8, the
#             base 4 bytes past a 16-byte boundary)
# Every value of every column occurs, every scalar-fallback condition (out / residual / bias)
# occurs with bf16 and with f32 output, and every activation with both output types.
EPILOGUES = (
    ("none", "none", F32, "n", "none"),
    ("al", "pad4", BF16, "n8", "gelu_erf"),
    ("off", "pad1", F32, "n3", "gelu_tanh"),
    ("al", "alias", F32, "off", "relu"),
    ("off", "pad4", BF16, "n3", "tanh"),
    ("al", "pad1", BF16, "off", "gelu_tanh"),
    ("none", "alias", F32, "n8", "gelu_erf"),
    ("off", "none", BF16, "n", "relu"),
    ("al", "none", F32, "n3", "tanh"),
    ("off", "pad4", F32, "off", "gelu_erf"),
    ("al", "pad1", BF16, "n", "none"),
    ("none", "pad4", BF16, "off", "relu"),
)
OUT_SENTINEL = -776.0        # exact in bf16; no case's output comes near it


def out_layout(N, layout, out_dtype):
    """-> (ldo, element offset of the view in its buffer)."""
    if layout == "n":
        return N, 0
    if layout == "n8":
        return N + 8, 0
    if layout == "n3":
        return N + 3, 0
    assert layout == "off"
    return N + 8, (1 if out_dtype == F32 else 2)


def epilogue(M, N, epi, gen, kind="randn"):
    """Seeded epilogue operands of one EPILOGUES row: bias [N] or None, the residual inside its
    [M + 1][ldr] NaN-padded buffer (alias: values only; the GPU test places them in the output
    buffer, whose padding holds the sentinel)."""
    bias_m, res_m, out_dtype, layout, act = epi
    ints = kind != "randn"
    bias = res = rbuf = None
    if bias_m != "none":
        bias = (torch.randint(-3, 4, (N,), generator=gen).to(F32) if ints
                else torch.randn(N, generator=gen))
    if res_m != "none":
        r = (torch.randint(-3, 4, (M, N), generator=gen).to(F32) if ints
             else torch.randn(M, N, generator=gen))
        ldo, _ = out_layout(N, layout, out_dtype)
        ldr = {"pad4": N + 4, "pad1": N + 1, "alias": ldo}[res_m]
        rbuf, res = strided(r, ldr, OUT_SENTINEL if res_m == "alias" else NAN)
    return dict(bias=bias, bias_off=bias_m == "off", res=res, rbuf=rbuf, alias=res_m == "alias",
                out_dtype=out_dtype, layout=layout, act=act)


def gemm_case(M, N, K, dt, epi, seed, lda=None, ldw=None, kind="randn"):
    """One strided zs_gemm problem with its float64 reference, float32 yardstick and tolerance."""
    c = operands(M, N, K, dt, seed, lda, ldw, kind)
    c.update(epilogue(M, N, epi, c.pop("gen"), kind))
    c.update(M=M, N=N, K=K, dt=dt, epi=epi, kind=kind)
    return c


def gemm_expect(c, mut="", **kw):
    """-> (ref64, yardstick, tol) of a gemm_case under the project's rule.  As in the other
    kernel tests the float64 reference and the float32 yardstick are the values before the output
    rounding; the bf16 term of the tolerance, 2^-8 |ref| elementwise, is what rounding the output
    itself may cost (half a bf16 step is at most 2^-8 of the value).  Comparing two rounded values
    instead would fail at a rounding tie: one bf16 step is up to 2^-7 of the value."""
    args = (c["a"], c["w"], c["bias"], c["res"], c["act"], F32)
    ref = gemm(*args, dtype=F64, mut=mut, **kw).double()
    if mut:
        return ref
    yard, tol = tolerance(ref, gemm(*args, dtype=F32), c["out_dtype"] == BF16)
    return ref, yard, tol


def ln_case(M, N, K, wdt, epi, seed, affine=True, ldx=None):
    """One zs_gemm_ln / zs_gemm_ln_f32 problem: f32 rows with a GPT-2-like outlier column inside
    an [M + 1][ldx] NaN-padded buffer, W of storage type ``wdt`` (contiguous: ldw = K)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 3 + 0.5
    x[:, 5] += 40.0
    xbuf, xv = strided(x, ldx or K)
    lw = (torch.randn(K, generator=g) * 0.2 + 1) if affine else None
    lb = (torch.randn(K, generator=g) * 0.1) if affine else None
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(wdt)
    c = dict(xbuf=xbuf, x=xv, ln_w=lw, ln_b=lb, w=w, M=M, N=N, K=K, eps=1e-5, epi=epi)
    c.update(epilogue(M, N, epi, g))
    return c


ACT_SLOPE = {"none": 1.0, "relu": 1.0, "tanh": 1.0, "gelu_erf": 1.13, "gelu_tanh": 1.13}


def ln_flip_allowance(c):
    """What a rounding tie of the normalised rows may cost an output.  zs_gemm_ln rounds
    LayerNorm(x) to bf16 before the product; where the float64 value lies within float32's reach
    of a rounding boundary, a correct float32 LayerNorm may round to the other neighbour, which
    moves that A element by one bf16 step and the sum of output (m, n) by step * |w[n, k]|
    (before bias and activation; ln_expect scales it by the activation's largest slope).  An element
    counts as near a boundary when its distance is within 4 x the float32 LayerNorm's largest
    relative deviation from float64 on this case (relative to max(|h|, 1)); nothing here comes
    from a kernel.  -> [M, N] float64, zero for rows without such an element."""
    h64 = layernorm(c["x"], c["ln_w"], c["ln_b"], c["eps"], F64)
    h32 = layernorm(c["x"], c["ln_w"], c["ln_b"], c["eps"], F32).double()
    scale = torch.clamp_min(h64.abs(), 1.0)
    thr = 4.0 * float(((h32 - h64).abs() / scale).max()) * scale
    r = h64.to(BF16).double()
    step = torch.exp2(torch.floor(torch.log2(torch.clamp_min(r.abs(), 1e-30))) - 7.0)
    near = (0.5 * step - (h64 - r).abs()) <= thr
    return (near * step) @ c["w"].double().abs().t()


def ln_expect(c, round_ln, mut=""):
    """As gemm_expect; the rounding of the normalised rows (round_ln) is part of both runs, and
    with it the tolerance adds ln_flip_allowance (the float64 reference itself is ambiguous at a
    rounding tie of an A element)."""
    args = (c["x"], c["ln_w"], c["ln_b"], c["eps"], c["w"], c["bias"], c["res"], c["act"], F32)
    ref = gemm_ln(*args, dtype=F64, round_ln=round_ln, mut=mut).double()
    if mut:
        return ref
    yard, tol = tolerance(ref, gemm_ln(*args, dtype=F32, round_ln=round_ln),
                          c["out_dtype"] == BF16)
    if round_ln is not None:
        # the moved A element changes the value BEFORE the activation: an activation's largest
        # slope carries it to the output (GELU: Phi(x) + x phi(x) <= 1.129 at x = sqrt(2), either form)
        tol = tol + ACT_SLOPE[c["act"]] * ln_flip_allowance(c)
    return ref, yard, tol


def lmhead_case(M, V, K, dt, seed, kind="grid", lda=None):
    """One zs_lmhead_topk_t problem: A strided with NaN padding, W contiguous (the entry takes no
    ldw) followed by one NaN row.  kind "grid" / "ints": every logit is exact in f32, so the
    float64 order is the kernel's order and ties are exact; "spike": all logits of a row equal
    (a = w = 1 / 8 everywhere) except one column per block, the issue's constant-plus-one-spike."""
    if kind == "spike":
        a = torch.full((M, K), 0.125)
        w = torch.full((V, K), 0.125)
        for b in range((V + LM_BN - 1) // LM_BN):     # column 40 of even blocks, 3 of odd ones
            n = b * LM_BN + (3 if b % 2 else 40)
            if n < V:
                w[n, :] = 0.25
        abuf, av = strided(a.to(dt), lda or K)
        wbuf, wv = strided(w.to(dt), K)
        return dict(abuf=abuf, a=av, wbuf=wbuf, w=wv, M=M, V=V, K=K, dt=dt, kind=kind)
    c = operands(M, V, K, dt, seed, lda, None, kind)
    c.pop("gen")
    c.update(M=M, V=V, K=K, dt=dt, kind=kind)
    return c


def margins(val):
    """Gaps between consecutive entries of the float64 top lists [.., k + 1] (finite ones)."""
    d = val[..., :-1] - val[..., 1:]
    return d[torch.isfinite(d)]


# ------------------------------------------------------------------ the shared sweeps
# One 12-epilogue sweep per epilogue implementation, at a ragged N (an nv < 8 column tail, N % 4
# != 0) and at an N % 8 == 0 (where ldo = N / N + 8 and ldr = N + 4 take the vector paths):
# route -> (M, N ragged, N aligned, K, operand dtype, split_k).  tests/test_gpu_gemm_kernels.py
# runs sweep(route) under the route's knobs; tests/test_gemm_ref.py draws the mutants' cases here.
SWEEPS = {
    "lean104": (69, 70, 72, 192, BF16, 1),       # 64 x 64 4-stage lean tile: epi_slab WN = 32
    "lean101": (133, 134, 136, 128, BF16, 1),    # 128 x 128 lean tile: epi_slab WN = 64
    "lean113": (133, 102, 104, 128, BF16, 1),    # 128 x 96 lean tile: epi_slab WN = 96
    "big18": (261, 262, 264, 128, BF16, 1),      # gemm_big_kernel: big_epilogue
    "ring": (69, 70, 72, 128, BF16, 1),          # gemm_fast_kernel bf16 (gemm_lean 0)
    "ring_f32": (69, 70, 72, 96, F32, 1),        # gemm_fast_kernel F32
    "splitk": (69, 70, 72, 160, BF16, 3),        # ring slabs (short last split) + splitk_reduce_kernel
    "splitk_f32": (69, 70, 72, 160, F32, 2),
    "staged": (130, 150, 152, 96, BF16, 1),      # gemm_kernel<bf16_t> (gemm_fast 0)
    "staged_f32": (130, 150, 152, 96, F32, 1),   # gemm_kernel<float> (f32_fast 0)
    "rows": (17, 1002, 1000, 256, BF16, 0),      # gemm_rows_kernel epilogue
    "skinny": (64, 70, 72, 256, BF16, 0),        # gemm_skinny_kernel: skinny_store
    "skinny_f32": (65, 70, 72, 256, F32, 0),
}


# The library's defaults of the knobs the GPU tests set (zs_tune_set has no getter, so the tests'
# context manager restores to these; tests/test_gemm_ref.py checks them against the g_*
# initialisers in csrc, lean128_ns against the ZS_LEAN128_NS default).
KNOB_DEFAULTS = dict(gemm_fast=1, f32_fast=1, fast_tile=0, fast_persist=1, fast_xcd=1, gemm_lean=1,
                     lean96=0, lean8w=0, lean128_ns=3, lm_prio=1, gemm_rows=1, rows_nt48=1,
                     rows_wide=0, skinny_mode=1, f32_tile=8)
SK_MAX_TILES = 4096          # gemm_skinny.hip: the int tile counters at the head of its workspace


def _seed(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 1000003
    return s


def k_per_split(K, split_k):
    """zs_gemm's split: k per slab rounded up to the 32-deep k tile."""
    return -(-(-(-K // split_k)) // 32) * 32


def sweep(route, aligned=False, only=None):
    """The route's cases over the whole epilogue table -> [(label, case)]."""
    M, Nr, Na, K, dt, _ = SWEEPS[route]
    N = Na if aligned else Nr
    out = []
    for i, epi in enumerate(EPILOGUES):
        if only is not None and i not in only:
            continue
        out.append((f"{route}/N{N}/e{i}", gemm_case(M, N, K, dt, epi, _seed(route, N, i))))
    return out


def sweep_case(route, i, aligned=False):
    return sweep(route, aligned, only=(i,))[0][1]


# mutant -> (kind of case, how to build it): every one is a case the GPU file runs
MUTANT_CASES = {
    "gelu_swap": ("gemm", lambda: sweep_case("lean104", 6)),          # f32 out, erf GELU
    "bias_shift_tail": ("gemm", lambda: sweep_case("lean101", 2)),    # bias, N % 8 = 6
    "drop_k8": ("gemm", lambda: sweep_case("lean104", 0)),
    "ldr_is_n": ("gemm", lambda: sweep_case("ring", 2)),              # ldr = N + 1
    "split_last": ("gemm", lambda: sweep_case("splitk", 0)),
    "no_ln_round": ("ln", lambda: ln_named("ln-K768-N202-aff")),
    "ln_affine_skipped": ("ln", lambda: ln_named("ln-K1024-N144-aff")),
    "tie_high": ("lm", "tie-V129-M64-K64-bf16-k8-ints"),
    "temp_mul": ("lm", "V129-M70-K64-f32_ring-k6-ints-t0.7"),
    "norm_sq": ("lm", "V100-M64-K96-bf16-k2-ints-norm"),
    "lse_block_max": ("lm", "V128-M65-K768-bf16-k5-grid"),
}


def lm_stat_tolerance(r64, r32):
    """Tolerances of the LM head's statistics -> dict(max, sumexp, lse) of (yardstick, tol).  The
    float32 yardstick sums a block's 128 exponentials the way torch does (pairwise); the kernels
    add 32 or 64 of them in one serial chain per lane, which on equal terms (the spike case)
    rounds the same way at every step.  So the sum-exp is held to the bound of a float32 sum of
    n = 128 positive terms in ANY order, n * 2^-24 * sum, on top of the rule; the log-sum-exp
    inherits it as an absolute term."""
    chain = LM_BN * 2.0 ** -24
    ymax, tmax = tolerance(r64["stat"][..., 0], r32["stat"][..., 0])
    yse, tse = tolerance(r64["stat"][..., 1], r32["stat"][..., 1])
    ylse, tlse = tolerance(r64["lse"], r32["lse"])
    return dict(max=(ymax, tmax), sumexp=(yse, tse + chain * r64["stat"][..., 1]),
                lse=(ylse, tlse + chain))


def lane_subsets(path, V, BM=64):
    """The column subsets of block 0 that one lane (one thread) of the LM head scans in index
    order before any merge: "ring" = lmhead_kernel's transposed register epilogue (for_token_cols
    of csrc/lmhead.hip: 32 columns per lane, 4-wide groups 8 apart in each 32-column MFMA tile, two
    tiles per wave row), "tile" = lmhead_tile_kernel's LDS tile epilogue (128 / (256 / BM)
    consecutive columns per thread)."""
    subs = []
    if path == "ring":
        for wr0 in (0, 64):
            for h in (0, 1):
                subs.append([wr0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h
                             for i in (0, 1) for e in range(16)])
    else:
        cpt = LM_BN // (256 // BM)
        subs = [list(range(s, s + cpt)) for s in range(0, LM_BN, cpt)]
    return [[n for n in sub if n < V] for sub in subs]


# ------------------------------------------------------------------ the LM head cases
# V: 3 (fewer columns than topk), 100 (one partial block), 128, 129 (a full block + 1 column),
# 1000 (8 blocks: several XCD-remap rounds, nwg % 8 != 0 at odd row-tile counts); M on both sides
# of the 64- / 128-row kernels; K on and off the K % 64 main loop; mode = bf16 | f32 on the ring
# (f32_fast 1) | f32 on the LDS tile epilogue (f32_fast 0).
LM_VS, LM_MS, LM_KS, LM_TOPKS = (3, 100, 128, 129, 1000), (1, 64, 65, 70, 130), (64, 96, 768), (1, 2, 5, 6, 8)
LM_MODES = ("bf16", "f32_ring", "f32_tile")


def lm_specs():
    """25 seeded cases: every (V, M) pair once, the other axes cycled with co-prime periods.
    -> [dict(id, M, V, K, mode, topk, row_norm, temp, stat, lda, kind, knobs)]"""
    out = []
    n = 0
    for r in range(5):
        for i in range(5):
            V, M = LM_VS[i], LM_MS[(i + r) % 5]
            K, mode = LM_KS[n % 3], LM_MODES[(n // 3) % 3]
            topk = LM_TOPKS[(i + 2 * r) % 5]
            row_norm = n % 4 == 1
            temp = 0.7 if n % 4 == 3 else 1.0
            # exact logits in every case: integers where the row norm divides them (gaps of
            # 1 / ||a|| stay >= 1e-3), else multiples of 1 / 64; the spike case is the constant row
            kind = "ints" if row_norm or n % 3 == 0 else ("spike" if n % 5 == 3 else "grid")
            out.append(dict(id=f"V{V}-M{M}-K{K}-{mode}-k{topk}-{kind}" + ("-norm" if row_norm else "")
                            + ("-t0.7" if temp != 1.0 else ""),
                            M=M, V=V, K=K, mode=mode, topk=topk, row_norm=row_norm, temp=temp,
                            stat=n % 6 != 4, lda=K + 8 if n % 2 == 0 else K, kind=kind, seed=100 + n,
                            knobs=dict(fast_xcd=0 if n % 4 == 2 else 1, lm_prio=0 if n % 5 == 1 else 1,
                                       f32_fast=0 if mode == "f32_tile" else 1)))
            n += 1
    # the tie cases on every epilogue: the constant row with one spike per block (topk 5: the
    # example of the tie-order fix) and small integers (many exact ties) at the 8-entry list
    for mode in LM_MODES:
        for V, M, topk, kind in ((1000, 70, 5, "spike"), (129, 64, 8, "ints"), (128, 130, 2, "spike")):
            out.append(dict(id=f"tie-V{V}-M{M}-K64-{mode}-k{topk}-{kind}", M=M, V=V, K=64, mode=mode,
                            topk=topk, row_norm=False, temp=1.0, stat=True, lda=64, kind=kind,
                            seed=200 + n,
                            # lm_prio only acts on bf16, K % 64 == 0, no row_norm: off once there
                            # on a case with a list (KMAX 8)
                            knobs=dict(fast_xcd=1, lm_prio=0 if (mode, kind) == ("bf16", "ints") else 1,
                                       f32_fast=0 if mode == "f32_tile" else 1)))
            n += 1
    return out


def lm_build(s):
    return lmhead_case(s["M"], s["V"], s["K"], BF16 if s["mode"] == "bf16" else F32, s["seed"],
                       s["kind"], s["lda"])


# ------------------------------------------------------------------ the LayerNorm-GEMM cases
LN_MS = (1, 16, 17, 64)
F32_EPIS = tuple(e for e in EPILOGUES if e[2] == F32)


def ln_specs():
    """zs_gemm_ln: K 768 / 1024, with the affine and normalise-only, N for the 48-, 64-
    (rows_nt48 2), 32- (N >= 1536) and 16-column tiles; M and ldx cycled; the affine cases take
    the f32-output epilogues in turn (the mutants' cases have the sharp tolerance), the
    normalise-only ones eight different rows of the table; ln_epi_specs runs the whole table.
    -> [dict(id, M, N, K, affine, epi, ldx, knobs, seed)]"""
    out = []
    n = 0
    for K in (768, 1024):
        for N, knobs in ((144, {}), (128, dict(rows_nt48=2)), (1542, {}), (202, {})):
            for affine in (True, False):
                epi = F32_EPIS[n % len(F32_EPIS)] if affine else EPILOGUES[(5 * (n // 2) + 1) % 12]
                out.append(dict(id=f"ln-K{K}-N{N}-" + ("aff" if affine else "norm"), M=LN_MS[n % 4],
                                N=N, K=K, affine=affine, epi=epi, ldx=K + 4 if n % 3 else K,
                                knobs=knobs, seed=300 + n))
                n += 1
    return out


def ln_epi_specs(affine):
    """The whole epilogue table on zs_gemm_ln in one LN mode (with the affine: LNM 1, K 768;
    normalise-only: LNM 2, K 1024), at a ragged N (202: 16-column tiles, a column tail with
    N % 4 != 0) and at an N % 8 == 0 (144: 48-column tiles), 17 rows, ldx = K + 4."""
    K = 768 if affine else 1024
    return [dict(id=f"ln-epi{i}-N{N}-" + ("aff" if affine else "norm"), M=17, N=N, K=K,
                 affine=affine, epi=epi, ldx=K + 4, knobs={}, seed=600 + 24 * affine + 12 * (N == 144) + i)
            for N in (202, 144) for i, epi in enumerate(EPILOGUES)]


def ln_f32_specs():
    """zs_gemm_ln_f32: LayerNorm (always with its affine) at K 768 / 1024 on 32-column tiles, no
    LayerNorm at K 768 / 1024 / 3072 on 16-column tiles; f32 output only."""
    out = []
    n = 0
    for ln, K in ((True, 768), (True, 1024), (False, 768), (False, 1024), (False, 3072)):
        for N in (70, 202):
            out.append(dict(id=f"lnf32-K{K}-N{N}-" + ("aff" if ln else "plain"), M=LN_MS[(n + 1) % 4],
                            N=N, K=K, affine=ln, epi=F32_EPIS[n % len(F32_EPIS)],
                            ldx=K + 4 if n % 2 else K, knobs={}, seed=400 + n))
            n += 1
    return out


def ln_build(s, wdt=BF16):
    return ln_case(s["M"], s["N"], s["K"], wdt, s["epi"], s["seed"], s["affine"], s["ldx"])


def ln_named(name):
    return ln_build([s for s in ln_specs() if s["id"] == name][0])


def lm_named(name):
    return [s for s in lm_specs() if s["id"] == name][0]
