"""Plain CPU references of the retrieval kernels (zs_sim_rank of csrc/lmhead.hip,
zs_sim_topk_finalize of csrc/gpt2.hip) and of zsaac/retrieval.py, written from their definitions,
and the cases the GPU tests run.

Pure torch / numpy on the CPU.  Similarities are gemm_ref.matmul: float64 is the reference,
float32 (k accumulated in chunks of 16) the yardstick; operands are taken in their storage type,
so bf16 cases are computed from the bf16-rounded operands.  Ranks are COUNTED
(#{greater} + #{equal at a lower index}), the top-k is a stable sort, the metrics are the
definitions of R@k / median / mean rank / mAP@10 on 0-based ranks.  Nothing here reads the
original project; tests/test_retrieval_ref.py ties these functions to the golden recorded from it
and asserts the input conditions of the GPU cases.

``rule`` names one deliberate mistake of a rank kernel (RULES).  It is only ever set by
tests/test_retrieval_ref.py, which shows on the CPU that the inputs of the GPU cases tell each of
them from the reference; no wrong kernel is ever run.
"""
from __future__ import annotations

import numpy as np
import torch

from gemm_ref import BF16, F32, F64, INF, LM_BN, NAN, PAD_IDX, matmul, strided  # noqa: F401

RULES = ("ge", "self", "tie_high", "drop_last_block", "pad_cols", "tgt_stride")


# ------------------------------------------------------------------ the ops
def ranks(sim, tgt, rule=""):
    """rank[m][t] = #{n != j : sim[m][n] > sim[m][j]} + #{n < j : sim[m][n] == sim[m][j]},
    tsim[m][t] = sim[m][j] for j = tgt[m][t] in [0, N); (-1, 0) outside.  int64 / sim's dtype."""
    M, N = sim.shape
    T = tgt.shape[1]
    flat = tgt.reshape(-1)
    if rule == "tgt_stride":       # tgt read as [M][T + 1]
        flat = torch.cat([flat, torch.full((M,), -1, dtype=tgt.dtype)])
    rank = torch.full((M, T), -1, dtype=torch.int64)
    tsim = torch.zeros(M, T, dtype=sim.dtype)
    n = torch.arange(N)
    n_eff = N
    if rule == "drop_last_block" and N % LM_BN:
        n_eff = N - N % LM_BN
    for m in range(M):
        for t in range(T):
            j = int(flat[m * (T + 1) + t] if rule == "tgt_stride" else tgt[m, t])
            if not 0 <= j < N:
                continue
            v = sim[m, j]
            row = sim[m]
            if rule == "ge":
                before = (row >= v) & (n != j)
            elif rule == "self":
                before = (row > v) | ((row == v) & (n <= j))
            elif rule == "tie_high":
                before = (row > v) | ((row == v) & (n > j))
            else:
                before = (row > v) | ((row == v) & (n < j))
            c = int(before[:n_eff].sum())
            if rule == "pad_cols" and N % LM_BN and 0.0 > float(v):
                c += LM_BN - N % LM_BN          # the zero rows behind the gallery, as columns
            rank[m, t] = c
            tsim[m, t] = v
    return rank, tsim


def topk(sim, k):
    """The k largest of each row: value descending, then index ascending (a stable sort of the
    negated row); with k > N the tail is (-inf, PAD_IDX).  -> (val, idx int64)."""
    M, N = sim.shape
    order = torch.sort(-sim, dim=1, stable=True).indices[:, :k]
    val = torch.gather(sim, 1, order)
    if k > N:
        val = torch.cat([val, torch.full((M, k - N), -INF, dtype=sim.dtype)], 1)
        order = torch.cat([order, torch.full((M, k - N), PAD_IDX, dtype=order.dtype)], 1)
    return val, order


def merge_partials(pv, pi, k):
    """The k first entries of each row's [nblk][kpart] partial lists in the order value
    descending, then index ascending (padding entries (-inf, PAD_IDX) are last in it)."""
    M = pv.shape[0]
    v = pv.reshape(M, -1).double().numpy()
    i = pi.reshape(M, -1).numpy().astype(np.int64)
    ov, oi = np.empty((M, k)), np.empty((M, k), dtype=np.int64)
    for m in range(M):
        o = np.lexsort((i[m], -v[m]))[:k]
        ov[m], oi[m] = v[m][o], i[m][o]
    return torch.from_numpy(ov), torch.from_numpy(oi)


def metrics(rank, mode, group_max=False):
    """(r1, r5, r10, r50, medr, meanr, mAP10) in float64 from 0-based ranks.
    "a2t": rank [n, per]: a clip counts with the best rank of its group; its AP@10 is
    sum_p p / pos_p over the group's 1-based positions pos_1 < pos_2 < ... that are <= 10, divided
    by the group size.  "t2a": rank [n]: mAP10 = mean over ALL queries of 1 / (rank + 1) where
    rank < 10 (0 elsewhere)."""
    r = np.asarray(rank, dtype=np.float64)
    if mode == "a2t":
        best = r.max(1) if group_max else r.min(1)
        ap = []
        for row in r:
            pos = sorted(x + 1 for x in row if x < 10)
            ap.append(sum((p + 1) / x for p, x in enumerate(pos)) / len(row))
        map10 = 100.0 * float(np.sum(ap)) / len(best)
    else:
        best = r.reshape(-1)
        map10 = 100.0 * float(np.sum(np.where(best < 10, 1.0 / (best + 1), 0.0))) / len(best)
    rec = [100.0 * float(np.mean(best < c)) for c in (1, 5, 10, 50)]
    return (*rec, float(np.floor(np.median(best)) + 1), float(best.mean() + 1), map10), best


def yardstick(q, g):
    """(sim64, yard, tau): the float32 chunked dot product's largest deviation from float64 on
    this data and the project's tolerance 4 x yard + 1e-6."""
    s64 = matmul(q, g, F64)
    yard = float((matmul(q, g, F32).double() - s64).abs().max())
    return s64, yard, 4.0 * yard + 1e-6


def brackets(sim64, tgt, tau):
    """[lo, hi] per (m, t): every rank an arithmetic within tau of float64 can give:
    lo = #{sim > t + tau}, hi = #{sim >= t - tau} - 1 (the target itself is in the second set)."""
    M, T = tgt.shape
    lo = torch.full((M, T), -1, dtype=torch.int64)
    hi = torch.full((M, T), -1, dtype=torch.int64)
    for m in range(M):
        for t in range(T):
            j = int(tgt[m, t])
            if 0 <= j < sim64.shape[1]:
                v = sim64[m, j]
                lo[m, t] = int((sim64[m] > v + tau).sum())
                hi[m, t] = int((sim64[m] >= v - tau).sum()) - 1
    return lo, hi


def min_gap(sim64):
    """The smallest distance between two values of one row."""
    s = torch.sort(sim64, dim=1).values
    return float((s[:, 1:] - s[:, :-1]).min())


# ------------------------------------------------------------------ the GPU cases
DTS = {"f32": F32, "bf16": BF16}
# (N, M, K, T, kind): kind "ints" = integers in [-3, 3]; "grid" = multiples of 1/8 in [-1, 1]
# (products multiples of 1/64); "equal" = every gallery row the same.  Every value is exact in
# bf16 and every partial sum in f32, so both dtypes give the float64 similarities bit for bit.
EXACT_CASES = (
    (3, 1, 64, 1, "ints"),
    (128, 64, 96, 5, "ints"),
    (129, 65, 64, 8, "grid"),
    (1000, 130, 1024, 5, "ints"),
    (1000, 65, 96, 8, "grid"),
    (129, 130, 1024, 1, "ints"),
    (1000, 65, 64, 8, "equal"),
    (128, 1, 1024, 8, "grid"),
)
# N = 1000 cases: column TIE_J and exact copies of its gallery row below and above it in its own
# 128-column block (384 .. 511) and in other blocks; slot 0 of every third row targets TIE_J
TIE_J, TIE_COPIES = 400, (100, 390, 410, 900)


def _seed(*parts):
    s = 0
    for p in parts:
        s = (s * 1000003 + (sum(map(ord, p)) if isinstance(p, str) else int(p))) % (2 ** 31 - 1)
    return s


def targets(M, N, T, gen, ties=False):
    """tgt [M][T] int32: random columns; slot 0 walks the edges (column 0, 127, 128, N - 1 where
    they exist, -1 and N: outside); with T > 1 every fourth row names one column twice."""
    tgt = torch.randint(0, N, (M, T), generator=gen).to(torch.int32)
    special = [c for c in (0, 127, 128, N - 1) if c < N] + [-1, N]
    for m in range(M):
        tgt[m, 0] = special[m % len(special)]
        if ties and m % 3 == 1:
            tgt[m, 0] = TIE_J
        if T > 1 and m % 4 == 2:
            tgt[m, T - 1] = tgt[m, 1]
    return tgt


def exact_case(N, M, K, T, kind, dt="f32", pad=8):
    """Operands of storage type ``dt`` in NaN-padded [rows + 1][K + pad] buffers, targets, and the
    float64 similarities / expected ranks."""
    g = torch.Generator().manual_seed(_seed("exact", N, M, K, T, kind))
    if kind == "grid":
        q = torch.randint(-8, 9, (M, K), generator=g).to(F32) / 8
        w = torch.randint(-8, 9, (N, K), generator=g).to(F32) / 8
    else:
        q = torch.randint(-3, 4, (M, K), generator=g).to(F32)
        w = torch.randint(-3, 4, (N, K), generator=g).to(F32)
    if kind == "equal":
        w = w[:1].repeat(N, 1)
    ties = N == 1000 and kind != "equal"
    if ties:
        for c in TIE_COPIES:
            w[c] = w[TIE_J]
    tgt = targets(M, N, T, g, ties)
    qbuf, qv = strided(q.to(DTS[dt]), K + pad)
    gbuf, gv = strided(w.to(DTS[dt]), K + pad)
    sim = matmul(qv, gv, F64)
    rank, tsim = ranks(sim, tgt)
    return dict(qbuf=qbuf, q=qv, gbuf=gbuf, g=gv, tgt=tgt, sim=sim, rank=rank, tsim=tsim,
                ties=ties, N=N, M=M, K=K, T=T)


def max_partial_sum(q, g):
    """The largest |partial sum| of any dot product taken in k order (float64)."""
    q, g = q.double(), g.double()
    acc = torch.zeros(q.shape[0], g.shape[0], dtype=F64)
    top = 0.0
    for k in range(q.shape[1]):
        acc += q[:, k:k + 1] * g[:, k][None, :]
        top = max(top, float(acc.abs().max()))
    return top


# real-valued unit vectors: Clotho-eval's gallery, a fifth of its queries
REAL_N, REAL_M, REAL_K, REAL_T = 1045, 209, 1024, 5
REAL_WIDTH_CAP = 4


def real_case(dt="f32", dups=False):
    """Unit rows "shared base + noise": query m is near gallery rows 5 m .. 5 m + 4 (its targets).
    ``dups``: gallery row TIE_J copied to TIE_COPIES and every query's targets are those five
    columns in index order (a rank kernel that takes the target's value from other arithmetic than
    the compared values misplaces them)."""
    g = torch.Generator().manual_seed(_seed("real", dups))
    base = torch.randn(REAL_M, REAL_K, generator=g, dtype=F64)
    q = base + 0.8 * torch.randn(REAL_M, REAL_K, generator=g, dtype=F64)
    w = base.repeat_interleave(REAL_T, 0) + 2.0 * torch.randn(REAL_N, REAL_K, generator=g, dtype=F64)
    q = (q / q.norm(dim=1, keepdim=True)).to(F32)
    w = (w / w.norm(dim=1, keepdim=True)).to(F32)
    tgt = (torch.arange(REAL_M)[:, None] * REAL_T + torch.arange(REAL_T)[None, :]).to(torch.int32)
    if dups:
        for c in TIE_COPIES:
            w[c] = w[TIE_J]
        tgt = torch.tensor(sorted(TIE_COPIES + (TIE_J,)), dtype=torch.int32).repeat(REAL_M, 1)
    qbuf, qv = strided(q.to(DTS[dt]), REAL_K + 8)
    gbuf, gv = strided(w.to(DTS[dt]), REAL_K + 8)
    sim, yard, tau = yardstick(qv, gv)
    lo, hi = brackets(sim, tgt, tau)
    return dict(qbuf=qbuf, q=qv, gbuf=gbuf, g=gv, tgt=tgt, sim=sim, yard=yard, tau=tau, lo=lo,
                hi=hi)


# ------------------------------------------------------------------ scripted top-k partials
def scripted_partials(M, nblk, kpart, seed, N=None):
    """[M][nblk][kpart] lists as zs_lmhead_topk writes them for a gallery of N columns (default: a
    last block of 5 columns): per block distinct columns of that block, values from a small set
    (ties within and across blocks), ordered by value descending, then index ascending; a block
    with fewer than kpart columns ends in padding entries."""
    N = N if N is not None else (nblk - 1) * LM_BN + 5
    g = torch.Generator().manual_seed(seed)
    pv = torch.full((M, nblk, kpart), -INF, dtype=F32)
    pi = torch.full((M, nblk, kpart), PAD_IDX, dtype=torch.int32)
    for m in range(M):
        for b in range(nblk):
            cols = min(LM_BN, N - b * LM_BN)
            n = min(kpart, cols)
            idx = torch.randperm(cols, generator=g)[:n] + b * LM_BN
            val = torch.randint(-2, 3, (n,), generator=g).to(F32) / 4
            o = np.lexsort((idx.numpy(), -val.numpy()))
            pv[m, b, :n] = val[o]
            pi[m, b, :n] = idx[o].to(torch.int32)
    return pv, pi


# ------------------------------------------------------------------ the golden's views
def golden_operands(gold, dt="f32"):
    """The golden's embeddings as the device path sees them: rows L2-normalised in float32, then
    rounded to ``dt``.  -> (audio [5 n, K], caps [5 n, K]) of that storage type."""
    def norm(x):
        x = torch.from_numpy(np.asarray(x)).float()
        return (x / x.norm(dim=1, keepdim=True).clamp(min=1e-12)).to(DTS[dt])
    return norm(gold["audio_embs"]), norm(gold["cap_embs"])


def golden_expect(audio, caps, per=5):
    """Float64 similarities and counted ranks of both directions from the given operands:
    dict(a2t=(sim, rank [n, per], top1), t2a=(sim, rank [n per], top1))."""
    n = audio.shape[0] // per
    a = audio[0:n * per:per]
    s_a = matmul(a, caps, F64)
    t_a = (torch.arange(n)[:, None] * per + torch.arange(per)[None, :]).to(torch.int32)
    s_t = matmul(caps[:n * per], a, F64)
    t_t = (torch.arange(n * per) // per)[:, None].to(torch.int32)
    return dict(a2t=(s_a, ranks(s_a, t_a)[0], topk(s_a, 1)[1][:, 0], t_a),
                t2a=(s_t, ranks(s_t, t_t)[0][:, 0], topk(s_t, 1)[1][:, 0], t_t))
