"""Plain CPU references of the teacher-forced scoring kernels (zs_gpt2_score_embed,
zs_lmhead_nll, zs_nll_finalize), one function per kernel, and the cases their tests share.

Pure torch on the CPU, float64 wherever a float is computed, from the dtype-rounded operands (a
bf16 case's reference multiplies the bf16 values exactly); nothing here reads a golden or the
original project.  tests/test_score_ref.py asserts the input conditions the GPU tests rely on
(float64 top-2 margins, the edges every case list must contain); tests/test_gpu_score_kernels.py
compares the kernels with these functions.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import torch

I32 = torch.int32
LM_BN = 128              # the LM head's column block


# ------------------------------------------------------------------ score_embed
def score_embed(hard_ids, hard_len, soft, soft_ld, n_soft, cap_ids, cap_len, wte, wpe, B, Smax):
    """Row b: [wte(hard[b][:H]) ; soft rows ; wte(cap[b][:T-1])] + wpe, zero from
    S = H + n_soft + max(T - 1, 0) on.  score_rows[b][t] = b*Smax + H + n_soft - 1 + t and
    tgt[b][t] = cap[b][t] for t < T; b*Smax and -1 beyond.  An id outside [0, V) is embedded as id
    0, its target (if a caption id) is -1, and it is counted.
    -> (x f64 [B, Smax, D], plen, score_rows, tgt, count)."""
    V, D = wte.shape
    Tmax, h_cap = cap_ids.shape[1], hard_ids.shape[1]
    w, pe, sf = wte.double(), wpe.double(), soft.double().reshape(-1)
    x = torch.zeros(B, Smax, D, dtype=torch.float64)
    plen = torch.zeros(B, dtype=I32)
    rows = torch.zeros(B, Tmax, dtype=I32)
    tgt = torch.full((B, Tmax), -1, dtype=I32)
    bad = 0

    def tok(i):
        return int(i) if 0 <= int(i) < V else 0

    for b in range(B):
        H, T = int(hard_len[b]), int(cap_len[b])
        assert 0 <= H <= h_cap and 0 <= T <= Tmax
        P = H + n_soft
        S = P + max(T - 1, 0)
        plen[b] = S
        for h in range(H):
            bad += not 0 <= int(hard_ids[b, h]) < V
        for p in range(S):
            if p < H:
                e = w[tok(hard_ids[b, p])]
            elif p < P:
                e = sf[b * soft_ld + (p - H) * D: b * soft_ld + (p - H + 1) * D]
            else:
                e = w[tok(cap_ids[b, p - P])]
            x[b, p] = e + pe[p]
        for t in range(Tmax):
            rows[b, t] = b * Smax + (P - 1 + t if t < T else 0)
            if t < T:
                ok = 0 <= int(cap_ids[b, t]) < V
                bad += not ok
                tgt[b, t] = int(cap_ids[b, t]) if ok else -1
    return x, plen, rows, tgt, bad


EMBED_HCAP, EMBED_NSOFT, EMBED_TMAX, EMBED_V = 3, 2, 4, 50


def embed_case(D: int, bad: str = "") -> Dict:
    """Every (H, T) of H in {0, 1, h_cap} x T in {0, 1, 2, Tmax}; ``bad``: one id outside the
    vocabulary ('cap_mid': an embedded caption id, 'cap_last': a caption's last id, a target
    only, 'hard': a hard prompt id)."""
    g = torch.Generator().manual_seed(11 + D)
    hs, ts = (0, 1, EMBED_HCAP), (0, 1, 2, EMBED_TMAX)
    B = len(hs) * len(ts)
    hard_len = torch.tensor([h for h in hs for _ in ts], dtype=I32)
    cap_len = torch.tensor([t for _ in hs for t in ts], dtype=I32)
    hard_ids = torch.randint(0, EMBED_V, (B, EMBED_HCAP), generator=g).to(I32)
    cap_ids = torch.randint(0, EMBED_V, (B, EMBED_TMAX), generator=g).to(I32)
    b_full = B - 1                                   # H = h_cap, T = Tmax
    cap_ids[b_full, 1], hard_ids[b_full, 0] = 7, 9   # (not id 0: what a bad id is embedded as)
    if bad == "cap_mid":
        cap_ids[b_full, 1] = EMBED_V
    elif bad == "cap_last":
        cap_ids[b_full, EMBED_TMAX - 1] = -3
    elif bad == "hard":
        hard_ids[b_full, 0] = EMBED_V + 7
    soft_ld = EMBED_NSOFT * D + 8                    # a padded soft stride
    return dict(B=B, hard_ids=hard_ids, hard_len=hard_len, cap_ids=cap_ids, cap_len=cap_len,
                soft=torch.randn(B, soft_ld, generator=g), soft_ld=soft_ld,
                wte=torch.randn(EMBED_V, D, generator=g), wpe=torch.randn(16, D, generator=g))


# ------------------------------------------------------------------ lmhead_nll + nll_finalize
def logits64(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return a.double() @ w.double().t()


def nll_rows(logits: torch.Tensor, tgt: torch.Tensor):
    """Per row of float64 logits [M, V]: lse, argmax (lower index on ties), the target's logit and
    logprob = logit[tgt] - lse; a row whose target is outside [0, V) is ignored (logprob 0).
    -> (lse, argmax int32, tgt_logit, logprob, valid)."""
    M, V = logits.shape
    lse = torch.logsumexp(logits, -1)
    mx = logits.max(-1).values
    amax = (logits == mx[:, None]).to(torch.int8).argmax(-1).to(I32)      # first maximum
    valid = (tgt >= 0) & (tgt < V)
    tl = logits.gather(1, tgt.clamp(0, V - 1).long()[:, None])[:, 0]
    lp = torch.where(valid, tl - lse, torch.zeros_like(lse))
    return lse, amax, tl, lp, valid


def caption_sums(logprob: torch.Tensor, valid: torch.Tensor, B: int, Tmax: int):
    """Per caption (rows b*Tmax .. b*Tmax + Tmax - 1): the float64 sum of its counted rows'
    log-probs and their number."""
    lp = torch.where(valid, logprob.double(), torch.zeros(1, dtype=torch.float64)).view(B, Tmax)
    return lp.sum(1), valid.view(B, Tmax).sum(1).to(I32)


def top2_margin(logits: torch.Tensor) -> torch.Tensor:
    v = logits.topk(2, dim=-1).values
    return v[:, 0] - v[:, 1]


def split_rows(M: int) -> Tuple[int, int]:
    """(B, Tmax) the M-row cases finalize as."""
    return {1: (1, 1), 64: (8, 8), 70: (7, 10)}[M]


LM_CASES = [(V, M, K, dt) for V in (81, 128, 1000) for M in (1, 64, 70) for K in (768, 96)
            for dt in ("f32", "bf16")] + [(50257, 70, 768, "bf16")]
MARGIN = 1e-3
SPIKE = 60.0             # the stability row: one logit about this far above the rest


def edge_targets(V: int) -> List[int]:
    """Targets at 0, 127, 128 (where the vocabulary has them), inside the partial last block, V - 1
    and the two ignored values -1 and V."""
    e = [0, 127, 128, (V // LM_BN) * LM_BN + (V % LM_BN) // 2 if V % LM_BN else None, V - 1]
    return [t for t in e if t is not None and 0 <= t < V] + [-1, V]


@functools.lru_cache(maxsize=None)
def lm_case(V: int, M: int, K: int, dt: str) -> Dict:
    """a [M, K], w [V, K] rounded to the case's dtype and tgt [M]: rows 0.. take edge_targets(V)
    (M = 1: the last vocabulary entry), the next row its own float64 argmax, the last row
    (M >= 64) is SPIKE / |w_j|^2 times a vocabulary row j -- logit j about SPIKE above every other
    -- with another column as target; every other target is random.  Computed once per case and
    shared (callers leave it unchanged).  The seed is advanced until
    every row's float64 top-2 margin is at least MARGIN (a property of the inputs alone)."""
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    for attempt in range(64):
        g = torch.Generator().manual_seed(1000 * attempt + V + 7 * M + K)
        a = torch.randn(M, K, generator=g)
        w = (torch.randn(V, K, generator=g) * 0.05).to(dtype).float()
        tgt = torch.randint(0, V, (M,), generator=g).to(I32)
        spike = None
        if M >= 64:
            j = int(torch.randint(0, V, (1,), generator=g))
            a[M - 1] = w[j] * (SPIKE / float((w[j].double() ** 2).sum()))
            spike = (M - 1, j)
            tgt[M - 1] = (j + 1 + V // 2) % V
        a = a.to(dtype).float()
        logits = logits64(a, w)
        if float(top2_margin(logits).min()) < MARGIN:
            continue
        edges = edge_targets(V)
        own = None
        if M == 1:
            tgt[0] = V - 1
        else:
            n = min(len(edges), M - 2)
            tgt[:n] = torch.tensor(edges[:n], dtype=I32)
            own = n
            tgt[own] = int(logits[own].argmax())
        return dict(a=a.to(dtype), w=w.to(dtype), tgt=tgt, logits=logits, spike=spike, own=own,
                    dtype=dtype, edges=edges)
    raise AssertionError("no seed gives the top-2 margin")
