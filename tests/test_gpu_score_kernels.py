"""The teacher-forced scoring kernels (zs_gpt2_score_embed, zs_lmhead_nll, zs_nll_finalize) one by
one against tests/score_ref.py (float64, from the dtype-rounded operands), at the smallest shapes
that cover every tile and edge: V of one partial block / one block / full blocks + a partial one
and the model's 50257, M of 1 / 64 / 70 rows (the 64- and 128-row tiles, a partial tile), K on
and off the K % 64 main loop, both dtypes.

Every output is filled with a sentinel and allocated with a guard row behind it.  Targets, counts,
ignored rows and argmax ids are exact (the cases' float64 top-2 margins are >= 1e-3, asserted on
the CPU in tests/test_score_ref.py).  lse / logprob tolerances: f32 the project's 1e-3 absolute
(test_lmhead_topk); bf16 -- products exact in f32, only the accumulation differs -- twice the
error of the existing zs_lmhead_topk's lse against the same float64 reference on the same inputs,
but no less than the f32 figure."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as R  # noqa: E402
from gpu_helpers import Out  # noqa: E402

pytestmark = pytest.mark.gpu
I32 = torch.int32
F32_TOL = 1e-3
SENT = -7.5


def _ops():
    from zsaac import ops
    return ops


def _run_nll(dev, a, w, tgt, B, Tmax):
    """lmhead_nll + nll_finalize into sentinel-filled outputs -> dict of CPU tensors."""
    ops = _ops()
    M, V = a.shape[0], w.shape[0]
    nblk = ops.lmhead_nblk(V)
    ps = Out(dev, (M, nblk, 2), torch.float32, SENT)
    pv = Out(dev, (M, nblk), torch.float32, SENT)
    pi = Out(dev, (M, nblk), I32, -7)
    tl = Out(dev, (M,), torch.float32, SENT)
    lp = Out(dev, (M,), torch.float32, SENT)
    lse = Out(dev, (M,), torch.float32, SENT)
    am = Out(dev, (M,), I32, -7)
    sm = Out(dev, (B,), torch.float32, SENT)
    cnt = Out(dev, (B,), I32, -7)
    t = tgt.to(dev)
    ops.lmhead_nll(a, w, t, ps.t, pv.t, pi.t, tl.t)
    ops.nll_finalize(ps.t, pv.t, pi.t, t, tl.t, V, B, Tmax, lp.t, am.t, sm.t, cnt.t, lse=lse.t)
    torch.cuda.synchronize()
    return dict(ps=ps.cpu(), pv=pv.cpu(), pi=pi.cpu(), tl=tl.cpu(), lp=lp.cpu(), lse=lse.cpu(),
                am=am.cpu(), sum=sm.cpu(), cnt=cnt.cpu())


def _topk_lse(dev, a, w):
    """lse of the existing zs_lmhead_topk's partials (merged in float64 on the host)."""
    ops = _ops()
    M, V = a.shape[0], w.shape[0]
    nblk = ops.lmhead_nblk(V)
    ps = torch.empty(M, nblk, 2, device=dev)
    pv = torch.empty(M, nblk, 1, device=dev)
    pi = torch.empty(M, nblk, 1, device=dev, dtype=I32)
    ops.lmhead_topk(a, w, 1, ps, pv, pi)
    p = ps.cpu().double()
    mx = p[..., 0].max(1).values
    return mx + (p[..., 1] * torch.exp(p[..., 0] - mx[:, None])).sum(1).log()


@pytest.mark.parametrize("case", R.LM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_lmhead_nll_finalize(cuda, case):
    V, M, K, dt = case
    d = R.lm_case(*case)
    B, Tmax = R.split_rows(M)
    a, w = d["a"].to(cuda), d["w"].to(cuda)
    lse, amax, tl, lp, valid = R.nll_rows(d["logits"], d["tgt"])
    got = _run_nll(cuda, a, w, d["tgt"], B, Tmax)
    tol = F32_TOL
    if dt == "bf16":
        err_topk = float((_topk_lse(cuda, a, w) - lse).abs().max())
        tol = max(2.0 * err_topk, F32_TOL)
        print(f"{case}: zs_lmhead_topk lse error {err_topk:.3e} -> tolerance {tol:.3e}")
    e_lse = float((got["lse"].double() - lse).abs().max())
    e_lp = float((got["lp"].double() - lp)[valid].abs().max())
    e_tl = float((got["tl"].double() - tl)[valid].abs().max())
    print(f"{case}: |lse err| {e_lse:.3e} |logprob err| {e_lp:.3e} |target logit err| {e_tl:.3e}")
    # exact: argmax, ignored rows (no target logit written, logprob 0, not counted), counts
    assert torch.equal(got["am"], amax)
    assert bool((got["tl"][~valid] == SENT).all()) and bool((got["tl"][valid] != SENT).all())
    assert bool((got["lp"][~valid] == 0).all())
    want_sum, want_cnt = R.caption_sums(got["lp"], valid, B, Tmax)
    assert torch.equal(got["cnt"], want_cnt)
    assert e_lse <= tol and e_lp <= tol and e_tl <= tol
    # the caption reduction against the float64 sum of the same row values
    assert bool(((got["sum"].double() - want_sum).abs() <= 1e-5 * want_sum.abs()).all())
    # the per-block partials: every (row, block) written, top-1 ids in their block
    nblk = got["pi"].shape[1]
    lo = torch.arange(nblk)[None, :] * R.LM_BN
    assert bool(((got["pi"] >= lo) & (got["pi"] < torch.clamp(lo + R.LM_BN, max=V))).all())
    assert bool((got["ps"] != SENT).all()) and bool((got["pv"] != SENT).all())
    assert bool((got["ps"][..., 0] == got["pv"]).all())         # a block's max is its top-1 value


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_lmhead_nll_rows_permute_and_repeat(cuda, dt):
    """Bitwise: a row's results do not depend on where it sits in the launch (the rows of an
    M = 70 launch permuted -> the outputs permuted), and two runs are equal."""
    V, M, K = 1000, 70, 768
    d = R.lm_case(V, M, K, dt)
    a, w = d["a"].to(cuda), d["w"].to(cuda)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5))
    assert not torch.equal(perm, torch.arange(M))
    one = _run_nll(cuda, a, w, d["tgt"], 1, M)
    two = _run_nll(cuda, a, w, d["tgt"], 1, M)
    moved = _run_nll(cuda, a[perm.to(cuda)].contiguous(), w, d["tgt"][perm], 1, M)
    for k in ("ps", "pv", "pi", "tl", "lp", "lse", "am", "sum", "cnt"):
        assert torch.equal(one[k], two[k]), k
    for k in ("ps", "pv", "pi", "tl", "lp", "lse", "am"):
        assert torch.equal(moved[k], one[k][perm]), k


@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("K", [128, 96])             # lean_mainloop; fast_mainloop (K % 64 != 0)
@pytest.mark.parametrize("M", [130, 40])             # the 128-row tile twice (one ragged); the 64-row
def test_lmhead_nll_partials_equal_lmhead_topk(cuda, M, K, dt, xcd):
    """Bitwise: zs_lmhead_nll's per-block statistics and top-1 are the ones zs_lmhead_topk
    (topk 1, part_stat given, no row_norm) writes on the same inputs -- what scoring relies on to
    agree with the beam's log-probs.  V = 1000: 8 blocks, the last one partial; both block orders."""
    from zsaac._lib import call
    from gemm_ref import KNOB_DEFAULTS
    ops = _ops()
    V = 1000
    d = R.lm_case(V, M, K, dt)
    a, w = d["a"].to(cuda), d["w"].to(cuda)
    nblk = ops.lmhead_nblk(V)
    assert nblk == 8
    call("zs_tune_set", b"fast_xcd", xcd)
    try:
        ps, pv, pi = (Out(cuda, (M, nblk, 2), torch.float32, SENT),
                      Out(cuda, (M, nblk, 1), torch.float32, SENT), Out(cuda, (M, nblk, 1), I32, -7))
        ops.lmhead_topk(a, w, 1, ps.t, pv.t, pi.t)
        torch.cuda.synchronize()
        got = _run_nll(cuda, a, w, d["tgt"], 1, M)
    finally:
        call("zs_tune_set", b"fast_xcd", KNOB_DEFAULTS["fast_xcd"])
    assert bool((ps.cpu() != SENT).all()) and bool((got["ps"] != SENT).all())
    assert torch.equal(got["ps"], ps.cpu())
    assert torch.equal(got["pv"], pv.cpu()[..., 0])
    assert torch.equal(got["pi"], pi.cpu()[..., 0])


@pytest.mark.parametrize("Tmax", [1, 67, 130])
def test_nll_finalize_caption_reduction(cuda, Tmax):
    """zs_nll_finalize alone on hand-made partials (one block, max 0, sum-exp 1: lse = 0, so
    logprob = the target logit exactly): sums in position order against the float64 sum to 1e-5
    relative, counts exact; Tmax below, at and beyond one wave's 64 positions; ignored rows mixed
    in; a caption without any target."""
    ops = _ops()
    B, V = 5, 81
    M = B * Tmax
    g = torch.Generator().manual_seed(Tmax)
    tl = -torch.rand(M, generator=g) * 20
    tgt = torch.randint(0, V, (M,), generator=g).to(I32)
    drop = torch.rand(M, generator=g) < 0.3
    tgt[drop] = torch.where(torch.rand(int(drop.sum()), generator=g) < 0.5, -1, V).to(I32)
    tgt.view(B, Tmax)[3] = -1                       # an empty caption
    valid = (tgt >= 0) & (tgt < V)
    ps = torch.tensor([0.0, 1.0]).repeat(M, 1, 1)
    lp, am = Out(cuda, (M,), torch.float32, SENT), Out(cuda, (M,), I32, -7)
    sm, cnt = Out(cuda, (B,), torch.float32, SENT), Out(cuda, (B,), I32, -7)
    ops.nll_finalize(ps.to(cuda), torch.zeros(M, 1, device=cuda),
                     torch.full((M, 1), 3, dtype=I32, device=cuda), tgt.to(cuda), tl.to(cuda), V,
                     B, Tmax, lp.t, am.t, sm.t, cnt.t)
    torch.cuda.synchronize()
    assert torch.equal(lp.cpu(), torch.where(valid, tl, torch.zeros(1)))
    assert bool((am.cpu() == 3).all())
    want_sum, want_cnt = R.caption_sums(tl, valid, B, Tmax)
    assert torch.equal(cnt.cpu(), want_cnt) and int(want_cnt[3]) == 0
    got = sm.cpu().double()
    assert float(got[3]) == 0.0
    assert bool(((got - want_sum).abs() <= 1e-5 * want_sum.abs()).all())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("D", [40, 300])             # below and beyond one pass of the block
@pytest.mark.parametrize("bad", ["", "cap_mid", "cap_last", "hard"])
def test_score_embed(cuda, D, bad, dt):
    """H in {0, 1, h_cap} x T in {0, 1, 2, Tmax}, Smax with and without spare rows; one id outside
    the vocabulary -> status 1, embedded as id 0, target -1.  x is e + wpe in f32 (one rounding of
    the exact sum: equal to the float64 reference rounded)."""
    ops = _ops()
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    d = R.embed_case(D, bad)
    wte, wpe = d["wte"].to(dtype), d["wpe"].to(dtype)
    B = d["B"]
    for Smax in (R.EMBED_HCAP + R.EMBED_NSOFT + R.EMBED_TMAX - 1, 11):
        want = R.score_embed(d["hard_ids"], d["hard_len"], d["soft"], d["soft_ld"], R.EMBED_NSOFT,
                             d["cap_ids"], d["cap_len"], wte.float(), wpe.float(), B, Smax)
        x = Out(cuda, (B * Smax, D), torch.float32, SENT)
        plen = Out(cuda, (B,), I32, -7)
        rows, tgt = Out(cuda, (B, R.EMBED_TMAX), I32, -7), Out(cuda, (B, R.EMBED_TMAX), I32, -7)
        status = torch.zeros(1, dtype=I32, device=cuda)
        ops.score_embed(d["hard_ids"].to(cuda), d["hard_len"].to(cuda), d["soft"].to(cuda),
                        d["soft_ld"], R.EMBED_NSOFT, d["cap_ids"].to(cuda), d["cap_len"].to(cuda),
                        wte.to(cuda), wpe.to(cuda), B, Smax, x.t, plen.t, rows.t, tgt.t, status)
        torch.cuda.synchronize()
        assert int(status.item()) == want[4] == (1 if bad else 0)
        assert torch.equal(plen.cpu(), want[1])
        assert torch.equal(rows.cpu(), want[2])
        assert torch.equal(tgt.cpu(), want[3])
        assert torch.equal(x.cpu().view(B, Smax, D), want[0].float())
