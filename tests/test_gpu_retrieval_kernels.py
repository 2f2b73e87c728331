"""zs_sim_rank (csrc/lmhead.hip) and zs_sim_topk_finalize (csrc/gpt2.hip) against
tests/retrieval_ref.py.  Operands are NaN-padded views of [rows + 1][ld] buffers (a padding column
or the extra row read shows as NaN), outputs are sentinel-filled with a guard row behind them.

Exact data (integers / multiples of 1/8: every similarity exact in f32, asserted on the CPU in
tests/test_retrieval_ref.py): ranks and target similarities are compared exactly, in both dtypes
and both block orders.  Real-valued unit vectors: every rank must lie in the bracket of the ranks
an arithmetic within tau = 4 x float32 yardstick + 1e-6 of float64 can give, no pair left out;
exact copies of a target's gallery row must follow the tie rule exactly."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_ref as R  # noqa: E402
from gemm_ref import KNOB_DEFAULTS  # noqa: E402
from gpu_helpers import Out  # noqa: E402

pytestmark = pytest.mark.gpu
I32 = torch.int32
SENT, ISENT = -7.5, -7


def _ops():
    from zsaac import ops
    return ops


@contextlib.contextmanager
def fast_xcd(v):
    from zsaac._lib import call
    call("zs_tune_set", b"fast_xcd", v)
    try:
        yield
    finally:
        call("zs_tune_set", b"fast_xcd", KNOB_DEFAULTS["fast_xcd"])


def _views(dev, c):
    R_, K = c["q"].shape
    N = c["g"].shape[0]
    return c["qbuf"].to(dev)[:R_, :K], c["gbuf"].to(dev)[:N, :K]


def _rank(dev, q, g, tgt):
    """zs_sim_rank into sentinel-filled outputs -> (rank, tgt_sim) on the CPU."""
    M, T = tgt.shape
    rank, sim = Out(dev, (M, T), I32, ISENT), Out(dev, (M, T), torch.float32, SENT)
    _ops().sim_rank(q, g, tgt.to(dev), sim.t, rank.t)
    torch.cuda.synchronize()
    return rank.cpu(), sim.cpu()


@pytest.fixture(scope="module")
def exact():
    return {(spec, dt): R.exact_case(*spec, dt=dt) for spec in R.EXACT_CASES for dt in ("f32", "bf16")}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("spec", R.EXACT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_sim_rank_exact(cuda, exact, spec, dt):
    c = exact[(spec, dt)]
    q, g = _views(cuda, c)
    for xcd in (1, 0):
        with fast_xcd(xcd):
            rank, sim = _rank(cuda, q, g, c["tgt"])
        assert torch.equal(rank.long(), c["rank"]), f"fast_xcd={xcd}"
        assert torch.equal(sim.double(), c["tsim"]), f"fast_xcd={xcd}"


@pytest.fixture(scope="module")
def real():
    return {(dt, dups): R.real_case(dt, dups) for dt in ("f32", "bf16") for dups in (False, True)}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sim_rank_real_brackets(cuda, real, dt):
    c = real[(dt, False)]
    q, g = _views(cuda, c)
    rank, sim = _rank(cuda, q, g, c["tgt"])
    want = torch.gather(c["sim"], 1, c["tgt"].long())
    err = float((sim.double() - want).abs().max())
    print(f"{dt}: yardstick {c['yard']:.2e} tau {c['tau']:.2e} |tgt_sim err| {err:.2e}")
    assert err <= c["tau"]
    assert bool(((rank.long() >= c["lo"]) & (rank.long() <= c["hi"])).all())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sim_rank_duplicates_follow_the_tie_rule(cuda, real, dt):
    """Gallery row TIE_J and its copies at 100 / 390 / 410 / 900 are the five targets of every
    query, in index order: equal similarities bit for bit and five consecutive ranks."""
    c = real[(dt, True)]
    q, g = _views(cuda, c)
    rank, sim = _rank(cuda, q, g, c["tgt"])
    assert bool((sim == sim[:, :1]).all())
    assert torch.equal(rank - rank[:, :1], torch.arange(5, dtype=I32).repeat(rank.shape[0], 1))
    assert bool(((rank.long() >= c["lo"]) & (rank.long() <= c["hi"])).all())
    assert float((sim.double() - torch.gather(c["sim"], 1, c["tgt"].long())).abs().max()) <= c["tau"]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sim_rank_rows_do_not_depend_on_the_launch(cuda, real, dt):
    """Bitwise: two runs are equal; the rows permuted give the outputs permuted; a row alone
    (M = 1, the 64-row tile) and the first 65 rows give that row's results of the full launch."""
    c = real[(dt, False)]
    q, g = _views(cuda, c)
    M = q.shape[0]
    one, two = _rank(cuda, q, g, c["tgt"]), _rank(cuda, q, g, c["tgt"])
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5))
    moved = _rank(cuda, q[perm.to(cuda)].contiguous(), g, c["tgt"][perm])
    assert torch.equal(moved[0], one[0][perm]) and torch.equal(moved[1], one[1][perm])
    for lo, hi in ((77, 78), (0, 65)):
        part = _rank(cuda, q[lo:hi], g, c["tgt"][lo:hi])
        assert torch.equal(part[0], one[0][lo:hi]) and torch.equal(part[1], one[1][lo:hi])


def test_sim_rank_refusals_leave_the_outputs_untouched(cuda):
    from zsaac._lib import ZsError, call
    c = R.exact_case(129, 65, 64, 8, "grid")
    q, g = _views(cuda, c)
    M, N, K, T = 65, 129, 64, 8
    ld = q.stride(0)
    tgt = c["tgt"].to(cuda)
    rank, sim = Out(cuda, (M, T), I32, ISENT), Out(cuda, (M, T), torch.float32, SENT)
    P = lambda t: t.data_ptr()                                               # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    good = dict(M=M, N=N, K=K, dtype=0, Q=P(q), ldq=ld, G=P(g), ldg=ld, tgt=P(tgt), T=T,
                tgt_sim=P(sim.t), rank=P(rank.t))
    bad = [dict(M=0), dict(N=0), dict(K=0), dict(M=-1), dict(K=48), dict(ldq=K + 4), dict(ldg=K + 4),
           dict(ldq=K - 8), dict(ldg=32), dict(dtype=2), dict(T=0), dict(T=9), dict(Q=None),
           dict(G=None), dict(tgt=None), dict(tgt_sim=None), dict(rank=None), dict(Q=P(q) + 4),
           dict(G=P(g) + 8), dict(M=1 << 30, T=2), dict(M=1 << 28, T=8)]
    for b in bad:
        a = dict(good, **b)
        with pytest.raises(ZsError):
            call("zs_sim_rank", a["M"], a["N"], a["K"], a["dtype"], a["Q"], a["ldq"], a["G"],
                 a["ldg"], a["tgt"], a["T"], a["tgt_sim"], a["rank"], st)
    torch.cuda.synchronize()
    assert bool((rank.cpu() == ISENT).all()) and bool((sim.cpu() == SENT).all())
    # the ops layer refuses host tensors and wrong dtypes before the library is reached
    with pytest.raises(ZsError):
        _ops().sim_rank(q.cpu(), g, tgt, sim.t, rank.t)
    with pytest.raises(ZsError):
        _ops().sim_rank(q, g, tgt.long(), sim.t, rank.t)


# ------------------------------------------------------------------ zs_sim_topk_finalize
@pytest.mark.parametrize("k,kpart", [(1, 8), (5, 8), (8, 8), (1, 1)])
@pytest.mark.parametrize("nblk", [1, 3, 393])
def test_sim_topk_finalize_scripted(cuda, nblk, k, kpart):
    """Hand-made partial lists: values from a set of five (ties within and across blocks),
    padding entries in the short last block; 6 rows (two blocks of 4 waves, one partial)."""
    M = 6
    pv, pi = R.scripted_partials(M, nblk, kpart, seed=100 * nblk + kpart)
    wv, wi = R.merge_partials(pv, pi, k)
    ov, oi = Out(cuda, (M, k), torch.float32, SENT), Out(cuda, (M, k), I32, ISENT)
    _ops().sim_topk_finalize(pv.to(cuda), pi.to(cuda), M, nblk, kpart, k, ov.t, oi.t)
    torch.cuda.synchronize()
    assert torch.equal(oi.cpu().long(), wi)
    assert torch.equal(ov.cpu().double(), wv)


def test_sim_topk_finalize_padding_comes_last(cuda):
    """One block of 5 columns, k = kpart = 8: five real entries, then (-inf, 0x7fffffff)."""
    pv, pi = R.scripted_partials(3, 1, 8, seed=9)
    ov, oi = Out(cuda, (3, 8), torch.float32, SENT), Out(cuda, (3, 8), I32, ISENT)
    _ops().sim_topk_finalize(pv.to(cuda), pi.to(cuda), 3, 1, 8, 8, ov.t, oi.t)
    torch.cuda.synchronize()
    assert bool((oi.cpu()[:, 5:] == R.PAD_IDX).all()) and bool((ov.cpu()[:, 5:] == -R.INF).all())
    assert bool((oi.cpu()[:, :5] < 5).all())
    from zsaac._lib import ZsError
    for kk, kp in ((0, 8), (9, 9), (5, 4)):
        with pytest.raises(ZsError):
            _ops().sim_topk_finalize(pv.to(cuda), pi.to(cuda), 3, 1, kp, kk, ov.t, oi.t)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("spec", [R.EXACT_CASES[i] for i in (0, 2, 3, 6)],
                         ids=lambda c: "-".join(map(str, c)))
def test_topk_behind_lmhead_topk_exact(cuda, exact, spec, dt):
    """zs_lmhead_topk with the gallery as W, then zs_sim_topk_finalize, on the exact data against
    the stable sort: indices and values exact (ties -> lower index, also across blocks)."""
    ops = _ops()
    c = exact[(spec, dt)]
    q, g = _views(cuda, c)
    g = g.contiguous()                              # zs_lmhead_topk takes W with contiguous rows
    M, N = c["M"], c["N"]
    nblk = ops.lmhead_nblk(N)
    for k in (1, 5, 8):
        pv = torch.empty(M, nblk, k, device=cuda)
        pi = torch.empty(M, nblk, k, device=cuda, dtype=I32)
        ops.lmhead_topk(q, g, k, None, pv, pi, M=M)
        ov, oi = Out(cuda, (M, k), torch.float32, SENT), Out(cuda, (M, k), I32, ISENT)
        ops.sim_topk_finalize(pv, pi, M, nblk, k, k, ov.t, oi.t)
        torch.cuda.synchronize()
        wv, wi = R.topk(c["sim"], k)
        assert torch.equal(oi.cpu().long(), wi), k
        assert torch.equal(ov.cpu().double(), wv), k
