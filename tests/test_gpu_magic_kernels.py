"""The magic-decoding and text-tower kernels (csrc/magic.hip, zs_l2norm_rows of csrc/norm.hip) one
by one against tests/magic_ref.py, at the shapes and edges where they can go wrong: row counts
that do not fill a block, strided rows, exact ties, ragged positions, histories scattered over
physical rows, frozen clips beside live ones.

Every output is filled with a sentinel and allocated with a guard row behind it; the guard must
come back unchanged.  Ids, flags, maps, lengths, copies and untouched regions are compared with
torch.equal.  Float outputs are compared with the float64 reference: the yardstick is the same
formula evaluated in float32 on the CPU, measured as its largest deviation from float64 on the
case's own data, and the tolerance is 4 x yardstick + 1e-6 (the rule of
test_gpu_glue.py::test_beam_step).  The input conditions of the cases (selection margins, the
situations each step scenario must contain, decoys that would win) are asserted on the CPU in
tests/test_magic_ref.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import magic_ref as M  # noqa: E402
from gpu_helpers import Out  # noqa: E402

pytestmark = pytest.mark.gpu
I32 = torch.int32
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
D = M.D
H_KINDS = ["f32", "bf16", "none"]


def _ops():
    from zsaac import ops
    return ops


def _check(name, got, ref64, ref32):
    """|got - float64 reference| <= 4 * yardstick + 1e-6, yardstick = max |float32 formula -
    float64| on this data; prints the three figures."""
    yard = float((ref32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    tol = 4.0 * yard + 1e-6
    print(f"{name}: error {err:.3e}, yardstick {yard:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (name, err, yard, tol)


def _h_out(dev, kind, shape):
    if kind == "none":
        return None
    return Out(dev, shape, F32 if kind == "f32" else BF16, -7.0)


# ------------------------------------------------------------------ text tower glue
@pytest.mark.parametrize("kind", H_KINDS)
def test_bert_embed_ln(cuda, kind):
    """T = 3 texts of L = 7 (21 rows: the last block holds one), a 50-row word table, ids with
    row 0, the last row and a [PAD] tail, a position table longer than L.
    Measured on an MI355X: x error 8.59e-07, yardstick 1.17e-06 (tolerance 5.68e-06), the same
    for every kind of h."""
    ops = _ops()
    T, L, V = 3, 7, 50
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, V - 1, (T, L), generator=g, dtype=I32)
    ids[0, 0], ids[1, 3], ids[2, 1] = 0, V - 1, V - 1
    ids[1, 5:] = 0
    ids[2, 3:] = 0
    word, pos = torch.randn(V, D, generator=g), torch.randn(L + 2, D, generator=g)
    type0, lw, lb = (torch.randn(D, generator=g) for _ in range(3))
    x = Out(cuda, (T * L, D), F32, -7.0)
    h = _h_out(cuda, kind, (T * L, D))
    ops.bert_embed_ln(ids.reshape(-1).to(cuda), L, word.to(cuda), pos.to(cuda), type0.to(cuda),
                      lw.to(cuda), lb.to(cuda), x.t, h.t if h else None)
    torch.cuda.synchronize()
    args = (ids.reshape(-1), L, word, pos, type0, lw, lb)
    got = x.cpu()
    _check(f"bert_embed_ln[{kind}]", got, M.bert_embed_ln(*args), M.bert_embed_ln(*args, dtype=F32))
    if h:
        assert torch.equal(h.cpu(), got.to(h.t.dtype))


@pytest.mark.parametrize("form", ["contiguous", "cls_rows"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("kind", H_KINDS)
def test_layernorm_dual(cuda, kind, rows, form):
    """Contiguous rows, and the CLS-row form: y, x and h are the first 768 columns of [rows,
    L*768] buffers (ldy = ldx = ldh = L*768, L = 3), whose other columns keep their sentinel.
    Measured on an MI355X: x error 3.88e-07 .. 7.03e-07 at yardsticks 4.58e-07 .. 8.09e-07; the
    closest case is 5 CLS rows, 7.03e-07 at yardstick 7.29e-07 (tolerance 3.92e-06)."""
    ops = _ops()
    ld = D if form == "contiguous" else 3 * D
    g = torch.Generator().manual_seed(rows)
    y = torch.randn(rows, ld, generator=g) * 2 + 0.5
    lw, lb = torch.randn(D, generator=g), torch.randn(D, generator=g)
    x = Out(cuda, (rows, ld), F32, -7.0)
    h = _h_out(cuda, kind, (rows, ld))
    ops.layernorm_dual(y.to(cuda)[:, :D], lw.to(cuda), lb.to(cuda), x.t[:, :D],
                       h.t[:, :D] if h else None)
    torch.cuda.synchronize()
    got = x.cpu()
    flat = torch.full((rows * ld,), -7.0)
    ref = [M.layernorm_dual(y.reshape(-1), rows, ld, lw, lb, 1e-12, flat, ld, dtype=dt).view(rows, ld)
           for dt in (F64, F32)]
    assert torch.equal(got[:, D:], ref[0][:, D:].float())               # the gaps
    _check(f"layernorm_dual[{kind}-{rows}-{form}]", got[:, :D], ref[0][:, :D], ref[1][:, :D])
    if h:
        hc = h.cpu()
        assert torch.equal(hc[:, :D], got[:, :D].to(hc.dtype))
        assert bool((hc[:, D:] == -7.0).all())


@pytest.mark.parametrize("inplace", [False, True])
def test_l2norm_rows(cuda, inplace):
    """M = 5 rows (two blocks) of C = 1024, one of them all zero (the eps branch: stays zero);
    out of place and in place, as the text tower and the audio encoder call it.
    Measured on an MI355X: error 1.15e-08, yardstick 8.13e-09 (tolerance 1.03e-06), both forms."""
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 1024, generator=g) * 3
    x[3] = 0.0
    if inplace:
        buf = Out(cuda, (5, 1024), F32, -7.0, init=x)
        assert ops.l2norm(buf.t, buf.t) is buf.t
    else:
        src = x.to(cuda)
        buf = Out(cuda, (5, 1024), F32, -7.0)
        ops.l2norm(src, buf.t)
    torch.cuda.synchronize()
    got = buf.cpu()
    if not inplace:
        assert torch.equal(src.cpu(), x)
    assert bool((got[3] == 0.0).all())
    _check(f"l2norm[inplace={inplace}]", got, M.l2norm_rows(x), M.l2norm_rows(x, dtype=F32))


# ------------------------------------------------------------------ row top-k
def _topk(dev, x, V, k, mode):
    ops = _ops()
    R = x.shape[0]
    val = Out(dev, (R, k), F32, -7.0)
    idx = Out(dev, (R, k), I32, -7)
    ops.row_topk(x.to(dev)[:, :V], k, val.t, idx.t, mode=mode)
    torch.cuda.synchronize()
    return val.cpu(), idx.cpu()


def _check_vals(name, got, ref64, ref32):
    inf = torch.isinf(ref64)
    assert torch.equal(got.double()[inf], ref64[inf])            # -inf stays -inf (mode 0)
    _check(name, got[~inf], ref64[~inf], ref32[~inf])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("V,ld,k", M.TOPK_CASES)
def test_row_topk(cuda, V, ld, k, mode):
    """Three random rows; V = 50257 is read through a view of row stride 2 V (as the prefill's
    logits are), the columns past V hold 1e9.  V = 1000 leaves threads without a column,
    V = 1025 gives one thread a second one; k = 1, 25, 64 and k = V at V = 40.
    Measured on an MI355X: mode 0 error at most 1.25e-06 (V = 40, yardstick 8.66e-07); closest to
    its bound V = 1025, k = 1: 4.93e-07 at yardstick 5.27e-08 (tolerance 1.21e-06).  Mode 1 error
    at most 1.06e-07 (V = 1025, k = 25, yardstick 4.61e-08)."""
    x = M.topk_case(V, ld, k)
    val, idx = _topk(cuda, x, V, k, mode)
    rv, ri = M.row_topk(x, V, k, mode)
    assert torch.equal(idx, ri)
    _check(f"row_topk[V={V} k={k} mode={mode}]", val, rv, M.row_topk(x, V, k, mode, dtype=F32)[0])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("V", [50257, 1000, 1025, 40])
def test_row_topk_exact_ties(cuda, V, mode):
    """magic_ref.topk_tie_rows: equal maxima in two waves and in the last column, in three
    slots of one thread, an all-equal row, a row with -inf entries (returned last, in index
    order, when k = V), equal runner-ups: the order is value descending, index ascending.
    Measured on an MI355X: mode 0 error at most 1.04e-06 (V = 1025, yardstick 1.72e-07, tolerance
    1.69e-06: the closest case of this file), mode 1 at most 3.49e-08."""
    x = M.topk_tie_rows(V)
    k = min(V, 64)
    val, idx = _topk(cuda, x, V, k, mode)
    rv, ri = M.row_topk(x, V, k, mode)
    assert torch.equal(idx, ri)
    _check_vals(f"row_topk ties[V={V} mode={mode}]", val, rv, M.row_topk(x, V, k, mode, dtype=F32)[0])


# ------------------------------------------------------------------ candidate rows
def test_magic_expand(cuda):
    """nbeams = 5, W = 3, Lmax = 11, pos from 1 to Lmax - 1; entries at t >= pos keep the sentinel."""
    ops = _ops()
    nb, W, Lmax = 5, 3, 11
    g = torch.Generator().manual_seed(4)
    kvrow = torch.randint(0, nb * W, (nb, Lmax), generator=g, dtype=I32)
    pos = torch.tensor([1, Lmax - 1, 4, 7, Lmax - 1], dtype=I32)
    kc = Out(cuda, (nb * W, Lmax), I32, -7)
    pc = Out(cuda, (nb * W,), I32, -7)
    ops.magic_expand(kvrow.to(cuda), pos.to(cuda), nb, W, Lmax, kc.t, pc.t)
    torch.cuda.synchronize()
    want_kv, want_pos = M.expand(kvrow, pos, W, torch.full((nb * W, Lmax), -7, dtype=I32))
    assert torch.equal(kc.cpu(), want_kv) and torch.equal(pc.cpu(), want_pos)
    assert int((want_kv == -7).sum()) == int(((Lmax - pos) * W).sum())


@pytest.mark.parametrize("name", list(M.MAXCOS_CASES))
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_magic_maxcos(cuda, dtype, name):
    """magic_ref.maxcos_case: 20 candidates (C = 2, b = 2, W = 5) and 5 (not a multiple of the 4
    per block), Lmax = 12, pos ragged per beam from 1 to 11, histories scattered over the clip's
    physical rows, every other slot of ctx a decoy that would win.  The whole of ctx is compared
    afterwards: the candidates' own rows are bit copies, nothing else changed.
    Measured on an MI355X: error 3.27e-08 .. 6.14e-08 at yardsticks 4.02e-08 .. 1.00e-07 (worst:
    bf16, 20 candidates, 6.14e-08 at yardstick 8.99e-08)."""
    ops = _ops()
    C, b, W, pos = M.MAXCOS_CASES[name]
    Lmax, R = M.MAXCOS_LMAX, C * b * W
    hid, ctx, kvrow, _ = M.maxcos_case(C, b, W, Lmax, pos, 3, dtype)
    pos_t = torch.tensor(pos, dtype=I32)
    ctx_d = Out(cuda, (R, Lmax, D), dtype, -7.0, init=ctx)
    mc = Out(cuda, (R,), F32, -7.0)
    ops.magic_maxcos(hid.to(cuda), R, W, ctx_d.t, Lmax, kvrow.to(cuda), pos_t.to(cuda), mc.t)
    torch.cuda.synchronize()
    r64, want_ctx = M.maxcos(hid, W, ctx, kvrow, pos_t)
    r32, _ = M.maxcos(hid, W, ctx, kvrow, pos_t, dtype=F32)
    assert torch.equal(ctx_d.cpu(), want_ctx)
    _check(f"maxcos[{name}-{dtype}]", mc.cpu(), r64, r32)


@pytest.mark.parametrize("E", M.SCORE_E)
@pytest.mark.parametrize("b,W,nact", M.SCORE_SHAPES)
def test_magic_score(cuda, b, W, nact, E):
    """C = 3 clips; every (alpha, beta, score_temp) of magic_ref.SCORE_MIX at CLAP temperature
    0.07; the clip's candidates past nact * W hold NaN inputs and must keep their sentinel.
    (8, 64, 8) fills the kernel's 512-entry array; E = 70 is no multiple of the wave.
    zs_magic_score (no score temperature) must equal zs_magic_score_t at 1.
    Measured on an MI355X: error at most 4.31e-06 (b 8, W 64, E 1024, at yardstick 5.32e-06);
    closest to its bound b 2, W 2, E 1024: 1.79e-06 at yardstick 1.29e-06 (tolerance 6.18e-06)."""
    ops = _ops()
    from zsaac._lib import call
    C = 3
    R = C * b * W
    pval, mc, text, audio = M.score_case(C, b, W, nact, E, 1)
    d = [t.to(cuda) for t in (pval, mc, text, audio)]
    init = torch.full((R,), -7.0)
    worst = (0.0, 0.0)
    for alpha, beta, stemp in M.SCORE_MIX:
        out = Out(cuda, (R,), F32, -7.0)
        ops.magic_score(d[0], d[1], d[2], d[3], C, b, W, nact, M.SCORE_TEMP, alpha, beta, out.t,
                        score_temp=stemp)
        torch.cuda.synchronize()
        got = out.cpu()
        args = (pval, mc, text, audio, b, W, nact, M.SCORE_TEMP, alpha, beta, stemp, init)
        r64, r32 = M.score(*args), M.score(*args, dtype=F32)
        idle = r64 == -7.0
        assert int(idle.sum()) == C * (b - nact) * W and bool((got[idle] == -7.0).all())
        yard = float((r32.double() - r64).abs().max())
        err = float((got.double() - r64).abs().max())
        worst = max(worst, (err, yard))
        assert err <= 4.0 * yard + 1e-6, (alpha, beta, stemp, err, yard)
        if stemp == 1.0:
            plain = Out(cuda, (R,), F32, -7.0)
            call("zs_magic_score", ops._p(d[0]), ops._p(d[1]), ops._p(d[2]), ops._p(d[3]), C, E, b,
                 W, nact, float(M.SCORE_TEMP), float(alpha), float(beta), ops._p(plain.t), ops._s())
            torch.cuda.synchronize()
            assert torch.equal(plain.cpu(), got)
    print(f"score[b={b} W={W} nact={nact} E={E}]: worst error {worst[0]:.3e} at yardstick {worst[1]:.3e}")


# ------------------------------------------------------------------ the step
def _dev_state(dev, state, hid_dtype):
    dev_s = {}
    for key in M.STATE_KEYS:
        t = state[key]
        dt = F32 if t.is_floating_point() else I32
        dev_s[key] = Out(dev, tuple(t.shape), dt, -7, init=t.to(dt))
    dev_s["sel_h"] = Out(dev, (state["scores"].numel(), D), hid_dtype, -7.0)
    return dev_s


def _launch(ops, dev_s, score_v, cand, C, b, W, first, greedy, step_no, max_steps_d, hid_d):
    ops.magic_step(score_v, cand, C, b, W, first, greedy, M.STOP, step_no, max_steps_d,
                   dev_s["scores"].t, dev_s["seq_len"].t, dev_s["stopped"].t, dev_s["tokens"].t,
                   dev_s["kvrow"].t, dev_s["pos"].t, dev_s["cdone"].t, dev_s["ntok"].t, hid_d,
                   dev_s["sel_h"].t)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dev_s.items()}


def _compare(got, ref, want_sel, tol, tag):
    for key in M.STATE_KEYS[2:]:
        assert torch.equal(got[key], ref[key]), (key, tag)
    assert torch.equal(got["seq_len"].double(), ref["seq_len"]), ("seq_len", tag)
    assert torch.equal(got["sel_h"], want_sel), ("sel_h", tag)
    err = float((got["scores"].double() - ref["scores"]).abs().max())
    assert err <= tol, ("scores", tag, err, tol)
    return err


STEP_CASES = [(b, W, False) for b, W in M.STEP_BEAM] + [(1, W, True) for W in M.STEP_GREEDY_W]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("b,W,greedy", STEP_CASES)
def test_magic_step(cuda, b, W, greedy, dtype):
    """magic_ref.step_scenario(b, W): eight calls on three clips with the state carried on the
    device and every state buffer (scores, seq_len, stopped, tokens, kvrow, pos, cdone, ntok,
    sel_h) compared with the reference after every call.  Clip 0 freezes when all its beams have
    stopped, clip 1 at its max_steps of 5, clip 2 runs the last legal step; the frozen clips are
    fed fresh scores, candidates and hidden rows and must not move.  The scenarios contain source
    permutations and duplicated sources (a beam rewritten before it is read), stopped beams that
    survive through their w = 0 row, ragged pos (asserted in tests/test_magic_ref.py).
    Measured on an MI355X: in every beam scenario the kernel's scores error equals the yardstick
    (the kernel evaluates the same float32 formula): 4.05e-06 (1, 1), 1.07e-06 (2, 2), 2.98e-07
    (3, 25), 7.15e-07 (5, 8), 9.54e-07 (8, 8), 4.77e-07 (8, 64); greedy scores are exactly 0."""
    ops = _ops()
    sc = M.step_scenario(b, W, greedy)
    C = sc.C
    tol = 4.0 * sc.yardstick() + 1e-6
    dev_s = _dev_state(cuda, sc.init, dtype)
    mx = sc.max_steps.to(cuda)
    want_sel = torch.full((C * b, D), -7.0, dtype=dtype)
    prev = sc.init
    worst = 0.0
    for s, ((score_v, cand), ref) in enumerate(zip(sc.inputs, sc.states)):
        hid = sc.hid(s, dtype)
        got = _launch(ops, dev_s, score_v.to(cuda), cand.to(cuda), C, b, W, s == 0, greedy, s, mx,
                      hid.to(cuda))
        moved = ref["ntok"].repeat_interleave(b) != prev["ntok"].repeat_interleave(b)
        want_sel[moved] = hid[ref["sel_c"][moved].long()]
        worst = max(worst, _compare(got, ref, want_sel, tol, (b, W, greedy, s)))
        if greedy:
            assert bool((got["scores"] == 0.0).all())
        prev = ref
    assert bool(prev["cdone"].all())
    print(f"step[b={b} W={W} greedy={greedy} {dtype}]: scores error {worst:.3e}, yardstick "
          f"{sc.yardstick():.3e}, tolerance {tol:.3e}")


@pytest.mark.parametrize("name", ["first", "greedy", "beam"])
def test_magic_step_exact_ties(cuda, name):
    """magic_ref.tie_cases: equal scores in the first branch (at the kept / dropped edge too),
    equal maxima in the greedy branch, and in the beam branch beams with equal scores, lengths and
    candidate scores (and a stopped beam's w = 0 row equal to live candidates): all values exact
    in float32, the lower flat index wins."""
    ops = _ops()
    c = M.tie_cases()[name]
    b, W = c["b"], c["W"]
    C = 2
    g = torch.Generator().manual_seed(9)
    hid = torch.randn(C * b * W, D, generator=g)
    info: list = []
    ref = M.step(c["state"], c["score"], c["cand"], b, W, c["first"], c["greedy"], M.STOP, c["step"],
                 c["max_steps"], info=info)
    assert [list(zip(d["src"], d["w"])) for d in info] == c["want"]
    dev_s = _dev_state(cuda, c["state"], F32)
    got = _launch(ops, dev_s, c["score"].float().to(cuda), c["cand"].to(cuda), C, b, W, c["first"],
                  c["greedy"], c["step"], c["max_steps"].to(cuda), hid.to(cuda))
    _compare(got, ref, hid[ref["sel_c"].long()], 0.0, name)
