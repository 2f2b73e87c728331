"""The tagging head's kernels (csrc/tagging.hip: zs_tag_prep, zs_tag_conv) and the row top-k
(zs_sim_topk_finalize driven over the clip rows) one by one against tests/tagging_ref.py, each
entry point called directly, at the smallest shapes that reach every branch: B in {1, 3} (one and
several workgroup rows), C in {32, 768} (one k-step per tap / the real width), N in {1, 16, 17,
527} (less than a tile, one tile, a ragged second tile, the real 4 x 128 + 15), ldf equal to N
and padded.

Every output is filled with a sentinel and has a guard row behind it (gpu_helpers.Out); the
padding columns of frame / clip must come back as the sentinel, and the tokens are followed by a
NaN row that must not be read.  f32 results and ``fine`` (both modes) are held to
encoder_ref.tolerance (4 x the float32 yardstick + 1e-6), xn in bf16 mode to the same rule plus
one bf16 step, bf16 logits / frame / clip to encoder_ref.tolerance_bf16 (2 x the deviation of the
twin that rounds xn and W where the kernel does).  tests/test_tagging_ref.py shows on the CPU
that these inputs tell each listed arithmetic error from the reference."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tagging_ref as T  # noqa: E402
from gpu_helpers import Out, offset  # noqa: E402
from test_gpu_encoder_kernels import Worst, _check, _check_bf16, _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
I32 = torch.int32
F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
SENT = -7.0
NAN = float("nan")


def _call(name, *args):
    from zsaac._lib import call
    return call(name, *args, torch.cuda.current_stream().cuda_stream)


def _code(dt):
    from zsaac._lib import ZS_BF16, ZS_F32
    return ZS_BF16 if dt == BF16 else ZS_F32


def _nm(dt):
    return "bf16" if dt == BF16 else "f32"


def _tokens(dev, x):
    """x [B][64][C] on the device with one NaN row behind it."""
    B, _, C = x.shape
    buf = torch.full((B * 64 + 1, C), NAN, device=dev)
    buf[:B * 64] = x.reshape(B * 64, C).to(dev)
    return buf


def _prep(dev, c, dt):
    """zs_tag_prep on a case -> (xn Out, fine Out, kept-alive inputs)."""
    B, _, C = c["x"].shape
    x = _tokens(dev, c["x"])
    lnw, lnb = c["lnw"].to(dev), c["lnb"].to(dev)
    xn = Out(dev, (B * 64, C), dt, SENT)
    fine = Out(dev, (B * 32, C), F32, SENT)
    _call("zs_tag_prep", x.data_ptr(), B, C, lnw.data_ptr(), lnb.data_ptr(), xn.t.data_ptr(),
          _code(dt), fine.t.data_ptr())
    torch.cuda.synchronize()
    return xn, fine


def _conv(dev, xn, c, dt, ldf, B=None, clip0=0, want_logits=True):
    """zs_tag_conv on xn (a device tensor [>= B * 64][C]) -> (frame, clip, logits) Outs."""
    from zsaac.encoder import pack_tscam
    C, N = c["W"].shape[1], c["W"].shape[0]
    B = B if B is not None else c["x"].shape[0]
    wp = pack_tscam(c["W"].to(dt)).to(dev)
    bias = c["bias"].to(dev)
    frame = Out(dev, (B * 32, ldf), F32, SENT)
    logits = Out(dev, (B * 32, ldf), F32, SENT)
    clip = Out(dev, (B, ldf), F32, SENT)
    src = xn[clip0 * 64:]
    _call("zs_tag_conv", src.data_ptr(), B, C, _code(dt), wp.data_ptr(), N, bias.data_ptr(),
          frame.t.data_ptr(), ldf, clip.t.data_ptr(), ldf,
          logits.t.data_ptr() if want_logits else None)
    torch.cuda.synchronize()
    return frame, clip, logits


def _pad_untouched(t, N):
    return bool((t[..., N:] == SENT).all())


@pytest.mark.parametrize("dt", DTS, ids=_nm)
def test_tag_prep(cuda, dt):
    worst = Worst(f"zs_tag_prep {_nm(dt)}")
    for B in T.CASE_B:
        for C in T.CASE_C:
            r64, r32, twin = T.case_refs(B, C, T.CASE_N[0])
            xn, fine = _prep(cuda, T.case(B, C, T.CASE_N[0]), dt)
            name = f"B {B} C {C}"
            got = xn.cpu().float().view(B, 64, C)
            ref32 = r32["xn"] if dt == F32 else twin["xn"]
            _check(name + " xn", got, r64["xn"], ref32, bf16=dt == BF16, worst=worst)
            _check(name + " fine", fine.cpu().view(B, 32, C), r64["fine"], r32["fine"], worst=worst)
    worst.show()


@pytest.mark.parametrize("padded", [False, True], ids=["ldf=N", "ldf>N"])
@pytest.mark.parametrize("dt", DTS, ids=_nm)
def test_tag_conv(cuda, dt, padded):
    """The conv on the reference's own xn (rounded to bf16 in bf16 mode: the operand zs_tag_prep
    would hand over, so the two kernels are judged separately)."""
    worst = Worst(f"zs_tag_conv {_nm(dt)}")
    for B, C, N in T.CASES:
        c = T.case(B, C, N)
        r64, r32, twin = T.case_refs(B, C, N)
        ldf = T.ldf_of(N, padded)
        src = (r32["xn"] if dt == F32 else twin["xn"]).reshape(B * 64, C).to(dt)
        xn = torch.full((B * 64 + 1, C), NAN, dtype=dt, device=cuda)
        xn[:B * 64] = src.to(cuda)
        frame, clip, logits = _conv(cuda, xn, c, dt, ldf)
        name = f"B {B} C {C} N {N} ldf {ldf}"
        for key, out, shape in (("z", logits, (B, 32, ldf)), ("frame", frame, (B, 32, ldf)),
                                ("clip", clip, (B, ldf))):
            got = out.cpu().view(*shape)
            assert _pad_untouched(got, N), f"{name}: {key} wrote past column N"
            if dt == F32:
                _check(f"{name} {key}", got[..., :N], r64[key], r32[key], worst=worst)
            else:
                _check_bf16(f"{name} {key}", got[..., :N], r64[key], twin[key], worst=worst)
    worst.show()


@pytest.mark.parametrize("dt", DTS, ids=_nm)
def test_prep_then_conv_chain(cuda, dt):
    """The two kernels chained as the engine chains them, at the real shape."""
    B, C, N = 3, 768, 527
    c = T.case(B, C, N)
    r64, r32, twin = T.case_refs(B, C, N)
    xn, _ = _prep(cuda, c, dt)
    frame, clip, _ = _conv(cuda, xn.t, c, dt, N, want_logits=False)
    for key, out, shape in (("frame", frame, (B, 32, N)), ("clip", clip, (B, N))):
        if dt == F32:
            _check(f"chain {key}", out.cpu().view(*shape), r64[key], r32[key])
        else:
            _check_bf16(f"chain {key}", out.cpu().view(*shape), r64[key], twin[key])


@pytest.mark.parametrize("dt", DTS, ids=_nm)
def test_clip_alone_equals_clip_in_batch_and_reruns_are_bit_equal(cuda, dt):
    B, C, N = 3, 768, 527
    c = T.case(B, C, N)
    xn, fine = _prep(cuda, c, dt)
    full = [o.cpu() for o in _conv(cuda, xn.t, c, dt, N)]
    again = [o.cpu() for o in _conv(cuda, xn.t, c, dt, N)]
    for a, b in zip(full, again):
        assert _same_bits(a, b), "two runs of one launch differ"
    alone = [o.cpu() for o in _conv(cuda, xn.t, c, dt, N, B=1, clip0=1)]
    assert _same_bits(alone[0], full[0][32:64]) and _same_bits(alone[2], full[2][32:64])
    assert _same_bits(alone[1], full[1][1:2])
    # the prep kernel, too: clip 1 alone
    c1 = dict(c, x=c["x"][1:2])
    xn1, fine1 = _prep(cuda, c1, dt)
    assert _same_bits(xn1.cpu(), xn.cpu()[64:128]) and _same_bits(fine1.cpu(), fine.cpu()[32:64])


@pytest.mark.parametrize("dt", DTS, ids=_nm)
def test_duplicate_rows_tie_and_topk_order(cuda, dt):
    """Rows 3 / 140 (different workgroups) and 20 / 21 of the weight are equal: their columns are
    bit-equal, and the row top-k (zs_sim_topk_finalize over the padded clip rows, as
    AudioEncoder.tag_topk drives it) lists equals lower index first, as tagging_ref.topk does."""
    c = T.dup_case()
    B, C, N = 2, 32, 150
    ldc = (N + 7) // 8 * 8
    xn, _ = _prep(cuda, c, dt)
    frame, clip, logits = _conv(cuda, xn.t, c, dt, ldc)
    f, cl, z = frame.cpu().view(B, 32, ldc), clip.cpu(), logits.cpu().view(B, 32, ldc)
    for a, b in ((3, 140), (20, 21)):
        assert _same_bits(z[..., a], z[..., b]) and _same_bits(f[..., a], f[..., b])
        assert _same_bits(cl[:, a], cl[:, b])
    # the tied classes become the row's best; padding as the engine keeps it
    v = clip.t.clone()
    v[:, N:] = float("-inf")
    v[:, [3, 140]] = 2.0
    v[:, [20, 21]] = 1.5
    idx = torch.full((B, ldc), 0x7fffffff, dtype=I32, device=cuda)
    idx[:, :N] = torch.arange(N, dtype=I32, device=cuda)
    for k in (1, 5, 8):
        ov = Out(cuda, (B, k), F32, SENT)
        oi = Out(cuda, (B, k), I32, -3)
        _call("zs_sim_topk_finalize", v.data_ptr(), idx.data_ptr(), B, ldc // 8, 8, k,
              ov.t.data_ptr(), oi.t.data_ptr())
        torch.cuda.synchronize()
        rv, ri = T.topk(v.cpu()[:, :N], k)
        assert torch.equal(oi.cpu().long(), ri) and torch.equal(ov.cpu(), rv), k
        assert oi.cpu()[:, :min(k, 4)].tolist() == [[3, 140, 20, 21][:k]] * B


def test_refusals_leave_outputs_untouched(cuda):
    """C % 32 != 0, C > 2048, N <= 0, B <= 0, ldf / ldc < N, a bad dtype, NULL pointers and
    misaligned operands are refused with ZS_ERR_ARG before any launch."""
    from zsaac._lib import ZsError
    buf = torch.zeros(1 << 16, device=cuda)
    out = torch.full((1 << 16,), SENT, device=cuda)
    p, o = buf.data_ptr(), out.data_ptr()
    o2 = o + (1 << 15)
    bad = [("zs_tag_prep", p, 1, 48, p, p, o, 0, o2), ("zs_tag_prep", p, 1, 2080, p, p, o, 0, o2),
           ("zs_tag_prep", p, 0, 32, p, p, o, 0, o2), ("zs_tag_prep", p, 1, 32, p, p, o, 2, o2),
           ("zs_tag_prep", None, 1, 32, p, p, o, 0, o2), ("zs_tag_prep", p, 1, 32, None, p, o, 0, o2),
           ("zs_tag_prep", p, 1, 32, p, p, None, 0, o2), ("zs_tag_prep", p, 1, 32, p, p, o, 0, None),
           ("zs_tag_conv", p, 1, 48, 0, p, 16, p, o, 16, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 0, p, 0, p, o, 16, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 0, p, -5, p, o, 16, o2, 16, None),
           ("zs_tag_conv", p, 0, 32, 0, p, 16, p, o, 16, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 0, p, 16, p, o, 15, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 0, p, 16, p, o, 16, o2, 15, None),
           ("zs_tag_conv", p, 1, 32, 7, p, 16, p, o, 16, o2, 16, None),
           ("zs_tag_conv", None, 1, 32, 0, p, 16, p, o, 16, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 0, None, 16, p, o, 16, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 0, p, 16, None, o, 16, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 0, p, 16, p, None, 16, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 0, p, 16, p, o, 16, None, 16, None),
           ("zs_tag_conv", p + 4, 1, 32, 0, p, 16, p, o, 16, o2, 16, None),
           ("zs_tag_conv", p, 1, 32, 1, p + 8, 16, p, o, 16, o2, 16, None)]
    for args in bad:
        with pytest.raises(ZsError):
            _call(*args)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert offset(torch.zeros(4), cuda).data_ptr() % 16 == 4      # what "misaligned" means here
