"""tests/encoder_ref.py on the CPU: (1) every reference equals its oracle in float64, (2) the
input conditions of the GPU cases in tests/test_gpu_encoder_kernels.py hold, (3) the inputs of
those cases tell each listed arithmetic error from the reference: the error is applied to the
float64 reference (never to a kernel) and must move a named GPU case's expected output by more
than twice that case's tolerance.

Three of the listed errors cannot be seen in any output, by construction; the tests below assert
exactly that and say why (test_unobservable_errors)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ref as R  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _sd64(sd):
    return {k: v.double() for k, v in sd.items()}


def _block_sd(C, heads, seed):
    from test_gpu_swin import _block_sd as mk
    return mk(C, heads, seed, None)


def _moved(ref, mutated, tol):
    """Does the mutated reference leave the tolerance band twice over somewhere (NaN counts)?"""
    d = (mutated - ref).abs()
    return bool(((d > 2 * tol) | torch.isnan(d)).any())


# ====================================================================== (1) ties to the oracle
@pytest.mark.parametrize("H,W,shift", [(16, 16, 0), (16, 16, 4), (16, 24, 4), (24, 16, 4),
                                       (8, 16, 0), (16, 8, 0), (8, 8, 0)])
def test_swin_block_and_window_attention_equal_oracle(H, W, shift):
    """R.swin_block (and with it R.window_attention: roll, regions, mask, bias table on token
    indices) == oracle.audio.swin_block in float64, square and non-square maps."""
    from oracle import audio as A
    C, heads, B = 96, 4, 2
    sd = _sd64(_block_sd(C, heads, 3))
    x = torch.randn(B, H * W, C, generator=R.gen(1), dtype=F64)
    ref = A.swin_block(x, sd, "blk.", H, W, heads, shift).reshape(-1, C)
    got = R.swin_block(x.reshape(-1, C), sd, B, H, W, C, heads, shift)
    assert float((got - ref).abs().max()) < 1e-12


def test_patch_merge_equals_oracle():
    from oracle import audio as A
    for (C, B, H, W) in R.PM_CASES:
        c = R.pm_case(C, B, H, W)
        sd = {"m.norm.weight": c["w"].double(), "m.norm.bias": c["b"].double(),
              "m.reduction.weight": torch.eye(4 * C, dtype=F64)}
        ref = A.patch_merging(c["x"].double().view(B, H * W, C), sd, "m.", H, W)
        got = R.patch_merge_ln(c["x"], c["w"], c["b"])
        assert float((got - ref.reshape(-1, 4 * C)).abs().max()) < 1e-12, (C, B, H, W)


@pytest.mark.parametrize("T_in", [3, 1001, 1023])
def test_wav2img_equals_oracle(T_in):
    """R.wav2img == oracle.audio.reshape_wav2img (torch's bicubic, align_corners) in float64, and
    its float32 twin == the float32 oracle up to the summation order of the four taps; T_in 2 and
    1024 are in test_wav2img_edges."""
    from oracle import audio as A
    x = R.w2i_case(3, T_in)
    ref = A.reshape_wav2img(x.double()[:, None])[:, 0]
    got = R.wav2img(x)
    assert float((got - ref).abs().max()) < 1e-9
    got32 = R.wav2img(x, dtype=F32)
    ref32 = A.reshape_wav2img(x[:, None])[:, 0]
    assert float((got32 - ref32).abs().max()) < 1e-4


def test_wav2img_edges():
    x = R.w2i_case(1, 1024)
    assert torch.equal(R.wav2img(x, dtype=F32), x.view(1, 4, 256, 64).permute(0, 1, 3, 2).reshape(1, 256, 256))
    from oracle import audio as A
    x = R.w2i_case(1, 2)
    ref = A.reshape_wav2img(x.double()[:, None])[:, 0]
    assert float((R.wav2img(x) - ref).abs().max()) < 1e-9


def test_logmel_equals_oracle():
    """Float64 rfft formulation == oracle.frontend.logmel (float32 conv-DFT) to float32 accuracy,
    and == the oracle's own float64 numpy formulation."""
    from oracle import frontend as OF
    wav = R.logmel_wav(5, 1920, 2)
    tb = R.tables()
    got = R.logmel(wav, tb["window"], tb["melW"])
    ref = torch.from_numpy(OF.logmel_numpy_fft(wav.numpy()))[:, 0].reshape(-1, 64)
    assert float((got - ref).abs().max()) < 1e-5      # the window table is float32 in ``got``
    assert float((got - OF.logmel(wav)[:, 0].reshape(-1, 64).double()).abs().max()) < 2e-3


def test_cnn_ops_equal_torch():
    for (cin, cout) in [(1, 64), (32, 96)]:
        c = R.conv_case(cin, cout, 2, 21, 16, F32)
        w4 = c["w"][:, :9 * cin].double().view(cout, 3, 3, cin).permute(0, 3, 1, 2)
        ref = F.conv2d(c["x"].double().permute(0, 3, 1, 2), w4, padding=1)
        ref = torch.relu(ref * c["scale"].double()[:, None, None] + c["shift"].double()[:, None, None])
        got = R.conv3x3_bn_relu(c["x"], c["w"], c["scale"], c["shift"])
        assert float((got.permute(0, 3, 1, 2) - ref).abs().max()) < 1e-12
    for (H, W) in R.POOL_SHAPES:
        x = R.pool_case(H, W, 64, F32)
        ref = F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert float((R.avgpool2(x) - ref).abs().max()) < 1e-14
    x = R.head_case(3, 7, 3, 300, F32).double()
    m = x.permute(0, 3, 1, 2).mean(3)                     # cnns.py: mean over mel, [B, C, time]
    assert float((R.cnn_head(x) - (m.max(2).values + m.mean(2))).abs().max()) < 1e-14


def test_norm_ops_equal_torch():
    c = R.ln_case(768, 5, 772, "rows")
    ref = F.layer_norm(c["x"].view(-1, 772)[c["rows"].long(), :768].double(), (768,),
                       c["w"].double(), c["b"].double(), R.LN_EPS)
    assert float((R.layernorm(c["x"], 5, 768, 772, c["rows"], c["w"], c["b"], R.LN_EPS) - ref).abs().max()) < 1e-12
    c = R.mp_case(3, 17, 260)
    ref = F.layer_norm(c["x"].double(), (260,), c["w"].double(), c["b"].double(), 1e-5).mean(1)
    assert float((R.ln_meanpool(c["x"], c["w"], c["b"]) - ref).abs().max()) < 1e-12
    c = R.patch_embed_case(1)
    ref = F.conv2d(c["img"].double()[:, None], c["w"].double().view(96, 1, 4, 4), c["b"].double(), stride=4)
    ref = F.layer_norm(ref.flatten(2).transpose(1, 2), (96,), c["lnw"].double(), c["lnb"].double(), 1e-5)
    assert float((R.patch_embed(c["img"], c["w"], c["b"], c["lnw"], c["lnb"]) - ref.reshape(-1, 96)).abs().max()) < 1e-11
    x = torch.randn(4, 33, generator=R.gen(0))
    assert float((R.l2norm(x, 1e-12) - F.normalize(x.double(), dim=-1)).abs().max()) < 1e-15


# ====================================================================== (2) input conditions
@pytest.mark.parametrize("B,T,silent", R.LOGMEL_CASES)
def test_logmel_inputs(B, T, silent):
    """Every mel power is at least 1e-6 of its frame's largest bin power, or the frame is exactly
    silent: float32 FFT cancellation never decides a value.  Clips differ, the frame counts are
    the ones the GPU cases rely on."""
    tb = R.tables()
    wav = R.logmel_wav(B, T, silent)
    mel, pw = R.mel_power(wav, tb["window"], tb["melW"])
    nf = T // R.HOP + 1
    quiet = pw.max(-1).values == 0
    ok = (mel >= 1e-6 * pw.max(-1, keepdim=True).values) | quiet[:, None]
    assert bool(ok.all()), float((mel / pw.max(-1, keepdim=True).values)[~quiet].min())
    if silent is not None:
        assert bool(quiet.view(B, nf)[silent].all()) and int(quiet.sum()) == nf
        ref = R.logmel_refs(B, T, silent, False)[0].view(B, nf, 64)
        assert bool((ref[silent] == -100.0).all())
    else:
        assert not bool(quiet.any())
    if B > 1:
        live = [b for b in range(B) if b != silent][:50]
        assert len({float(wav[b].abs().sum()) for b in live}) == len(live)


def test_logmel_frame_counts():
    nf = R.LOGMEL_T // R.HOP + 1
    assert nf == 7
    base = [f * R.HOP - 512 for f in range(nf)]
    assert [b >= 0 and b + 1024 <= R.LOGMEL_T for b in base] == [False, False, True, True, True, False, False]
    assert 900 * nf > R.LOGMEL_WAVE_STRIDE and 900 * nf <= R.LOGMEL_BLOCK_STRIDE
    assert 1180 * nf > R.LOGMEL_BLOCK_STRIDE
    assert (1 * nf) % 2 == 1 and 513 // R.HOP + 1 == 2


def test_window_attention_inputs():
    """Softmax rows have spread; in every shifted case on a map of at least 16 x 16 all nine region
    labels occur; at least one window mixes masked and unmasked keys; the bias decides rows."""
    for dt in (F32, BF16):
        for (B, H, W, heads, hd, shift) in R.wa_cases((24, 32)):
            c = R.wa_case(B, H, W, heads, hd, shift, dt)
            s, reg = R.softmax_stats(c["qkv"], B, H, W, c["C"], heads, shift, c["table"])
            live = s > -50           # a 1 x 1 corner region (shift 1, 7) leaves one live key
            spread = s.amax(-1) - torch.where(live, s, s.max()).amin(-1)
            assert float(spread[live.sum(-1) >= 8].min()) > 2.0
            if shift > 0:
                if H >= 16 and W >= 16:
                    assert sorted(reg.unique().tolist()) == list(range(9))
                mixed = (reg != reg[:, :1]).any(-1)
                assert bool(mixed.any())
                assert len(reg.unique()) >= 4
    c = R.wa_case(2, 8, 16, 2, 24, 0, F32)
    s, _ = R.softmax_stats(c["qkv"], 2, 8, 16, c["C"], 2, 0, c["table"])
    s0, _ = R.softmax_stats(c["qkv"], 2, 8, 16, c["C"], 2, 0, torch.zeros_like(c["table"]))
    assert float((s.argmax(-1) != s0.argmax(-1)).float().mean()) > 0.1


def test_layernorm_inputs():
    assert len(set(R.LN_ROWS)) < len(R.LN_ROWS) and max(R.LN_ROWS) == 6
    c = R.ln_case(768, 8, 768, "special")
    x = c["x"].view(8, 768)
    assert abs(float(x[1].mean()) - 1e3) < 1 and 0.8 < float(x[1].std()) < 1.2
    assert float(x[2].std()) == 0.0
    y = R.layernorm(c["x"], 8, 768, 768, None, c["w"], c["b"], R.LN_EPS)
    assert torch.equal(y[2], c["b"].double())
    for (name, C, M, ldx, ldy, kind) in R.ln_cases():
        c = R.ln_case(C, M, ldx, kind)
        assert bool(torch.isnan(c["x"].view(-1, ldx)[:, C:]).all())
    nv = {-(-(C // 4) // 64) for C in R.LN_C if C % 4 == 0 and C <= 1024}
    assert nv == {1, 2, 3, 4}


def test_other_inputs():
    """Dispatch branches reached: patch-merge VPL 6 / 12 / 24 and the block kernel, meanpool CPL
    4 / 12 / 32, conv tiles; the head's means are negative; ReLU clips; cast ties are ties."""
    vpl = {(6 if 4 * C <= 384 else 12 if 4 * C <= 768 else 24 if 4 * C <= 1536 else 0)
           for (C, _, _, _) in R.PM_CASES}
    assert vpl == {0, 6, 12, 24}
    assert any((B * H * W // 4) % 4 for (_, B, H, W) in R.PM_CASES)
    assert {4 if C <= 256 else 12 if C <= 768 else 32 for C in R.MP_C} == {4, 12, 32}
    assert R.mp_max_c(160 * 1024) == 2048 and R.mp_max_c(64 * 1024) == 1024
    x = R.head_case(3, 31, 2, 2048, F32)
    assert float((x.double().mean(2).max(1).values < 0).float().mean()) > 0.5
    c = R.conv_case(64, 128, 2, 21, 16, F32)
    y = R.conv3x3_bn_relu(c["x"], c["w"], c["scale"], c["shift"])
    assert 0.2 < float((y == 0).float().mean()) < 0.8
    assert 3 * 5 * 9 > 128 and any(co % 64 for (_, co) in R.CONV_CH)
    x = R.cast_case(257)
    assert x[:4].view(torch.int32).bitwise_and(0xFFFF).tolist() == [0x8000] * 4
    assert R.cast(x[:2], BF16).view(torch.int16).tolist() == [0x3F80, 0x3F82]   # ties to even


# ====================================================================== (3) the cases catch errors
def _wa_tol(c, B, H, W, heads, shift, dt):
    a = (c["qkv"], B, H, W, c["C"], heads, shift, c["table"])
    r64 = R.window_attention(*a)
    if dt == F32:
        return r64, R.tolerance(r64, R.window_attention(*a, dtype=F32))[1]
    tw = R.window_attention(*a, dtype=F32, p_round=BF16, out_round=BF16)
    return r64, torch.full_like(r64, R.tolerance_bf16(r64, tw)[1])


@pytest.mark.parametrize("mut,case", [
    ("wa_hw_swap", (2, 8, 16, 2, 24, 4)), ("wa_hw_swap", (2, 16, 8, 2, 32, 0)),
    ("wa_roll_sign", (2, 8, 16, 2, 24, 1)), ("wa_roll_sign", (1, 16, 24, 2, 32, 7)),
    ("wa_relpos_T", (2, 8, 8, 2, 24, 0)), ("wa_mask_shift0", (2, 8, 8, 2, 24, 0)),
    ("wa_mask_shift0", (1, 16, 24, 2, 32, 0))])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_window_attention_errors_caught(mut, case, dt):
    """Caught by test_gpu_encoder_kernels.py::test_window_attention (f32, bf16 MFMA and VALU) at
    the named case; the same index errors in the fused block by ::test_swin_block."""
    assert case in R.wa_cases((24, 32))
    B, H, W, heads, hd, shift = case
    c = R.wa_case(*case, dt)
    r64, tol = _wa_tol(c, B, H, W, heads, shift, dt)
    bad = R.window_attention(c["qkv"], B, H, W, c["C"], heads, shift, c["table"], mut=mut)
    assert _moved(r64, bad, tol)


@pytest.mark.parametrize("mut,case", [("wa_hw_swap", (96, 3, 8, 16, 4)), ("wa_roll_sign", (96, 1, 16, 8, 4)),
                                      ("wa_relpos_T", (192, 1, 16, 8, 0)), ("wa_mask_shift0", (384, 3, 16, 8, 0))])
def test_swin_block_errors_caught(mut, case):
    """Caught by test_gpu_encoder_kernels.py::test_swin_block at the named case."""
    assert case in R.SWIN_CASES
    C, B, H, W, shift = case
    sd = _block_sd(C, C // 24, C + shift)
    x = R.swin_x(C, B, H, W)
    r64 = R.swin_block(x, sd, B, H, W, C, C // 24, shift)
    tw = R.swin_block(x, sd, B, H, W, C, C // 24, shift, dtype=F32, rnd=BF16)
    tol = R.tolerance_bf16(r64, tw)[1]
    bad = R.swin_block(x, sd, B, H, W, C, C // 24, shift, mut=mut)
    assert _moved(r64, bad, torch.full_like(r64, tol))


def test_unobservable_errors():
    """Three listed errors change no output, whatever the inputs:
    * region thresholds H - ws and H - shift swapped: rows are labelled 0 / 2 instead of 1 / 2
      inside the last window row (0 everywhere else, as before).  The mask only compares labels
      inside one window, and a window never spans the H - ws boundary, so every window sees the
      same partition: the mask, and the output, are identical.
    * the mask applied at shift 0 with shift 0's own labels: every slot of the last window row is
      then labelled 1 (no row reaches H - 0), again one label per window, no mask.  (The mask of
      the shifted block applied to an unshifted one is what wa_mask_shift0 models, and is caught.)
    * the second frame of the last odd pair not zero: the two real spectra are separated exactly
      (A_k = (Z_k + conj Z_{N-k}) / 2), so frame a's power does not depend on what is packed
      beside it, and the missing frame is never stored; a store of it is caught by the guard row.
    """
    for case in [(2, 8, 16, 2, 24, 4), (1, 16, 24, 2, 32, 1), (1, 16, 24, 2, 24, 7)]:
        B, H, W, heads, hd, shift = case
        _, reg = R.window_tokens(B, H, W, shift)
        _, bad = R.window_tokens(B, H, W, shift, mut="wa_thresh_swap")
        same = lambda r: r[:, :, None] == r[:, None, :]
        assert not torch.equal(reg, bad) and torch.equal(same(reg), same(bad))
        _, reg0 = R.window_tokens(B, H, W, 0)
        assert bool(same(reg0).all())
    # packing any second frame beside the last one leaves its separated power unchanged
    import numpy as np
    g = R.gen(5)
    a, b = torch.randn(1024, generator=g, dtype=F64).numpy(), torch.randn(1024, generator=g, dtype=F64).numpy()
    z = np.fft.fft(a + 1j * b)
    zc = np.conj(np.roll(z[::-1], 1))
    pa = np.abs((z + zc) / 2)[:513] ** 2
    assert np.allclose(pa, np.abs(np.fft.rfft(a)) ** 2, rtol=1e-9, atol=1e-9)


def test_patch_merge_error_caught():
    """parts 1 and 2 swapped: caught by ::test_patch_merge_ln at every case with H, W >= 2."""
    for dt in (F32, BF16):
        C, B, H, W = R.PM_CASES[1]
        c = R.pm_case(C, B, H, W)
        r64 = R.patch_merge_ln(c["x"], c["w"], c["b"])
        r32 = R.patch_merge_ln(c["x"], c["w"], c["b"], dtype=F32, round_to=None if dt == F32 else dt)
        tol = R.tolerance(r64, r32, dt == BF16)[1]
        assert _moved(r64, R.patch_merge_ln(c["x"], c["w"], c["b"], mut="pm_part_swap"), tol)


@pytest.mark.parametrize("mut,case,stride", [
    ("lm_edge_repeat", (1, 1920, None), 0), ("lm_edge_repeat", (3, 513, None), 0),
    ("lm_pair_swap", (5, 1920, 2), 0),
    ("lm_stale_power", (900, 1920, 450), R.LOGMEL_WAVE_STRIDE),
    ("lm_stale_power", (1180, 1920, 7), R.LOGMEL_BLOCK_STRIDE)])
def test_logmel_errors_caught(mut, case, stride):
    """Caught by ::test_logmel at the named case (lm_stale_power: B = 900 for the wave kernel,
    whose second iteration starts at frame 6144; B = 1180 for the block kernel, at frame 8192)."""
    assert case in R.LOGMEL_CASES
    tb = R.tables()
    r64, r32 = R.logmel_refs(*case, False)
    tol = R.tolerance(r64, r32)[1]
    bad = R.logmel(R.logmel_wav(*case), tb["window"], tb["melW"], mut=mut, stride=stride)
    assert _moved(r64, bad, tol)


def test_layernorm_errors_caught():
    """mean over ldx: ::test_layernorm[pad4-*] (the NaN tail reaches the output); rows[row]
    against row: ::test_layernorm[rows-C768]."""
    for (mut, name) in [("ln_mean_ldx", "pad4-C768"), ("ln_rows_ident", "rows-C768")]:
        (_, C, M, ldx, ldy, kind), = [c for c in R.ln_cases() if c[0] == name]
        c = R.ln_case(C, M, ldx, kind)
        a = (c["x"], M, C, ldx, c["rows"], c["w"], c["b"], R.LN_EPS)
        r64 = R.layernorm(*a)
        tol = R.tolerance(r64, R.layernorm(*a, dtype=F32, round_to=BF16), True)[1]
        assert _moved(r64, R.layernorm(*a, mut=mut), tol)


def test_meanpool_head_pool_conv_wav2img_errors_caught():
    """mp_div16: ::test_ln_meanpool at N = 1, 15, 17; head_axes: ::test_cnn_head (31, 2, 2048);
    conv_tap_T and conv_no_border: ::test_conv3x3 (2, 21, 16) and (3, 5, 9); pool_odd_col:
    ::test_avgpool2 (16, 21) and (5, 7); w2i_no_clamp: ::test_wav2img at T_in 2 and 3 (at 1001
    the out-of-range taps carry weights below 3e-4 and the float32 source index costs more)."""
    for N in (1, 15, 17):
        c = R.mp_case(3, N, 768)
        r64 = R.ln_meanpool(c["x"], c["w"], c["b"])
        tol = R.tolerance(r64, R.ln_meanpool(c["x"], c["w"], c["b"], dtype=F32))[1]
        assert _moved(r64, R.ln_meanpool(c["x"], c["w"], c["b"], mut="mp_div16"), tol)
    for dt in (F32, BF16):
        rt = None if dt == F32 else dt
        x = R.head_case(3, 31, 2, 2048, dt)
        r64 = R.cnn_head(x)
        tol = R.tolerance(r64, R.cnn_head(x, dtype=F32))[1]
        x7 = R.head_case(3, 7, 3, 300, dt)           # wrong axes need H != W to show in the shape-free sum
        assert _moved(R.cnn_head(x7), R.cnn_head(x7, mut="head_axes"),
                      R.tolerance(R.cnn_head(x7), R.cnn_head(x7, dtype=F32))[1])
        assert _moved(r64, R.cnn_head(x, mut="head_axes"), tol)
        for shape in [(2, 21, 16), (3, 5, 9)]:
            c = R.conv_case(64, 128, *shape, dt)
            a = (c["x"], c["w"], c["scale"], c["shift"])
            r64 = R.conv3x3_bn_relu(*a)
            tol = R.tolerance(r64, R.conv3x3_bn_relu(*a, dtype=F32, round_to=rt), dt == BF16)[1]
            for mut in ("conv_tap_T", "conv_no_border"):
                assert _moved(r64, R.conv3x3_bn_relu(*a, mut=mut), tol), (mut, shape)
        for (H, W) in [(16, 21), (5, 7)]:
            x = R.pool_case(H, W, 64, dt)
            r64 = R.avgpool2(x)
            tol = R.tolerance(r64, R.avgpool2(x, dtype=F32, round_to=rt), dt == BF16)[1]
            assert _moved(r64, R.avgpool2(x, mut="pool_odd_col"), tol)
    for T_in in (2, 3):
        x = R.w2i_case(3, T_in)
        r64 = R.wav2img(x)
        tol = R.tolerance(r64, R.wav2img(x, dtype=F32))[1]
        assert _moved(r64, R.wav2img(x, mut="w2i_no_clamp"), tol)


def test_every_listed_error_is_exercised():
    """Each name of encoder_ref.MUTANTS is applied by a test of this file."""
    text = open(os.path.abspath(__file__)).read()
    for m in R.MUTANTS:
        assert f'"{m}"' in text, m
