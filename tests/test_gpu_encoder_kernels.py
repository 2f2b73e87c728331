"""The audio encoder's non-GEMM kernels (csrc/frontend.hip, norm.hip, cnn.hip, window_attention of
attn.hip, swin.hip) one by one against tests/encoder_ref.py, each entry point called directly, at
the smallest shapes at which every dispatch branch can still go wrong.

Every output is filled with a sentinel and allocated with a guard row behind it; the guard must
come back unchanged.  Padding that must not be read (ldx tails, gaps between clips) holds NaN,
padding that must not be written (ldy tails) the sentinel; both are compared bit for bit.
Copies and casts are compared with torch.equal.  Float outputs are compared with the float64
reference under the rule of mistral_ref.tolerance: the yardstick is the same formula in float32
on the CPU (rounded to bf16 where the kernel stores bf16), measured as its largest deviation from
float64 on the case's own data; the tolerance is 4 x yardstick + 1e-6, plus one bf16 step of the
reference (2^-8 |ref|, elementwise) for a bf16 output.  The two bf16 kernels with internal
rounding points (window attention in bf16, the fused Swin block) are held, in the max norm, to
2 x the largest deviation of a float32 twin that rounds where the kernel rounds
(encoder_ref.tolerance_bf16).  The input conditions of the cases are asserted on the CPU in
tests/test_encoder_ref.py, which also shows that these inputs tell each of the listed arithmetic
errors from the reference."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ref as R  # noqa: E402
from gpu_helpers import Out, offset  # noqa: E402

pytestmark = pytest.mark.gpu
I32, I64 = torch.int32, torch.int64
F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
SENT = -7.0


def _call(name, *args):
    from zsaac._lib import call
    return call(name, *args, torch.cuda.current_stream().cuda_stream)


def _code(dt):
    from zsaac._lib import ZS_BF16, ZS_F32
    return ZS_BF16 if dt == BF16 else ZS_F32


def _rt(dt):
    return None if dt == F32 else dt


def _nm(dt):
    return "bf16" if dt == BF16 else "f32"


def _ptr(t):
    return t.data_ptr() if t is not None else None


class Worst:
    """The case closest to its bound, printed once per test."""

    def __init__(self, what):
        self.what, self.r, self.line = what, -1.0, ""

    def add(self, r, line):
        if r > self.r:
            self.r, self.line = r, line

    def show(self):
        print(f"{self.what}: closest to its bound: {self.line}")


def _check(name, got, ref64, ref32, bf16=False, worst=None):
    """|got - float64 reference| <= tolerance (mistral_ref.tolerance) elementwise."""
    yard, tol = R.tolerance(ref64, ref32, bf16)
    err = (got.double() - ref64).abs()
    ratio = (err / tol).nan_to_num(nan=float("inf"))
    i = int(ratio.argmax())
    line = (f"{name}: error {float(err.max()):.3e}, yardstick {yard:.3e}, tolerance "
            f"{float(tol.reshape(-1)[i]):.3e} (closest: error {float(err.reshape(-1)[i]):.3e})")
    if worst is not None:
        worst.add(float(ratio.reshape(-1)[i]), line)
    assert bool((err <= tol).all()), line


def _check_bf16(name, got, ref64, twin, worst=None):
    """max |got - float64 reference| <= 2 x max |twin - float64 reference|; prints the ratio of
    the kernel's error to the yardstick."""
    yard, tol = R.tolerance_bf16(ref64, twin)
    err = float((got.double() - ref64).abs().max())
    line = f"{name}: error {err:.3e}, yardstick {yard:.3e}, ratio {err / yard:.2f}"
    print(line)
    if worst is not None:
        worst.add(err / yard, line)
    assert err <= tol and bool(torch.isfinite(got).all()), line


def _dev(dev, *ts):
    """The tensors on the device; the caller keeps them alive until it has synchronised (a
    temporary's memory is handed to the next allocation while a launch may still need it)."""
    return [t.to(dev) for t in ts]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _off_out(dev, shape, dtype, sentinel, k):
    """An Out-like output that starts k elements into its buffer (a guard on both sides)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * k + shape[-1],), sentinel, dtype=dtype, device=dev)

    class V:
        t = buf[k:k + n].view(*shape)

        @staticmethod
        def cpu():
            assert bool((buf[:k] == sentinel).all()) and bool((buf[k + n:] == sentinel).all()), "guard overwritten"
            return V.t.cpu()
    return V


# ------------------------------------------------------------------ host checks
def test_host_checks_refuse(cuda):
    """Arguments outside the contract of include/zsaac.h are refused by the host wrappers with
    ZS_ERR_ARG before any launch, and a zeroed buffer stays zero: T = 512 for zs_logmel; T_in 1 and
    1025, B 0 and NULL buffers for zs_wav2img; B 0 / NULL for zs_patch_embed; odd H for
    zs_patch_merge_ln; Cin 48, B 0, NULL and a B H W past an int for zs_conv3x3_bn_relu; NULL and
    overflow for zs_avgpool2 and zs_cnn_head; NULL, B 0, shift 8 and overflow for
    zs_window_attention; ldx < C and a NULL weight for zs_layernorm; C = 2112 for zs_ln_meanpool.
    Head dim 16 in f32 is ZS_ERR_UNSUPPORTED."""
    from zsaac._lib import ZsError
    buf = torch.zeros(1 << 16, device=cuda)
    ids = torch.zeros(64, dtype=I32, device=cuda)
    p, i = buf.data_ptr(), ids.data_ptr()
    big = 1 << 16
    bad = [("zs_logmel", p, 1, 512, p, p, p, i, i, None, None, None, None, p),
           ("zs_logmel", p, 0, 1920, p, p, p, i, i, None, None, None, None, p),
           ("zs_logmel", None, 1, 1920, p, p, p, i, i, None, None, None, None, p),
           ("zs_wav2img", p, 1, 1, p), ("zs_wav2img", p, 1, 1025, p), ("zs_wav2img", p, 0, 8, p),
           ("zs_wav2img", None, 1, 8, p), ("zs_wav2img", p, 1, 8, None),
           ("zs_patch_embed", p, 0, p, p, p, p, p), ("zs_patch_embed", p, 1, p, p, p, p, None),
           ("zs_patch_merge_ln", p, 1, 3, 2, 4, p, p, p, 0), ("zs_patch_merge_ln", p, 1, 2, 3, 4, p, p, p, 0),
           ("zs_conv3x3_bn_relu", p, 1, 2, 2, 48, p, 64, p, p, p, 0),
           ("zs_conv3x3_bn_relu", p, 0, 2, 2, 32, p, 64, p, p, p, 0),
           ("zs_conv3x3_bn_relu", p, 1, 2, 2, 32, None, 64, p, p, p, 0),
           ("zs_conv3x3_bn_relu", p, big, big, 1, 32, p, 64, p, p, p, 0),
           ("zs_avgpool2", None, 1, 2, 2, 4, p, 0), ("zs_avgpool2", p, big, big, 2, 1, p, 0),
           ("zs_avgpool2", p, 1, 1, 2, 4, p, 0),
           ("zs_cnn_head", p, 1, 2, 2, 4, None, 0), ("zs_cnn_head", p, 1024, big, 32, 1, p, 0),
           ("zs_window_attention", None, 1, 8, 8, 48, 2, 8, 0, p, p, 0),
           ("zs_window_attention", p, 0, 8, 8, 48, 2, 8, 0, p, p, 0),
           ("zs_window_attention", p, 1, 8, 8, 48, 2, 8, 8, p, p, 0),
           ("zs_window_attention", p, 1, 8, 12, 48, 2, 8, 0, p, p, 0),
           ("zs_window_attention", p, big, big, 8, 48, 2, 8, 0, p, p, 0),
           ("zs_layernorm", p, 2, 8, 4, None, p, p, 1e-5, p, 8, 0),
           ("zs_layernorm", p, 2, 8, 8, None, None, p, 1e-5, p, 8, 0),
           ("zs_ln_meanpool", p, 1, 4, 2112, p, p, p), ("zs_ln_meanpool", p, 1, 0, 64, p, p, p)]
    for args in bad:
        with pytest.raises(ZsError, match=r"failed \(-1\)"):     # ZS_ERR_ARG, before any launch
            _call(*args)
    with pytest.raises(ZsError, match=r"failed \(-4\)"):         # ZS_ERR_UNSUPPORTED
        _call("zs_window_attention", p, 1, 8, 8, 32, 2, 8, 0, p, p, 0)
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


# ------------------------------------------------------------------ front end
@pytest.mark.parametrize("wave", [1, 0])
def test_logmel(cuda, wave):
    """Both kernels (logmel_wave 1: one wave per frame pair; 0: one block per 4 frames), with and
    without bn0.  T = 1920: 7 frames per clip, 2-4 interior (the wave kernel's fast path), 0, 1, 5,
    6 reflected.  B = 1: an odd total, the last pair half empty; B = 5 with clip 2 exactly silent
    (-100 dB); B = 900 (6300 frames: the wave kernel's grid-stride loop runs a second time from
    frame 6144, with the prefetch); B = 1180 (8260 frames: the block kernel's loop too, from
    8192); T = 513 (2 frames, reflected at both ends) and 640.  Clips differ, so a frame in the
    wrong slot shows.
    Measured on an MI355X (dB): wave kernel closest to its bound at B 900 with bn0, error
    1.194e-05 at yardstick 4.786e-06 (tolerance 2.014e-05); block kernel 9.159e-06 there."""
    from zsaac._lib import call
    from zsaac.frontend import make_tables
    tb = make_tables(cuda)
    bn = [t.to(cuda) for t in R.logmel_bn()]
    worst = Worst(f"logmel[wave{wave}]")
    call("zs_tune_set", b"logmel_wave", wave)
    try:
        for (B, T, silent) in R.LOGMEL_CASES:
            wav = R.logmel_wav(B, T, silent).to(cuda)
            nf = T // R.HOP + 1
            for with_bn in (False, True):
                out = Out(cuda, (B * nf, 64), F32, SENT)
                b4 = [_ptr(t) for t in bn] if with_bn else [None] * 4
                _call("zs_logmel", wav.data_ptr(), B, T, _ptr(tb["window"]), _ptr(tb["twiddle"]),
                      _ptr(tb["melW"]), _ptr(tb["mel_lo"]), _ptr(tb["mel_hi"]), *b4, out.t.data_ptr())
                torch.cuda.synchronize()
                r64, r32 = R.logmel_refs(B, T, silent, with_bn)
                _check(f"logmel[wave{wave}-B{B}-T{T}-bn{int(with_bn)}]", out.cpu(), r64, r32, worst=worst)
    finally:
        call("zs_tune_set", b"logmel_wave", 1)
    worst.show()


def test_wav2img(cuda):
    """T_in = 2, 3 (every tap clamped), 1001 (the model's), 1023, and 1024 (scale 1: the output is
    the folded input bit for bit); B 1 and 3.
    Measured on an MI355X: closest at T_in 1001, error 1.602e-03 = the yardstick (tolerance
    6.409e-03): the float32 source index scale * t near 1000 costs 6e-5 of a sample, on values of
    +-15, in the kernel and the twin alike."""
    worst = Worst("wav2img")
    for T_in in R.W2I_T:
        for B in R.W2I_B:
            x = R.w2i_case(B, T_in)
            out = Out(cuda, (B * 256, 256), F32, SENT)
            xd = x.to(cuda)
            _call("zs_wav2img", xd.data_ptr(), B, T_in, out.t.data_ptr())
            torch.cuda.synchronize()
            got = out.cpu().view(B, 256, 256)
            if T_in == 1024:
                assert torch.equal(got, x.view(B, 4, 256, 64).permute(0, 1, 3, 2).reshape(B, 256, 256))
            _check(f"wav2img[T{T_in}-B{B}]", got, R.wav2img(x), R.wav2img(x, dtype=F32), worst=worst)
    worst.show()


@pytest.mark.parametrize("B", [1, 3])
def test_patch_embed(cuda, B):
    """Conv2d(1 -> 96, k4 s4) + LayerNorm per token; the image is a ramp plus noise, every token's
    4 x 4 patch distinct.
    Measured on an MI355X: B 1 error 1.388e-06 at yardstick 1.237e-06 (tolerance 5.946e-06), B 3
    1.093e-06 at 1.029e-06."""
    c = R.patch_embed_case(B)
    d = {k: v.to(cuda) for k, v in c.items()}
    out = Out(cuda, (B * 4096, 96), F32, SENT)
    _call("zs_patch_embed", d["img"].data_ptr(), B, d["w"].data_ptr(), d["b"].data_ptr(),
          d["lnw"].data_ptr(), d["lnb"].data_ptr(), out.t.data_ptr())
    torch.cuda.synchronize()
    a = (c["img"], c["w"], c["b"], c["lnw"], c["lnb"])
    worst = Worst("patch_embed")
    _check(f"patch_embed[B{B}]", out.cpu(), R.patch_embed(*a), R.patch_embed(*a, dtype=F32), worst=worst)
    worst.show()


def test_pack_clips(cuda):
    """Cropped and zero-padded clips, exact; T = 4 (one float4 per clip); clips at offsets that are
    no multiple of 4 floats with NaN behind each: no NaN reaches the output."""
    for (T, lens, gaps) in R.PACK_CASES:
        flat, off = R.pack_case(T, lens, gaps)
        out = Out(cuda, (len(lens), T), F32, SENT)
        fd, od, ld = _dev(cuda, flat, torch.tensor(off, dtype=I64), torch.tensor(lens, dtype=I32))
        _call("zs_pack_clips", fd.data_ptr(), od.data_ptr(), ld.data_ptr(), len(lens), T, out.t.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), R.pack_clips(flat, off, lens, T)), (T, lens)
    assert any(o % 4 for o in R.pack_case(*R.PACK_CASES[2])[1])


# ------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("ydt", DTS)
def test_layernorm(cuda, ydt):
    """C = 4, 256 (NV 1), 260, 512 (NV 2), 768 (NV 3), 1024 (NV 4), 1028 (strided: C > 1024), 770
    (strided: C % 4), 1; M = 1, 5, 8 (M % 4 != 0: idle waves in the last block); ldx = ldy = C + 4
    with NaN / sentinel tails; ldx = C + 1 (strided); x, y, and w and b one float past a 16-byte
    boundary (strided); rows with a repeat and the source's last row; a row of mean 1e3 and spread
    1, a constant row (eps decides: the output is b) and a row of magnitude 1e-4, each against its
    own yardstick; M = 0 writes nothing.
    Measured on an MI355X: f32 closest at pad4-C1028 row 3, error 5.528e-07 at yardstick 2.660e-07
    (tolerance 2.064e-06); bf16 errs by its yardstick (at most 7.770e-03, tolerance 3.905e-02)."""
    worst = Worst(f"layernorm[{_nm(ydt)}]")
    for (name, C, M, ldx, ldy, kind) in R.ln_cases():
        c = R.ln_case(C, M, ldx, kind)
        x = offset(c["x"], cuda) if kind == "xoff" else c["x"].to(cuda)
        w, b = (offset(c["w"], cuda), offset(c["b"], cuda)) if kind == "wboff" else (c["w"].to(cuda), c["b"].to(cuda))
        rows = c["rows"].to(cuda) if c["rows"] is not None else None
        y = _off_out(cuda, (M, ldy), ydt, SENT, 4 // (2 if ydt == BF16 else 4)) if kind == "yoff" \
            else Out(cuda, (M, ldy), ydt, SENT)
        if kind == "yoff":
            assert y.t.data_ptr() % 8 == 4
        _call("zs_layernorm", x.data_ptr(), M, C, ldx, _ptr(rows), w.data_ptr(), b.data_ptr(),
              R.LN_EPS, y.t.data_ptr(), ldy, _code(ydt))
        torch.cuda.synchronize()
        got = y.cpu()
        assert bool((got[:, C:] == SENT).all()), name
        assert _same_bits(x.cpu().reshape(-1), c["x"]), name
        a = (c["x"], M, C, ldx, c["rows"], c["w"], c["b"], R.LN_EPS)
        r64, r32 = R.layernorm(*a), R.layernorm(*a, dtype=F32, round_to=_rt(ydt))
        for m in range(M):                  # row by row: the special rows have their own yardsticks
            _check(f"layernorm[{name}-{_nm(ydt)}-row{m}]", got[m, :C], r64[m], r32[m], ydt == BF16, worst)
    y = Out(cuda, (4, 8), ydt, SENT)
    assert _call("zs_layernorm", y.t.data_ptr(), 0, 8, 8, None, y.t.data_ptr(), y.t.data_ptr(),
                 R.LN_EPS, y.t.data_ptr(), 8, _code(ydt)) == 0
    torch.cuda.synchronize()
    assert bool((y.cpu() == SENT).all())
    worst.show()


@pytest.mark.parametrize("ydt", DTS)
def test_patch_merge_ln(cuda, ydt):
    """C = 96, 192, 384 (the model's widths: VPL 6, 12, 24), 388 (4C > 1536: the block kernel), 5;
    (H, W) = (2, 2), (4, 8), (8, 4); B 1 and 3 (3 x 1 x 1 = 3 tokens: the last block of the wave
    kernel is part empty).
    Measured on an MI355X: f32 closest at C 192, B 3, 8 x 4, error 7.052e-07 at yardstick 6.815e-07
    (tolerance 3.726e-06); bf16 errs by its yardstick (1.535e-02, tolerance 7.771e-02)."""
    worst = Worst(f"patch_merge_ln[{_nm(ydt)}]")
    for (C, B, H, W) in R.PM_CASES:
        c = R.pm_case(C, B, H, W)
        ntok = B * H * W // 4
        y = Out(cuda, (ntok, 4 * C), ydt, SENT)
        xd, wd, bd = _dev(cuda, c["x"], c["w"], c["b"])
        _call("zs_patch_merge_ln", xd.data_ptr(), B, H, W, C, wd.data_ptr(), bd.data_ptr(),
              y.t.data_ptr(), _code(ydt))
        torch.cuda.synchronize()
        a = (c["x"], c["w"], c["b"])
        _check(f"patch_merge_ln[C{C}-B{B}-{H}x{W}-{_nm(ydt)}]", y.cpu(), R.patch_merge_ln(*a),
               R.patch_merge_ln(*a, dtype=F32, round_to=_rt(ydt)), ydt == BF16, worst)
    worst.show()


def test_ln_meanpool(cuda):
    """C = 48, 256 (CPL 4), 260, 768 (CPL 12), 772, 1024 (CPL 32) and the largest C the device's
    LDS limit per workgroup admits (64 C bytes of dynamic LDS; 2048 on gfx950's 160 KiB); the next
    multiple of 64 above it is refused.  N = 1, 15 (waves without a token), 16, 17, 64; B 1, 3.
    Measured on an MI355X: the device reports 163840 bytes, largest C 2048 (128 KiB of dynamic
    LDS launches and is correct), 2112 refused; closest at C 772, N 1, B 1: error 6.393e-07 at
    yardstick 3.144e-07 (tolerance 2.257e-06)."""
    from zsaac._lib import ZsError
    cmax = R.mp_max_c(torch.cuda.get_device_properties(0).shared_memory_per_block)
    print(f"ln_meanpool: LDS per workgroup {torch.cuda.get_device_properties(0).shared_memory_per_block}, largest C {cmax}")
    worst = Worst("ln_meanpool")
    for C in R.MP_C + (cmax,):
        for N in R.MP_N:
            for B in R.MP_B:
                c = R.mp_case(B, N, C)
                out = Out(cuda, (B, C), F32, SENT)
                xd, wd, bd = _dev(cuda, c["x"], c["w"], c["b"])
                _call("zs_ln_meanpool", xd.data_ptr(), B, N, C, wd.data_ptr(), bd.data_ptr(),
                      out.t.data_ptr())
                torch.cuda.synchronize()
                a = (c["x"], c["w"], c["b"])
                _check(f"ln_meanpool[C{C}-N{N}-B{B}]", out.cpu(), R.ln_meanpool(*a),
                       R.ln_meanpool(*a, dtype=F32), worst=worst)
    buf = torch.zeros(4 * (cmax + 64), device=cuda)
    with pytest.raises(ZsError, match=r"failed \(-1\)"):
        _call("zs_ln_meanpool", buf.data_ptr(), 1, 1, cmax + 64, buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
    worst.show()


def test_cast(cuda):
    """n = 1, 255, 256, 257 to bf16 (round to nearest even, values on a tie included) and to f32
    (a copy), bit-exact against torch."""
    for n in (1, 255, 256, 257):
        x = R.cast_case(n)
        for dt in DTS:
            y = Out(cuda, (n,), dt, SENT)
            xd = x.to(cuda)
            _call("zs_cast", xd.data_ptr(), n, y.t.data_ptr(), _code(dt))
            torch.cuda.synchronize()
            assert _same_bits(y.cpu(), R.cast(x, dt)), (n, dt)


# ------------------------------------------------------------------ CNN14
@pytest.mark.parametrize("dt", DTS)
def test_conv3x3(cuda, dt):
    """(Cin, Cout) = (1, 64) (the tap-gather loader), (64, 64), (64, 128), (32, 96) and (32, 160)
    (Cout no multiple of the 64 / 128 column tile), (128, 256); (B, H, W) = (1, 1, 1) (every tap
    but the centre outside), (1, 3, 5), (2, 21, 16), (3, 5, 9) (M = 135: a second, part-empty row
    tile).  The shift is negative for about half the channels: ReLU clips.
    Measured on an MI355X: f32 closest at (128, 256), 2 x 21 x 16 (K = 1152), error 7.905e-06 at
    yardstick 2.058e-06 (tolerance 9.232e-06: the MFMA's k-order against torch's matmul, both
    plain float32); bf16 errs by its yardstick (1.547e-02, tolerance 7.756e-02)."""
    worst = Worst(f"conv3x3[{_nm(dt)}]")
    for (Cin, Cout) in R.CONV_CH:
        for (B, H, W) in R.CONV_SHAPES:
            c = R.conv_case(Cin, Cout, B, H, W, dt)
            out = Out(cuda, (B * H * W, Cout), dt, SENT)
            xd, wd, sc, sh = _dev(cuda, c["x"], c["w"], c["scale"], c["shift"])
            _call("zs_conv3x3_bn_relu", xd.data_ptr(), B, H, W, Cin, wd.data_ptr(), Cout, sc.data_ptr(),
                  sh.data_ptr(), out.t.data_ptr(), _code(dt))
            torch.cuda.synchronize()
            a = (c["x"], c["w"], c["scale"], c["shift"])
            _check(f"conv3x3[{Cin}-{Cout}-{B}x{H}x{W}-{_nm(dt)}]", out.cpu().view(B, H, W, Cout),
                   R.conv3x3_bn_relu(*a), R.conv3x3_bn_relu(*a, dtype=F32, round_to=_rt(dt)), dt == BF16, worst)
    worst.show()


@pytest.mark.parametrize("dt", DTS)
def test_avgpool2(cuda, dt):
    """(H, W) = (2, 2), (21, 16) (odd H), (16, 21) (odd W), (5, 7) (both); C 1 and 64.
    Measured on an MI355X: error = yardstick in every case (f32 at most 1.490e-07, bf16 3.906e-03)."""
    worst = Worst(f"avgpool2[{_nm(dt)}]")
    for (H, W) in R.POOL_SHAPES:
        for C in R.POOL_C:
            x = R.pool_case(H, W, C, dt)
            out = Out(cuda, (2 * (H // 2), W // 2, C), dt, SENT)
            xd = x.to(cuda)
            _call("zs_avgpool2", xd.data_ptr(), 2, H, W, C, out.t.data_ptr(), _code(dt))
            torch.cuda.synchronize()
            _check(f"avgpool2[{H}x{W}-C{C}-{_nm(dt)}]", out.cpu().view(2, H // 2, W // 2, C), R.avgpool2(x),
                   R.avgpool2(x, dtype=F32, round_to=_rt(dt)), dt == BF16, worst)
    worst.show()


@pytest.mark.parametrize("dt", DTS)
def test_cnn_head(cuda, dt):
    """(H, W, C) = (1, 1, 1), (31, 2, 2048) (CNN14's last map), (7, 3, 300) (C no multiple of the
    256-thread block); B 1 and 3; inputs of mean -3, so every maximum is negative.
    Measured on an MI355X: f32 closest at (31, 2, 2048), B 1, error 1.073e-06 at yardstick
    7.633e-07 (tolerance 4.053e-06); bf16 inputs 5.904e-07 = yardstick."""
    worst = Worst(f"cnn_head[{_nm(dt)}]")
    for (H, W, C) in R.HEAD_SHAPES:
        for B in R.HEAD_B:
            x = R.head_case(B, H, W, C, dt)
            out = Out(cuda, (B, C), F32, SENT)
            xd = x.to(cuda)
            _call("zs_cnn_head", xd.data_ptr(), B, H, W, C, out.t.data_ptr(), _code(dt))
            torch.cuda.synchronize()
            _check(f"cnn_head[{H}x{W}x{C}-B{B}-{_nm(dt)}]", out.cpu(), R.cnn_head(x), R.cnn_head(x, dtype=F32),
                   worst=worst)
    worst.show()


# ------------------------------------------------------------------ window attention
@pytest.mark.parametrize("mode", ["f32", "bf16-mfma", "bf16-valu"])
def test_window_attention(cuda, mode):
    """f32 on the VALU kernel, bf16 on the MFMA kernel (window_mfma 1) and on the VALU kernel
    (window_mfma 0).  (H, W) = (8, 8), (8, 16), (16, 8), (16, 24); shift 0, 4, 1, 7; head dim 24
    and 32, and 8 and 16 on the MFMA kernel; (B, heads) = (1, 3) at 8 x 8: 3 (window, head) items,
    the MFMA block's last wave idle.  Bias table with spread +-3.
    Measured on an MI355X: f32 closest at 8 x 16, shift 1, hd 32: error 2.486e-06 at yardstick
    1.323e-06 (tolerance 6.291e-06).  bf16: kernel error / yardstick = 1.00 in every one of the 72
    MFMA cases (errors 5.36e-03 .. 9.85e-03) and the 36 VALU cases (6.82e-03 .. 7.81e-03): the
    largest error is the bf16 rounding of the largest output element, which kernel and twin
    round alike (the bound is 2.00); nothing to explain from the summation order."""
    from zsaac._lib import call
    dt = F32 if mode == "f32" else BF16
    hds = (24, 32, 8, 16) if mode == "bf16-mfma" else (24, 32)
    worst = Worst(f"window_attention[{mode}]")
    call("zs_tune_set", b"window_mfma", 0 if mode == "bf16-valu" else 1)
    try:
        for (B, H, W, heads, hd, shift) in R.wa_cases(hds):
            c = R.wa_case(B, H, W, heads, hd, shift, dt)
            C = c["C"]
            out = Out(cuda, (B * H * W, C), dt, SENT)
            qd, td = _dev(cuda, c["qkv"], c["table"])
            _call("zs_window_attention", qd.data_ptr(), B, H, W, C, heads, 8, shift, td.data_ptr(),
                  out.t.data_ptr(), _code(dt))
            torch.cuda.synchronize()
            a = (c["qkv"], B, H, W, C, heads, shift, c["table"])
            name = f"window_attention[{mode}-{H}x{W}-s{shift}-hd{hd}-B{B}-h{heads}]"
            r64 = R.window_attention(*a)
            if mode == "f32":
                _check(name, out.cpu(), r64, R.window_attention(*a, dtype=F32), worst=worst)
            else:
                tw = R.window_attention(*a, dtype=F32, p_round=BF16 if mode == "bf16-mfma" else None,
                                        out_round=BF16)
                _check_bf16(name, out.cpu(), r64, tw, worst)
    finally:
        call("zs_tune_set", b"window_mfma", 1)
    worst.show()


# ------------------------------------------------------------------ fused Swin block
def test_swin_block(cuda):
    """C = 96, 192, 384; (H, W) = (8, 8), (8, 16), (16, 8); B 1 and 3; shift 0 and 4; x updated in
    place in a sentinel-guarded buffer.  Weights as tests/test_gpu_swin.py builds them.
    Measured on an MI355X, kernel error / yardstick (bound 2.00), cases in the order of
    encoder_ref.SWIN_CASES: 1.00, 1.00, 0.95, 1.00, 1.00, 1.00, 1.00, 1.00, 1.00, 1.00, 1.00, 1.00
    (errors 9.26e-03 .. 1.18e-02 on outputs of magnitude 5; yardsticks 9.26e-03 .. 1.20e-02): the
    twin rounds at the kernel's rounding points and reproduces it to a few 1e-5, so both sit at
    the same distance from float64; nothing to explain from the summation order."""
    from test_gpu_swin import _block_sd, _kernel_blk
    worst = Worst("swin_block")
    for (C, B, H, W, shift) in R.SWIN_CASES:
        heads = C // 24
        sd = _block_sd(C, heads, C + shift, cuda)
        blk = _kernel_blk(sd, C, cuda)
        x0 = R.swin_x(C, B, H, W)
        x = Out(cuda, (B * H * W, C), F32, SENT, init=x0)
        _call("zs_swin_block", x.t.data_ptr(), B, H, W, C, heads, shift, _ptr(blk["n1"][0]), _ptr(blk["n1"][1]),
              _ptr(blk["qkv_p"]), _ptr(blk["qkv_bp"]), _ptr(blk["rel"]), _ptr(blk["proj_p"]),
              _ptr(blk["proj_b"]), _ptr(blk["n2"][0]), _ptr(blk["n2"][1]), _ptr(blk["fc1_p"]),
              _ptr(blk["fc1_b"]), _ptr(blk["fc2_p"]), _ptr(blk["fc2_b"]))
        torch.cuda.synchronize()
        r64 = R.swin_block(x0, sd, B, H, W, C, heads, shift)
        tw = R.swin_block(x0, sd, B, H, W, C, heads, shift, dtype=F32, rnd=BF16)
        _check_bf16(f"swin_block[C{C}-B{B}-{H}x{W}-s{shift}]", x.cpu(), r64, tw, worst)
    worst.show()
