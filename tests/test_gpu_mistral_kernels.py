"""The Mistral decoder's non-GEMM kernels (csrc/mistral.hip) one by one against
tests/mistral_ref.py, at the shapes and edges where they can go wrong: row widths that leave
threads idle or need up to four passes, split counts that reach the unrolled group and the tail
of the slab sum, padded split strides, key counts on both sides of the attention loop's 32-key
step, every head grouping, the prefill form, bf16 and f32.

Every output is filled with a sentinel and allocated with a guard row behind it; the guard must
come back unchanged.  Slab padding, cache positions a kernel must not read and the caches'
unwritten rows hold NaN or a sentinel and are compared bit for bit.  Ids and copies are compared
with torch.equal.  Float outputs are compared with the float64 reference under the rule of
test_gpu_magic_kernels.py::_check: the yardstick is the same formula evaluated in float32 on the
CPU (rounded to bf16 where the kernel rounds), measured as its largest deviation from float64 on
the case's own data; the tolerance is 4 x yardstick + 1e-6, plus one bf16 step of the reference
(2^-8 |ref|, elementwise) for a bf16 output.  The input conditions of the cases are asserted on
the CPU in tests/test_mistral_ref.py, which also shows that these inputs tell each of the listed
arithmetic errors from the reference."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mistral_ref as R  # noqa: E402
from gpu_helpers import Out  # noqa: E402

pytestmark = pytest.mark.gpu
I32 = torch.int32
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
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


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _check(name, got, ref64, ref32, bf16=False):
    """|got - float64 reference| <= tolerance (mistral_ref.tolerance) elementwise; prints the
    largest error, the yardstick and the tolerance at the element closest to its bound."""
    yard, tol = R.tolerance(ref64, ref32, bf16)
    err = (got.double() - ref64).abs()
    i = int((err / tol).nan_to_num(nan=float("inf")).argmax())
    print(f"{name}: error {float(err.max()):.3e}, yardstick {yard:.3e}, tolerance "
          f"{float(tol.reshape(-1)[i]):.3e} (closest: error {float(err.reshape(-1)[i]):.3e})")
    assert bool((err <= tol).all()), (name, float(err.reshape(-1)[i]), yard, float(tol.reshape(-1)[i]))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def test_host_checks_refuse(cuda):
    """Arguments outside the contract of include/zsaac.h are refused by the host wrappers (an
    error code, nothing launched): D past the four passes or not a multiple of 4, a split stride
    that breaks the 16-byte loads, F % 8 != 0, Lmax 0 and a NULL buffer for zs_mistral_rope_kv,
    M > 32 for zs_mistral_add_ss, ld < N for zs_scale_cols."""
    from zsaac._lib import ZsError
    buf = torch.zeros(4096, device=cuda)
    ids = torch.zeros(8, dtype=I32, device=cuda)
    p, i = buf.data_ptr(), ids.data_ptr()
    bad = [("zs_mistral_add_rmsnorm", p, None, 1, 0, 1, 16388, R.EPS, None, p, 0),
           ("zs_mistral_add_rmsnorm", p, None, 1, 0, 1, 6, R.EPS, None, p, 0),
           ("zs_mistral_add_rmsnorm", p, p, 2, 18, 1, 16, R.EPS, None, p, 0),
           ("zs_mistral_silu_mul", p, 1, 24, 1, 12, p, 0),
           ("zs_mistral_silu_mul", p, 2, 18, 1, 8, p, 0),
           ("zs_mistral_rope_kv", p, 1, 0, 1, 4, 4, i, 1, p, p, p, p, p, 0, 0),
           ("zs_mistral_rope_kv", p, 1, 0, 1, 4, 4, i, 1, p, p, None, p, p, 8, 0),
           ("zs_mistral_rope_kv", p, 1, 0, 1, 6, 4, i, 1, p, p, p, p, p, 8, 0),
           ("zs_mistral_add_ss", p, None, 1, 0, 33, 512, p, p),
           ("zs_scale_cols", p, 2, 8, 4, p)]
    for args in bad:
        with pytest.raises(ZsError, match=r"failed \(-1\)"):     # ZS_ERR_ARG, before any launch
            _call(*args)
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


# ------------------------------------------------------------------ residual add + RMSNorm
@pytest.mark.parametrize("hdt", DTS)
@pytest.mark.parametrize("D", R.NORM_D)
def test_add_rmsnorm(cuda, D, hdt):
    """D = 4 (one live thread of 1024), 1024, 4096 (exactly one pass), 4100 (a second pass with
    one live thread), 8192, 16384 (four passes); M 1 and 3 (row 1 of magnitude 1e-4: eps
    decides; every row is checked against its own yardstick); y NULL with ss = 0, and 1 / 4 / 5 /
    6 / 9 slabs dense and with ss = M D + 8 (NaN between the slabs); w NULL and given.  x is
    updated in place, bit-unchanged when y is NULL.
    Measured on an MI355X: f32 h error 2.07e-10 .. 1.39e-06 at yardsticks 2.07e-10 .. 1.57e-06,
    closest to its bound at D 8192, M 3, 4 padded slabs, w given: 1.385e-06 at yardstick 5.70e-07
    (tolerance 3.28e-06); x at most 2.22e-06 = its yardstick (D 4100, 9 slabs, tolerance
    9.88e-06); bf16 h error = yardstick in every case (at most 3.11e-02, a fifth of the
    tolerance)."""
    for M in R.NORM_M:
        for nsplit, pad in [(0, 0)] + [(n, p) for n in R.NORM_NSPLIT for p in (0, 8)]:
            c = R.residual_case(M, D, nsplit, pad)
            yd = c["y"].to(cuda) if nsplit else None
            for w in (None, c["w"]):
                x = Out(cuda, (M, D), F32, SENT, init=c["x"])
                h = Out(cuda, (M, D), hdt, SENT)
                wd = w.to(cuda) if w is not None else None
                _call("zs_mistral_add_rmsnorm", x.t.data_ptr(), _ptr(yd), nsplit, c["ss"], M, D,
                      R.EPS, _ptr(wd), h.t.data_ptr(), _code(hdt))
                torch.cuda.synchronize()
                a = (c["x"], c["y"], nsplit, c["ss"], M, D, R.EPS, w)
                x64, h64 = R.add_rmsnorm(*a)
                x32, h32 = R.add_rmsnorm(*a, dtype=F32, round_to=_rt(hdt))
                tag = (f"add_rmsnorm[D{D}-M{M}-ns{nsplit}-pad{pad}-w{int(w is not None)}-"
                       f"{'bf16' if hdt == BF16 else 'f32'}]")
                gx, gh = x.cpu(), h.cpu()
                if nsplit == 0:
                    assert torch.equal(gx, c["x"]), tag
                for m in range(M):           # row by row: the 1e-4 row has its own yardstick
                    if nsplit:
                        _check(f"{tag} x row {m}", gx[m], x64[m], x32[m])
                    _check(f"{tag} h row {m}", gh[m], h64[m], h32[m], hdt == BF16)


@pytest.mark.parametrize("M,D", R.ADD_SS_SHAPES)
def test_add_ss(cuda, M, D):
    """M = 32 at D = 512 (one chunk) and 4096 (eight), M = 5 at 4096; 5 / 6 / 9 slabs (the
    unrolled group of slab_sum4, group + tail, two groups), dense and padded ss with NaN between
    the slabs, and y NULL.  xb is the f32 x rounded once; every rss entry outside [:D/512, :M]
    keeps its NaN.  Row 1 (magnitude 1e-4, rss of 1e-5) is checked against its own yardstick.
    Measured on an MI355X: x error = yardstick, at most 2.03e-06 (tolerance 9.11e-06); rss
    (sums of about 5000) error 4.93e-04 .. 1.17e-03 at yardsticks 5.40e-04 .. 1.25e-03, closest
    M 5, D 4096, 6 slabs: 8.13e-04 at 6.24e-04 (tolerance 2.50e-03)."""
    nch = D // 512
    for nsplit, pad in [(0, 0)] + [(n, p) for n in R.ADD_SS_NSPLIT for p in (0, 8)]:
        c = R.residual_case(M, D, nsplit, pad, seed=1)
        yd = c["y"].to(cuda) if nsplit else None
        x = Out(cuda, (M, D), F32, SENT, init=c["x"])
        xb = Out(cuda, (M, D), BF16, SENT)
        rss = Out(cuda, (8, 32), F32, R.NAN)                  # NaN guard: compared below
        _call("zs_mistral_add_ss", x.t.data_ptr(), _ptr(yd), max(nsplit, 1), c["ss"], M, D,
              xb.t.data_ptr(), rss.t.data_ptr())
        torch.cuda.synchronize()
        a = (c["x"], c["y"], nsplit, c["ss"], M, D)
        (x64, r64), (x32, r32) = R.add_ss(*a), R.add_ss(*a, dtype=F32)
        tag = f"add_ss[M{M}-D{D}-ns{nsplit}-pad{pad}]"
        got = x.cpu()
        small = torch.arange(M) == 1          # the 1e-4 row against a yardstick of its own
        if nsplit == 0:
            assert torch.equal(got, c["x"]), tag
        else:
            _check(tag + " x", got[~small], x64[~small], x32[~small])
            _check(tag + " x small row", got[small], x64[small], x32[small])
        assert torch.equal(xb.cpu(), got.bfloat16()), tag
        full = rss.buf.cpu()
        assert bool(torch.isnan(full[8 * 32:]).all()), "guard row overwritten"
        full = full[:8 * 32].view(8, 32)
        _check(tag + " rss", full[:nch, :M][:, ~small], r64[:, ~small], r32[:, ~small])
        _check(tag + " rss small row", full[:nch, :M][:, small], r64[:, small], r32[:, small])
        assert bool(torch.isnan(full[nch:]).all()) and bool(torch.isnan(full[:, M:]).all()), tag


# ------------------------------------------------------------------ input rows
@pytest.mark.parametrize("tdt", DTS)
@pytest.mark.parametrize("D", [1024, 260])
@pytest.mark.parametrize("form", R.EMBED_FORMS + ["decode"])
def test_embed(cuda, form, D, tdt):
    """Prefill rows [embed(hard) ; soft ; embed(tag)] for B = 2 with each part absent in turn
    (NULL passed for it), and the decode form embed[tok]; D = 1024 and 260 (the second pass of
    the 256-thread copy holds 4 live threads), bf16 and f32 tables, ids 0, V - 1 and the pad id.
    Exact."""
    B = 2
    if form == "decode":
        _, _, _, emb = R.embed_case((1, 0, 0), D, tdt)
        tok = torch.tensor([0, R.EMBED_V - 1, R.EMBED_PAD, 7, 7], dtype=I32)
        hard = soft = tail = None
        H = ns = nt = 0
        M = tok.numel()
    else:
        H, ns, nt = form
        hard, soft, tail, emb = R.embed_case(form, D, tdt)
        tok, M = None, B * (H + ns + nt)
    d = [t.to(cuda) if t is not None else None for t in (hard, soft, tail, tok, emb)]
    x = Out(cuda, (M, D), F32, SENT)
    _call("zs_mistral_embed", _ptr(d[0]), H, _ptr(d[1]), ns, _ptr(d[2]), nt, _ptr(d[3]),
          d[4].data_ptr(), D, M, x.t.data_ptr(), _code(tdt))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), R.embed(hard, soft, tail, tok, emb))


# ------------------------------------------------------------------ RoPE + KV append
def _cache_checks(tag, got_k, got_v, k0, v0, k64, v64, k32, v32, seq, pos, bf16):
    """Rows (seq[m], :, pos[m]) against the reference, every other row bit-unchanged."""
    rows = (seq, slice(None), pos.long())
    _check(tag + " k rows", got_k[rows].float(), k64[rows], k32[rows], bf16)
    _check(tag + " v rows", got_v[rows].float(), v64[rows], v32[rows], bf16)
    keep = torch.ones(got_k.shape[:3], dtype=torch.bool)
    keep[rows] = False
    assert _same_bits(got_k[keep], k0[keep]) and _same_bits(got_v[keep], v0[keep]), tag


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", ["ragged", "prefill"])
@pytest.mark.parametrize("H,KVH", R.HEADS)
def test_rope_kv(cuda, H, KVH, form, dt):
    """Heads (8, 2), (4, 4), (6, 1); 1 slab and 3 slabs with ss padded by 8 (NaN in the
    padding); rows_per_seq 1 with ragged pos {0, 1, 31, 32, 71} (Lmax 72), and the prefill form:
    2 sequences of 5 rows at pos 0..4.  q, the written cache rows, and every other cache row
    (sentinel) bit-unchanged.
    Measured on an MI355X: f32 q error 1.52e-07 .. 5.96e-07 at yardsticks 1.94e-07 .. 6.48e-07
    (closest (6, 1) prefill, 3 slabs: 5.96e-07 at 5.56e-07, tolerance 3.23e-06), k rows at most
    6.41e-07 = yardstick, v rows at most 4.17e-07 = yardstick; bf16 error = yardstick (the
    rounding of the largest element, 7.6e-03 .. 1.56e-02), a fifth of the tolerance."""
    M, pos, rps, S = R.rope_case(H, KVH, form)
    cos, sin = R.rope_tables()
    cd, sd, pd = cos.to(cuda), sin.to(cuda), pos.to(cuda)
    k0 = torch.full((S, KVH, R.LMAX, R.HD), SENT).to(dt)
    for nsplit in R.ROPE_NSPLIT:
        qkv, ss = R.qkv_case(M, H, KVH, nsplit)
        qd = qkv.to(cuda)
        q = Out(cuda, (M, H * R.HD), dt, SENT)
        kc = Out(cuda, tuple(k0.shape), dt, SENT)
        vc = Out(cuda, tuple(k0.shape), dt, SENT)
        _call("zs_mistral_rope_kv", qd.data_ptr(), nsplit, ss, M, H, KVH, pd.data_ptr(), rps,
              cd.data_ptr(), sd.data_ptr(), q.t.data_ptr(), kc.t.data_ptr(), vc.t.data_ptr(),
              R.LMAX, _code(dt))
        torch.cuda.synchronize()
        a = (qkv, nsplit, ss, M, H, KVH, pos, rps, cos, sin, k0, k0)
        q64, k64, v64 = R.rope_kv(*a)
        q32, k32, v32 = R.rope_kv(*a, dtype=F32, round_to=_rt(dt))
        tag = f"rope_kv[{H}/{KVH}-{form}-ns{nsplit}-{'bf16' if dt == BF16 else 'f32'}]"
        _check(tag + " q", q.cpu().float(), q64, q32, dt == BF16)
        _cache_checks(tag, kc.cpu(), vc.cpu(), k0, k0, k64, v64, k32, v32,
                      torch.arange(M) // rps, pos, dt == BF16)


# ------------------------------------------------------------------ attention
def _attention(cuda, H, KVH, form, dt):
    c = R.att_case(H, KVH, form, dt)
    M = c["M"]
    qd, kd, vd, pd = (c[k].to(cuda) for k in ("q", "kc", "vc", "pos"))
    out = Out(cuda, (M, H * R.HD), dt, SENT)
    _call("zs_mistral_attention", qd.data_ptr(), M, H, KVH, pd.data_ptr(), c["rps"],
          kd.data_ptr(), vd.data_ptr(), R.LMAX, out.t.data_ptr(), _code(dt))
    torch.cuda.synchronize()
    a = (c["q"], M, H, KVH, c["pos"], c["rps"], c["kc"], c["vc"])
    got = out.cpu().float()
    assert bool(torch.isfinite(got).all())
    _check(f"attention[{H}/{KVH}-{form}-{'bf16' if dt == BF16 else 'f32'}]", got,
           R.attention(*a), R.attention(*a, dtype=F32, round_to=_rt(dt)), dt == BF16)
    assert _same_bits(kd.cpu(), c["kc"]) and _same_bits(vd.cpu(), c["vc"])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", R.ATT_FORMS)
@pytest.mark.parametrize("H,KVH", R.HEADS)
def test_attention(cuda, H, KVH, form, dt):
    """q and the caches in the tested type (exact inputs).  ragged9: one row per sequence at pos
    {0, 7, 8, 31, 32, 33, 63, 64, 71}; ragged3: pos {0, 33, 71} ((6, 1): 18 waves, the last block
    has two live); prefill5 / prefill33: two sequences of P rows at pos 0..P-1 (rows_per_seq =
    P).  Cache positions past each sequence's largest pos hold NaN; the output is finite.
    Measured on an MI355X: f32 error 1.28e-07 .. 5.61e-07 at yardsticks 1.85e-07 .. 8.54e-07,
    closest (8, 2) prefill5: 5.61e-07 at 3.53e-07 (tolerance 2.41e-06); bf16 error = yardstick,
    at most 7.77e-03 (tolerance 3.9e-02)."""
    _attention(cuda, H, KVH, form, dt)


@pytest.mark.parametrize("dt", DTS)
def test_attention_online_softmax(cuda, dt):
    """H = KVH = 4, pos {71, 40}: key 36 scores more than 20 above every key of the first 32-key
    step (asserted in test_mistral_ref.py), so the running maximum and the rescaling of the
    accumulated sums carry the result.
    Measured on an MI355X: error = yardstick = 2.09e-10 (f32) / 2.11e-10 (bf16): the output is
    the v row of key 36 up to the other keys' weight of e^-30."""
    _attention(cuda, 4, 4, "online", dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("nsplit", R.DEC_NSPLIT)
@pytest.mark.parametrize("H,KVH", R.HEADS)
def test_decode_attention(cuda, H, KVH, nsplit, dt):
    """The fused decode step for 8 sequences at pos {0, 1, 8, 31, 32, 33, 64, 71}; 1 / 5 / 6
    slabs (ss padded by 8, NaN in the padding).  The caches hold NaN at every position >= pos
    before the call: row pos of each cache against rope_kv's reference, every other position
    bit-unchanged, the output (finite) against the composition with q and the new k / v rounded
    to the cache type.
    Measured on an MI355X: f32 out error 2.57e-07 .. 2.52e-06 at yardsticks 2.72e-07 .. 4.01e-06,
    closest (4, 4), 6 slabs: 1.505e-06 at 8.42e-07 (tolerance 4.37e-06); f32 k / v rows at most
    9.61e-07 / 8.94e-07 = yardstick; bf16 out and rows error = yardstick (7.5e-03 .. 2.83e-02), a
    fifth of the tolerance."""
    c = R.dec_case(H, KVH, nsplit, dt)
    M = c["M"]
    cos, sin = R.rope_tables()
    qd, cd, sd, pd = c["qkv"].to(cuda), cos.to(cuda), sin.to(cuda), c["pos"].to(cuda)
    kc = Out(cuda, tuple(c["kc"].shape), dt, SENT, init=c["kc"])
    vc = Out(cuda, tuple(c["vc"].shape), dt, SENT, init=c["vc"])
    out = Out(cuda, (M, H * R.HD), dt, SENT)
    _call("zs_mistral_decode_attention", qd.data_ptr(), nsplit, c["ss"], M, H, KVH, pd.data_ptr(),
          cd.data_ptr(), sd.data_ptr(), kc.t.data_ptr(), vc.t.data_ptr(), R.LMAX,
          out.t.data_ptr(), _code(dt))
    torch.cuda.synchronize()
    a = (c["qkv"], nsplit, c["ss"], M, H, KVH, c["pos"], cos, sin, c["kc"], c["vc"])
    o64, _, _ = R.decode_attention(*a, cache_round=_rt(dt))
    o32, _, _ = R.decode_attention(*a, dtype=F32, cache_round=_rt(dt), out_round=_rt(dt))
    r = (c["qkv"], nsplit, c["ss"], M, H, KVH, c["pos"], 1, cos, sin, c["kc"], c["vc"])
    _, k64, v64 = R.rope_kv(*r)
    _, k32, v32 = R.rope_kv(*r, dtype=F32, round_to=_rt(dt))
    tag = f"decode_attention[{H}/{KVH}-ns{nsplit}-{'bf16' if dt == BF16 else 'f32'}]"
    _cache_checks(tag, kc.cpu(), vc.cpu(), c["kc"], c["vc"], k64, v64, k32, v32, torch.arange(M),
                  c["pos"], dt == BF16)
    got = out.cpu().float()
    assert bool(torch.isfinite(got).all())
    _check(tag + " out", got, o64, o32, dt == BF16)


# ------------------------------------------------------------------ SiLU * up, column scaling
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,F", R.SILU_SHAPES)
def test_silu_mul(cuda, M, F, dt):
    """F = 8 and 1032, M = 1 and 5 (M F / 4 is never a multiple of the 256-thread block: the
    last block is partly idle); 1 / 5 / 6 slabs, ss padded by 8 with NaN; gates of +-100, +-81
    and +-20 in row 0: the result is finite and equals float64 silu * up.  The scripted gates
    (products of hundreds) and the rest are checked against yardsticks of their own.
    Measured on an MI355X: error = yardstick in every case (the kernel's expression is the
    float32 formula): f32 scripted at most 6.46e-05 (tolerance 2.59e-04), rest at most 2.43e-05
    (tolerance 9.81e-05); bf16 a fifth of the tolerance."""
    for nsplit in R.SILU_NSPLIT:
        gu, ss = R.silu_case(M, F, nsplit)
        gd = gu.to(cuda)
        act = Out(cuda, (M, F), dt, SENT)
        _call("zs_mistral_silu_mul", gd.data_ptr(), nsplit, ss, M, F, act.t.data_ptr(), _code(dt))
        torch.cuda.synchronize()
        got = act.cpu().float()
        assert bool(torch.isfinite(got).all())
        a = (gu, nsplit, ss, M, F)
        r64, r32 = R.silu_mul(*a), R.silu_mul(*a, dtype=F32, round_to=_rt(dt))
        big = torch.zeros(M, F, dtype=torch.bool)          # the scripted gates: products of
        big[0, :len(R.SILU_GATES)] = True                  # hundreds, a yardstick of their own
        tag = f"silu_mul[M{M}-F{F}-ns{nsplit}-{'bf16' if dt == BF16 else 'f32'}]"
        _check(tag + " scripted", got[big], r64[big], r32[big], dt == BF16)
        _check(tag + " rest", got[~big], r64[~big], r32[~big], dt == BF16)


@pytest.mark.parametrize("M,N", [(3, 12), (5, 1028)])
def test_scale_cols(cuda, M, N):
    """ld = N + 4: the four columns past N keep their sentinel; exact against the f32 product
    (measured on an MI355X: 2.38e-07 from float64 = the yardstick, tolerance 1.95e-06)."""
    ld = N + 4
    g = R.gen(M + N)
    x0 = torch.randn(M, ld, generator=g)
    x0[:, N:] = SENT
    scale = torch.randn(N, generator=g)
    x = Out(cuda, (M, ld), F32, SENT, init=x0)
    sd = scale.to(cuda)
    _call("zs_scale_cols", x.t.data_ptr(), M, N, ld, sd.data_ptr())
    torch.cuda.synchronize()
    got = x.cpu()
    assert torch.equal(got, R.scale_cols(x0, M, N, ld, scale, dtype=F32))
    assert bool((got[:, N:] == SENT).all())
    _check(f"scale_cols[{M}x{N}]", got, R.scale_cols(x0, M, N, ld, scale),
           R.scale_cols(x0, M, N, ld, scale, dtype=F32))
