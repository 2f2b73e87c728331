"""The GPT-2 / mapper / cross attention kernels of csrc/attn.hip one by one against
tests/attn_ref.py: zs_decode_attention under every plan of its dispatch table (and both f32
fallback kernels), zs_decode_attention_map, the scalar and the MFMA row attention,
zs_row_attention_kv, zs_kv_write and zs_cross_attention, at the positions, lengths, head counts
and strides where they can go wrong.

Every output is allocated with a sentinel fill and a guard row behind it that must come back
unchanged.  Cache slots a kernel must not use hold NaN, masked key rows +-1e4, padding columns a
sentinel; caches and copies are compared bit for bit.  References are computed on the CPU from
the CPU copies of the inputs.  Float outputs are compared with the float64 reference under the
project's rule (attn_ref.tolerance): yardstick = the float32 formula's largest deviation from
float64 on the case's own data, tolerance 4 x yardstick + 1e-6, plus 2^-8 |ref| elementwise for
a bf16 output.  Every test prints the worst error, the yardstick and the tolerance before it
asserts.  tests/test_attn_ref.py asserts the input conditions and shows on the CPU that these
inputs tell each mutant of attn_ref.MUTANTS from the reference.

ZSAAC_ATTN_ERRORS=<file>: every comparison's figures are written there when the module ends
(profiles/attn_kernel_errors.txt is such a run)."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402
from gpu_helpers import Out  # noqa: E402

pytestmark = pytest.mark.gpu
I32 = torch.int32
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTS = [F32, BF16]
SENT = -7.0
_RECORDS = []


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("ZSAAC_ATTN_ERRORS")
    if path and _RECORDS:
        with open(path, "w") as f:
            f.write("# what: yardstick (float32 formula vs float64), largest tolerance, kernel's "
                    "worst error, worst error / tolerance\n")
            for r in _RECORDS:
                f.write("%-64s yard %.3e tol %.3e err %.3e ratio %.3f\n" % r)


def _call(name, *args):
    from zsaac._lib import call
    return call(name, *args, torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def knobs(**kw):
    """zs_tune_set under try / finally, restored to attn_ref.KNOB_DEFAULTS."""
    from zsaac._lib import call
    try:
        for k, v in kw.items():
            call("zs_tune_set", k.encode(), v)
        yield
    finally:
        for k in kw:
            call("zs_tune_set", k.encode(), R.KNOB_DEFAULTS[k])


def _code(dt):
    from zsaac._lib import ZS_BF16, ZS_F32
    return ZS_BF16 if dt == BF16 else ZS_F32


def _name(dt):
    return "bf16" if dt == BF16 else "f32"


def _rt(dt):
    return None if dt == F32 else dt


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _check(name, got, ref64, ref32, bf16=False):
    """|got - float64 reference| <= tolerance elementwise; prints and records the figures."""
    yard, tol = R.tolerance(ref64, ref32, bf16)
    err = (got.double() - ref64).abs()
    ratio = float((err / tol).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    _RECORDS.append((name, yard, float(tol.max()), float(err.max()), ratio))
    print("%s: error %.3e, yardstick %.3e, tolerance %.3e, error / tolerance %.3f"
          % (name, float(err.max()), yard, float(tol.max()), ratio))
    assert ratio <= 1.0, (name, float(err.max()), yard, ratio)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _padded(cuda, rows, E, ld, dt):
    """An output of ``rows`` rows of E with row stride ld: the columns past E and the guard row
    keep the sentinel."""
    o = Out(cuda, (rows, ld), dt, SENT)
    return o, o.t[:, :E]


def _padding_kept(o, E):
    full = o.cpu()
    return bool((full[:, E:] == SENT).all()), full[:, :E]


# ------------------------------------------------------------------ decode attention
def _plan_name(dt, heads, small, split, da5):
    """attn.hip's decode_plan for a direct call of up to small_rmax rows."""
    bf = dt == BF16
    if small:
        if bf and split == 4:
            return "kpp32-dpp-split4"
        if split and heads % 2 == 0:
            return "kpp%d-dpp-split2" % (64 if bf and split != 3 else 32)
        return "kpp128-dpp-split1" if bf else "fallback"
    if not bf:
        return "fallback"
    return {6: "kpp16-dpp", 4: "kpp16-bperm", 3: "kpp32-bperm", 2: "kpp64-bperm"}[da5] + "-split1"


_REFS = {}


def _decode_refs(data, dt, heads, form):
    """float64 reference, float32 yardstick run and the caches after the call, once per case."""
    key = (data, dt, heads, form)
    if key not in _REFS:
        c = R.decode_case(data, dt, heads, form)
        a = (c["qkv"], c["R"], c["D"], heads, c["kc"], c["vc"], c["Lmax"], c["pos"], c["kvrow"])
        o64, k1, v1 = R.decode_attention(*a)
        o32, _, _ = R.decode_attention(*a, dtype=F32, round_to=_rt(dt))
        _REFS[key] = (c, o64, o32, k1, v1)
    return _REFS[key]


def _decode(cuda, tag, data, dt, heads, form):
    c, o64, o32, k1, v1 = _decode_refs(data, dt, heads, form)
    qd, pd = c["qkv"].to(cuda), c["pos"].to(cuda)
    kvd = c["kvrow"].to(cuda) if c["kvrow"] is not None else None
    kc = Out(cuda, tuple(c["kc"].shape), dt, SENT, init=c["kc"])
    vc = Out(cuda, tuple(c["vc"].shape), dt, SENT, init=c["vc"])
    out = Out(cuda, (c["R"], c["D"]), dt, SENT)
    _call("zs_decode_attention", qd.data_ptr(), c["R"], c["D"], heads, kc.t.data_ptr(),
          vc.t.data_ptr(), c["Lmax"], pd.data_ptr(), _ptr(kvd), out.t.data_ptr(), _code(dt))
    torch.cuda.synchronize()
    got = out.cpu().float()
    assert bool(torch.isfinite(got).all()), tag
    # slot p holds the row's k / v bit for bit; everything else, NaN included, is bit-unchanged
    assert _same_bits(kc.cpu(), k1) and _same_bits(vc.cpu(), v1), tag
    _check(tag, got, o64, o32, dt == BF16)


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("heads", R.DEC_HEADS)
def test_decode_attention_every_plan(cuda, heads, dt):
    """zs_decode_attention, one row per position of {0, 1, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64,
    65, 95, 96, 127, 128, 129, 135} (Lmax 136: key counts on both sides of every phase length and
    SPLIT round), under every knob setting of the dispatch table: small_attn on with attn_split
    0 / 1 / 3 / 4, small_attn off with decode_attn5 6 / 4 / 3 / 2 -- for bf16 the eight
    decode_attn6_kernel<bf16> instantiations, for f32 decode_attn6_kernel<float, 32, DPP, 2> and
    decode_attn4_kernel<float> (5 heads are odd: bf16 runs {128, DPP, 1}, f32 the fallback; 6
    heads leave idle waves in the second block row) -- each on the "flat", "rising" and "hot"
    data.  Cache slots j >= p hold NaN before the call (slot 0 of the p == 0 row is loaded and
    discarded by value); afterwards slot p holds the row's k / v and all else is bit-unchanged.
    Measured on an MI355X: f32 error 2.29e-07 .. 3.61e-05 at yardsticks 2.94e-07 .. 2.95e-05
    (the largest on "rising", whose outputs are single v rows), closest decode_attn4_kernel, 6
    heads, "rising": 3.606e-05 at 1.462e-05 (tolerance 5.949e-05); decode_attn6_kernel<float> at
    most 0.40 of its tolerance (6 heads, "hot"); bf16 error = yardstick in every plan (the
    rounding of the output, 4.74e-03 .. 7.73e-03), a fifth of the tolerance."""
    for small, split, da5 in R.DEC_PLANS:
        with knobs(small_attn=small, attn_split=split, decode_attn5=da5):
            for data in R.DATA:
                tag = "decode[%s-h%d-%s-%s]" % (_name(dt), heads, _plan_name(dt, heads, small, split, da5), data)
                _decode(cuda, tag, data, dt, heads, "ragged")


@pytest.mark.parametrize("data", R.DATA)
@pytest.mark.parametrize("form", ["edge", "long"])
def test_decode_attention_f32_long_fallback(cuda, form, data):
    """The f32 fallback kernels at the threshold between them (small_attn off, 4 heads): "edge" =
    decode_attn4_kernel<float> at its largest Lmax 512 (136,768 B of dynamic LDS) and positions
    {0, 254, 255, 256, 257, 511}, both sides of the stride of its 256-thread score loop; "long" =
    decode_attn_kernel<float> at Lmax 520 and positions {0, 63, 64, 511, 512, 513, 519}: its
    64-thread score loop takes up to nine strides.
    Measured on an MI355X: Lmax 520 error 3.82e-07 .. 1.22e-04 at yardsticks 2.08e-07 .. 6.64e-05,
    closest "hot": 5.613e-06 at 2.103e-06 (tolerance 9.413e-06); Lmax 512 (the launch succeeds)
    error 1.01e-07 .. 1.03e-04 at yardsticks 2.03e-07 .. 3.60e-05, closest "rising": 1.030e-04 at
    3.603e-05 (tolerance 1.451e-04)."""
    with knobs(small_attn=0):
        _decode(cuda, "decode[f32-h4-fallback-Lmax%d-%s]" % (R.decode_case(data, F32, 4, form)["Lmax"], data),
                data, F32, 4, form)


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("form", ["beam40", "beam10"])
def test_decode_attention_beam_rows(cuda, form, dt):
    """The beam form: 40 rows = 8 clips x 5 beams (beam_xcd at its default 5: the XCD row
    permutation, checked against float64) and 10 rows (the ungrouped path); a clip's beams share
    a position of {16, 31, 32, 33, 64, 65, 128, 135} and kvrow stays within the clip.  12 and 5
    heads, the default plan and the large-R plan, "flat" and "rising".
    Measured on an MI355X: f32 error 1.88e-07 .. 4.22e-05 at yardsticks 3.07e-07 .. 1.86e-05, closest
    decode_attn4_kernel, 5 heads, 10 rows, "rising": 1.157e-05 at 3.158e-06 (tolerance
    1.363e-05); bf16 error = yardstick (3.52e-03 .. 7.77e-03), a fifth of the tolerance."""
    for heads in (12, 5):
        for small in (1, 0):
            with knobs(small_attn=small):
                for data in ("flat", "rising"):
                    plan = _plan_name(dt, heads, small, 3, 6)
                    _decode(cuda, "decode[%s-h%d-%s-%s-%s]" % (_name(dt), heads, plan, form, data),
                            data, dt, heads, form)


@pytest.mark.parametrize("da5", [6, 4, 3, 2])
def test_decode_attention_map(cuda, da5):
    """zs_decode_attention_map for every decode_attn5 value: 24 physical rows of 6 heads, the
    active subset 1, 4, ..., 22 at positions {0, 16, 17, 32, 64, 65, 128, 135} followed by three
    padding slots (rowmap >= nphys) whose qkv rows hold NaN; without cpos, and with cpos while
    ``pos`` holds other positions.  Outputs equal the float64 reference of the physical rows,
    padding rows are zero, idle physical rows are bit-unchanged.
    Measured on an MI355X: error = yardstick = 3.815e-03 for every knob value, with and without
    cpos (tolerance 2.832e-02)."""
    H = R.MAP_HEADS
    for with_cpos in (False, True):
        m = R.map_case(with_cpos)
        c = m["c"]
        a = (m["qkv_c"], m["Rb"], c["D"], H, c["kc"], c["vc"], c["Lmax"], m["pos"], None,
             m["rowmap"], m["cpos"], R.MAP_NPHYS)
        o64, k1, v1 = R.decode_attention(*a)
        o32, _, _ = R.decode_attention(*a, dtype=F32, round_to=BF16)
        qd, pd, rd = m["qkv_c"].to(cuda), m["pos"].to(cuda), m["rowmap"].to(cuda)
        cd = m["cpos"].to(cuda) if with_cpos else None
        kc = Out(cuda, tuple(c["kc"].shape), BF16, SENT, init=c["kc"])
        vc = Out(cuda, tuple(c["vc"].shape), BF16, SENT, init=c["vc"])
        out = Out(cuda, (m["Rb"], c["D"]), BF16, SENT)
        with knobs(decode_attn5=da5):
            _call("zs_decode_attention_map", qd.data_ptr(), m["Rb"], rd.data_ptr(), R.MAP_NPHYS,
                  c["D"], H, kc.t.data_ptr(), vc.t.data_ptr(), c["Lmax"], pd.data_ptr(), _ptr(cd),
                  out.t.data_ptr(), _code(BF16))
            torch.cuda.synchronize()
        got = out.cpu().float()
        na = len(R.MAP_ACTIVE)
        assert bool((got[na:] == 0).all()) and bool(torch.isfinite(got).all())
        gk, gv = kc.cpu(), vc.cpu()
        assert _same_bits(gk, k1) and _same_bits(gv, v1)
        idle = [r for r in range(R.MAP_NPHYS) if r not in R.MAP_ACTIVE]
        assert _same_bits(gk[idle], c["kc"][idle]) and _same_bits(gv[idle], c["vc"][idle])
        _check("decode_map[da5 %d-cpos%d]" % (da5, with_cpos), got, o64, o32, True)


# ------------------------------------------------------------------ row attention
def _kv_views(c, cuda):
    """q, k, v on the device such that k and v are views of ONE device buffer (as on the CPU)."""
    if c["q"]._base is not None and c["q"]._base is c["k"]._base:
        buf = c["q"]._base.to(cuda)
        E = c["E"]
        return buf[:, :E], buf[:, E:2 * E], buf[:, 2 * E:]
    kv = c["k"]._base.to(cuda)
    return c["q"].to(cuda), kv[:, :c["E"]], kv[:, c["E"]:]


def _row(cuda, tag, c, causal, dt, p_round=None):
    B, L, H, hd, E = c["B"], c["L"], c["heads"], c["hd"], c["E"]
    qd, kd, vd = _kv_views(c, cuda)
    ld = c["lens"].to(cuda)
    o, view = _padded(cuda, B * L, E, c["ldo"], dt)
    _call("zs_row_attention", qd.data_ptr(), c["ldq"], kd.data_ptr(), vd.data_ptr(), c["ldkv"], B,
          L, ld.data_ptr(), H, hd, int(causal), c["scale"], view.data_ptr(), c["ldo"], _code(dt))
    torch.cuda.synchronize()
    kept, got = _padding_kept(o, E)
    assert kept, tag
    a = (c["q"], c["ldq"], c["k"], c["v"], c["ldkv"], B, L, c["lens"], H, hd, causal, c["scale"])
    r64 = R.row_attention(*a, p_round=p_round)
    r32 = R.row_attention(*a, p_round=p_round, dtype=F32, round_to=_rt(dt))
    i = torch.arange(L)[None]
    ok = (i < (c["lens"].long()[:, None] if causal else torch.full((B, 1), L))).reshape(-1)
    assert bool(torch.isfinite(got.float()).all()), tag
    _check(tag, got.float()[ok], r64[ok], r32[ok], dt == BF16)


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hd,L", [(hd, L) for hd in (64, 96) for L in R.ROW_L[hd]])
def test_row_attention_scalar(cuda, hd, L, causal, dt):
    """The scalar row_attn_kernel (row_mfma 0 forces bf16 onto it too): hd 64 at L {1, 27, 64,
    65, 130, 256} and hd 96 at L {20, 65} -- one and more than one 64-query block, and at L 130 /
    256 (hd 64) 66,560 B / 131,072 B of dynamic LDS, past the 64 KiB a kernel gets by default.
    lens {L, L - 5, 3, 1}; k / v rows j >= lens[b] hold +-1e4; q / k / v as the column blocks of
    one packed buffer and as separate buffers; ldo = E + 8 with a sentinel between the rows.
    Rows i < lens[b] are compared when causal, all rows when not.
    Measured on an MI355X: every launch succeeds, L 130 and 256 included; f32 error at most
    1.13e-06 at yardsticks up to 9.29e-07, closest hd 64, L 130, not causal, packed: 1.125e-06
    at 5.991e-07 (tolerance 3.396e-06); bf16 error = yardstick, at most 7.81e-03, a fifth of the
    tolerance."""
    H = R.ROW_HEADS[hd]
    with knobs(row_mfma=0):
        for packed in (True, False):
            c = R.row_case("flat", dt, hd, H, 4, L, packed)
            tag = "row_scalar[%s-hd%d-L%d-%s-%s]" % (_name(dt), hd, L, "causal" if causal else "full",
                                                    "packed" if packed else "separate")
            _row(cuda, tag, c, causal, dt)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("L", R.MFMA_L)
def test_row_attention_mfma(cuda, L, causal):
    """row_attn_mfma_kernel (bf16, hd 64, L <= 32) at L {1, 5, 16, 17, 27, 31, 32}, B 5, 12
    heads, lens {L, L - 5, 3, 1, L}, packed and separate buffers; the reference rounds the
    unnormalised probabilities to bf16 before P.V as the kernel does.  With ldo % 4 != 0 the call
    falls back to the scalar kernel and is compared with the unrounded reference.
    Measured on an MI355X: error = yardstick in every case, at most 7.80e-03 (MFMA) and 7.81e-03
    (ldo % 4 != 0, scalar): a fifth of the tolerance; __expf does not show beside the rounding of
    the output."""
    for packed in (True, False):
        c = R.row_case("flat", BF16, 64, 12, 5, L, packed)
        tag = "row_mfma[L%d-%s-%s]" % (L, "causal" if causal else "full", "packed" if packed else "separate")
        _row(cuda, tag, c, causal, BF16, p_round=BF16)
    c = dict(R.row_case("flat", BF16, 64, 12, 5, L, True))
    c["ldo"] = c["E"] + 2
    _row(cuda, "row_mfma_ldo2_scalar[L%d-%s]" % (L, "causal" if causal else "full"), c, causal, BF16)


@pytest.mark.parametrize("row_stride", [1, 5])
@pytest.mark.parametrize("L", R.MFMA_L)
def test_row_attention_kv(cuda, L, row_stride):
    """zs_row_attention_kv: the causal MFMA attention of a packed qkv plus the cache write, Lmax =
    L + 3, row_stride 1 and 5: the attention rows against float64, all L rows of k / v (rows past
    lens[b] included) in the cache bit for bit as attn_ref.kv_write puts them, every other slot
    keeps its sentinel.
    Measured on an MI355X: error = yardstick, at most 7.70e-03, a fifth of the tolerance."""
    B, H, Lmax = 5, 12, L + 3
    c = R.row_case("flat", BF16, 64, H, B, L, True)
    E = c["E"]
    qkv = c["q"]._base
    qd, ld = qkv.to(cuda), c["lens"].to(cuda)
    shape = (B * row_stride, H, Lmax, 64)
    kc, vc = Out(cuda, shape, BF16, SENT), Out(cuda, shape, BF16, SENT)
    o, view = _padded(cuda, B * L, E, E + 8, BF16)
    _call("zs_row_attention_kv", qd.data_ptr(), B, L, ld.data_ptr(), H, 0.125, view.data_ptr(),
          E + 8, kc.t.data_ptr(), vc.t.data_ptr(), Lmax, row_stride)
    torch.cuda.synchronize()
    kept, got = _padding_kept(o, E)
    assert kept
    z = torch.full(shape, SENT, dtype=BF16)
    k1, v1 = R.kv_write(qkv, B, L, E, H, None, row_stride, z, z)
    assert _same_bits(kc.cpu(), k1) and _same_bits(vc.cpu(), v1)
    a = (c["q"], c["ldq"], c["k"], c["v"], c["ldkv"], B, L, c["lens"], H, 64, True, 0.125)
    ok = (torch.arange(L)[None] < c["lens"].long()[:, None]).reshape(-1)
    r64 = R.row_attention(*a, p_round=BF16)
    r32 = R.row_attention(*a, p_round=BF16, dtype=F32, round_to=BF16)
    _check("row_kv[L%d-stride%d]" % (L, row_stride), got.float()[ok], r64[ok], r32[ok], True)


def test_row_attention_refusals(cuda):
    """Outside the contract: L = 33, ldo % 4 != 0 and a qkv pointer off 16 bytes for
    zs_row_attention_kv; L past the bound, an unsupported head dim and more LDS than a workgroup
    can have for zs_row_attention.  An error code, nothing written."""
    from zsaac._lib import ZsError
    buf = torch.zeros(1 << 16, device=cuda, dtype=BF16)
    out = torch.zeros(1 << 16, device=cuda, dtype=BF16)
    lens = torch.ones(4, dtype=I32, device=cuda)
    p, o, l = buf.data_ptr(), out.data_ptr(), lens.data_ptr()
    bad = [("zs_row_attention_kv", p, 1, 33, l, 2, 0.125, o, 128, o, o, 40, 1),
           ("zs_row_attention_kv", p, 1, 8, l, 2, 0.125, o, 130, o, o, 40, 1),
           ("zs_row_attention_kv", p + 2, 1, 8, l, 2, 0.125, o, 128, o, o, 40, 1),
           ("zs_row_attention", p, 64, p, p, 64, 1, 257, l, 1, 64, 1, 0.125, o, 64, _code(BF16)),
           ("zs_row_attention", p, 96, p, p, 96, 1, 256, l, 1, 96, 1, 0.125, o, 96, _code(BF16))]
    for args in bad:
        with pytest.raises(ZsError, match=r"failed \(-1\)"):
            _call(*args)
    with pytest.raises(ZsError):
        _call("zs_row_attention", p, 32, p, p, 32, 1, 8, l, 1, 32, 1, 0.125, o, 32, _code(BF16))
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ------------------------------------------------------------------ cache write
@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("given,n,row_stride", R.KVW_CASES)
def test_kv_write(cuda, given, n, row_stride, dt):
    """zs_kv_write: pos0 NULL and {0, 5, Lmax - n}, n 1 and 3, row_stride 1 and 5, 3 rows of 3
    heads (R n D is no multiple of the 256-thread block): bit-equal to attn_ref.kv_write, every
    other slot keeps the sentinel."""
    c = R.kvw_case(dt, given, n, row_stride)
    qd = c["qkv"].to(cuda)
    pd = c["pos0"].to(cuda) if given else None
    kc, vc = Out(cuda, c["shape"], dt, SENT), Out(cuda, c["shape"], dt, SENT)
    _call("zs_kv_write", qd.data_ptr(), R.KVW_R, n, c["D"], R.KVW_HEADS, _ptr(pd), row_stride,
          kc.t.data_ptr(), vc.t.data_ptr(), R.KVW_LMAX, _code(dt))
    torch.cuda.synchronize()
    z = torch.full(c["shape"], SENT).to(dt)
    k1, v1 = R.kv_write(c["qkv"], R.KVW_R, n, c["D"], R.KVW_HEADS, c["pos0"], row_stride, z, z)
    assert int((k1 != SENT).sum()) == R.KVW_R * n * c["D"]
    assert _same_bits(kc.cpu(), k1) and _same_bits(vc.cpu(), v1)


# ------------------------------------------------------------------ cross attention
@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("hd", R.CROSS_HD)
def test_cross_attention(cuda, hd, dt):
    """zs_cross_attention, 4 heads of hd {256, 100, 64, 24} (four, two, one and a partial round of
    the 64 lanes), B {1, 3}, Lq {1, 2}, Lk {1, 3, 5, 64}; k / v the two halves of one [B Lk][2E]
    buffer, ldq = ldo = E + 8 (NaN / a sentinel between the rows); "flat" and "hot" data.
    Measured on an MI355X: f32 error at most 9.77e-06 at yardsticks up to 6.28e-05 ("hot": scores
    of 92 carry an absolute float32 error of 1e-5), closest hd 256, B 1, Lq 1, Lk 3, "hot":
    7.944e-06 at 5.411e-06 (tolerance 2.265e-05); bf16 error = yardstick, at most 7.75e-03, a
    fifth of the tolerance."""
    H = R.CROSS_HEADS
    for data in ("flat", "hot"):
        for B, Lq, Lk in R.CROSS_SHAPES:
            c = R.cross_case(data, dt, hd, B, Lq, Lk)
            E = c["E"]
            qb, kv = c["q"]._base.to(cuda), c["k"]._base.to(cuda)
            o, view = _padded(cuda, B * Lq, E, c["ldo"], dt)
            _call("zs_cross_attention", qb.data_ptr(), c["ldq"], kv.data_ptr(),
                  kv[:, E:].data_ptr(), c["ldkv"], B, Lq, Lk, H, hd, c["scale"], view.data_ptr(),
                  c["ldo"], _code(dt))
            torch.cuda.synchronize()
            kept, got = _padding_kept(o, E)
            tag = "cross[%s-hd%d-B%d-Lq%d-Lk%d-%s]" % (_name(dt), hd, B, Lq, Lk, data)
            assert kept and bool(torch.isfinite(got.float()).all()), tag
            a = (c["q"], c["ldq"], c["k"], c["v"], c["ldkv"], B, Lq, Lk, H, hd, c["scale"])
            _check(tag, got.float(), R.cross_attention(*a),
                   R.cross_attention(*a, dtype=F32, round_to=_rt(dt)), dt == BF16)


def test_cross_attention_refusals(cuda):
    """Lk = 65 and hd = 257 are refused (an error code, nothing written)."""
    from zsaac._lib import ZsError
    buf = torch.zeros(1 << 16, device=cuda)
    out = torch.zeros(1 << 12, device=cuda)
    p, o = buf.data_ptr(), out.data_ptr()
    for Lk, hd in ((65, 64), (5, 257)):
        with pytest.raises(ZsError, match=r"failed \(-1\)"):
            _call("zs_cross_attention", p, hd, p, p, hd, 1, 1, Lk, 1, hd, 0.125, o, hd, _code(F32))
    torch.cuda.synchronize()
    assert bool((out == 0).all())
