"""tests/attn_ref.py on the CPU: each reference against an independent formulation
(torch's scaled_dot_product_attention in float64 with an explicit mask, nn.MultiheadAttention
with identity projections, oracle/caption.py's GPT-2 attention lines, decode against prefill),
the input conditions the GPU cases of tests/test_gpu_attn_kernels.py rely on, and every mutant of
attn_ref.MUTANTS told from the float64 reference by more than twice the tolerance of each GPU
case meant to catch it."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

F64, F32, BF16, I32 = R.F64, R.F32, R.BF16, R.I32
DTS = [F32, BF16]


def _rt(dt):
    return None if dt == F32 else dt


# ------------------------------------------------------------------ ties
def test_knob_defaults_match_the_source():
    """attn_ref.KNOB_DEFAULTS (what the GPU tests restore to) against attn.hip's initialisers."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "zero-shot-aac_amd", "csrc", "attn.hip")
    text = open(path).read()
    for k, v in R.KNOB_DEFAULTS.items():
        m = re.search(r"^int g_%s = (\d+);" % k, text, re.M)
        assert m and int(m.group(1)) == v, k


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hd,L", [(64, 27), (96, 20), (64, 65)])
def test_row_attention_equals_sdpa(hd, L, causal):
    """row_attention == F.scaled_dot_product_attention in float64 with the explicit mask
    (key < lens[b], key <= query when causal), at the oracle's prefill shape (hd 64, L 27), the
    mapper's (hd 96, L 20) and past one 64-query block."""
    H, B = R.ROW_HEADS[hd], 4
    c = R.row_case("flat", F32, hd, H, B, L, True)
    got = R.row_attention(c["q"], c["ldq"], c["k"], c["v"], c["ldkv"], B, L, c["lens"], H, hd,
                          causal, c["scale"])
    qh, kh, vh = (t.double().reshape(B, L, H, hd).transpose(1, 2) for t in (c["q"], c["k"], c["v"]))
    j = torch.arange(L)
    mask = (j[None, None] < c["lens"][:, None, None]).expand(B, L, L).clone()
    if causal:
        mask &= j[None, None, :] <= j[None, :, None]
    ref = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask[:, None], scale=c["scale"])
    ref = ref.transpose(1, 2).reshape(B * L, H * hd)
    assert float((got - ref).abs().max()) < 1e-12


def test_row_attention_equals_oracle_gpt2_lines():
    """The causal prefill form against oracle/caption.py's gpt2_hidden attention lines (scores
    masked with finfo.min under tril, softmax, att @ v) on the oracle's shape: 12 heads of 64."""
    B, L, H, hd = 2, 27, 12, 64
    c = R.row_case("flat", F32, hd, H, B, L, True)
    got = R.row_attention(c["q"], c["ldq"], c["k"], c["v"], c["ldkv"], B, L, None, H, hd, True, 0.125)
    q, k, v = (t.double().reshape(B, L, H, hd).transpose(1, 2) for t in (c["q"], c["k"], c["v"]))
    att = (q @ k.transpose(-1, -2)) * (hd ** -0.5)
    causal = torch.ones(L, L, dtype=torch.bool).tril(0)
    att = att.masked_fill(~causal, torch.finfo(att.dtype).min).softmax(-1)
    ref = (att @ v).transpose(1, 2).reshape(B * L, H * hd)
    assert float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max()) < 1e-12   # v rows of 1e4


def test_decode_equals_prefill_row():
    """kv_write of tokens 0..n-1, then decode_attention of token n == row n of the causal
    prefill over n + 1 tokens (the oracle's use_cache step against its full recompute)."""
    Rw, H, Lmax, n = 3, 12, 40, 17
    D = 64 * H
    g = R.gen("prefill")
    qkv = torch.randn(Rw * (n + 1), 3 * D, generator=g)
    first = qkv.view(Rw, n + 1, 3 * D)[:, :n].reshape(-1, 3 * D)
    z = torch.full((Rw, H, Lmax, 64), R.NAN)
    kc, vc = R.kv_write(first, Rw, n, D, H, None, 1, z, z)
    last = qkv.view(Rw, n + 1, 3 * D)[:, n].contiguous()
    pos = torch.full((Rw,), n, dtype=I32)
    out, kc2, vc2 = R.decode_attention(last, Rw, D, H, kc, vc, Lmax, pos)
    ref = R.row_attention(qkv[:, :D], 3 * D, qkv[:, D:2 * D], qkv[:, 2 * D:], 3 * D, Rw, n + 1,
                          None, H, 64, True, 0.125)
    assert float((out - ref.view(Rw, n + 1, D)[:, n]).abs().max()) < 1e-12
    assert torch.equal(kc2[:, :, n], last[:, D:2 * D].view(Rw, H, 64))
    assert bool(torch.isnan(kc2[:, :, n + 1:]).all())


@pytest.mark.parametrize("form", ["ragged", "beam40"])
def test_decode_equals_sdpa(form):
    """decode_attention per row == scaled_dot_product_attention over the gathered keys."""
    c = R.decode_case("flat", F32, 6, form)
    out, _, _ = R.decode_attention(c["qkv"], c["R"], c["D"], 6, c["kc"], c["vc"], c["Lmax"],
                                   c["pos"], c["kvrow"])
    D = c["D"]
    x = c["qkv"].double()
    for r in range(c["R"]):
        p = int(c["pos"][r])
        K = torch.empty(6, p + 1, 64, dtype=F64)
        V = torch.empty(6, p + 1, 64, dtype=F64)
        for j in range(p):
            s = int(c["kvrow"][r, j]) if c["kvrow"] is not None else r
            K[:, j], V[:, j] = c["kc"][s, :, j].double(), c["vc"][s, :, j].double()
        K[:, p], V[:, p] = x[r, D:2 * D].view(6, 64), x[r, 2 * D:].view(6, 64)
        ref = F.scaled_dot_product_attention(x[r, :D].view(6, 1, 64), K, V, scale=0.125)
        assert float((out[r] - ref.reshape(-1)).abs().max()) < 1e-12, r


@pytest.mark.parametrize("hd", R.CROSS_HD)
def test_cross_attention_equals_multihead_attention(hd):
    """cross_attention == nn.MultiheadAttention (float64, identity projections, no bias)."""
    B, Lq, Lk, H = 3, 2, 5, R.CROSS_HEADS
    c = R.cross_case("flat", F32, hd, B, Lq, Lk)
    E = c["E"]
    got = R.cross_attention(c["q"], c["ldq"], c["k"], c["v"], c["ldkv"], B, Lq, Lk, H, hd, c["scale"])
    mha = torch.nn.MultiheadAttention(E, H, bias=False, batch_first=True, dtype=F64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(E, dtype=F64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(E, dtype=F64))
        ref, _ = mha(c["q"].double().reshape(B, Lq, E), c["k"].double().reshape(B, Lk, E),
                     c["v"].double().reshape(B, Lk, E), need_weights=False)
    assert float((got - ref.reshape(B * Lq, E)).abs().max()) < 1e-12


# ------------------------------------------------------------------ input conditions
def test_position_lists_hold_the_boundaries():
    """Key counts (p + 1) on both sides of every phase length and of every SPLIT round."""
    keys = {p + 1 for p in R.DEC_POS}
    for n in R.PHASES + [k * s for k, s in R.SPLITS]:
        assert {n, n + 1} <= keys, n
    assert {1, 2, R.DEC_LMAX} <= keys
    assert {p + 1 for p in R.LONG_POS} >= {1, 64, 65, 512, 513, 514, R.LONG_LMAX}
    assert {p + 1 for p in R.EDGE_POS} >= {1, 256, 257, R.EDGE_LMAX} and R.EDGE_LMAX == 512
    assert set(R.BEAM_POS) & {31, 32, 64, 128} and set(R.MAP_POS) >= {0, 16, 32, 64, 128, 135}
    for form, n in (("ragged", len(R.DEC_POS)), ("beam40", 40), ("beam10", 10), ("long", 7)):
        c = R.decode_case("flat", BF16, 12, form)
        assert c["R"] == n and (form == "beam10" or int(c["pos"].max()) == c["Lmax"] - 1)
    assert 40 % (8 * R.KNOB_DEFAULTS["beam_xcd"]) == 0 and 10 % (8 * R.KNOB_DEFAULTS["beam_xcd"])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("heads", R.DEC_HEADS)
def test_rising_maximum_rises_in_every_phase(heads, dt):
    """"rising": for every row, head and phase length, the maximum of every phase exceeds that of
    the phase before by more than 0.25 -- the rescale of the online softmax carries the result."""
    for form in ("ragged", "beam40"):
        for sc in R.decode_scores(R.decode_case("rising", dt, heads, form)):
            for kpp in R.PHASES:
                mx = torch.stack([sc[:, b:b + kpp].max(-1).values for b in range(0, sc.shape[1], kpp)])
                if mx.shape[0] > 1:
                    assert float((mx[1:] - mx[:-1]).min()) > 0.25, (form, kpp)


@pytest.mark.parametrize("dt", DTS)
def test_hot_scores_overflow_float32(dt):
    """"hot": every score's exp overflows float32 without the max subtraction (decode, row and
    cross attention cases), while the spread within a row stays below 20."""
    big = float(torch.finfo(F32).max)
    for heads in R.DEC_HEADS:
        for sc in R.decode_scores(R.decode_case("hot", dt, heads)):
            assert float(torch.exp(sc).min()) > big and float(sc.max() - sc.min()) < 20
    for hd in R.CROSS_HD:
        c = R.cross_case("hot", dt, hd, 3, 2, 64)
        sc = (c["q"].double().reshape(6, 4, hd)[:3, :, None] * c["k"].double().reshape(3, 64, 4, hd)
              .transpose(1, 2)[:, :, :]).sum(-1) * c["scale"]
        assert float(torch.exp(sc).min()) > big


def test_kvrow_never_reads_an_appended_slot():
    """No kvrow entry j < p points at a slot (row, pos[row]) appended in the same call, every
    entry is a valid row, and a beam's sources stay within its clip."""
    for form in ("beam40", "beam10"):
        c = R.decode_case("flat", BF16, 12, form)
        kv, pos = c["kvrow"].long(), c["pos"].long()
        assert int(kv.min()) >= 0 and int(kv.max()) < c["R"]
        assert bool((kv // 5 == (torch.arange(c["R"]) // 5)[:, None]).all())
        j = torch.arange(c["Lmax"])[None]
        live = j < pos[:, None]
        assert not bool((live & (pos[kv] == j)).any())
        assert bool((kv != torch.arange(c["R"])[:, None])[live].any())


def test_cache_slots_from_pos_on_hold_nan():
    for form in ("ragged", "beam40", "map", "long", "edge"):
        c = R.decode_case("flat", F32, 6, form)
        for r in range(c["R"]):
            p = int(c["pos"][r])
            assert bool(torch.isnan(c["kc"][r, :, p:]).all()) and bool(torch.isnan(c["vc"][r, :, p:]).all())
            assert bool(torch.isfinite(c["kc"][r, :, :p]).all())


# ------------------------------------------------------------------ the mutants
def _caught(ref, mut, tol):
    """Some element of the mutant is further than 2 x tolerance from the reference (or not
    finite)."""
    return not bool(((mut - ref).abs() <= 2.0 * tol).all())


def _decode_refs(data, dt, heads, form):
    c = R.decode_case(data, dt, heads, form)
    a = (c["qkv"], c["R"], c["D"], heads, c["kc"], c["vc"], c["Lmax"], c["pos"], c["kvrow"])
    o64, _, _ = R.decode_attention(*a)
    o32, _, _ = R.decode_attention(*a, dtype=F32, round_to=_rt(dt))
    return a, o64, R.tolerance(o64, o32, dt == BF16)[1]


DECODE_MUTANTS = ([(m, d, "ragged") for m in ("strict", "stale_new", "clamp_dup", "scale1", "head_shift")
                   for d in R.DATA] +
                  [(m, "flat", f) for m in ("strict", "stale_new", "clamp_dup") for f in ("long", "edge")] +
                  [("no_rescale:%d" % k, "rising", f) for k in R.PHASES for f in ("ragged", "beam40")] +
                  [("drop_slice:%d:%d" % ks, d, "ragged") for ks in R.SPLITS for d in ("flat", "hot")] +
                  [(m, d, f) for m in ("kvrow_self", "kvrow_row0") for d in R.DATA
                   for f in ("beam40", "beam10")])


@pytest.mark.parametrize("mut,data,form,dt", [(m, d, f, dt) for m, d, f in DECODE_MUTANTS for dt in DTS
                                              if f not in ("long", "edge") or dt == F32])   # f32 only
def test_decode_mutants_are_caught(mut, data, form, dt):
    for heads in ([4] if form in ("long", "edge") else R.DEC_HEADS):
        a, o64, tol = _decode_refs(data, dt, heads, form)
        m64, _, _ = R.decode_attention(*a, mut=mut)
        assert _caught(o64, m64, tol), (mut, data, form, heads)


def test_map_mutants_are_caught():
    for with_cpos in (False, True):
        m = R.map_case(with_cpos)
        c = m["c"]
        a = (m["qkv_c"], m["Rb"], c["D"], R.MAP_HEADS, c["kc"], c["vc"], c["Lmax"], m["pos"], None,
             m["rowmap"], m["cpos"], R.MAP_NPHYS)
        o64, _, _ = R.decode_attention(*a)
        o32, _, _ = R.decode_attention(*a, dtype=F32, round_to=BF16)
        tol = R.tolerance(o64, o32, True)[1]
        assert bool(torch.isfinite(o64).all()) and bool((o64[len(R.MAP_ACTIVE):] == 0).all())
        for mut in ("strict", "stale_new", "clamp_dup", "scale1", "head_shift"):
            assert _caught(o64, R.decode_attention(*a, mut=mut)[0], tol), mut
        if with_cpos:          # positions taken from pos although cpos is given
            b = a[:10] + (None,) + a[11:]
            assert _caught(o64, R.decode_attention(*b)[0].nan_to_num(nan=1e9), tol)


def _row_args(c, causal):
    return (c["q"], c["ldq"], c["k"], c["v"], c["ldkv"], c["B"], c["L"], c["lens"], c["heads"],
            c["hd"], causal, c["scale"])


def _valid_rows(c, causal):
    i = torch.arange(c["L"])[None]
    n = c["lens"].long()[:, None] if causal else torch.full((c["B"], 1), c["L"])
    return (i < n).reshape(-1)


# (len_ignored cannot show in the causal rows i < lens[b], the only ones compared there)
ROW_MUTANTS = [("noncausal", True), ("causal_strict", True), ("len_ignored", False), ("scale1", True), ("scale1", False), ("head_shift", True),
               ("head_shift", False)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mut,causal", ROW_MUTANTS)
def test_row_mutants_are_caught(mut, causal, dt):
    """On the scalar kernel's cases (every hd and L but L = 1, where nothing can be masked) and
    the MFMA kernel's (bf16, p rounded to bf16)."""
    cases = [(hd, R.ROW_HEADS[hd], 4, L, None) for hd in (64, 96) for L in R.ROW_L[hd] if L < 256]
    if dt == BF16:
        cases += [(64, 12, 5, L, BF16) for L in R.MFMA_L]
    for hd, H, B, L, pr in cases:
        if L == 1 or (L <= 5 and mut == "len_ignored"):
            continue
        for packed in (True, False):
            c = R.row_case("flat", dt, hd, H, B, L, packed)
            a = _row_args(c, causal)
            r64 = R.row_attention(*a, p_round=pr)
            r32 = R.row_attention(*a, p_round=pr, dtype=F32, round_to=_rt(dt))
            ok = _valid_rows(c, causal)
            tol = R.tolerance(r64[ok], r32[ok], dt == BF16)[1]
            assert bool(torch.isfinite(r64[ok]).all())
            assert _caught(r64[ok], R.row_attention(*a, p_round=pr, mut=mut)[ok], tol), (hd, L, packed)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("data", ["flat", "hot"])
def test_cross_mutants_are_caught(data, dt):
    """batch0_keys on every B = 3 case with more than one key, hd_trunc on hd 100 and 24 (more
    than one key), scale1 on every case with more than one key."""
    for hd in R.CROSS_HD:
        for B, Lq, Lk in R.CROSS_SHAPES:
            if Lk == 1:
                continue
            c = R.cross_case(data, dt, hd, B, Lq, Lk)
            a = (c["q"], c["ldq"], c["k"], c["v"], c["ldkv"], B, Lq, Lk, R.CROSS_HEADS, hd, c["scale"])
            r64 = R.cross_attention(*a)
            tol = R.tolerance(r64, R.cross_attention(*a, dtype=F32, round_to=_rt(dt)), dt == BF16)[1]
            muts = ["scale1"] if data == "flat" else []
            muts += ["batch0_keys"] if B == 3 else []
            muts += ["hd_trunc"] if hd % 64 else []
            for mut in muts:
                assert _caught(r64, R.cross_attention(*a, mut=mut), tol), (mut, hd, B, Lq, Lk)


def test_every_mutant_has_a_case():
    used = {m.split(":")[0] for m, _, _ in DECODE_MUTANTS} | {m for m, _ in ROW_MUTANTS}
    used |= {"batch0_keys", "hd_trunc"}
    assert used == set(R.MUTANTS)
