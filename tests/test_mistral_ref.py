"""CPU tests that pin tests/mistral_ref.py, the reference the Mistral kernel GPU tests compare
against: one decoder layer composed from its functions against oracle/mistral.py (prefill and a
decode step with past, in float64), the glu column formula against zsaac.mistral.glu_interleave,
embed against clap_to_gpt's concatenation; the input conditions of every case of
tests/test_gpu_mistral_kernels.py, so a bad seed or an edited list fails here and not on the GPU;
and, for each arithmetic error listed in mistral_ref.MUTANTS, that the inputs of a GPU case move
the expected output by more than twice that case's tolerance (a kernel with that error is then
more than one tolerance away from the reference, whatever its own rounding)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mistral_ref as R  # noqa: E402
from oracle import mistral as OM  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


# ------------------------------------------------------------------ one layer against the oracle
def _weights(H, KVH, F, seed):
    g = R.gen(seed)
    D = H * R.HD
    p = "model.layers.0."

    def mat(n, k):
        return torch.randn(n, k, generator=g, dtype=F64) / k ** 0.5

    def vec():
        return torch.randn(D, generator=g, dtype=F64) * 0.5 + 1.0

    return {p + "self_attn.q_proj.weight": mat(D, D),
            p + "self_attn.k_proj.weight": mat(KVH * R.HD, D),
            p + "self_attn.v_proj.weight": mat(KVH * R.HD, D),
            p + "self_attn.o_proj.weight": mat(D, D),
            p + "input_layernorm.weight": vec(), p + "post_attention_layernorm.weight": vec(),
            p + "mlp.gate_proj.weight": mat(F, D), p + "mlp.up_proj.weight": mat(F, D),
            p + "mlp.down_proj.weight": mat(D, F), "model.norm.weight": vec()}


def _layer(x, sd, H, KVH, pos, rps, kc, vc, decode):
    """One decoder layer + the final norm from the mistral_ref ops; plain @ for the projections,
    one slab each."""
    from zsaac.mistral import glu_interleave
    p = "model.layers.0."
    M, D = x.shape
    F = sd[p + "mlp.gate_proj.weight"].shape[0]
    cos, sin = R.rope_tables()
    x, h = R.add_rmsnorm(x, None, 0, 0, M, D, R.EPS, sd[p + "input_layernorm.weight"])
    wqkv = torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"])
    qkv = (h @ wqkv.t()).reshape(-1)
    if decode:
        att, kc, vc = R.decode_attention(qkv, 1, 0, M, H, KVH, pos, cos, sin, kc, vc)
    else:
        q, kc, vc = R.rope_kv(qkv, 1, 0, M, H, KVH, pos, rps, cos, sin, kc, vc)
        att = R.attention(q, M, H, KVH, pos, rps, kc, vc)
    y = (att @ sd[p + "self_attn.o_proj.weight"].t()).reshape(-1)
    x, h = R.add_rmsnorm(x, y, 1, M * D, M, D, R.EPS, sd[p + "post_attention_layernorm.weight"])
    wgu = glu_interleave(torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]]))
    act = R.silu_mul((h @ wgu.t()).reshape(-1), 1, M * 2 * F, M, F)
    y = (act @ sd[p + "mlp.down_proj.weight"].t()).reshape(-1)
    x, h = R.add_rmsnorm(x, y, 1, M * D, M, D, R.EPS, sd["model.norm.weight"])
    return h, kc, vc


@pytest.mark.parametrize("H,KVH", [(8, 2), (4, 4)])
def test_layer_matches_oracle(H, KVH):
    """Prefill (B = 2, P = 5, rows_per_seq = P), then a decode step with past at position P:
    fixes rotate_half, the [L][64] table form, the head mapping, the causal mask, the glu
    columns and the position the step's k / v are written to."""
    B, P, F = 2, 5, 64
    D = H * R.HD
    sd = _weights(H, KVH, F, seed=H)
    g = R.gen(1)
    x = torch.randn(B, P, D, generator=g, dtype=F64)
    ref, past = OM.forward(x, sd, H, KVH, R.EPS)
    kc = torch.full((B, KVH, R.LMAX, R.HD), R.NAN, dtype=F64)
    vc = kc.clone()
    pos = torch.arange(P, dtype=R.I32).repeat(B)
    h, kc, vc = _layer(x.view(B * P, D), sd, H, KVH, pos, P, kc, vc, decode=False)
    assert float((h.view(B, P, D) - ref).abs().max()) < 1e-11
    assert float((kc[:, :, :P] - past[0][0]).abs().max()) < 1e-12
    assert float((vc[:, :, :P] - past[0][1]).abs().max()) < 1e-12
    assert bool(torch.isnan(kc[:, :, P:]).all()) and bool(torch.isnan(vc[:, :, P:]).all())

    xn = torch.randn(B, 1, D, generator=g, dtype=F64)
    ref2, past2 = OM.forward(xn, sd, H, KVH, R.EPS, past, P)
    h2, kc2, vc2 = _layer(xn.view(B, D), sd, H, KVH, torch.full((B,), P, dtype=R.I32), 1, kc, vc,
                          decode=True)
    assert float((h2.view(B, 1, D) - ref2).abs().max()) < 1e-11
    assert float((kc2[:, :, :P + 1] - past2[0][0]).abs().max()) < 1e-12
    assert float((vc2[:, :, :P + 1] - past2[0][1]).abs().max()) < 1e-12
    assert bool(torch.isnan(kc2[:, :, P + 1:]).all())


@pytest.mark.parametrize("F", [8, 16, 1032])
def test_glu_cols_match_interleave(F):
    from zsaac.mistral import glu_interleave
    rows = glu_interleave(torch.arange(2 * F)[:, None]).view(-1)     # row r holds source row
    g, u = R.glu_cols(F)
    assert torch.equal(rows[g], torch.arange(F))
    assert torch.equal(rows[u], F + torch.arange(F))


def test_embed_matches_clap_to_gpt():
    D, B, ns = 8, 2, 2
    hard, _, tail, emb = R.embed_case((3, ns, 2), D, F32)
    g = R.gen(5)
    mlp = {"clap_project.model.0.weight": torch.randn(6, 4, generator=g),
           "clap_project.model.0.bias": torch.randn(6, generator=g),
           "clap_project.model.2.weight": torch.randn(ns * D, 6, generator=g),
           "clap_project.model.2.bias": torch.randn(ns * D, generator=g)}
    pe, soft = OM.clap_to_gpt(torch.randn(B, 4, generator=g), hard.long(), tail.long(),
                              {"model.embed_tokens.weight": emb}, mlp, prefix_length=ns)
    assert torch.equal(R.embed(hard, soft, tail, None, emb), pe.reshape(-1, D))
    tok = torch.tensor([0, R.EMBED_V - 1], dtype=R.I32)
    assert torch.equal(R.embed(None, None, None, tok, emb), emb[tok.long()])


# ------------------------------------------------------------------ input conditions of the GPU cases
@pytest.mark.parametrize("name", ["ROPE_POS", "ATT_POS", "DEC_POS"])
def test_pos_sets_straddle_the_key_steps(name):
    pos = getattr(R, name)
    assert min(pos) == 0 and max(pos) == R.LMAX - 1
    for edge in (32, 64):
        assert any(p < edge for p in pos) and any(p >= edge for p in pos), (name, edge)
    if name != "ROPE_POS":                    # key counts on both sides of a 32-key step
        assert 31 in pos and 32 in pos and 33 in pos and 64 in pos


@pytest.mark.parametrize("name", ["NORM_NSPLIT", "ADD_SS_NSPLIT", "SILU_NSPLIT", "DEC_NSPLIT"])
def test_nsplit_lists_reach_group_and_tail(name):
    """slab_sum4 sums slab 0, then groups of 4, then a tail of up to 3."""
    ns = getattr(R, name)
    assert any((n - 1) // 4 >= 1 and (n - 1) % 4 >= 1 for n in ns), name      # both in one call
    assert any((n - 1) // 4 >= 1 and (n - 1) % 4 == 0 for n in ns), name      # groups only


@pytest.mark.parametrize("M,F", R.SILU_SHAPES)
def test_silu_cases_hold_their_gates(M, F):
    assert (M * F // 4) % 256 != 0
    for ns in R.SILU_NSPLIT:
        gu, ss = R.silu_case(M, F, ns)
        s = R.slab_sum(gu, ns, ss, M * 2 * F).view(M, 2 * F)
        g, _ = R.glu_cols(F)
        got = s[0, g[:len(R.SILU_GATES)]].tolist()
        assert got == R.SILU_GATES
        assert max(got) > 80 and min(got) < -80 and 20.0 in got and -20.0 in got
        ref = R.silu_mul(gu, ns, ss, M, F)
        assert bool(torch.isfinite(ref).all())
        assert bool(torch.isfinite(R.silu_mul(gu, ns, ss, M, F, F32)).all())
        if ns > 1:
            assert bool(torch.isnan(gu[M * 2 * F:ss]).all())


@pytest.mark.parametrize("dt", [F32, BF16])
def test_online_case_raises_the_running_max(dt):
    c = R.att_case(4, 4, "online", dt)
    jump = R.step_max_jump(c["q"], c["kc"], c["pos"], 4, 4)
    assert float(jump.min()) > 20.0, jump
    assert R.ONLINE_KEY >= 32 and min(R.ONLINE_POS) > R.ONLINE_KEY


@pytest.mark.parametrize("H,KVH", R.HEADS)
def test_attention_cases_mask_with_nan(H, KVH):
    """Positions past a sequence's largest pos are NaN (a read past pos shows), everything a
    query may read is finite, and the reference output is finite."""
    for form in R.ATT_FORMS + (["online"] if H == KVH else []):
        c = R.att_case(H, KVH, form, BF16)
        S = c["kc"].shape[0]
        for s in range(S):
            last = int(c["pos"][s * c["rps"]:(s + 1) * c["rps"]].max())
            assert bool(torch.isfinite(c["kc"][s, :, :last + 1].float()).all())
            assert last == R.LMAX - 1 or bool(torch.isnan(c["vc"][s, :, last + 1:].float()).all())
        assert bool(torch.isfinite(R.attention(c["q"], c["M"], H, KVH, c["pos"], c["rps"],
                                               c["kc"], c["vc"])).all())
    c = R.dec_case(H, KVH, 5, F32)
    for m, p in enumerate(R.DEC_POS):
        assert bool(torch.isnan(c["kc"][m, :, p:]).all())
        assert bool(torch.isnan(c["vc"][m, :, p:]).all())
    assert (3 * 6) % 4 == 2                                 # (6, 1) at M = 3: two live waves


def test_residual_cases():
    for D in R.NORM_D:
        assert D % 4 == 0 and D <= 16384
    assert [-(-D // 4096) for D in R.NORM_D] == [1, 1, 1, 2, 2, 4]       # passes of 1024 x 4
    assert 4 < 4 * 1024 and 4100 - 4096 == 4                              # idle / one live thread
    c = R.residual_case(3, 1024, 5, 8)
    xn, _ = R.add_rmsnorm(c["x"], c["y"], 5, c["ss"], 3, 1024, R.EPS, None)
    ms = (xn * xn).mean(-1)
    assert float(ms[1]) < 0.01 * R.EPS and float(ms[0]) > 1.0            # eps decides row 1
    assert bool(torch.isnan(c["y"][3 * 1024:c["ss"]]).all())             # NaN between the slabs
    assert R.residual_case(3, 1024, 0, 0)["y"] is None
    for M, D in R.ADD_SS_SHAPES:
        assert D % 512 == 0 and M <= 32
    assert (32, 512) in R.ADD_SS_SHAPES and (32, 4096) in R.ADD_SS_SHAPES


# ------------------------------------------------------------------ the cases tell the mutants apart
def _caught(ref64, ref32, mut64, bf16):
    _, tol = R.tolerance(ref64, ref32, bf16)
    d = (mut64 - ref64).abs()
    return bool((~(d <= 2.0 * tol)).any())               # a NaN counts as caught


def _rt(dt):
    return None if dt == F32 else dt


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mut,H,KVH,form", [
    ("kvh_mod", 8, 2, "ragged9"), ("scale8", 8, 2, "ragged9"), ("scale8", 4, 4, "ragged9"),
    ("scale8", 6, 1, "ragged3"), ("strict", 8, 2, "prefill5"), ("strict", 4, 4, "prefill33"),
    ("seq_m", 8, 2, "prefill5"), ("seq_m", 6, 1, "prefill33")])
def test_attention_cases_catch(mut, H, KVH, form, dt):
    c = R.att_case(H, KVH, form, dt)
    M = 2 if mut == "seq_m" else c["M"]         # rows whose wrong sequence exists (in bounds)
    a = (c["q"][:M], M, H, KVH, c["pos"][:M], c["rps"], c["kc"], c["vc"])
    ref64, ref32 = R.attention(*a), R.attention(*a, dtype=F32, round_to=_rt(dt))
    assert _caught(ref64, ref32, R.attention(*a, mut=mut), dt == BF16)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mut,form", [("sin_sign", "ragged"), ("sin_sign", "prefill"),
                                      ("seq_m", "prefill")])
def test_rope_cases_catch(mut, form, dt):
    H, KVH = 8, 2
    M, pos, rps, S = R.rope_case(H, KVH, form)
    qkv, ss = R.qkv_case(M, H, KVH, 3)
    cos, sin = R.rope_tables()
    kc = torch.full((S, KVH, R.LMAX, R.HD), -7.0)
    a = (qkv, 3, ss, M, H, KVH, pos, rps, cos, sin, kc, kc)
    q64, k64, _ = R.rope_kv(*a)
    q32, k32, _ = R.rope_kv(*a, dtype=F32, round_to=_rt(dt))
    if mut == "seq_m":                           # rows 0, 1: the sequences that exist
        _, km, _ = R.rope_kv(qkv, 3, ss, 2, H, KVH, pos[:2], rps, cos, sin, kc, kc, mut=mut)
        assert _caught(k64[1, :, 1], k32[1, :, 1], km[1, :, 1], dt == BF16)
        assert not torch.equal(km[0, :, 1], k64[0, :, 1])
    else:
        qm, km, _ = R.rope_kv(*a, mut=mut)
        assert _caught(q64, q32, qm, dt == BF16)
        rows = (torch.arange(M) // rps, slice(None), pos.long())
        assert _caught(k64[rows], k32[rows], km[rows], dt == BF16)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mut,H,KVH,ns", [
    ("p_all", 8, 2, 1), ("p_all", 4, 4, 5), ("p_all", 6, 1, 6), ("no_tail", 8, 2, 6),
    ("sin_sign", 4, 4, 1), ("kvh_mod", 8, 2, 5), ("scale8", 6, 1, 1)])
def test_decode_cases_catch(mut, H, KVH, ns, dt):
    c = R.dec_case(H, KVH, ns, dt)
    cos, sin = R.rope_tables()
    a = (c["qkv"], ns, c["ss"], c["M"], H, KVH, c["pos"], cos, sin, c["kc"], c["vc"])
    ref64 = R.decode_attention(*a, cache_round=_rt(dt))[0]
    ref32 = R.decode_attention(*a, dtype=F32, cache_round=_rt(dt), out_round=_rt(dt))[0]
    assert bool(torch.isfinite(ref64).all())
    mt = R.decode_attention(*a, cache_round=_rt(dt), mut=mut)[0]
    assert _caught(ref64, ref32, mt, dt == BF16)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_residual_cases_catch(dt):
    for M, D, pad in [(3, 1024, 0), (1, 4096, 8), (3, 16384, 8)]:        # the tail of slab_sum4
        c = R.residual_case(M, D, 6, pad)
        a = (c["x"], c["y"], 6, c["ss"], M, D, R.EPS, c["w"])
        (x64, h64), (x32, h32) = R.add_rmsnorm(*a), R.add_rmsnorm(*a, dtype=F32, round_to=_rt(dt))
        xm, hm = R.add_rmsnorm(*a, mut="no_tail")
        assert _caught(x64, x32, xm, False) and _caught(h64, h32, hm, dt == BF16)
    for M, D in R.ADD_SS_SHAPES:
        c = R.residual_case(M, D, 6, 8)
        a = (c["x"], c["y"], 6, c["ss"], M, D)
        (x64, r64), (x32, r32) = R.add_ss(*a), R.add_ss(*a, dtype=F32)
        xm, rm = R.add_ss(*a, mut="no_tail")
        assert _caught(x64, x32, xm, False) and _caught(r64, r32, rm, False)
    for D in (8192, 16384):                                              # the later passes' squares
        for ns in (0, 5):
            c = R.residual_case(3, D, ns, 0)
            a = (c["x"], c["y"], ns, c["ss"], 3, D, R.EPS, None)
            h64, h32 = R.add_rmsnorm(*a)[1], R.add_rmsnorm(*a, dtype=F32, round_to=_rt(dt))[1]
            assert _caught(h64, h32, R.add_rmsnorm(*a, mut="skip_pass2")[1], dt == BF16)
    if dt == F32:                                 # one live thread in the second pass
        c = R.residual_case(1, 4100, 0, 0)
        a = (c["x"], None, 0, 0, 1, 4100, R.EPS, None)
        assert _caught(R.add_rmsnorm(*a)[1], R.add_rmsnorm(*a, dtype=F32)[1],
                       R.add_rmsnorm(*a, mut="skip_pass2")[1], False)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("M,F", R.SILU_SHAPES)
def test_silu_cases_catch(M, F, dt):
    for mut, ns in (("up8", 1), ("up8", 5), ("no_tail", 6)):
        gu, ss = R.silu_case(M, F, ns)
        a = (gu, ns, ss, M, F)
        ref64, ref32 = R.silu_mul(*a), R.silu_mul(*a, dtype=F32, round_to=_rt(dt))
        mt = R.silu_mul(*a, mut=mut)
        # up8: only the even quads' reads stay inside the row
        even = ((torch.arange(F) // 4) % 2 == 0) if mut == "up8" else slice(None)
        assert _caught(ref64[:, even], ref32[:, even], mt[:, even], dt == BF16), (mut, ns)
