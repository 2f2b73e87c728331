"""GPU: the C5 Mistral caption decoder (zsaac/mistral.py, csrc/mistral.hip) against the
reference goldens (tests/golden/mistral.npz) and the pinned oracle (oracle/mistral.py).

f32 parity mode: generated ids bit-exact for every clip and language.  fp8 perf mode (weight-only
fp8 e4m3, bf16 activations): ids equal to the reference up to the first step whose reference
top-2 logit margin is below 0.5 (the fp8/bf16 logit error is far below that; past such a step
the two decodes may legitimately follow different branches).  Kernels: the fp8 row GEMM against
torch on dequantised weights."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, KVH, EPS = 8, 2, 1e-5


def _strip(row, eos=2):
    row = [int(t) for t in row]
    return row[:row.index(eos) + 1] if eos in row else row


@pytest.fixture(scope="module")
def setup(golden):
    from oracle import mistral as OM
    from zsaac import synthetic as S
    g = golden("mistral.npz")
    sd = S.mistral_state_dict()
    mlp = S.mlp_mapper_state_dict(31, prefix_length=10, d=1024)
    emb = torch.from_numpy(g["clap_emb"])[:, None]
    hard = torch.from_numpy(g["hard_ids"])
    pes = {t: OM.clap_to_gpt(emb, hard, torch.from_numpy(g[f"tag_{t}"]), sd, mlp) for t in ("en", "fr")}
    return g, sd, pes


def _run(cuda, g, sd, pes, mode):
    from zsaac.mistral import MistralDecoder, MistralWeights
    w = MistralWeights(sd, cuda, mode, n_heads=H, n_kv_heads=KVH, eps=EPS)
    dec = MistralDecoder(w, max_batch=8, max_prompt=32, max_new=40)
    hard = torch.from_numpy(g["hard_ids"]).to(torch.int32).to(cuda)
    out = {}
    for t, (pe, soft) in pes.items():
        tag = torch.from_numpy(g[f"tag_{t}"]).to(torch.int32).to(cuda)
        out[t] = dec.generate(hard, soft.contiguous().to(cuda), tag, max_length=60)
    return out


def test_mistral_f32_bit_exact(cuda, setup):
    """f32: ids equal the reference's; a row may only part at a step where the reference's own
    top-2 logits tie to f32 rounding (margin < 1e-4: 'fr' clip 4 has a 0.0 margin at step 12)."""
    from oracle import mistral as OM
    g, sd, pes = setup
    out = _run(cuda, g, sd, pes, "f32")
    exact = 0
    for t in ("en", "fr"):
        ref = g[f"ids_{t}"]
        margins = []
        OM.generate(pes[t][0], sd, H, KVH, EPS, margins=margins)
        for b in range(ref.shape[0]):
            r = _strip(ref[b])
            n = next((i for i, m in enumerate(margins[b]) if m < 1e-4), len(r))
            assert out[t][b][:n] == r[:n], (t, b, n)
            exact += out[t][b] == r
    print(f"f32 mistral: {exact}/12 rows exact end to end")
    assert exact >= 11


def test_mistral_fp8_ids_until_small_margin(cuda, setup):
    from oracle import mistral as OM
    g, sd, pes = setup
    out = _run(cuda, g, sd, pes, "fp8")
    agree = total = 0
    for t in ("en", "fr"):
        margins = []
        ref = OM.generate(pes[t][0], sd, H, KVH, EPS, margins=margins)
        for b in range(len(ref)):
            n = next((i for i, m in enumerate(margins[b]) if m < 0.5), len(ref[b]))
            assert out[t][b][:n] == ref[b][:n], (t, b, n)
            agree += sum(int(x == y) for x, y in zip(out[t][b], ref[b]))
            total += len(ref[b])
    print(f"fp8 mistral: token agreement {agree}/{total}")


# one-shot tiles: the first three; the persistent stream kernel (M <= 32, more than one 128 x 1024
# item per CU): the down shape (2 items per workgroup), gate-sized with 3 items per workgroup, a
# column tail (16528 % 128 = 16) and a clamped last run, and 4 items at M = 7
@pytest.mark.parametrize("M,N,K", [(32, 6144, 4096), (7, 1008, 1024), (64, 256, 14336),
                                   (32, 4096, 14336), (20, 16528, 4096), (7, 28672, 4096)])
def test_fp8_gemm_rows(cuda, M, N, K):
    _fp8_gemm_rows_check(cuda, M, N, K)


def _fp8_gemm_rows_check(cuda, M, N, K):
    from zsaac._lib import call
    from zsaac.mistral import dequantize_fp8, fp8_pack_tiles, quantize_fp8
    g = torch.Generator().manual_seed(M + N)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    a = torch.randn(M, K, generator=g).bfloat16()
    q, s = quantize_fp8(w)
    ref = a.float() @ dequantize_fp8(q, s).t()
    ns = call("zs_fp8_splits", K)
    out = torch.empty(ns, M, N, device=cuda)
    ad, qd, sd = a.to(cuda), fp8_pack_tiles(q).to(cuda), s.to(cuda)   # keep the copies alive
    call("zs_fp8_gemm_rows", ad.data_ptr(), K, qd.data_ptr(), sd.data_ptr(),
         M, N, K, out.data_ptr(), M * N, N, torch.cuda.current_stream().cuda_stream)
    got = out.sum(0).cpu()
    assert float((got - ref).abs().max()) < 1e-3 * float(ref.abs().max()) + 1e-4


@pytest.mark.parametrize("M,N,K,ks,kh", [(32, 4096, 14336, 2, 1), (7, 1008, 2048, 2, 1),
                                         (32, 2048, 4096, 4, 1), (20, 4096, 4096, 1, 1),
                                         (32, 4096, 4096, 1, 2), (9, 1040, 4096, 2, 2),
                                         (1, 6144, 4096, 4, 2)])
def test_fp8_gemm_run(cuda, M, N, K, ks, kh):
    """zs_fp8_gemm_run's slabs (runs of ks splits, 1 / kh of each, summed in registers) sum to
    the product."""
    from zsaac._lib import call
    from zsaac.mistral import dequantize_fp8, fp8_pack_tiles, quantize_fp8
    g = torch.Generator().manual_seed(M + N + ks)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    a = torch.randn(M, K, generator=g).bfloat16()
    q, s = quantize_fp8(w)
    ref = a.float() @ dequantize_fp8(q, s).t()
    ns = call("zs_fp8_splits", K) // ks * kh
    out = torch.full((ns, M, N), float("nan"), device=cuda)
    ad, qd, sd = a.to(cuda), fp8_pack_tiles(q).to(cuda), s.to(cuda)
    call("zs_fp8_gemm_run", ad.data_ptr(), K, qd.data_ptr(), sd.data_ptr(), M, N, K, ks, kh,
         out.data_ptr(), M * N, N, None, 0, None, 0, 0.0, torch.cuda.current_stream().cuda_stream)
    got = out.sum(0).cpu()
    assert float((got - ref).abs().max()) < 1e-3 * float(ref.abs().max()) + 1e-4


@pytest.mark.parametrize("M,F,K", [(32, 14336, 4096), (5, 1024, 2048), (17, 1032, 1024)])
def test_fp8_gemm_run_glu(cuda, M, F, K):
    """GLU epilogue: act = silu(gate) * up straight from the glu-interleaved gate|up matrix, and
    the prefill consumer (zs_mistral_silu_mul over slabs of the same matrix) agrees."""
    from zsaac._lib import ZS_BF16, call
    from zsaac.mistral import dequantize_fp8, fp8_pack_tiles, glu_interleave, quantize_fp8
    g = torch.Generator().manual_seed(M + F)
    gate, up = torch.randn(F, K, generator=g) / K ** 0.5, torch.randn(F, K, generator=g) / K ** 0.5
    a = torch.randn(M, K, generator=g).bfloat16()
    q, s = quantize_fp8(glu_interleave(torch.cat([gate, up])))
    wd = dequantize_fp8(q, s)
    # the interleave is a row permutation: undo it on the dequantised matrix for the reference
    r = torch.arange(2 * F)
    c = r % 16
    j = 8 * (r // 16) + 4 * (c // 8) + c % 4
    src = torch.where((c // 4) % 2 == 0, j, F + j)
    wcat = torch.empty_like(wd)
    wcat[src] = wd
    y = a.float() @ wcat.t()
    ref = torch.nn.functional.silu(y[:, :F]) * y[:, F:]
    st = torch.cuda.current_stream().cuda_stream
    ad, qd, sd = a.to(cuda), fp8_pack_tiles(q).to(cuda), s.to(cuda)
    act = torch.full((M, F + 8), float("nan"), device=cuda, dtype=torch.bfloat16)
    call("zs_fp8_gemm_run", ad.data_ptr(), K, qd.data_ptr(), sd.data_ptr(), M, 2 * F, K,
         call("zs_fp8_splits", K), 1, None, 0, 0, act.data_ptr(), F + 8, None, 0, 0.0, st)
    got = act[:, :F].float().cpu()
    tol = 1e-2 * float(ref.abs().max()) + 1e-3
    assert float((got - ref).abs().max()) < tol
    assert torch.isnan(act[:, F:].float()).all()              # nothing past F columns written
    ns = call("zs_fp8_splits", K)
    slab = torch.empty(ns, M, 2 * F, device=cuda)
    call("zs_fp8_gemm_rows", ad.data_ptr(), K, qd.data_ptr(), sd.data_ptr(), M, 2 * F, K,
         slab.data_ptr(), M * 2 * F, 2 * F, st)
    act2 = torch.empty(M, F, device=cuda, dtype=torch.bfloat16)
    call("zs_mistral_silu_mul", slab.data_ptr(), ns, M * 2 * F, M, F, act2.data_ptr(), ZS_BF16, st)
    assert float((act2.float().cpu() - ref).abs().max()) < tol


@pytest.mark.parametrize("M,D,N,ns", [(32, 4096, 6144, 4), (6, 1024, 1040, 3), (17, 2048, 512, 0)])
def test_add_ss_then_normed_gemm(cuda, M, D, N, ns):
    """zs_mistral_add_ss (x += slab sum, bf16 copy, partial sums of squares) + zs_fp8_gemm_run
    with rss (the RMSNorm row factor applied after the product) == RMSNorm(x + y) @ W^T."""
    from zsaac._lib import call
    from zsaac.mistral import dequantize_fp8, fp8_pack_tiles, quantize_fp8
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 3
    y = torch.randn(max(ns, 1), M, D, generator=g)
    w = torch.randn(N, D, generator=g) / D ** 0.5
    q, s = quantize_fp8(w)
    xs = x + (y.sum(0) if ns else 0)
    hn = xs * torch.rsqrt(xs.pow(2).mean(1, keepdim=True) + 1e-5)
    ref = hn @ dequantize_fp8(q, s).t()
    st = torch.cuda.current_stream().cuda_stream
    xd, yd = x.to(cuda), y.to(cuda)
    xb = torch.empty(M, D, device=cuda, dtype=torch.bfloat16)
    rss = torch.full((8 * 32,), float("nan"), device=cuda)
    call("zs_mistral_add_ss", xd.data_ptr(), yd.data_ptr() if ns else None, ns, M * D, M, D,
         xb.data_ptr(), rss.data_ptr(), st)
    assert torch.allclose(xd.cpu(), xs, atol=1e-5)
    assert torch.equal(xb.cpu(), xs.bfloat16())
    nch = D // 512
    ss_ref = xs.pow(2).view(M, nch, 512).sum(2).t()
    assert torch.allclose(rss.view(8, 32)[:nch, :M].cpu(), ss_ref, rtol=1e-5)
    qd, sd = fp8_pack_tiles(q).to(cuda), s.to(cuda)
    nsl = call("zs_fp8_splits", D)
    out = torch.empty(nsl, M, N, device=cuda)
    call("zs_fp8_gemm_run", xb.data_ptr(), D, qd.data_ptr(), sd.data_ptr(), M, N, D, 1, 1,
         out.data_ptr(), M * N, N, None, 0, rss.data_ptr(), nch, 1e-5, st)
    got = out.sum(0).cpu()
    assert float((got - ref).abs().max()) < 1e-2 * float(ref.abs().max())


def test_dropin_clap_caption_mistralai(cuda, golden):
    """ClapCaption_Mistralai_prompt driven like predict_mistralai_multilingual.py:95-111 (peft
    attribute path, clap_to_gpt with the language tag, LMmodel.generate), f32 parity mode."""
    from models.caption_model import ClapCaption_Mistralai_prompt
    from zsaac import synthetic as S
    g = golden("mistral.npz")
    cfg = dict(vocab_size=32000, hidden_size=1024, intermediate_size=3072, num_hidden_layers=2,
               num_attention_heads=8, num_key_value_heads=2, rms_norm_eps=1e-5)
    m = ClapCaption_Mistralai_prompt(10, clip_length=10, prefix_size=1024, num_layers=8,
                                     mapping_type="mlp", mistral_config=cfg)
    sd = {"LMmodel.base_model.model." + k: v for k, v in S.mistral_state_dict().items()}
    sd.update(S.mlp_mapper_state_dict(31, prefix_length=10, d=1024))
    m.load_state_dict(sd)
    m = m.set_mode("f32").to(cuda).eval()
    prefix = torch.from_numpy(g["clap_emb"])[:, None].to(cuda)
    hard = torch.from_numpy(g["hard_ids"]).to(cuda)
    with torch.no_grad():
        eh = m.LMmodel.base_model.model.model.embed_tokens(hard)
        tk = torch.from_numpy(g["tag_en"])[None].repeat(prefix.shape[0], 1).to(cuda)
        et = m.LMmodel.base_model.model.model.embed_tokens(tk)
        pe, _ = m.clap_to_gpt(prefix, eh, et)
        am = torch.ones(pe.shape[:-1]).long().to(cuda)
        ids = m.LMmodel.generate(inputs_embeds=pe, attention_mask=am, do_sample=False,
                                 max_length=60, eos_token_id=2, pad_token_id=2)
    assert torch.equal(ids.cpu(), torch.from_numpy(g["ids_en"]))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_decode_attention_fused_vs_unfused(cuda, dt):
    """zs_mistral_decode_attention (RoPE + KV append + attention in one launch, the decode step)
    against zs_mistral_rope_kv + zs_mistral_attention on the same slabs and caches: identical
    cache rows, outputs within f32 reassociation (the key p term joins the softmax last).
    A consistency check only: both sides share the scale, the head mapping, the reductions and
    the online softmax, and the random caches hide a read past pos.  Each of the three kernels
    is compared with a float64 reference in tests/test_gpu_mistral_kernels.py (test_rope_kv,
    test_attention, test_attention_online_softmax, test_decode_attention)."""
    from zsaac import ops
    from zsaac._lib import call
    M, H, KVH, Lmax, ns = 5, 8, 2, 40, 3
    NQKV = (H + 2 * KVH) * 128
    g = torch.Generator().manual_seed(1)
    slab = torch.randn(ns, M, NQKV, generator=g).to(cuda)
    pos = torch.tensor([0, 3, 17, 38, 39], dtype=torch.int32).to(cuda)
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2).float() / 128))
    fr = torch.arange(Lmax).float()[:, None] * inv[None]
    cos, sin = fr.cos().to(cuda).contiguous(), fr.sin().to(cuda).contiguous()
    kc = torch.randn(M, KVH, Lmax, 128, generator=g).to(cuda, dt)
    vc = torch.randn(M, KVH, Lmax, 128, generator=g).to(cuda, dt)
    kc2, vc2 = kc.clone(), vc.clone()
    q = torch.empty(M, H * 128, device=cuda, dtype=dt)
    a1, a2 = torch.empty_like(q), torch.empty_like(q)
    st = torch.cuda.current_stream().cuda_stream
    call("zs_mistral_rope_kv", slab.data_ptr(), ns, M * NQKV, M, H, KVH, pos.data_ptr(), 1,
         cos.data_ptr(), sin.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), Lmax,
         ops.dt(q), st)
    call("zs_mistral_attention", q.data_ptr(), M, H, KVH, pos.data_ptr(), 1, kc.data_ptr(),
         vc.data_ptr(), Lmax, a1.data_ptr(), ops.dt(q), st)
    call("zs_mistral_decode_attention", slab.data_ptr(), ns, M * NQKV, M, H, KVH,
         pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc2.data_ptr(), vc2.data_ptr(), Lmax,
         a2.data_ptr(), ops.dt(q), st)
    torch.cuda.synchronize()
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    tol = 2e-5 if dt == torch.float32 else 2e-2
    assert float((a1.float() - a2.float()).abs().max()) < tol


@pytest.mark.parametrize("M,N,K", [(200, 1008, 2048), (928, 6144, 4096)])
def test_fp8_prefill_unpack_gemm(cuda, M, N, K):
    """The prefill form of the fp8 GEMM (M > 64): zs_fp8_unpack_bf16 (tile-packed codes -> bf16,
    exact) + the tiled bf16 GEMM + zs_scale_cols against the dequantised reference."""
    from zsaac import ops
    from zsaac._lib import call
    from zsaac.mistral import dequantize_fp8, fp8_pack_tiles, quantize_fp8
    g = torch.Generator().manual_seed(M + N)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    a = torch.randn(M, K, generator=g).bfloat16()
    q, s = quantize_fp8(w)
    ref = a.float() @ dequantize_fp8(q, s).t()
    ad, qd, sd = a.to(cuda), fp8_pack_tiles(q).to(cuda), s.to(cuda)
    wb = torch.empty(N, K, device=cuda, dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    call("zs_fp8_unpack_bf16", qd.data_ptr(), N, K, wb.data_ptr(), st)
    assert torch.equal(wb.cpu().float(), q.view(torch.float8_e4m3fn).float())
    out = torch.empty(M, N, device=cuda)
    ops.gemm(ad, wb, out, split_k=1)
    call("zs_scale_cols", out.data_ptr(), M, N, N, sd.data_ptr(), st)
    got = out.cpu()
    assert float((got - ref).abs().max()) < 1e-3 * float(ref.abs().max()) + 1e-4


def test_dropin_generate_trims_and_reuses_engine(cuda, golden):
    """HF generate's output width is the longest generated row (every row emitted eos earlier
    than max_length - P -> fewer columns), not max_length - P; one decoder is reused across
    calls whose prompt length changes (en / fr tags) and rebuilt only when the capacity grows."""
    from models.caption_model import ClapCaption_Mistralai_prompt
    from oracle import mistral as OM
    from zsaac import synthetic as S
    g = golden("mistral.npz")
    cfg = dict(vocab_size=32000, hidden_size=1024, intermediate_size=3072, num_hidden_layers=2,
               num_attention_heads=8, num_key_value_heads=2, rms_norm_eps=1e-5)
    msd = S.mistral_state_dict(eos_boost=6.0)
    mlp = S.mlp_mapper_state_dict(31, prefix_length=10, d=1024)
    m = ClapCaption_Mistralai_prompt(10, clip_length=10, prefix_size=1024, num_layers=8,
                                     mapping_type="mlp", mistral_config=cfg)
    sd = {"LMmodel.base_model.model." + k: v for k, v in msd.items()}
    sd.update(mlp)
    m.load_state_dict(sd)
    m = m.set_mode("f32").to(cuda).eval()
    lm = m.LMmodel.base_model.model
    emb = torch.from_numpy(g["clap_emb"])[:, None]
    hard = torch.from_numpy(g["hard_ids"])
    decs = []
    for t in ("en", "fr", "en"):
        pe, _ = OM.clap_to_gpt(emb, hard, torch.from_numpy(g[f"tag_{t}"]), msd, mlp)
        ref = OM.generate(pe, msd, H, KVH, EPS, max_length=60)
        with torch.no_grad():
            ids = m.LMmodel.generate(inputs_embeds=pe.to(cuda), attention_mask=None,
                                     do_sample=False, max_length=60, eos_token_id=2,
                                     pad_token_id=2).cpu()
        width = max(len(r) for r in ref)
        assert width < 60 - pe.shape[1], "eos boost too weak for the trim check"
        assert ids.shape == (len(ref), width), (t, ids.shape, width)
        for b, r in enumerate(ref):
            assert ids[b, :len(r)].tolist() == r, (t, b)
            assert bool((ids[b, len(r):] == 2).all())
        decs.append(lm.engine(cuda, 32, 64, 60))
    assert decs[0] is decs[1] is decs[2]
    big = lm.engine(cuda, 64, 64, 60)
    assert big is not decs[0] and big.B >= 64
    assert lm.engine(cuda, 8, 16, 10) is big


@pytest.mark.parametrize("mode", ["fp8", "f32"])
def test_generate_concurrent_equals_sequential(cuda, setup, mode):
    """zsaac.mistral.generate_concurrent (the language tags of a batch on separate streams and
    decoders sharing the weights, advanced in chunks without blocking on one another) returns
    exactly each decoder's sequential generate ids."""
    from zsaac import ops
    from zsaac.mistral import MistralDecoder, MistralWeights, generate_concurrent
    g, sd, pes = setup
    w = MistralWeights(sd, cuda, mode, n_heads=H, n_kv_heads=KVH, eps=EPS)
    hard = torch.from_numpy(g["hard_ids"]).to(torch.int32).to(cuda)
    jobs = [(hard, soft.contiguous().to(cuda), torch.from_numpy(g[f"tag_{t}"]).to(torch.int32).to(cuda), 60)
            for t, (pe, soft) in pes.items()]
    seq = MistralDecoder(w, max_batch=8, max_prompt=32, max_new=40)
    ref = [seq.generate(*j) for j in jobs]
    decs = [MistralDecoder(w, max_batch=8, max_prompt=32, max_new=40) for _ in jobs]
    streams = ops.dedicated_streams(len(jobs), cuda)
    for _ in range(2):          # the second pass replays graphs captured in the first
        out = generate_concurrent(decs, streams, jobs)
        torch.cuda.synchronize()
        assert out == ref
