"""CPU: the grid decode's references (tests/grid_ref.py) against torch's own layer_norm / softmax /
gelu / linear / argmax in float64, the fragment helpers against ops.pack_*, the bf16 host fold of
Gpt2Weights against its definition, the mirrored workspace layout against decode_grid.hip, the
input conditions the GPU cases (tests/test_gpu_grid_kernels.py) rely on, and every mutant of
grid_ref.MUTANTS told from the reference by more than twice the tolerance on those cases' inputs."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zero-shot-aac_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grid_ref as G  # noqa: E402
from grid_ref import BF16, F32, F64, I32  # noqa: E402

CSRC = os.path.join(ROOT, "zero-shot-aac_amd", "csrc")


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ against torch's own ops
def test_ln_linear_is_layer_norm_then_linear():
    g = _g(0)
    x = (torch.randn(5, 768, generator=g) + 3.0).bfloat16()
    w = torch.randn(40, 768, generator=g).bfloat16()
    b, gam, beta = torch.randn(40, generator=g), 1 + 0.1 * torch.randn(768, generator=g), torch.randn(768, generator=g)
    for ln in (None, (gam, beta)):
        want = Fn.linear(Fn.layer_norm(x.double(), (768,), None if ln is None else gam.double(),
                                       None if ln is None else beta.double(), 1e-5), w.double(), b.double())
        assert torch.allclose(G.ln_linear(x, w, b, ln=ln), want, rtol=1e-12, atol=1e-12)
    # the float32 forms are the same function to float32 accuracy: the fold and normalise-first
    want = Fn.linear(Fn.layer_norm(x.double(), (768,), None, None, 1e-5), w.double(), b.double())
    cs = w.double().sum(1).float()
    for got in (G.ln_linear(x, w, b, cs, F32), G.ln_linear(x, w, b, None, F32, kstep=16)):
        assert got.dtype == F32 and torch.allclose(got.double(), want, rtol=1e-4, atol=1e-3)


def test_phase_a_writes_q_and_the_cache_slot():
    g = _g(1)
    R, Lmax = 3, 9
    x = torch.randn(R, 768, generator=g).bfloat16()
    w, b = (0.1 * torch.randn(2304, 768, generator=g)).bfloat16(), torch.randn(2304, generator=g)
    kc, vc = G._cache(R + 1, Lmax, BF16), G._cache(R + 1, Lmax, BF16)
    pos = torch.tensor([1, 8, 4], dtype=I32)
    q, k2, v2 = G.phase_a(x, w, b, None, kc[:R], vc[:R], pos)
    y = Fn.linear(Fn.layer_norm(x.double(), (768,)), w.double(), b.double()).bfloat16().double()
    assert torch.equal(q, y[:, :768])
    for r in range(R):
        p = int(pos[r])
        assert torch.equal(k2[r, :, p].reshape(-1), y[r, 768:1536])
        assert torch.equal(v2[r, :, p].reshape(-1), y[r, 1536:])
        keep = [j for j in range(Lmax) if j != p]
        assert bool((k2[r][:, keep] == G.SENT).all()) and bool((v2[r][:, keep] == G.SENT).all())


def test_phase_b_is_scaled_dot_product_attention():
    c = G.case_b("bf16")
    for r in (0, 2, 8, 18):
        p = int(c["pos"][r])
        q = c["q"][r].double().view(1, 12, 1, 64)
        K, V = c["kc"][r, :, :p + 1].double()[None], c["vc"][r, :, :p + 1].double()[None]
        want = Fn.scaled_dot_product_attention(q, K, V).reshape(768)
        got = G.phase_b(c["q"][r:r + 1], c["kc"][r:r + 1], c["vc"][r:r + 1], c["pos"][r:r + 1], F64, None)
        assert torch.allclose(got[0], want, rtol=1e-10, atol=1e-10), r
    # the float32 online softmax is the same function
    y = G.phase_b(c["q"], c["kc"], c["vc"], c["pos"], F32, None)
    x = G.phase_b(c["q"], c["kc"], c["vc"], c["pos"], F64, None)
    assert float((y.double() - x).abs().max()) < 1e-4


def test_phase_ce_and_d_and_f_are_linear_gelu_argmax():
    g = _g(2)
    a, w, b = torch.randn(4, 3072, generator=g).bfloat16(), torch.randn(768, 3072, generator=g).bfloat16(), torch.randn(768, generator=g)
    xo = torch.randn(4, 768, generator=g)
    assert torch.allclose(G.phase_ce(a, w, b, xo), Fn.linear(a.double(), w.double(), b.double()) + xo.double(),
                          rtol=1e-12, atol=1e-12)
    assert torch.allclose(G.phase_ce(a, w, b, xo, F32).double(), G.phase_ce(a, w, b, xo), rtol=1e-4, atol=1e-3)
    x = torch.randn(4, 768, generator=g).bfloat16()
    wf, bf_ = (0.1 * torch.randn(3072, 768, generator=g)).bfloat16(), torch.randn(3072, generator=g)
    hid, pre = G.phase_d(x, wf, bf_, None, F64, None)
    want = Fn.gelu(Fn.linear(Fn.layer_norm(x.double(), (768,)), wf.double(), bf_.double()), approximate="tanh")
    assert torch.allclose(hid, want, rtol=1e-12, atol=1e-12)
    fast, _ = G.phase_d(x, wf, bf_, wf.double().sum(1).float(), F32, None)
    assert torch.allclose(fast.double(), want, rtol=1e-4, atol=1e-4)
    V = 37
    wh = torch.zeros(48, 768)
    wh[:V] = 0.1 * torch.randn(V, 768, generator=g)
    wh[30] = wh[5] = 0.05 * Fn.layer_norm(x[0].float(), (768,))      # row 0: ids 5 and 30 tie on top
    bh = torch.zeros(48)
    bh[:V] = torch.randn(V, generator=g)
    bh[30] = bh[5]
    lg, best, ids = G.phase_f(x, wh.bfloat16(), bh, None, V, 0.7)
    want = Fn.linear(Fn.layer_norm(x.double(), (768,)), wh.bfloat16().double()[:V], bh.double()[:V]) / torch.tensor(0.7, dtype=F32).double()
    assert lg.shape == (4, V) and torch.allclose(lg, want, rtol=1e-12, atol=1e-12)
    assert torch.equal(best, lg.max(-1).values) and int(ids[0]) == 5 and float(lg[0, 5]) == float(lg[0, 30])
    assert torch.equal(ids[1:], want[1:].argmax(-1)) and int(want[0].argmax()) in (5, 30)
    assert int(G.phase_f(x, wh.bfloat16(), bh, None, V, 0.7, mut="tie_high")[2][0]) == 30


def test_key_decode_inverts_the_order_preserving_key():
    import numpy as np
    vals = np.array([0.0, -0.0, 1.5, -1.5, 3e38, -3e38, 1e-40, -37.25], dtype=np.float32)
    ids = np.array([0, 5, 9216, 50256, 1, 2, 3, (1 << 24) - 1], dtype=np.uint32)
    u = vals.view(np.uint32)
    fk = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint64)      # common.h f2key
    keys = torch.from_numpy(((fk << np.uint64(32)) | (~ids).astype(np.uint64)).view(np.int64).copy())
    v, i = G.key_decode(keys)
    assert np.array_equal(v.numpy().view(np.uint32), u) and np.array_equal(i.numpy(), ids.astype(np.int64))
    order = np.argsort(keys.numpy().view(np.uint64), kind="stable")      # the key orders as the float
    assert np.all(np.diff(vals[order].astype(np.float64)) >= 0)


def test_step_chains_the_phases_and_folded_equals_unfolded():
    """step() on unfolded weights (LayerNorm affines applied) equals step() on the tables folded
    in float64 (no rounding): the fold is an identity; and the hand-off option moves it by about
    a bf16 step, not more."""
    g = _g(3)
    r = lambda *s: torch.randn(*s, generator=g).double()
    R, Lmax, V = 2, 6, 33
    aff = lambda: (1 + 0.1 * r(768), 0.1 * r(768))
    layers, folded = [], []
    for _ in range(12):
        ly = dict(ln1=aff(), attn_w=0.05 * r(2304, 768), attn_b=0.02 * r(2304), proj_w=0.02 * r(768, 768),
                  proj_b=0.02 * r(768), ln2=aff(), fc_w=0.05 * r(3072, 768), fc_b=0.02 * r(3072),
                  mproj_w=0.01 * r(768, 3072), mproj_b=0.02 * r(768))
        layers.append(ly)
        f = dict(ly)
        for wk, bk, lk in (("attn_w", "attn_b", "ln1"), ("fc_w", "fc_b", "ln2")):
            f[wk], f[bk], f[lk] = ly[wk] * ly[lk][0][None, :], ly[bk] + ly[wk] @ ly[lk][1], None
        folded.append(f)
    wte, wpe, lnf = 0.1 * r(V, 768), 0.05 * r(Lmax, 768), aff()
    m = dict(wte=wte, wpe=wpe, layers=layers, lnf=lnf, head_w=wte, head_b=torch.zeros(V, dtype=F64), V=V)
    mf = dict(m, layers=folded, lnf=None, head_w=wte * lnf[0][None, :], head_b=wte @ lnf[1])
    tok, pos = torch.tensor([3, 32], dtype=I32), torch.tensor([1, 4], dtype=I32)
    kc = [r(R, 12, Lmax, 64) for _ in range(12)]
    vc = [r(R, 12, Lmax, 64) for _ in range(12)]
    a, b = G.step(m, tok, pos, kc, vc), G.step(mf, tok, pos, kc, vc)
    assert torch.allclose(a["x"], b["x"], rtol=1e-9, atol=1e-9)
    assert torch.allclose(a["logits"], b["logits"], rtol=1e-9, atol=1e-9)
    assert torch.allclose(a["k"][11], b["k"][11], rtol=1e-9, atol=1e-9)
    h = G.step(m, tok, pos, kc, vc, handoff=BF16)
    d = float((h["x"] - a["x"]).abs().max())
    assert 0 < d < 0.1 * float(a["x"].abs().max())


# ------------------------------------------------------------------ fragment helpers
def test_fragment_helpers_match_ops_packing_and_round_trip():
    from zsaac import ops
    g = _g(4)
    for K in (768, 3072):
        x = torch.randn(64, K, generator=g)
        xb = x.bfloat16()
        # transposed roles: an activation [64][K] in fragment order is a [N = 64][K] weight's
        assert torch.equal(G.frag_pack(xb), ops.pack_b_fragments(xb).reshape(-1))
        assert torch.equal(G.frag_pack(x), ops.pack_f32_fragments(x).reshape(-1))
        assert torch.equal(G.frag_unpack(G.frag_pack(xb), 64, K), xb)
        assert torch.equal(G.frag_unpack(G.frag_pack(x), 64, K), x)
    w = torch.randn(41, 64, generator=g)
    for t in (w, w.bfloat16()):
        P = (ops.pack_f32_fragments if t.dtype == F32 else ops.pack_b_fragments)(t)
        U = G.frag_unpack(P, 48, 64)
        assert torch.equal(U[:41], t) and bool((U[41:] == 0).all())
        assert torch.equal(G.frag_pack(t), P.reshape(-1))
    part = G.frag_pack(torch.ones(17, 768).bfloat16(), nrows=64, fill=G.SENT)
    U = G.frag_unpack(part, 64, 768)
    assert bool((U[:17] == 1).all()) and bool((U[17:] == G.SENT).all())
    # the kernel's own formula (frag_off, bf16): ((((row >> 4) KS + (col >> 5)) 64 + (row & 15) +
    # 16 ((col >> 3) & 3)) 8 + (col & 7))
    idx = G.frag_index(64, 768, 8)
    for row, col in ((0, 0), (17, 40), (63, 767), (33, 255)):
        assert int(idx[row, col]) == ((((row >> 4) * 24 + (col >> 5)) * 64 + (row & 15) + 16 * ((col >> 3) & 3)) * 8 + (col & 7))
    idx = G.frag_index(64, 768, 4)
    for row, col in ((0, 0), (17, 40), (63, 767), (33, 255)):
        assert int(idx[row, col]) == ((((row >> 4) * 48 + (col >> 4)) * 64 + (row & 15) + 16 * ((col >> 2) & 3)) * 4 + (col & 3))


# ------------------------------------------------------------------ the workspace mirror
def _ws_consts(text, env):
    env = dict(env)
    for name, expr in re.findall(r"^constexpr int (WS_\w+) = ([^;]+);", text, re.M):
        env[name] = int(eval(expr, {"__builtins__": {}}, env))
    return env


def test_workspace_layout_mirrors_decode_grid():
    src = open(os.path.join(CSRC, "decode_grid.hip")).read()
    m = re.search(r"^#define DG_NSH (\d+)", src, re.M)
    base = dict(NSH=int(m.group(1)), RM=G.RM, D=G.D, DFF=G.DFF)
    for k, v in (("D", G.D), ("DFF", G.DFF), ("RM", G.RM), ("NLY", G.NLY), ("NH", G.NH), ("HD", G.HD)):
        assert re.search(r"constexpr int [^;]*\b%s = %d\b" % (k, v), src), k
    head, tail = src.split("namespace f32 {", 1)
    b = _ws_consts(head, base)
    f = _ws_consts(tail.split("}  // namespace f32", 1)[0], b)
    assert b["WS_SYNC_BYTES"] == G.WS_SYNC_BYTES and b["WS_KEY"] == G.WS_KEY
    assert b["WS_KEY"] + 2 * 64 * 8 <= b["WS_CLM"] < b["WS_SYNC_BYTES"]
    lay = G.ws_layout("bf16")
    for k in ("Q", "ATT", "XB", "HID", "X", "BYTES"):
        assert b["WS_" + k] == lay[k], k
    lay = G.ws_layout("f32")
    for k in ("Q", "ATT", "XB", "HID", "BYTES"):
        assert f["WS_" + k] == lay[k], k
    assert "WS_X" not in {n for n, _ in re.findall(r"^constexpr int (WS_\w+) = ([^;]+);", tail, re.M)}
    # the launch order the window indexes: A .. E per block, then F, then the bookkeeping
    body = src[src.index("int dg_phase_step("):src.index("// `steps` decode steps as phase launches")]
    assert re.findall(r"in\(5 \* (?:l \+ (\d)|NLY(?: \+ (\d))?)\)\) hipLaunchKernelGGL\(\(?(?:dg_phase_kernel<G, PH_(\w)>|dg_book_kernel)", body) == [
        ("0", "", "A"), ("1", "", "B"), ("2", "", "C"), ("3", "", "D"), ("4", "", "E"), ("", "", "F"), ("", "1", "")]
    body = src[src.index('extern "C" int zs_gpt2_decode_phases_f32('):]
    assert re.findall(r"in\(5 \* (?:l \+ (\d)|NLY(?: \+ (\d))?)\)\) hipLaunchKernelGGL\((?:f32::dg32_phase_kernel<PH_(\w)>|dg_book_kernel)", body) == [
        ("0", "", "A"), ("1", "", "B"), ("2", "", "C"), ("3", "", "D"), ("4", "", "E"), ("", "", "F"), ("", "1", "")]
    assert src.count("hipLaunchKernelGGL((dg_phase_kernel") == 6 and src.count("hipLaunchKernelGGL(f32::dg32_phase_kernel") == 6
    assert [G.launch(3, p) for p in "ABCDE"] == [15, 16, 17, 18, 19] and G.launch(0, "F") == 60
    assert G.launch(0, "book") == 61 == G.LAUNCHES - 1


# ------------------------------------------------------------------ the bf16 host fold
def _small_sd(g, Dm, N, V, npos):
    r = lambda *s: torch.randn(*s, generator=g)
    p = "gpt.transformer."
    sd = {p + "wte.weight": r(V, Dm), p + "wpe.weight": r(npos, Dm),
          p + "ln_f.weight": 1 + 0.1 * r(Dm), p + "ln_f.bias": 0.1 * r(Dm)}
    for i in range(12):
        h = p + f"h.{i}."
        sd.update({h + "ln_1.weight": 1 + 0.1 * r(Dm), h + "ln_1.bias": 0.1 * r(Dm),
                   h + "ln_2.weight": 1 + 0.1 * r(Dm), h + "ln_2.bias": 0.1 * r(Dm),
                   h + "attn.c_attn.weight": r(Dm, N), h + "attn.c_attn.bias": r(N),
                   h + "attn.c_proj.weight": r(Dm, Dm), h + "attn.c_proj.bias": r(Dm),
                   h + "mlp.c_fc.weight": r(Dm, N), h + "mlp.c_fc.bias": r(N),
                   h + "mlp.c_proj.weight": r(N, Dm), h + "mlp.c_proj.bias": r(Dm)})
    return sd


def _once(got, want64):
    """got (f32) is want64 rounded once: within half an f32 step (a little slack for the order
    of the float64 sum)."""
    return bool(((got.double() - want64).abs() <= want64.abs() * 2.0 ** -24 * 1.01 + 1e-30).all())


def test_bf16_fold_of_gpt2weights():
    """Gpt2Weights (bf16, folded): the bf16 twin of test_pack_f32_folds_layernorm_affine, on a
    small model through the real constructor.  W' = bf16(W g) bit for bit; bias table row 0 =
    b + W beta in f64 rounded once; row 1 = the f64 sum of the ROUNDED W' (exact in f64, so bit
    for bit) -- and not the sum of the unrounded W g; the same for the folded head, both rows of
    lm_bias, and zero past V."""
    from zsaac import decoder as dec
    g = _g(5)
    Dm, N, V = 64, 96, 40
    sd = _small_sd(g, Dm, N, V, 16)
    w = dec.Gpt2Weights(sd, torch.device("cpu"), BF16, prefix="gpt.transformer.")
    assert w.folded
    w.packed_layer_ptrs()
    p = "gpt.transformer."
    differs = 0
    for i, pk in enumerate(w._packed):
        h = p + f"h.{i}."
        for wk, bk, sw, lk in (("attn_w", "attn_b", "attn.c_attn", "ln_1"), ("fc_w", "fc_b", "mlp.c_fc", "ln_2")):
            W, b = sd[h + sw + ".weight"].t().float(), sd[h + sw + ".bias"].float()
            gam, beta = sd[h + lk + ".weight"].float(), sd[h + lk + ".bias"].float()
            Wp = G.frag_unpack(pk[wk], N, Dm)
            assert Wp.dtype == BF16 and torch.equal(Wp, (W * gam[None, :]).bfloat16())
            tab = pk[bk]
            assert tab.shape == (2, N) and tab.dtype == F32
            assert _once(tab[0], b.double() + (W.double() * beta.double()[None, :]).sum(1))
            assert torch.equal(tab[1], Wp.double().sum(1).float())
            differs += int((tab[1] != (W * gam[None, :]).double().sum(1).float()).sum())
            f = G.fold(W, b, gam, beta, BF16)           # the cases' own fold is this fold
            assert torch.equal(f["w"], Wp) and torch.equal(f["cs"], tab[1]) and _once(f["b"], tab[0].double())
        for wk, bk, sw in (("proj_w", "proj_b", "attn.c_proj"), ("mproj_w", "mproj_b", "mlp.c_proj")):
            W = sd[h + sw + ".weight"].t()
            assert torch.equal(G.frag_unpack(pk[wk], W.shape[0], W.shape[1]), W.bfloat16())
            assert torch.equal(pk[bk], sd[h + sw + ".bias"].float())
    assert differs > 12 * 2 * N // 2           # the rounded sums are a different table
    wte, gam, beta = sd[p + "wte.weight"].float(), sd[p + "ln_f.weight"].float(), sd[p + "ln_f.bias"].float()
    Vp = 48
    Wh = G.frag_unpack(w.wte_packed(), Vp, Dm)
    assert torch.equal(Wh[:V], (wte * gam[None, :]).bfloat16()) and bool((Wh[V:] == 0).all())
    lmb = w.lm_bias()
    assert lmb.shape == (2, Vp) and bool((lmb[:, V:] == 0).all())
    assert _once(lmb[0, :V], (wte.double() * beta.double()[None, :]).sum(1))
    assert torch.equal(lmb[1, :V], Wh[:V].double().sum(1).float())
    assert int((lmb[1, :V] != (wte * gam[None, :]).double().sum(1).float()).sum()) > V // 2


# ------------------------------------------------------------------ the GPU cases' conditions
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_case_conditions_a_and_d(mode):
    for R in G.RS:
        kinds = [G.ROW_KINDS[(i + R) % 4] for i in range(R)]
        if R == 1:
            assert kinds == [16]
        else:
            assert set(kinds) == set(G.ROW_KINDS)
        for c in (G.case_a(mode, 0, R), G.case_a(mode, G.LAYER, R), G.case_d(mode, R)):
            x = c["x"]
            assert x.dtype == G._st(mode) and x.shape == (R, 768)
            ratio = G.row_ratio(x)
            for i, k in enumerate(kinds):
                if k == "eq":
                    assert bool((x[i] == x[i, 0]).all()) and float(x[i, 0]) != 0.0
                elif k == 0:
                    assert float(ratio[i]) < 0.1
                else:
                    assert abs(float(ratio[i]) / k - 1) < 0.1, (i, k, float(ratio[i]))
        for layer in (0, G.LAYER):
            c = G.case_a(mode, layer, R)
            pos, tok = c["pos"], c["tok"]
            assert int(pos.min()) >= 1 and int(pos.max()) <= min(c["Lmax"] - 1, 1023)
            assert int(tok.min()) >= 0 and int(tok.max()) < c["V"] and len(set(tok.tolist())) == R
            if R > 1:
                assert 1 in pos.tolist() and c["Lmax"] - 1 in pos.tolist() and len(set(pos.tolist())) > 1
        pre = G.case_d(mode, R)["pre"]
        if R > 1:
            finite = pre[torch.isfinite(pre).all(-1)]
            assert float(finite.min()) < -10 and float(finite.max()) > 10
            assert float(finite.abs().min()) < 1e-3
    # the tables: g != 1 and beta != 0 went into the fold, and rounding moved the column sums
    t = G.layer_tables("bf16")
    assert int((t["attn"]["cs"] != t["attn"]["cs_u"]).sum()) > 2000


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_case_conditions_b(mode):
    c = G.case_b(mode)
    pos = c["pos"].tolist()
    assert c["Lmax"] == 100 and set(G.B_POS) <= set(pos) and G.B_POS[-1] == c["Lmax"] - 1
    assert min(pos) >= 1 and max(pos) <= c["Lmax"] - 1
    hist = torch.cat([c["kc"][r, :, :pos[r]].float().reshape(-1) for r in range(c["R"]) if r != G.B_ONE[0]])
    assert 0.9 < float(hist.std()) < 1.1
    vv = torch.cat([c["vc"][r, :, :pos[r] + 1].float().reshape(-1) for r in range(c["R"])])
    assert 0.9 < float(vv.std()) < 1.1

    def scores(r, h):
        q = c["q"][r, 64 * h:64 * h + 64].double()
        return (c["kc"][r, h, :pos[r] + 1].double() @ q) / 8

    s = scores(*G.B_SPAN)
    assert pos[G.B_SPAN[0]] == 99 and float(s.min()) < -40 and float(s.max()) > 40
    assert float(torch.exp(s.float()).max()) == float("inf")       # no max subtraction: overflow
    s = torch.softmax(scores(*G.B_ONE), 0)
    assert pos[G.B_ONE[0]] == 65 and int(s.argmax()) == 40 and float(s[40]) > 0.99
    s = torch.softmax(scores(*G.B_NEW), 0)
    assert int(s.argmax()) == pos[G.B_NEW[0]] == 64 and float(s[-1]) > 0.99
    for r in range(c["R"]):            # nothing but the sentinel past pos, and in the spare row
        assert bool((c["kc"][r, :, pos[r] + 1:] == G.SENT).all())
    assert bool((c["kc"][c["R"]] == G.SENT).all()) and bool((c["vc"][c["R"]] == G.SENT).all())


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("variant", list(G.F_VARIANTS))
def test_case_conditions_f(mode, variant):
    c = G.case_f(mode, variant)
    lg, best, ids = c["ref"]
    V = c["V"]
    assert V == 9217 and V % 16 == 1 and V >= 16 * 192 * 3 and c["w"].shape[0] == 16 * 577
    assert bool((c["w"][V:] == 0).all()) and bool((c["b"][V:] == 0).all())
    assert c["R"] >= 8
    for r, tie in G.F_TIES:
        assert all(float(lg[r, v]) == float(best[r]) for v in tie) and int(ids[r]) == min(tie)
        assert int((lg[r] == best[r]).sum()) == len(tie)
        if len(tie) == 2:
            assert torch.equal(c["w"][tie[0]], c["w"][tie[1]]) and float(c["b"][tie[0]]) == float(c["b"][tie[1]])
    assert int(ids[0]) == V - 1                                   # the last block's one real column
    (a, b_), (c2, d) = G.F_TIES[1][1], G.F_TIES[2][1]
    assert a // 4 == b_ // 4 and c2 // 16 == d // 16 and c2 // 4 != d // 4
    assert [(t[1] - t[0]) // 16 for _, t in G.F_TIES[3:6]] == [48, 96, 192]
    assert G.F_TIES[6][1][1] // 16 == G.F_TIES[6][1][0] // 16 + 1
    if variant == "t07neg":
        assert c["temperature"] == 0.7 and float(lg.max()) < 0 and c["R"] == 64
    else:
        assert c["temperature"] == 1.0 and float(lg.max()) > 0
    # at most a quarter of the rows may accept either of two ids; the planted ones never do
    cand = G.f_candidates(c)
    assert all(cand[r][1] for r, _ in G.F_TIES)
    assert sum(1 for _, strict in cand if not strict) <= c["R"] // 4


def test_case_conditions_book():
    f = G.case_f("bf16", "t1")
    ids = f["ref"][2]
    for name in G.BOOK_CASES:
        b = G.book_case(name)
        st = b["state"]
        assert b["R"] == f["R"] and int(ids[1]) == b["stop0"] and int(ids[0]) == b["stop1"]
        assert all(int(st["done"][r]) == 1 for r in G.BOOK_DONE) and int(st["done"].sum()) == len(G.BOOK_DONE)
        assert 0 not in G.BOOK_DONE and 1 not in G.BOOK_DONE
        new = G.book(st, f["ref"][1], ids, b["max_steps"], b["stop0"], b["stop1"])
        assert int(new["done"][0]) == 1 and int(new["done"][1]) == 1 and int(new["done"][3]) == 0
        assert int(new["all_done"][0]) == int(name == "last")
        assert int(st["pos"].min()) >= 1 and int(st["pos"].max()) <= 39


# ------------------------------------------------------------------ the mutants
def _moved(ref, mut, tol):
    """The mutant leaves the reference by more than twice the tolerance somewhere (or is not
    finite where the reference is)."""
    d = (mut.double() - ref.double()).abs()
    bad = ~torch.isfinite(mut.double()) & torch.isfinite(ref.double())
    return bool(bad.any()) or bool((torch.nan_to_num(d) > 2 * tol).any())


def _tol(ref, yard, bf16):
    return G.row_tolerance(ref, yard, bf16=bf16)[1]


def test_every_mutant_is_listed():
    assert set(MUTANT_CHECKS) == set(G.MUTANTS)


def _mut_a(mut):
    for layer in (0, G.LAYER):
        c = G.case_a("bf16", layer, 64)
        got = G.mutate_a(c, mut)
        assert any(_moved(r, m, _tol(r, y, True)) for r, m, y in zip(c["ref"], got, c["yard"])), layer


def _mut_d(mut):
    c = G.case_d("bf16", 64)
    assert _moved(c["ref"], G.mutate_d(c, mut), _tol(c["ref"], c["yard"], True))


def _mut_b(mut):
    c = G.case_b("bf16")
    assert _moved(c["ref"], G.mutate_b(c, mut), _tol(c["ref"], c["yard"], True))


def _mut_ce(mut):
    for which, layer in (("C", 0), ("C", G.LAYER), ("E", G.LAYER)):
        c = G.case_ce("bf16", which, layer, 17)
        assert _moved(c["ref"], G.mutate_ce(c, mut), _tol(c["ref"], c["yard"], False)), (which, layer)


def _mut_f(variants):
    def check(mut):
        for v in variants:
            c = G.case_f("bf16", v)
            _, tol = G.f_tolerance(c)
            lg, best, ids = c["ref"]
            _, mbest, mids = G.mutate_f(c, mut)
            wrong_id = [r for r in range(c["R"]) if int(mids[r]) != int(ids[r])]
            # a wrong id counts when the GPU test would refuse it: outside the row's candidates
            cand = G.f_candidates(c)
            refused = [r for r in wrong_id if cand[r][1] or int(mids[r]) not in cand[r][0]]
            assert refused or _moved(best, mbest, tol), v
    return check


MUTANT_CHECKS = {
    "cs_unrounded": lambda m: (_mut_a(m), _mut_d(m)),
    "eps_dropped": lambda m: (_mut_a(m), _mut_d(m)),
    "kv_slot_off_by_one": _mut_a,
    "scale_dropped": _mut_b,
    "new_key_dropped": _mut_b,
    "chunk_tail_dropped": _mut_b,
    "gelu_erf": _mut_d,
    "resid_from_xb": _mut_ce,
    "tie_high": _mut_f(("t1", "t07neg")),
    "temp_mul": _mut_f(("t07neg",)),
    "pad_column_wins": _mut_f(("t07neg",)),
}


@pytest.mark.parametrize("mut", G.MUTANTS)
def test_mutant_is_told_from_the_reference(mut):
    MUTANT_CHECKS[mut](mut)
