"""CPU tests that pin tests/gemm_ref.py, the reference the GEMM-family GPU tests compare against:
gemm / gemm_ln against torch.nn.functional.linear / gelu / layer_norm in float64, lmhead against
torch.topk / logsumexp on data without ties, the tie order on its own against a stable sort and
against an emulation of lmhead_kernel's register insertion (the loop before the tie-order fix
must fail, the fixed one pass); the input conditions of the cases of
tests/test_gpu_gemm_kernels.py, so a bad seed or an edited table fails here and not on the GPU;
and, for each arithmetic error listed in gemm_ref.MUTANTS, that the inputs of a GPU case move the
expected output by more than twice that case's tolerance (a kernel with that error is then more
than one tolerance away from the reference, whatever its own rounding)."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
Fn = torch.nn.functional


# ------------------------------------------------------------------ against torch's own ops
@pytest.mark.parametrize("act", R.ACTS)
def test_gemm_matches_torch(act):
    g = torch.Generator().manual_seed(1)
    a = torch.randn(9, 48, generator=g).bfloat16()
    w = torch.randn(13, 48, generator=g).bfloat16()
    bias, res = torch.randn(13, generator=g), torch.randn(9, 13, generator=g)
    fn = {"none": lambda x: x, "gelu_erf": Fn.gelu, "gelu_tanh": lambda x: Fn.gelu(x, approximate="tanh"),
          "relu": torch.relu, "tanh": torch.tanh}[act]
    want = fn(Fn.linear(a.double(), w.double(), bias.double())) + res.double()
    got = R.gemm(a, w, bias, res, act, F32, F64)
    assert float((got - want).abs().max()) < 1e-13
    # the float32 twin is the same formula: close, not equal, and independent of a BLAS blocking
    y32 = R.gemm(a, w, bias, res, act, F32, F32)
    assert y32.dtype == F32 and 0 < float((y32.double() - want).abs().max()) < 1e-5
    # output rounding comes last
    assert torch.equal(R.gemm(a, w, bias, res, act, BF16, F64), want.bfloat16().double())
    assert float((R.gemm(a, w, None, None, act, F32, F64) - fn(a.double() @ w.double().t())).abs().max()) < 1e-13


@pytest.mark.parametrize("affine", [True, False])
def test_gemm_ln_matches_torch(affine):
    c = R.ln_case(5, 24, 768, BF16, R.EPILOGUES[2], 7, affine=affine, ldx=772)
    x = c["x"].double()
    h = Fn.layer_norm(x, (768,), c["ln_w"].double() if affine else None,
                      c["ln_b"].double() if affine else None, 1e-5)
    assert float((R.layernorm(c["x"], c["ln_w"], c["ln_b"], 1e-5) - h).abs().max()) < 1e-12
    for rnd in (BF16, None):
        hr = h.bfloat16().double() if rnd is not None else h
        want = Fn.gelu(Fn.linear(hr, c["w"].double(), c["bias"].double()), approximate="tanh") + c["res"].double()
        got = R.gemm_ln(c["x"], c["ln_w"], c["ln_b"], 1e-5, c["w"], c["bias"], c["res"], "gelu_tanh",
                        F32, F64, round_ln=rnd)
        assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("row_norm,temp", [(False, 1.0), (True, 1.0), (False, 0.7)])
def test_lmhead_matches_torch_without_ties(row_norm, temp):
    g = torch.Generator().manual_seed(2)
    M, V, K, topk = 7, 300, 64, 5
    a, w = torch.randn(M, K, generator=g), torch.randn(V, K, generator=g)
    r = R.lmhead(a, w, topk, row_norm, temp)
    x = a.double()
    if row_norm:
        x = Fn.normalize(x, dim=-1, eps=1e-12)
    logits = x @ w.double().t() / float(torch.tensor(temp, dtype=F32))
    assert float((r["logits"] - logits).abs().max()) < 1e-12
    assert float((r["lse"] - torch.logsumexp(logits, -1)).abs().max()) < 1e-12
    tv, ti = torch.topk(logits, topk, dim=-1)
    assert torch.equal(r["gidx"], ti) and float((r["gval"] - tv).abs().max()) < 1e-12
    for b in range(3):
        blk = logits[:, b * 128:(b + 1) * 128]
        n = min(topk, blk.shape[1])
        tv, ti = torch.topk(blk, n, dim=-1)
        assert torch.equal(r["idx"][:, b, :n], ti + b * 128)
        assert float((r["val"][:, b, :n] - tv).abs().max()) < 1e-12
        assert torch.equal(r["stat"][:, b, 0], r["logits"][:, b * 128:(b + 1) * 128].max(-1)[0])
        lse = r["stat"][:, b, 0] + torch.log(r["stat"][:, b, 1])
        assert float((lse - torch.logsumexp(blk, -1)).abs().max()) < 1e-12
    # the partial last block (300 = 2 x 128 + 44) is full here; a short one is padded
    r3 = R.lmhead(a, w[:3], topk)
    assert r3["idx"][0, 0].tolist()[3:] == [R.PAD_IDX] * 2
    assert r3["val"][0, 0].tolist()[3:] == [-R.INF] * 2


# ------------------------------------------------------------------ the tie order
def test_tie_order_is_value_desc_then_index_asc():
    rnd = random.Random(5)
    for _ in range(300):
        n, k = rnd.randint(1, 40), rnd.choice(R.LM_TOPKS)
        vals = [float(rnd.randint(-2, 2)) for _ in range(n)]
        want = sorted(((v, i) for i, v in enumerate(vals)), key=lambda p: (-p[0], p[1]))[:k]
        want += [(-R.INF, R.PAD_IDX)] * (k - len(want))
        v, i = R.topk_sorted(torch.tensor([vals], dtype=F64), torch.arange(n)[None], k)
        assert list(zip(v[0].tolist(), i[0].tolist())) == want
    # the example of the fix: all logits 1 except column 40
    vals = [1.0] * 128
    vals[40] = 2.0
    v, i = R.topk_sorted(torch.tensor([vals], dtype=F64), torch.arange(128)[None], 5)
    assert i[0].tolist() == [40, 0, 1, 2, 3]


def test_register_insertion_old_loop_fails_new_loop_passes():
    """lmhead_kernel's select-only register insertion, emulated: the parent's bubble compares the
    displaced entry with strict > against its successor, so among equals it slides past (wrong
    lists); the kernel's loop now moves every entry behind the new one down: the stable order."""
    rnd = random.Random(1)
    bad = {False: 0, True: 0}
    for _ in range(2000):
        k = rnd.choice((2, 5, 8))
        vals = [float(rnd.randint(-2, 2)) for _ in range(32)]
        want = sorted(((v, i) for i, v in enumerate(vals)), key=lambda p: (-p[0], p[1]))[:k]
        for fixed in (False, True):
            bad[fixed] += R.bubble_insert(vals, k, fixed) != want
    assert bad[True] == 0 and bad[False] > 100, bad
    # the spike example, in the lane that holds column 40 on the ring epilogue
    lane = [s for s in R.lane_subsets("ring", 128) if 40 in s][0]
    vals = [2.0 if n == 40 else 1.0 for n in lane]
    assert [lane[i] for _, i in R.bubble_insert(vals, 5, True)] == [40, 0, 1, 2, 3]
    assert [lane[i] for _, i in R.bubble_insert(vals, 5, False)] == [40, 1, 2, 3, 8]


# ------------------------------------------------------------------ input conditions of the GPU cases
def _nan_outside(buf, rows, cols):
    m = torch.ones_like(buf, dtype=torch.bool)
    m[:rows, :cols] = False
    return bool(torch.isnan(buf[m].float()).all()) and not bool(torch.isnan(buf[~m].float()).any())


def test_sweep_cases_are_strided_and_padded_with_nan():
    seen = set()
    for route, (M, Nr, Na, K, dt, split) in R.SWEEPS.items():
        assert Nr % 8 and Nr % 4 and Na % 8 == 0 and K % 32 == 0
        for aligned in (False, True):
            for label, c in R.sweep(route, aligned):
                assert c["a"].dtype == dt and _nan_outside(c["abuf"], M, K), label
                assert _nan_outside(c["wbuf"], c["N"], K), label
                if c["rbuf"] is not None and not c["alias"]:
                    assert _nan_outside(c["rbuf"], M, c["N"]) and c["res"].stride(0) > c["N"], label
                seen.add(c["epi"])
    assert seen == set(R.EPILOGUES)
    # the table: every value of every column, and every scalar-fallback condition with either
    # output type
    cols = list(zip(*R.EPILOGUES))
    assert set(cols[0]) == {"none", "al", "off"} and set(cols[1]) == {"none", "pad4", "pad1", "alias"}
    assert set(cols[3]) == {"n", "n8", "n3", "off"} and set(cols[4]) == set(R.ACTS)
    for od in (F32, BF16):
        rows = [e for e in R.EPILOGUES if e[2] == od]
        assert {e[3] for e in rows} == {"n", "n8", "n3", "off"}
        assert {e[0] for e in rows} == {"none", "al", "off"}
        assert {"pad4", "pad1"} <= {e[1] for e in rows}
        assert set(R.ACTS) <= {e[4] for e in rows} | ({"none"} if od == BF16 else set())
    assert {e[2] for e in R.EPILOGUES if e[1] == "alias"} == {F32}      # the residual is f32


def test_strided_operand_builder():
    c = R.gemm_case(5, 9, 64, BF16, R.EPILOGUES[1], 3, lda=72, ldw=80)
    assert c["abuf"].shape == (6, 72) and c["wbuf"].shape == (10, 80)
    assert c["a"].stride(0) == 72 and c["w"].stride(0) == 80
    assert _nan_outside(c["abuf"], 5, 64) and _nan_outside(c["wbuf"], 9, 64)
    c2 = R.gemm_case(5, 9, 64, BF16, R.EPILOGUES[1], 3, lda=72, ldw=80)
    assert torch.equal(c["a"], c2["a"]) and torch.equal(c["res"], c2["res"])        # seeded
    ci = R.gemm_case(5, 9, 64, F32, R.EPILOGUES[3], 3, kind="ints")
    assert float(ci["a"].abs().max()) <= 3 and torch.equal(ci["a"], ci["a"].round())
    assert torch.equal(ci["bias"], ci["bias"].round()) and torch.equal(ci["res"], ci["res"].round())


def test_lm_cases_conditions():
    specs = R.lm_specs()
    assert len({s["id"] for s in specs}) == len(specs)
    for key, want in (("V", R.LM_VS), ("M", R.LM_MS), ("K", R.LM_KS), ("topk", R.LM_TOPKS),
                      ("mode", R.LM_MODES)):
        assert {s[key] for s in specs} == set(want)
    assert {(s["V"], s["M"]) for s in specs} >= {(v, m) for v in R.LM_VS for m in R.LM_MS}
    for mode in R.LM_MODES:
        mine = [s for s in specs if s["mode"] == mode]
        assert {s["K"] for s in mine} == set(R.LM_KS)
        assert {min(s["topk"], 2) + (s["topk"] > 5) for s in mine} == {1, 2, 3}     # KMAX 1, 5, 8
        assert {s["M"] <= 64 for s in mine} == {True, False}                        # BM 64, 128
        assert {s["row_norm"] for s in mine} == {True, False}
        assert {s["temp"] for s in mine} == {1.0, 0.7}
        assert {s["knobs"]["fast_xcd"] for s in mine} == {0, 1}
    assert {s["knobs"]["lm_prio"] for s in specs} == {0, 1}
    # lm_prio acts only on the bf16 K % 64 == 0 main loop without row_norm: off there on a list
    assert any(s["knobs"]["lm_prio"] == 0 and s["mode"] == "bf16" and s["K"] % 64 == 0
               and not s["row_norm"] and s["topk"] >= 2 for s in specs)
    assert {s["stat"] for s in specs} == {True, False}
    assert not any(s["row_norm"] and s["temp"] != 1.0 for s in specs)      # refused by the entry
    for s in specs:
        c = R.lm_build(s)
        assert _nan_outside(c["abuf"], s["M"], s["K"]) and _nan_outside(c["wbuf"], s["V"], s["K"]), s["id"]
        assert c["abuf"].shape[1] == s["lda"] and s["lda"] % 8 == 0
        k1 = s["topk"] + 1
        r = R.lmhead(c["a"], c["w"], k1, s["row_norm"], s["temp"])
        # exact logits: the float32 run gives the same bits where nothing is divided
        if not s["row_norm"] and s["temp"] == 1.0:
            assert torch.equal(R.lmhead(c["a"], c["w"], k1, dtype=F32)["logits"].double(), r["logits"])
        # top-(k + 1) margins: 0 (a tie: the order is checked) or >= 1e-3
        for lists in (r["val"], r["gval"]):
            d = R.margins(lists)
            assert bool(((d == 0) | (d >= 1e-3)).all()), (s["id"], float(d[d > 0].min()))
        if s["kind"] in ("ints", "spike") and s["topk"] > 1 and s["V"] >= 100:
            # ties inside one lane's column subset that the old insertion loop gets wrong
            path = "tile" if s["mode"] == "f32_tile" else "ring"
            wrong = ties = 0
            for row in range(min(s["M"], 8)):
                for blk in range((s["V"] + 127) // 128):
                    lo = blk * 128
                    for sub in R.lane_subsets(path, s["V"] - lo, 64 if s["M"] <= 64 else 128):
                        vals = r["logits"][row, lo:lo + 128][sub].tolist()
                        ties += len(set(vals)) < len(vals)
                        kmax = 5 if s["topk"] <= 5 else 8
                        wrong += R.bubble_insert(vals, kmax, False) != R.bubble_insert(vals, kmax, True)
            assert ties > 0 and (wrong > 0 or not s["id"].startswith("tie-")), s["id"]


def test_ln_cases_conditions():
    specs = R.ln_specs()
    assert {s["M"] for s in specs} == set(R.LN_MS) and {s["K"] for s in specs} == {768, 1024}
    assert {s["ldx"] - s["K"] for s in specs} == {0, 4}
    for s in specs + R.ln_f32_specs():
        c = R.ln_build(s)
        assert _nan_outside(c["xbuf"], s["M"], s["K"]), s["id"]
        assert float(c["x"][:, 5].min()) > 25                    # the outlier column
    assert {(s["K"], s["affine"]) for s in R.ln_f32_specs()} == {
        (768, True), (1024, True), (768, False), (1024, False), (3072, False)}
    assert all(s["epi"][2] == F32 for s in R.ln_f32_specs())
    # the whole epilogue table on zs_gemm_ln, with and without the affine, ragged and aligned N
    for affine in (True, False):
        sw = R.ln_epi_specs(affine)
        assert all(s["affine"] == affine for s in sw)
        for N in (202, 144):
            assert [s["epi"] for s in sw if s["N"] == N] == list(R.EPILOGUES)
        assert 202 % 4 and 144 % 48 == 0 and len({s["seed"] for s in sw}) == len(sw)
        for s in sw[::5]:
            assert _nan_outside(R.ln_build(s)["xbuf"], s["M"], s["K"]), s["id"]


def test_activation_slopes_bound_the_derivative():
    """ACT_SLOPE (what carries an A-element rounding tie through the epilogue) bounds each
    activation's slope, and tightly."""
    x = torch.linspace(-8, 8, 160001, dtype=F64)
    for act in R.ACTS:
        y = R.act_apply(x, act)
        slope = float(((y[1:] - y[:-1]) / (x[1:] - x[:-1])).abs().max())
        assert slope <= R.ACT_SLOPE[act] <= slope + 2e-3, (act, slope)


def test_knob_defaults_match_the_library():
    """gemm_ref.KNOB_DEFAULTS (what the GPU tests restore to) against the g_* initialisers."""
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "zero-shot-aac_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("gemm.hip", "lmhead.hip", "gemm_rows.hip", "gemm_skinny.hip"))
    for k, v in R.KNOB_DEFAULTS.items():
        m = re.search(r"^(?:static )?int g_%s = (\w+);" % k, text, re.M)
        assert m, k
        init = m.group(1)
        if not init.isdigit():                   # lean128_ns: a macro with a default
            init = re.search(r"^#define %s (\d+)" % init, text, re.M).group(1)
        assert int(init) == v, (k, init)
        assert re.search(r'strcmp\(key, "%s"\)' % k, text), k
    assert re.search(r"constexpr int SK_MAX_TILES = %d;" % R.SK_MAX_TILES, text)


# ------------------------------------------------------------------ the mutants
def _moved(ref, mut, tol):
    return bool((~((ref - mut).abs() <= 2 * tol)).any())       # NaN counts as moved


def test_mutant_list_is_complete():
    assert set(R.MUTANT_CASES) == set(R.MUTANTS)


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_mutant_moves_a_gpu_case(mut):
    kind, build = R.MUTANT_CASES[mut]
    if kind == "gemm":
        c = build()
        ref, yard, tol = R.gemm_expect(c)
        kps = R.k_per_split(c["K"], R.SWEEPS["splitk"][5])
        assert _moved(ref, R.gemm_expect(c, mut, k_per_split=kps), tol)
    elif kind == "ln":
        c = build()
        ref, yard, tol = R.ln_expect(c, BF16)
        assert _moved(ref, R.ln_expect(c, BF16, mut), tol)
    else:
        s = R.lm_named(build)
        assert s["stat"] or mut != "lse_block_max"
        c, topk, row_norm, temp = R.lm_build(s), s["topk"], s["row_norm"], s["temp"]
        r64 = R.lmhead(c["a"], c["w"], topk, row_norm, temp)
        r32 = R.lmhead(c["a"], c["w"], topk, row_norm, temp, dtype=F32)
        rm = R.lmhead(c["a"], c["w"], topk, row_norm, temp, mut=mut)
        if mut == "tie_high":
            assert not torch.equal(r64["idx"], rm["idx"])        # indices are compared exactly
        elif mut == "lse_block_max":
            # against the bound the GPU test applies to the sum-exp (with the summation term)
            yard, tol = R.lm_stat_tolerance(r64, r32)["sumexp"]
            assert _moved(r64["stat"][..., 1], rm["stat"][..., 1], tol)
            yard, tol = R.lm_stat_tolerance(r64, r32)["lse"]
            assert _moved(r64["lse"], rm["lse"], tol)
        else:
            fin = torch.isfinite(r64["val"])
            yard, tol = R.tolerance(r64["val"][fin], r32["val"][fin])
            assert _moved(r64["val"][fin], rm["val"][fin], tol)
