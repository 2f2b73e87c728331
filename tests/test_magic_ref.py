"""CPU tests that pin tests/magic_ref.py, the reference the magic-kernel GPU tests compare
against: its step / maxcos / score functions against oracle/magic.py on scripted data, and the
input conditions (selection margins, the situations every scenario must contain, decoys that
would win) of every case of tests/test_gpu_magic_kernels.py, so a bad seed fails here and not on
the GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import magic_ref as M  # noqa: E402
from oracle import magic as OM  # noqa: E402

P0 = 3      # prompt rows in front of the generated tokens


# ------------------------------------------------------------------ step against generate_beam_magic
ORACLE_STEP = [(b, W, seed) for b in (1, 2, 3, 5, 8) for W in (b, 25, 64) for seed in (0, 1, 2)]
ALL_STOP = {0: None, 1: 4, 2: 7}      # the step at which every candidate is the stop token


@pytest.mark.parametrize("b,W,seed", ORACLE_STEP)
def test_step_ref_matches_oracle(monkeypatch, b, W, seed):
    """oracle.magic.generate_beam_magic with compute_magic_score scripted (the scores and
    candidate ids of a Scenario, the rows in beam order) against magic_ref.step on the same
    script: token lists best-first and final scores.  Seeds 1 and 2 stop every beam at step 4 / 7
    of 10."""
    entry = 10
    sc = M.Scenario(1, b, W, False, 100 + seed, (P0,), (entry,), entry, P0 + entry + 1, (0.15,),
                    (ALL_STOP[seed],))
    assert M.selection_margin([d for info in sc.info for d in info]) >= M.MARGIN
    calls = []

    def scripted(generated, sd, width, input_token, *a, **kw):
        s = generated.shape[1] - P0
        bsz = generated.shape[0]
        assert width == W and bsz == (1 if s == 0 else b)
        calls.append(s)
        score_v, cand = sc.inputs[s]
        return (score_v.view(b, W)[:bsz].clone().view(bsz, 1, W),
                cand.view(b, W)[:bsz].long().clone())
    monkeypatch.setattr(OM, "compute_magic_score", scripted)
    sd = {"gpt.transformer.wte.weight": torch.zeros(M.VOCAB, 2)}
    toks, scores = OM.generate_beam_magic(torch.zeros(1, P0, 2), sd, None, None, None, 1.0,
                                          beam_size=b, entry_length=entry, magic_width=W,
                                          stop_token_index=M.STOP)
    final = sc.states[-1]
    rt, rs = M.beam_result(final, 0, b)
    assert all(x - y >= 1e-4 for x, y in zip(rs[:-1], rs[1:])), rs   # argsort's tie order is no contract
    assert rt == toks
    assert max(abs(x - y) for x, y in zip(rs, scores)) <= 1e-5, (rs, scores)
    # the oracle left its loop exactly when the reference froze the clip
    assert int(final["ntok"][0]) == len(calls) and int(final["cdone"][0]) == 1
    if ALL_STOP[seed] is not None:
        assert len(calls) <= ALL_STOP[seed] + 1 < entry and bool(final["stopped"].all())
        for key in M.STATE_KEYS:          # later calls change nothing
            assert torch.equal(sc.states[len(calls) - 1][key], final[key]), key


@pytest.mark.parametrize("W,stop_at,seed", [(15, 4, 0), (15, None, 1), (1, 2, 2), (64, 6, 3)])
def test_greedy_ref_matches_oracle(W, stop_at, seed):
    """The greedy branch against oracle.magic.ranking's argmax and magic_search's stop rule
    (append the chosen id, leave after the stop token) on random hidden states."""
    g = torch.Generator().manual_seed(seed)
    steps, Dh = 8, 16
    ids, inputs = [], []
    alive = True
    for s in range(steps):
        ctx = torch.randn(1, P0 + s, Dh, generator=g).repeat_interleave(W, 0)
        nxt = torch.randn(W, 1, Dh, generator=g)
        probs = torch.rand(1, W, generator=g)
        clap = torch.log_softmax(torch.randn(1, W, generator=g), -1)
        sel, sv = OM.ranking(ctx, nxt, probs, 0.1, 0.2, clap, W)
        top = torch.sort(sv[0], descending=True).values
        assert W == 1 or float(top[0] - top[1]) >= 1e-6     # argmax ties are no contract of torch.max
        cand = torch.randint(20, M.VOCAB, (W,), generator=g, dtype=M.I32)
        if W > 1:
            cand[(int(sel[0]) + 1) % W] = M.STOP            # offered, not taken
        if stop_at == s:
            cand[int(sel[0])] = M.STOP
        inputs.append((sv[0].clone(), cand))
        if alive:
            ids.append(int(cand[int(sel[0])]))
            alive = ids[-1] != M.STOP
    state = M.step_init(1, 1, W, (P0,), steps, P0 + steps + 1)
    mx = torch.tensor([steps], dtype=M.I32)
    for s, (sv, cand) in enumerate(inputs):
        state = M.step(state, sv, cand, 1, W, s == 0, True, M.STOP, s, mx)
    assert state["tokens"][0, :int(state["ntok"][0])].tolist() == ids
    assert int(state["cdone"][0]) == 1 and float(state["scores"][0]) == 0.0
    assert (ids[-1] == M.STOP) == (stop_at is not None) and len(ids) == (stop_at + 1 if stop_at is not None else steps)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("alpha,beta", [(0.1, 0.2), (0.6, 1.0)])
def test_maxcos_score_ref_matches_oracle(b, alpha, beta):
    """maxcos + score against oracle.magic.ranking fed with clap_log_softmax (prefix_length 1,
    one clip, every beam active); the beams' contexts are scattered over the physical rows."""
    W, p, E, Lmax, temp = 5, 4, 32, 7, 0.07
    g = torch.Generator().manual_seed(b)
    R = b * W
    ctx_b = torch.randn(b, p, M.D, generator=g)
    hid = torch.randn(R, M.D, generator=g) + ctx_b[:, 0].repeat_interleave(W, 0) * 0.5
    probs = -torch.rand(b, W, generator=g) * 8
    text, audio = torch.randn(R, E, generator=g), torch.randn(1, E, generator=g)
    clap = OM.clap_log_softmax(audio, text, temp)
    _, want = OM.ranking(ctx_b.repeat_interleave(W, 0), hid[:, None, :], probs, alpha, beta, clap, W, 1)
    ctx = torch.full((R, Lmax, M.D), 100.0)
    kvrow = torch.full((b, Lmax), M.JUNK, dtype=M.I32)
    for t in range(p):
        rows = torch.randperm(R, generator=g)[:b]
        kvrow[:, t] = rows.to(M.I32)
        ctx[rows, t] = ctx_b[:, t]
    pos = torch.full((b,), p, dtype=M.I32)
    mc, ctx2 = M.maxcos(hid, W, ctx, kvrow, pos)
    assert torch.equal(ctx2[torch.arange(R), p], hid)
    ctx2[torch.arange(R), p] = ctx[torch.arange(R), p]
    assert torch.equal(ctx2, ctx)
    got = M.score(probs.reshape(-1), mc, text, audio, b, W, b, temp, alpha, beta, 1.0,
                  torch.zeros(R))
    assert float((got - want.reshape(-1).double()).abs().max()) <= 2e-5
    half = M.score(probs.reshape(-1), mc, text, audio, b, W, b, temp, alpha, beta, 0.5, torch.zeros(R))
    assert torch.allclose(half, got * 2.0, rtol=1e-12, atol=0)


def test_small_refs():
    x = torch.tensor([[1.0, 3.0, 3.0, -float("inf"), 2.0, 3.0, 9.0]])
    v, i = M.row_topk(x, 6, 4, 0)                       # the 9 lies past V
    assert i.tolist() == [[1, 2, 5, 4]]
    assert abs(float(v[0, 0]) - (3.0 - float(torch.logsumexp(x[0, :6].double(), 0)))) < 1e-12
    v1, i1 = M.row_topk(x, 6, 6, 1)
    assert i1.tolist() == [[1, 2, 5, 4, 0, 3]] and float(v1[0, 5]) == 0.0
    assert abs(float(v1.sum()) - 1.0) < 1e-12
    kv = torch.arange(12, dtype=M.I32).view(2, 6)
    out, pc = M.expand(kv, torch.tensor([2, 5]), 2, torch.full((4, 6), -7, dtype=M.I32))
    assert out.tolist() == [[0, 1, -7, -7, -7, -7]] * 2 + [[6, 7, 8, 9, 10, -7]] * 2
    assert pc.tolist() == [2, 2, 5, 5]
    n = M.l2norm_rows(torch.tensor([[3.0, 4.0], [0.0, 0.0]]))
    assert n.tolist() == [[0.6, 0.8], [0.0, 0.0]]
    g = torch.Generator().manual_seed(0)
    y = torch.randn(2, M.D, generator=g, dtype=torch.float64)
    w, b = torch.randn(M.D, generator=g), torch.randn(M.D, generator=g)
    ref = torch.nn.functional.layer_norm(y, (M.D,), w.double(), b.double(), 1e-12)
    flat = torch.full((2 * 2 * M.D,), -7.0)
    got = M.layernorm_dual(y.reshape(-1), 2, M.D, w, b, 1e-12, flat, 2 * M.D)
    assert float((M.rows_view(got, 2, 2 * M.D) - ref).abs().max()) < 1e-12
    assert bool((got.view(2, 2, M.D)[:, 1] == -7.0).all())


# ------------------------------------------------------------------ input conditions of the GPU cases
STEP_SCENARIOS = [(b, W, False) for b, W in M.STEP_BEAM] + [(1, W, True) for W in M.STEP_GREEDY_W]


@pytest.mark.parametrize("b,W,greedy", STEP_SCENARIOS)
def test_gpu_step_scenario_conditions(b, W, greedy):
    """Margins and content of the scenario test_gpu_magic_kernels.py replays at (b, W)."""
    sc = M.step_scenario(b, W, greedy)
    assert M.selection_margin([d for info in sc.info for d in info]) >= M.MARGIN
    # float32 makes the same choices (the yardstick compares like with like)
    for a, f in zip(sc.states, sc.replay(M.F32)):
        for key in M.STATE_KEYS[2:] + ("sel_c",):
            assert torch.equal(a[key], f[key]), key
        assert torch.equal(a["seq_len"], f["seq_len"].double())
    y = sc.yardstick()
    print(f"step ({b}, {W}, greedy={greedy}): yardstick {y:.3e}, situations {sorted(sc.props())}")
    assert y < 1e-4
    want = {"ragged_pos", "frozen_by_limit_beside_live", "frozen_by_stop_beside_live",
            "last_legal_step"}
    if greedy:
        want.add("greedy_stop")
        if W > 1:
            want.add("stop_offered_not_taken")
    elif b >= 2:
        want |= {"overwritten_before_read", "stopped_survives"}
    props = sc.props()
    assert want <= props, want - props
    if not greedy and b >= 2:
        assert props & {"source_permutation", "duplicated_source"}
    # positions stay inside the maps and the token rows
    for st in sc.states:
        assert int(st["pos"].max()) <= M.STEP_LMAX - 1 and int(st["ntok"].max()) <= M.STEP_SMAX
    # a frozen clip keeps every field over the later calls
    for k in range(M.STEP_C):
        froze = [s for s, st in enumerate(sc.states) if int(st["cdone"][k])][0]
        for st in sc.states[froze + 1:]:
            for key in ("scores", "seq_len", "stopped", "tokens", "kvrow", "pos", "sel_c"):
                assert torch.equal(st[key][k * b:(k + 1) * b], sc.states[froze][key][k * b:(k + 1) * b])
            assert int(st["ntok"][k]) == froze + 1


def test_gpu_step_scenarios_between_them():
    props = set()
    for b, W in M.STEP_BEAM:
        props |= M.step_scenario(b, W, False).props()
    assert {"source_permutation", "duplicated_source", "overwritten_before_read"} <= props


@pytest.mark.parametrize("name", ["first", "greedy", "beam"])
def test_gpu_step_tie_cases(name):
    """The exact-tie steps hold the ties they claim (equal selection values, in float32 too) and
    the reference resolves them by flat index."""
    c = M.tie_cases()[name]
    for dt in (M.F64, M.F32):
        st = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in c["state"].items()}
        info: list = []
        M.step(st, c["score"], c["cand"], c["b"], c["W"], c["first"], c["greedy"], M.STOP,
               c["step"], c["max_steps"], info=info)
        for d, want in zip(info, c["want"]):
            assert list(zip(d["src"], d["w"])) == want
            n = len(want)
            assert d["top"][n - 1] == d["top"][n], "a tie at the kept / dropped edge"
            if name == "beam":
                assert len(set(d["top"])) == 1


@pytest.mark.parametrize("name", list(M.MAXCOS_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gpu_maxcos_case_conditions(name, dtype):
    """Every slot of ctx outside the beams' histories would beat every true cosine; no history
    slot is written by the launch; positions run from 1 to Lmax - 1."""
    C, b, W, pos = M.MAXCOS_CASES[name]
    Lmax = M.MAXCOS_LMAX
    hid, ctx, kvrow, used = M.maxcos_case(C, b, W, Lmax, pos, 3, dtype)
    mc, _ = M.maxcos(hid, W, ctx, kvrow, torch.tensor(pos))
    assert len(set(pos)) == len(pos) and max(pos) <= Lmax - 1 and min(pos) >= 1
    if name == "20cand":
        assert min(pos) == 1 and max(pos) == Lmax - 1
    written = {(c, pos[c // W]) for c in range(C * b * W)}
    assert not (written & used)
    h = hid.double()
    h = h / h.norm(dim=-1, keepdim=True)
    decoy = torch.ones(ctx.shape[:2], dtype=torch.bool)
    for r, t in used:
        decoy[r, t] = False
    d = ctx.double()[decoy]
    d = d / d.norm(dim=-1, keepdim=True)
    assert float((d @ h.t()).min()) > float(mc.max()) + 0.05
    for j in range(C * b):                  # a history is spread over several rows of its clip
        rows = kvrow[j, :pos[j]].tolist()
        assert all(j // b * b * W <= r < (j // b + 1) * b * W for r in kvrow[j].tolist())
        assert pos[j] < 3 or len(set(rows)) >= 2


@pytest.mark.parametrize("V", [50257, 1000, 1025, 40])
def test_gpu_topk_tie_rows(V):
    x = M.topk_tie_rows(V)
    k = min(V, 64)
    _, i = M.row_topk(x, V, k, 0)
    assert i[0, :3].tolist() == [5, M.topk_tie_second(V), V - 1]
    if V > 3072:
        assert i[1, :3].tolist() == [7, 1031, 2055]
        assert i[4, :4].tolist() == [3000, 6, 1030, 2054]
    assert i[2].tolist() == list(range(k))
    fin = [c for c in range(V) if c % 3]
    if k == V:                              # every column is returned: the -inf ones last, in order
        assert i[3, len(fin):].tolist() == [c for c in range(V) if c % 3 == 0]
    assert torch.equal(x.float().double(), x.double())


@pytest.mark.parametrize("b,W,nact", M.SCORE_SHAPES)
def test_gpu_score_case_conditions(b, W, nact):
    for E in M.SCORE_E:
        pval, mc, text, audio = M.score_case(3, b, W, nact, E, 1)
        out = M.score(pval, mc, text, audio, b, W, nact, M.SCORE_TEMP, 0.1, 0.2, 1.0,
                      torch.full((3 * b * W,), -7.0))
        idle = (torch.arange(3 * b * W) % (b * W)) >= nact * W
        assert bool((out[idle] == -7.0).all()) and bool(torch.isfinite(out[~idle]).all())
        assert bool(torch.isnan(text[idle]).all()) and int(idle.sum()) == 3 * (b - nact) * W
        t, a = text[~idle].double(), audio.double()[(torch.arange(3 * b * W) // (b * W))[~idle]]
        cos = (t * a).sum(-1) / (t.norm(dim=-1) * a.norm(dim=-1))
        assert float(cos.max()) > 0.3 and float(cos.min()) < 0.1     # CLAP-like spread
