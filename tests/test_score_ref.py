"""CPU: the input conditions tests/test_gpu_score_kernels.py relies on (tests/score_ref.py), the
references against the oracle's own arithmetic, CaptionScores on hand-made tensors, and the
scoring ops' refusal of host tensors."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as R  # noqa: E402

I32 = torch.int32


# ------------------------------------------------------------------ lm cases
@pytest.mark.parametrize("case", R.LM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_lm_case_conditions(case):
    """Every row's float64 top-2 margin is >= 1e-3 (the GPU test asserts exact argmax ids), the
    operands are exactly representable in the case's dtype, and the special rows are what they
    claim."""
    V, M, K, dt = case
    d = R.lm_case(*case)
    assert d["a"].shape == (M, K) and d["w"].shape == (V, K) and d["tgt"].shape == (M,)
    assert float(R.top2_margin(d["logits"]).min()) >= R.MARGIN
    assert torch.equal(R.logits64(d["a"].float(), d["w"].float()), d["logits"])
    lse, amax, tl, lp, valid = R.nll_rows(d["logits"], d["tgt"])
    assert torch.equal(amax.long(), d["logits"].argmax(-1))      # (no ties at this margin)
    if d["own"] is not None:
        assert int(d["tgt"][d["own"]]) == int(amax[d["own"]])
    if d["spike"] is not None:
        r, j = d["spike"]
        row = d["logits"][r].clone()
        assert int(amax[r]) == j and int(d["tgt"][r]) != j
        top = float(row[j])
        row[j] = -math.inf
        assert 40.0 <= top - float(row.max()) and 55.0 <= top <= 65.0
        assert float(lp[r]) < -40.0
    assert bool(((lp <= 0) & torch.isfinite(lp)).all())
    assert bool((lp[~valid] == 0).all())


def test_lm_cases_cover_every_edge():
    """Across the case list: targets 0, 127, 128, V - 1, one inside a partial last block, the
    ignored -1 and V, a row whose target is its argmax, a spike row; V with one partial block, one
    full block, full blocks + a partial one, and the model's vocabulary; the 64-row tile, the
    128-row tile with a partial tile, one row; K on and off the K % 64 path; both dtypes."""
    seen = set()
    for case in R.LM_CASES:
        V, M, K, dt = case
        d = R.lm_case(*case)
        t = d["tgt"].tolist()
        nfull = (V // R.LM_BN) * R.LM_BN
        for name, ok in (("0", 0 in t), ("127", 127 in t and V > 127), ("128", 128 in t and V > 128),
                         ("V-1", V - 1 in t), ("-1", -1 in t), ("V", V in t),
                         ("partial", V % R.LM_BN != 0 and any(nfull <= x < V - 1 for x in t)),
                         ("own", d["own"] is not None), ("spike", d["spike"] is not None)):
            if ok:
                seen.add((name, dt))
        seen.add(("V", V)), seen.add(("M", M)), seen.add(("K64", K % 64 == 0, dt))
    for dt in ("f32", "bf16"):
        for name in ("0", "127", "128", "V-1", "-1", "V", "partial", "own", "spike"):
            assert (name, dt) in seen, (name, dt)
        assert ("K64", True, dt) in seen and ("K64", False, dt) in seen
    assert {("V", 81), ("V", 128), ("V", 1000), ("V", 50257), ("M", 1), ("M", 64), ("M", 70)} <= seen
    assert all(K % 32 == 0 for _, _, K, _ in R.LM_CASES)


def test_nll_rows_equals_log_softmax():
    d = R.lm_case(1000, 70, 768, "f32")
    lse, amax, tl, lp, valid = R.nll_rows(d["logits"], d["tgt"])
    ls = torch.log_softmax(d["logits"], -1)
    want = ls.gather(1, d["tgt"].clamp(0, 999).long()[:, None])[:, 0]
    assert float((lp[valid] - want[valid]).abs().max()) < 1e-12
    s, n = R.caption_sums(lp, valid, *R.split_rows(70))
    assert int(n.sum()) == int(valid.sum()) and abs(float(s.sum()) - float(lp.sum())) < 1e-9
    # ties: the first maximum
    z = torch.zeros(2, 5, dtype=torch.float64)
    z[1, 3] = z[1, 4] = 2.0
    assert R.nll_rows(z, torch.tensor([0, 4], dtype=I32))[1].tolist() == [0, 3]


# ------------------------------------------------------------------ embed cases
def test_embed_case_conditions():
    d = R.embed_case(40)
    hs, ts = set(d["hard_len"].tolist()), set(d["cap_len"].tolist())
    assert {0, 1, R.EMBED_HCAP} <= hs and {0, 1, R.EMBED_TMAX} <= ts
    Smax = R.EMBED_HCAP + R.EMBED_NSOFT + R.EMBED_TMAX - 1
    x, plen, rows, tgt, bad = R.score_embed(d["hard_ids"], d["hard_len"], d["soft"], d["soft_ld"],
                                            R.EMBED_NSOFT, d["cap_ids"], d["cap_len"], d["wte"],
                                            d["wpe"], d["B"], Smax)
    assert bad == 0 and int(plen.max()) == Smax
    for b in range(d["B"]):
        H, T = int(d["hard_len"][b]), int(d["cap_len"][b])
        assert int(plen[b]) == H + R.EMBED_NSOFT + max(T - 1, 0)
        assert bool((x[b, int(plen[b]):] == 0).all())
        assert tgt[b, :T].tolist() == d["cap_ids"][b, :T].tolist() and bool((tgt[b, T:] == -1).all())
        # the row that predicts cap[t] holds cap[t - 1] (or the last soft row)
        assert rows[b, :T].tolist() == [b * Smax + H + R.EMBED_NSOFT - 1 + t for t in range(T)]
        assert all(b * Smax <= r < b * Smax + max(int(plen[b]), 1) for r in rows[b].tolist())
    for kind in ("cap_mid", "cap_last", "hard"):
        e = R.embed_case(40, kind)
        out = R.score_embed(e["hard_ids"], e["hard_len"], e["soft"], e["soft_ld"], R.EMBED_NSOFT,
                            e["cap_ids"], e["cap_len"], e["wte"], e["wpe"], e["B"], Smax)
        assert out[4] == 1
        assert int((out[3] != tgt).sum()) == (0 if kind == "hard" else 1)
        assert not torch.equal(out[0], x) or kind == "cap_last"


def test_score_layout_matches_oracle_conditioning():
    """The scored sequence is the one generate2 conditions on: with the oracle's GPT-2 on
    [wte(hard) ; soft ; wte(cap[:-1])], the row at H + n - 1 + t predicts cap[t] -- teacher-forced
    on a golden's own greedy ids the argmax there is that id."""
    import numpy as np
    from oracle import caption as OC
    from zsaac import synthetic as S
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                  "c1_greedy.npz")))
    sd = S.gpt2_state_dict(seed=0, std=0.1, emb_std=0.1, stop_boost=2.0)
    sd.update(S.mlp_mapper_state_dict(1))
    b, T = 3, 3
    H = int(g["hard_len"][b])
    ids = torch.from_numpy(g["greedy_ids"][b, :T])
    emb = torch.nn.functional.normalize(torch.from_numpy(g["clap_emb"][b:b + 1]), dim=-1)
    with torch.no_grad():
        pe = OC.clap_to_gpt(emb[None], torch.from_numpy(g["hard_ids"][b:b + 1, :H]), sd)
        seq = torch.cat((pe, sd["gpt.transformer.wte.weight"][ids[:-1]][None]), dim=1)
        logits = OC.gpt2_logits(seq, sd)[0][0]
    assert seq.shape[1] == H + 10 + T - 1
    assert logits[H + 10 - 1:].argmax(-1).tolist() == ids.tolist()


# ------------------------------------------------------------------ CaptionScores
def _scores():
    from zsaac.score import CaptionScores
    lp = torch.tensor([[-1.0, -2.0, 0.0], [0.0, 0.0, 0.0], [-0.5, 0.0, 0.0]])
    tg = torch.tensor([[5, 6, -1], [-1, -1, -1], [9, -1, -1]], dtype=I32)
    am = torch.tensor([[5, 7, -1], [-1, -1, -1], [9, -1, -1]], dtype=I32)
    return CaptionScores(lp, am, lp.sum(1), torch.tensor([2, 0, 1], dtype=I32), tg,
                         torch.zeros(1, dtype=I32))


def test_caption_scores_arithmetic():
    from zsaac._lib import ZsError
    from zsaac.score import CaptionScores
    s = _scores()
    m = s.mean_nll()
    assert m[0] == 1.5 and math.isnan(float(m[1])) and m[2] == 0.5
    assert s.perplexity() == pytest.approx(math.exp(3.5 / 3))
    assert s.accuracy() == pytest.approx(2 / 3)
    both = CaptionScores.cat([s, _scores()])
    assert both.n_tokens.tolist() == [2, 0, 1, 2, 0, 1]
    assert both.perplexity() == pytest.approx(s.perplexity())
    empty = CaptionScores(torch.zeros(1, 2), torch.full((1, 2), -1, dtype=I32), torch.zeros(1),
                          torch.zeros(1, dtype=I32), torch.full((1, 2), -1, dtype=I32))
    assert math.isnan(empty.perplexity()) and math.isnan(empty.accuracy())
    assert math.isnan(float(empty.mean_nll()[0]))
    bad = _scores()
    bad.status = torch.ones(1, dtype=I32)
    with pytest.raises(ZsError):
        bad.mean_nll()


def test_reference_ids_follow_the_training_tokenisation():
    from zsaac.predict import reference_ids

    class Tok:
        def encode(self, s):
            return [ord(c) for c in s]
    assert reference_ids(Tok(), {"caption": "A dog"}, 67) == [ord(c) for c in "A dog."]
    assert reference_ids(Tok(), "A dog.", 67) == [ord(c) for c in "A dog."]
    assert reference_ids(Tok(), "A dog barks", 4) == [ord(c) for c in "A do"]


# ------------------------------------------------------------------ ops refuse host tensors
def test_scoring_ops_refuse_cpu_tensors():
    from zsaac import ops
    from zsaac._lib import ZsError
    V, K, M = 81, 32, 2
    f = torch.zeros
    with pytest.raises(ZsError):
        ops.lmhead_nll(f(M, K), f(V, K), f(M, dtype=I32), f(M, 1, 2), f(M, 1), f(M, 1, dtype=I32), f(M))
    with pytest.raises(ZsError):
        ops.nll_finalize(f(M, 1, 2), f(M, 1), f(M, 1, dtype=I32), f(M, dtype=I32), f(M), V, 1, M,
                         f(M), f(M, dtype=I32), f(1), f(1, dtype=I32))
    with pytest.raises(ZsError):
        ops.score_embed(f(1, 3, dtype=I32), f(1, dtype=I32), f(1, 64), 64, 2, f(1, 4, dtype=I32),
                        f(1, dtype=I32), f(V, K), f(16, K), 1, 8, f(8, K), f(1, dtype=I32),
                        f(1, 4, dtype=I32), f(1, 4, dtype=I32), f(1, dtype=I32))


def test_scoring_entries_validate_before_launch():
    """Bad shapes fail on the host with a message (no launch): K % 32, M = B x Tmax, Smax."""
    from zsaac import _lib
    lib = _lib.lib()
    assert lib.zs_lmhead_nll(4, 30, 81, 0, None, 32, None, None, None, None, None, None, None) == -1
    assert "zs_lmhead_nll" in _lib.last_error()
    assert lib.zs_nll_finalize(None, None, None, None, None, 6, 1, 81, 2, 4, None, None, None,
                               None, None, None) == -1
    assert "M = B x Tmax" in _lib.last_error()
    assert lib.zs_gpt2_score_embed(None, None, 3, None, 64, 2, None, None, 4, None, None, 50, 1,
                                   7, 32, None, None, None, None, None, 0, None) == -1
    assert "Smax" in _lib.last_error()
