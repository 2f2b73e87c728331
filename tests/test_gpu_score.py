"""Teacher-forced scoring end to end (zsaac.score.CaptionScorer) against the CPU oracle.

Reference recipe (float64 log-softmax of the oracle's f32 logits): the golden's weights
(S.gpt2_state_dict(**golden_gpt2_kw(g)) + S.mlp_mapper_state_dict(1)), F.normalize(emb),
OC.clap_to_gpt, the caption's wte rows appended (all but the last), OC.gpt2_logits.  Teacher-forced
on a golden's own greedy ids this recipe reproduces those ids.

Tolerances: f32 per token 2 x 1e-4 x max|reference logit| -- the project's full-logit bound
(test_gpt_full_logits) applied to the target logit and to the lse; a sum over tokens that bound
times the token count; bf16 at the first scored position 2 x the golden's bf16_ref_err (the
position that error was measured at; a log-prob is a difference of two such quantities).  Later
bf16 positions are printed, not asserted."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
LOGIT_REL = 1e-4        # test_gpt_full_logits: max |logit error| <= 1e-4 x max|logit|


def _load(name):
    from tools.idparity import load
    return load(name)


def _sd(g):
    from tools.idparity import golden_gpt2_kw
    from zsaac import synthetic as S
    sd = S.gpt2_state_dict(**golden_gpt2_kw(g))
    sd.update(S.mlp_mapper_state_dict(1))
    return sd


def _pipe(sd, dtype, batch, beam=0, audio_sd=None):
    from zsaac import synthetic as S
    from zsaac.pipeline import CaptionConfig, CaptionPipeline
    cfg = CaptionConfig(dtype=dtype, batch=batch, beam=beam)
    return CaptionPipeline(sd, audio_sd, S.label_table(), S.label_token_table(), cfg)


def _oracle(sd, emb, hard, ids):
    """(float64 log-softmax rows [T, V] predicting ids[0..T-1], max |logit| of those rows)."""
    from oracle import caption as OC
    with torch.no_grad():
        pe = OC.clap_to_gpt(torch.nn.functional.normalize(emb.float(), dim=-1)[None],
                            torch.as_tensor(hard, dtype=torch.long)[None], sd)
        tail = sd["gpt.transformer.wte.weight"][torch.as_tensor(ids[:-1], dtype=torch.long)]
        logits = OC.gpt2_logits(torch.cat((pe, tail[None]), dim=1), sd)[0][0][pe.shape[1] - 1:]
    assert logits.shape[0] == len(ids)
    return torch.log_softmax(logits.double(), -1), float(logits.abs().max())


def _ref_logprobs(sd, emb, hard, ids):
    ls, mx = _oracle(sd, emb, hard, ids)
    return ls.gather(1, torch.as_tensor(ids, dtype=torch.long)[:, None])[:, 0], mx


@pytest.fixture(scope="module")
def c1():
    g = _load("c1_greedy")
    sd = _sd(g)
    from zsaac.score import CaptionScorer
    pipe = _pipe(sd, torch.float32, 4)
    return g, sd, pipe, CaptionScorer(pipe)


def test_f32_logprobs_match_oracle(cuda, c1):
    """c1_greedy clips 0, 1, 3, 4 (hard prompts of 12-15 ids, assembled on the device), their
    greedy captions cut to 67 / 30 / 7 / 1 tokens: a ragged batch."""
    g, sd, pipe, scorer = c1
    clips, cuts = [0, 1, 3, 4], [67, 30, 7, 1]
    caps = [g["greedy_ids"][b, :min(int(g["greedy_len"][b]), T)].tolist() for b, T in zip(clips, cuts)]
    assert len({len(c) for c in caps}) == 4 and len(caps[3]) == 1
    emb = torch.from_numpy(g["clap_emb"][clips])
    res = scorer.score_emb(emb.to(cuda), caps).cpu()
    assert res.n_tokens.tolist() == [len(c) for c in caps]
    for i, b in enumerate(clips):
        H, T = int(g["hard_len"][b]), len(caps[i])
        assert 12 <= H <= 15
        want, mx = _ref_logprobs(sd, emb[i:i + 1], g["hard_ids"][b, :H], caps[i])
        bound = 2 * LOGIT_REL * mx
        err = float((res.token_logprob[i, :T].double() - want).abs().max())
        print(f"clip {b}: T {T} max|logit| {mx:.2f} max |logprob err| {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert bool((res.token_logprob[i, T:] == 0).all())
        assert res.target_ids[i, :T].tolist() == caps[i] and bool((res.target_ids[i, T:] == -1).all())
        assert res.argmax_ids[i, :T].tolist() == caps[i]          # its own greedy ids
        assert abs(float(res.sum_logprob[i]) - float(want.sum())) <= T * bound
    assert res.accuracy() == 1.0
    total = sum(len(c) for c in caps)
    assert res.perplexity() == pytest.approx(math.exp(-float(res.sum_logprob.double().sum()) / total))


def test_empty_caption_and_bad_device_id(cuda, c1):
    from zsaac._lib import ZsError
    g, sd, pipe, scorer = c1
    emb = torch.from_numpy(g["clap_emb"][:2]).to(cuda)
    caps = [[], g["greedy_ids"][1, :5].tolist()]
    res = scorer.score_emb(emb, caps)
    m = res.mean_nll().cpu()
    assert res.n_tokens.tolist() == [0, 5] and float(res.sum_logprob[0]) == 0.0
    assert math.isnan(float(m[0])) and float(m[1]) > 0
    # the same captions as a device (ids, len) pair give the same scores
    ids = torch.zeros(2, 5, dtype=torch.int64)
    ids[1] = torch.tensor(caps[1])
    ln = torch.tensor([0, 5])
    dev = scorer.score_emb(emb, (ids.to(cuda), ln.to(cuda)))
    assert torch.equal(dev.check().token_logprob, res.token_logprob)
    host = scorer.score_emb(emb, (ids, ln))
    assert torch.equal(host.check().token_logprob, res.token_logprob)
    # an id outside the vocabulary: a host list is refused at once, a device tensor when read
    ids[1, 2] = 50257
    with pytest.raises(ZsError):
        scorer.score_emb(emb, (ids, ln))
    bad = scorer.score_emb(emb, (ids.to(cuda), ln.to(cuda)))
    with pytest.raises(ZsError):
        bad.mean_nll()
    with pytest.raises(ZsError):
        scorer.score_emb(emb, [[1] * 68, [2]])


def test_f32_argmax_reproduces_margin_flat_goldens(cuda):
    """c2_margin_flat, all 32 clips teacher-forced on their greedy ids: argmax_ids equals the
    golden id at every position, none skipped (the golden's smallest margin, 0.0117, against a
    logit bound of 2 x 1e-4 x 33.5 = 6.7e-3)."""
    from zsaac.score import CaptionScorer
    g = _load("c2_margin_flat")
    n = g["clap_emb"].shape[0]
    ln = g["greedy_len"]
    assert n == 32 and float(min(g["margin"][b, :ln[b]].min() for b in range(n))) > 0.0116
    pipe = _pipe(_sd(g), torch.float32, n)
    caps = [g["greedy_ids"][b, :ln[b]].tolist() for b in range(n)]
    res = CaptionScorer(pipe).score_emb(torch.from_numpy(g["clap_emb"]).to(cuda), caps).cpu()
    for b in range(n):
        assert res.argmax_ids[b, :ln[b]].tolist() == caps[b], b
    assert res.accuracy() == 1.0 and int(res.n_tokens.sum()) == int(ln.sum())


def test_beam_scores_equal_scored_beams(cuda, c1):
    """Two independent paths: generate_beam(3)'s running scores (KV-cache decode, f32) against the
    scorer's sum_logprob over each returned beam's seq_len tokens (one full prefill)."""
    from zsaac.score import CaptionScorer, beam_captions
    _, sd, _, _ = c1
    g = _load("beam")
    C, beam = g["clap_emb"].shape[0], 3
    pipe = _pipe(sd, torch.float32, C, beam=beam)
    emb = torch.from_numpy(g["clap_emb"]).to(cuda)
    out = pipe.caption_emb(emb)
    caps, _ = beam_captions(out)
    scores = out.scores.cpu().double()
    hard, hl = out.hard_ids.cpu(), out.hard_len.cpu()
    scorer = CaptionScorer(pipe)
    for i in range(beam):
        mine = [caps[c * beam + i] for c in range(C)]
        res = scorer.score_prompted(emb, out.hard_ids, out.hard_len, mine).cpu()
        for c in range(C):
            _, mx = _oracle(sd, torch.from_numpy(g["clap_emb"][c:c + 1]), hard[c, :int(hl[c])],
                            mine[c])
            bound = len(mine[c]) * 2 * LOGIT_REL * mx
            d = abs(float(res.sum_logprob[c]) - float(scores[c, i]))
            print(f"clip {c} beam {i}: {len(mine[c])} tokens, |sum - beam score| {d:.3e} (bound {bound:.3e})")
            assert int(res.n_tokens[c]) == len(mine[c]) and d <= bound


def test_bf16_first_position_within_golden_error(cuda):
    """c2_gpt2init in bf16: the first scored position of every caption against the oracle, within
    2 x the golden's bf16_ref_err; the later positions' mean |bf16 - f32| is printed (DESIGN)."""
    from zsaac.score import CaptionScorer
    g = _load("c2_gpt2init")
    sd = _sd(g)
    n, ln = g["clap_emb"].shape[0], g["greedy_len"]
    caps = [g["greedy_ids"][b, :ln[b]].tolist() for b in range(n)]
    emb = torch.from_numpy(g["clap_emb"])
    r16 = CaptionScorer(_pipe(sd, torch.bfloat16, n)).score_emb(emb.to(cuda), caps).cpu()
    r32 = CaptionScorer(_pipe(sd, torch.float32, n)).score_emb(emb.to(cuda), caps).cpu()
    tol = 2.0 * float(g["bf16_ref_err"])
    errs = []
    for b in range(n):
        H = int(g["hard_len"][b])
        want, _ = _ref_logprobs(sd, emb[b:b + 1], g["hard_ids"][b, :H], caps[b][:1])
        errs.append(abs(float(r16.token_logprob[b, 0]) - float(want[0])))
    later = torch.cat([(r16.token_logprob[b, 1:ln[b]] - r32.token_logprob[b, 1:ln[b]]).abs()
                       for b in range(n)])
    print(f"bf16 logprob: first position max |err vs oracle| {max(errs):.4f} (2 x bf16_ref_err = "
          f"{tol:.4f}); later positions mean |bf16 - f32| {float(later.mean()):.4f} max "
          f"{float(later.max()):.4f} over {later.numel()} tokens; perplexity bf16 "
          f"{r16.perplexity():.4f} f32 {r32.perplexity():.4f}")
    assert max(errs) <= tol


def test_score_wav_equals_score_emb_of_encode(cuda, c1):
    from zsaac import synthetic as S
    from zsaac.score import CaptionScorer
    g, sd, _, _ = c1
    asd = S.htsat_state_dict(3)
    asd.update(S.audio_proj_state_dict(5))
    pipe = _pipe(sd, torch.bfloat16, 2, audio_sd=asd)
    scorer = CaptionScorer(pipe, max_caption_tokens=8)
    wav = S.synthetic_waveforms(2).to(cuda)
    caps = [g["greedy_ids"][0, :8].tolist(), g["greedy_ids"][1, :3].tolist()]
    a = scorer.score_wav(wav, caps).cpu()
    b = scorer.score_emb(pipe.encode(wav).clone(), caps).cpu()
    assert torch.equal(a.token_logprob, b.token_logprob) and torch.equal(a.argmax_ids, b.argmax_ids)
    assert a.n_tokens.tolist() == [8, 3] and bool((a.token_logprob[0] < 0).all())


def test_scorer_refuses_too_many_positions(cuda, c1):
    from zsaac._lib import ZsError
    from zsaac.score import CaptionScorer
    pipe = c1[2]
    with pytest.raises(ZsError):
        CaptionScorer(pipe, max_caption_tokens=257 - pipe.h_cap - 10 + 1)


def test_predict_score_writes_nll(cuda, golden, tmp_path):
    """python -m zsaac.predict --score on test_gpu_harness.py's synthetic test_dir: nll.txt's
    per-clip mean NLL and the corpus perplexity against the oracle."""
    from oracle import caption as OC
    from test_gpu_harness import N_CLIPS, _make_test_dir
    from zsaac import bpe, predict
    from zsaac.tokenizer import compose_prompt_text
    root = str(tmp_path)
    sd, names, table, clips = _make_test_dir(root, golden)
    argv = ["--test_dir", root, "--test_data", os.path.join(root, "test.pkl"), "--dtype", "f32",
            "--batch", "4", "--score"]
    assert predict.main(argv) == 0
    assert not os.path.exists(os.path.join(root, "output.txt"))
    lines = open(os.path.join(root, "nll.txt")).read().splitlines()
    assert len(lines) == N_CLIPS + 1 and lines[-1].startswith("perplexity: ")
    tok = bpe.GPT2BPE.from_dir(os.path.join(root, "tokenizer"))
    nll, ntok = 0.0, 0
    for c, line in zip(clips, lines):
        key, mean, n, refs = line.split("\t")
        ids = tok.encode(c["caption"][0]["caption"] + ".")
        assert key == c["audio_id"] and int(n) == len(ids) and int(refs) == 1
        nll += float(mean) * int(n)
        ntok += int(n)
    assert float(lines[-1].split()[1]) == pytest.approx(math.exp(nll / ntok), rel=1e-4)
    for c, line in zip(clips[:3], lines[:3]):
        emb = c["audio_embedding"].float()
        idx = OC.sound_effect_choice(emb, table, 3)[0].tolist()
        hard = tok.encode(compose_prompt_text([names[i].lower() for i in idx]))
        ids = tok.encode(c["caption"][0]["caption"] + ".")
        want, mx = _ref_logprobs(sd, emb, hard, ids)
        assert abs(float(line.split("\t")[1]) + float(want.mean())) <= 2 * LOGIT_REL * mx + 1e-6
