"""GPU: sampled decoding end to end (Gpt2Decoder.sample, CaptionPipeline.sample_emb, generate2's
do_sample, MistralForCausalLM.generate(do_sample=True), predict --sample) on the synthetic
models the other GPU tests use, f32 parity mode.

Where a sampled token is compared with the float64 sampler (tests/sample_ref.py) it is compared on
decisive draws only (sample_ref's definition), applied to the decoder's OWN logits of that step."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
LOGIT_REL = 1e-4        # test_gpu_score.py's rule: |logit error| <= 1e-4 x max |logit|
STOPS = (13, 764)       # generate2 stops on '.' and ' .'
SETTING = dict(temperature=0.9, top_k=50, top_p=0.9)
SEED = 20240607


@pytest.fixture(scope="module")
def c1(cuda):
    from test_gpu_score import _load, _pipe, _sd
    g = _load("c1_greedy")
    sd = _sd(g)
    pipe = _pipe(sd, torch.float32, 6)
    emb = torch.from_numpy(g["clap_emb"][:5]).to(cuda)
    greedy = pipe.caption_emb(emb)
    ids, ln = greedy.ids.cpu().numpy().copy(), greedy.lengths.cpu().numpy().copy()
    for b in range(5):      # the pipeline's greedy is the golden's
        assert ids[b, :ln[b]].tolist() == g["greedy_ids"][b, :g["greedy_len"][b]].tolist()
    return g, sd, pipe, emb, ids, ln


@pytest.fixture(scope="module")
def sampled(c1):
    """Five clips x 3 samples with every step's logits kept: shared by the tests below."""
    g, sd, pipe, emb, _, _ = c1
    out = pipe.sample_emb(emb, 3, seed=SEED, keep_logits=True, **SETTING)
    return out, out.ids.cpu().numpy(), out.lengths.cpu().numpy(), out.logprobs.cpu().numpy()


@pytest.mark.parametrize("kw", [dict(top_k=1), dict(top_p=1e-6), dict(top_k=1, temperature=0.7)])
def test_top1_and_tiny_top_p_equal_greedy(c1, kw):
    g, sd, pipe, emb, gids, gln = c1
    assert gln.min() < 8 < gln.max()            # rows that stop early and rows that do not
    for seed in (0, 1, 2 ** 40 + 5):
        out = pipe.sample_emb(emb, 3, seed=seed, **kw)
        ids, ln = out.ids.cpu().numpy(), out.lengths.cpu().numpy()
        for j in range(3):
            assert np.array_equal(ln[:, j], gln) and np.array_equal(ids[:, j], gids), (kw, seed, j)


def _check_steps(out, ids, ln, rows, row_ids, steps, name):
    """Every token of ``rows`` at ``steps`` against the float64 sampler on the kept logits.
    Returns (draws compared, draws checked)."""
    n_dec = n_all = 0
    R = ids.shape[0] * ids.shape[1]
    fid, fln = ids.reshape(R, -1), ln.reshape(R)
    for t in steps:
        live = [r for r in rows if fln[r] > t]
        if not live:
            break
        lg = out.logits[t][live].cpu().numpy()
        recs = S.sample_rows(lg, lg.shape[1], SETTING["temperature"], SETTING["top_k"],
                             SETTING["top_p"], SEED, t, row_id=[row_ids[r] for r in live])
        for r, rec in zip(live, recs):
            n_all += 1
            if rec["decisive"]:
                n_dec += 1
                assert fid[r, t] == rec["tok"], (name, r, t, fid[r, t], rec["tok"])
    print(f"{name}: {n_all - n_dec} of {n_all} draws indecisive")
    assert n_dec * 8 >= n_all * 7
    return n_dec, n_all


def test_tokens_equal_reference_on_own_logits(sampled):
    """All 15 rows at steps 0 .. 3, and EVERY step (up to 67: later step words, longer K/V
    context, past the host's all-done checks every 8 steps) of rows 0, 7 and 14, one sample each
    of clips 0, 2 and 4.  (The float64 sampler costs 16 ms a draw at V = 50257: every step of
    every row would be a thousand draws.)  Measured on an MI355X: 60 + 148 draws, none indecisive,
    all equal."""
    out, ids, ln, lp = sampled
    assert out.logits.shape[1:] == (15, 50257)
    _check_steps(out, ids, ln, range(15), list(range(15)), range(4), "sample[5 clips x 3, steps 0-3]")
    full = (0, 7, 14)
    assert max(ln.reshape(-1)[r] for r in full) > 16          # beyond two all-done checks
    n_dec, n_all = _check_steps(out, ids, ln, full, list(range(15)), range(4, ids.shape[2]),
                                "sample[rows 0, 7, 14, steps 4-66]")
    assert n_all == sum(max(int(ln.reshape(-1)[r]) - 4, 0) for r in full)
    assert len({tuple(ids[b, j, :ln[b, j]]) for b in range(5) for j in range(3)}) > 5   # it samples


def test_stop_handling(sampled):
    out, ids, ln, lp = sampled
    steps = ids.shape[2]
    assert ln.min() >= 1 and ln.max() <= steps and (ln < steps).any()
    for b in range(5):
        for j in range(3):
            n = ln[b, j]
            assert not np.isin(ids[b, j, :n - 1], STOPS).any()
            assert n == steps or ids[b, j, n - 1] in STOPS
            assert not ids[b, j, n:].any() and not lp[b, j, n:].any()
            assert (lp[b, j, :n] < 0).all() and np.isfinite(lp[b, j, :n]).all()


def test_clip_alone_equals_third_of_five(c1, sampled):
    g, sd, pipe, emb, _, _ = c1
    out, ids, ln, lp = sampled
    alone = pipe.sample_emb(emb[2:3].clone(), 3, seed=SEED, keep_logits=True, clip_offset=2, **SETTING)
    aid, aln = alone.ids.cpu().numpy(), alone.lengths.cpu().numpy()
    for j in range(3):
        same = np.nonzero(aid[0, j] != ids[2, j])[0]
        if len(same) == 0:
            assert aln[0, j] == ln[2, j]
            continue
        t = int(same[0])        # the first step that differs must be an indecisive draw
        lg = alone.logits[t][j:j + 1].cpu().numpy()
        rec = S.sample_rows(lg, lg.shape[1], SETTING["temperature"], SETTING["top_k"],
                            SETTING["top_p"], SEED, t, row_id=[6 + j])[0]
        print(f"sample {j}: differs at step {t}, decisive {rec['decisive']}")
        assert not rec["decisive"]
    # another clip offset is another draw
    other = pipe.sample_emb(emb[2:3].clone(), 3, seed=SEED, clip_offset=0, **SETTING)
    assert not np.array_equal(other.ids.cpu().numpy(), aid)


def test_sum_logprob_equals_scorer(c1, sampled):
    from zsaac.score import CaptionScorer
    g, sd, pipe, emb, _, _ = c1
    out, ids, ln, lp = sampled
    scorer = CaptionScorer(pipe)
    mx = float(out.logits.abs().max())
    bound = 2 * LOGIT_REL * mx
    sums = out.sum_logprob().cpu().numpy()
    worst = 0.0
    for b in (0, 3):
        caps = [ids[b, j, :ln[b, j]].tolist() for j in range(3)]
        res = scorer.score_emb(emb[b:b + 1].expand(3, -1).contiguous(), caps).cpu()
        for j in range(3):
            T = len(caps[j])
            err = float(np.abs(res.token_logprob[j, :T].numpy() - lp[b, j, :T]).max())
            worst = max(worst, err)
            assert err <= bound
            assert abs(float(res.sum_logprob[j]) - float(sums[b, j])) <= T * bound
    print(f"max |logprob - scorer| {worst:.3e} (bound {bound:.3e}, max |logit| {mx:.2f})")
    assert np.allclose(out.mean_logprob().cpu().numpy(), sums / ln)


# ------------------------------------------------------------------ generate2
@pytest.fixture(scope="module")
def dropin(cuda, golden):
    from test_gpu_dropin import GPT2_KW
    from models.caption_model import ClapCaption_prompt
    from zsaac import synthetic as Sy
    m = ClapCaption_prompt(10, clip_length=10, prefix_size=1024, num_layers=8, mapping_type="mlp")
    sd = Sy.gpt2_state_dict(**GPT2_KW)
    sd.update(Sy.mlp_mapper_state_dict(1))
    m.load_state_dict(sd)
    m = m.to(cuda).eval()
    g = golden("c1_greedy.npz")
    pes = {}
    for clip in (0, 3):
        n = int(g["hard_len"][clip])
        prefix = torch.nn.functional.normalize(torch.from_numpy(g["clap_emb"][clip:clip + 1]), dim=-1)
        hard = torch.from_numpy(g["hard_ids"][clip:clip + 1, :n]).to(cuda)
        with torch.no_grad():
            pes[clip], _ = m.clap_to_gpt(prefix[None].to(cuda), m.gpt.transformer.wte(hard))
    return m, g, pes


def test_generate2_default_path_unchanged(dropin):
    import gpt2_prefix_eval as G
    from zsaac.tokenizer import IdTokenizer
    m, g, pes = dropin
    for clip, pe in pes.items():
        want = g["greedy_ids"][clip, :g["greedy_len"][clip]].tolist()
        for kw in (dict(do_sample=False), dict(do_sample=False, seed=9, entry_count=3, top_p=0.3)):
            out = G.generate2(m, IdTokenizer(), embed=pe, **kw)
            assert [int(t) for t in out.split()] == want
        # the filters at their argmax settings reach the same text through the sampler
        out = G.generate2(m, IdTokenizer(), embed=pe, do_sample=True, top_p=1e-6, seed=4)
        assert [int(t) for t in out.split()] == want


def test_generate2_samples_reproducible(dropin):
    import gpt2_prefix_eval as G
    from zsaac.tokenizer import IdTokenizer
    m, g, pes = dropin
    pe = pes[0]
    kw = dict(embed=pe, entry_count=4, top_p=0.9, temperature=1.1, entry_length=12)
    a = G.generate2_samples(m, IdTokenizer(), seed=3, **kw)
    assert len(a) == 4 and len(set(a)) > 1 and all(len(t.split()) <= 12 for t in a)
    assert a == G.generate2_samples(m, IdTokenizer(), seed=3, **kw)
    assert a != G.generate2_samples(m, IdTokenizer(), seed=4, **kw)
    assert G.generate2(m, IdTokenizer(), do_sample=True, seed=3, **kw) == a[0]


# ------------------------------------------------------------------ Mistral
def test_mistral_generate_do_sample(cuda, golden):
    from models.caption_model import ClapCaption_Mistralai_prompt
    from zsaac import synthetic as Sy
    g = golden("mistral.npz")
    cfg = dict(vocab_size=32000, hidden_size=1024, intermediate_size=3072, num_hidden_layers=2,
               num_attention_heads=8, num_key_value_heads=2, rms_norm_eps=1e-5)
    m = ClapCaption_Mistralai_prompt(10, clip_length=10, prefix_size=1024, num_layers=8,
                                     mapping_type="mlp", mistral_config=cfg)
    sd = {"LMmodel.base_model.model." + k: v for k, v in Sy.mistral_state_dict().items()}
    sd.update(Sy.mlp_mapper_state_dict(31, prefix_length=10, d=1024))
    m.load_state_dict(sd)
    m = m.set_mode("f32").to(cuda).eval()
    prefix = torch.from_numpy(g["clap_emb"])[:, None].to(cuda)
    hard = torch.from_numpy(g["hard_ids"]).to(cuda)
    with torch.no_grad():
        eh = m.LMmodel.base_model.model.model.embed_tokens(hard)
        tk = torch.from_numpy(g["tag_en"])[None].repeat(prefix.shape[0], 1).to(cuda)
        pe, _ = m.clap_to_gpt(prefix, eh, m.LMmodel.base_model.model.model.embed_tokens(tk))
    kw = dict(inputs_embeds=pe, attention_mask=torch.ones(pe.shape[:-1]).long().to(cuda),
              max_length=60, eos_token_id=2, pad_token_id=2)
    want = torch.from_numpy(g["ids_en"])
    assert torch.equal(m.LMmodel.generate(do_sample=True, top_k=1, **kw).cpu(), want)
    assert torch.equal(m.LMmodel.generate(do_sample=True, top_k=0, top_p=1e-6, seed=5, **kw).cpu(), want)
    B, new = pe.shape[0], 60 - pe.shape[1]
    torch.manual_seed(77)
    a = m.LMmodel.generate(do_sample=True, top_k=20, top_p=0.95, temperature=1.3,
                           num_return_sequences=2, **kw).cpu()
    assert a.shape[0] == 2 * B and 1 <= a.shape[1] <= new and a.dtype == torch.long
    assert int(a.min()) >= 0 and int(a.max()) < 32000
    torch.manual_seed(77)
    b = m.LMmodel.generate(do_sample=True, top_k=20, top_p=0.95, temperature=1.3,
                           num_return_sequences=2, **kw).cpu()
    assert torch.equal(a, b)
    c = m.LMmodel.generate(do_sample=True, top_k=20, top_p=0.95, temperature=1.3,
                           num_return_sequences=2, **kw).cpu()         # the generator moved on
    assert c.shape != a.shape or not torch.equal(a, c)
    assert not torch.equal(a[0::2], a[1::2])                           # the two samples differ
    with pytest.raises(NotImplementedError):
        m.LMmodel.generate(do_sample=True, num_beams=2, **kw)


# ------------------------------------------------------------------ predict --sample
def test_predict_sample_writes_samples(cuda, golden, tmp_path, capsys):
    from test_gpu_harness import N_CLIPS, _make_test_dir
    from zsaac import predict
    root = str(tmp_path)
    _make_test_dir(root, golden)
    base = ["--test_dir", root, "--test_data", os.path.join(root, "test.pkl"), "--dtype", "f32",
            "--batch", "4"]
    for bad in (["--isbeam"], ["--score"], ["--magic", "--clap", "x", "--bert_vocab", "y"]):
        with pytest.raises(SystemExit) as e:
            predict.main(base + ["--sample", "3"] + bad)
        assert e.value.code == 2
        assert "--sample cannot be combined with --isbeam, --magic or --score" in capsys.readouterr().err
    assert not os.path.exists(os.path.join(root, "samples.json"))
    argv = base + ["--sample", "3", "--seed", "1", "--top_p", "0.9", "--temperature", "1.1"]
    assert predict.main(argv) == 0
    smp = json.load(open(os.path.join(root, "samples.json")))["samples"]
    pred = json.load(open(os.path.join(root, "output.txt")))["predictions"]
    assert len(smp) == len(pred) == N_CLIPS
    for s, p in zip(smp, pred):
        caps = s["captions"]
        assert s["filename"] == p["filename"] and len(caps) == 3
        for c in caps:
            assert c["tokens"] >= 1 and c["sum_logprob"] < 0
            assert c["mean_logprob"] == pytest.approx(c["sum_logprob"] / c["tokens"], rel=1e-5)
        best = max(caps, key=lambda c: c["mean_logprob"])
        assert p["caption"] == best["caption"] and p["prefix"]
    assert len({c["caption"] for s in smp for c in s["captions"]}) > N_CLIPS
    first = open(os.path.join(root, "samples.json")).read()
    assert predict.main(argv) == 0
    assert open(os.path.join(root, "samples.json")).read() == first       # reproducible
