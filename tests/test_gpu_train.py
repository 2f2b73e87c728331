"""Training the MLP mapper on the device (zsaac.train.MapperTrainer) against the float64 oracle:
autograd through OC.mlp_mapper + OC.gpt2_logits (tests/train_ref.py::oracle_loss, the recipe of
tests/test_gpu_score.py::_oracle without no_grad) and torch.optim.AdamW.  Synthetic weights
(S.gpt2_state_dict() + S.mlp_mapper_state_dict(1)).

Bounds.  f32 gradients, per tensor and for d_soft: max|g - g64| <= 1e-4 x max|g64|, the project's
full-logit bound LOGIT_REL carried over to gradients; the loss: the scorer's 2 x 1e-4 x
max|logit|.  bf16 gradients: relative L2 error against float64 on the bf16-rounded weights <=
2 x that of the oracle run entirely in torch.bfloat16 on the CPU (the two round in different
places).  Training, f32: |loss_k - ref_k| <= 1 % of (ref_0 - ref_k); bf16: a strict decrease and
a total decrease of at least half the reference's.  The measured figures are printed (and kept
in profiles/train_grad_errors.txt)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
LOGIT_REL = 1e-4
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
T25 = [464, 2128, 286, 257, 3290, 21405, 981, 257, 1097, 8318, 416, 290, 2130, 6130, 287, 262,
       4469, 351, 617, 2344, 19280, 1474, 262, 2975, 13]
CAPS = [T25, [32, 5385, 318, 2712, 13], [13]]


@pytest.fixture(scope="module")
def sd():
    from zsaac import synthetic as S
    d = S.gpt2_state_dict()
    d.update(S.mlp_mapper_state_dict(1))
    return d


@pytest.fixture(scope="module")
def emb():
    from zsaac import synthetic as S
    return S.synthetic_clap_embeddings(3)


def _pipe(sd, dtype, batch):
    from zsaac import synthetic as S
    from zsaac.pipeline import CaptionConfig, CaptionPipeline
    cfg = CaptionConfig(dtype=dtype, batch=batch)
    return CaptionPipeline(sd, None, S.label_table(), S.label_token_table(), cfg)


@pytest.fixture(scope="module")
def pipes(sd):
    """The pipelines of the gradient tests: never trained."""
    return {F32: _pipe(sd, F32, 3), BF16: _pipe(sd, BF16, 3)}


@pytest.fixture(scope="module")
def train_pipes(sd):
    """The pipelines the training tests train in place (a new MapperTrainer re-seats the mapper's
    operands from the state dict, so each of those tests starts from the same weights)."""
    return {F32: _pipe(sd, F32, 3), BF16: _pipe(sd, BF16, 3)}


def _hards(tr, B):
    ids, ln = tr.hard_ids[:B].cpu(), tr.hard_len[:B].cpu()
    return [ids[b, :int(ln[b])].tolist() for b in range(B)]


def _prefix(emb, dtype):
    return torch.nn.functional.normalize(emb.double(), dim=-1).to(dtype)


@pytest.fixture(scope="module")
def grads_case(cuda, sd, emb, pipes):
    """The f32 trainer's gradients of the 3-clip batch (captions of 25 / 5 / 1 tokens, hard
    prompts assembled on the device) and the float64 / float32 oracle's, computed once."""
    from zsaac.train import MapperTrainer
    tr = MapperTrainer(pipes[F32], sd)
    got = tr.loss_and_grads(emb.to(cuda), CAPS)
    hards = _hards(tr, 3)
    assert got.n_tokens.tolist() == [25, 5, 1] and all(len(h) >= 7 for h in hards)
    ref = R.oracle_grads(R.cast_sd(sd, F64), _prefix(emb, F64), hards, CAPS)
    return tr, got, hards, ref


def test_f32_gradients_match_the_float64_oracle(cuda, sd, emb, grads_case):
    tr, got, hards, (loss64, ds64, g64, mx) = grads_case
    loss32, ds32, g32, _ = R.oracle_grads(R.cast_sd(sd, F32), _prefix(emb, F32), hards, CAPS)
    err = abs(float(got.loss) - float(loss64))
    print(f"loss {float(got.loss):.6f} ref {float(loss64):.6f} err {err:.3e} "
          f"(bound {2 * LOGIT_REL * mx:.3e}, max|logit| {mx:.2f})")
    fails = []
    if err > 2 * LOGIT_REL * mx:
        fails.append("loss")
    items = [("d_soft", got.d_soft.cpu(), ds64, ds32)] + [(k, got.grads[k].cpu(), g64[k], g32[k])
                                                          for k in R.KEYS]
    for name, g, r64, r32 in items:
        top = float(r64.abs().max())
        e = float((g.double() - r64).abs().max())
        y = float((r32.double() - r64).abs().max())
        print(f"{name}: max|g64| {top:.3e} max err {e:.3e} rel {e / top:.3e} "
              f"(bound 1e-4) f32 yardstick rel {y / top:.3e} ratio {e / max(y, 1e-300):.2f}")
        assert g.shape == r64.shape and bool(torch.isfinite(g).all())
        if e > LOGIT_REL * top:
            fails.append(name)
    assert not fails, fails


def test_f32_gradients_are_bit_identical_from_run_to_run(cuda, emb, grads_case):
    tr, got, _, _ = grads_case
    again = tr.loss_and_grads(emb.to(cuda), CAPS)
    assert torch.equal(again.loss, got.loss) and torch.equal(again.d_soft, got.d_soft)
    for k in R.KEYS:
        assert torch.equal(again.grads[k], got.grads[k])
    # given hard prompts are the device-assembled ones
    given = tr.loss_and_grads(emb.to(cuda), CAPS, hard=(tr.hard_ids[:3].clone(), tr.hard_len[:3].clone()))
    assert torch.equal(given.loss, got.loss) and torch.equal(given.d_soft, got.d_soft)


def test_bf16_gradients(cuda, sd, emb, pipes, grads_case):
    from zsaac.train import MapperTrainer
    hards = grads_case[2]
    tr = MapperTrainer(pipes[BF16], sd)
    got = tr.loss_and_grads(emb.to(cuda), CAPS)
    assert _hards(tr, 3) == hards
    loss64, ds64, g64, _ = R.oracle_grads(R.cast_sd(sd, F64, BF16), _prefix(emb, F64), hards, CAPS)
    lossb, dsb, gb, _ = R.oracle_grads(R.cast_sd(sd, BF16), _prefix(emb, BF16), hards, CAPS)
    print(f"loss {float(got.loss):.4f} ref {float(loss64):.4f} cpu-bf16 {float(lossb):.4f}")
    fails = []
    items = [("d_soft", got.d_soft.cpu(), ds64, dsb)] + [(k, got.grads[k].cpu(), g64[k], gb[k])
                                                         for k in R.KEYS]
    for name, g, r64, rb in items:
        n = float(r64.norm())
        e = float((g.double() - r64).norm()) / n
        y = float((rb.double() - r64).norm()) / n
        cos = float((g.double().flatten() @ r64.flatten()) / (g.double().norm() * n))
        print(f"{name}: rel L2 err {e:.3e} cpu-bf16 yardstick {y:.3e} (bound {2 * y:.3e}) cos {cos:.6f}")
        assert bool(torch.isfinite(g).all())
        if e > 2 * y:
            fails.append(name)
    assert not fails, fails
    again = tr.loss_and_grads(emb.to(cuda), CAPS)
    assert torch.equal(again.d_soft, got.d_soft) and torch.equal(again.loss, got.loss)


@pytest.fixture(scope="module")
def train_ref_run(sd, emb, grads_case):
    """The float64 loop with torch.optim.AdamW: B = 2, captions of 25 and 5 tokens, lr 1e-4,
    weight decay 0.01, no noise, 4 steps -> (losses, trained tensors)."""
    hards = grads_case[2][:2]
    losses, params = R.oracle_train(R.cast_sd(sd, F64), _prefix(emb[:2], F64), hards, CAPS[:2],
                                    4, 1e-4, 0.01)
    print("float64 losses", [f"{v:.4f}" for v in losses])
    assert all(b < a for a, b in zip(losses, losses[1:]))         # its own strict decrease
    return hards, losses, params


def test_f32_training_follows_the_reference_and_round_trips(cuda, sd, emb, train_pipes,
                                                            train_ref_run, tmp_path):
    from zsaac import safeload
    from zsaac.score import CaptionScorer
    from zsaac.train import MapperTrainer
    hards, ref, params = train_ref_run
    pipe = train_pipes[F32]
    tr = MapperTrainer(pipe, sd, lr=1e-4, weight_decay=0.01)
    e2 = emb[:2].to(cuda)
    losses = [float(tr.step(e2, CAPS[:2])) for _ in range(4)]
    tr.check()
    assert _hards(tr, 2) == hards
    print("f32 losses", [f"{v:.6f}" for v in losses], "ref", [f"{v:.6f}" for v in ref])
    with torch.no_grad():
        mx0 = R.oracle_loss(R.cast_sd(sd, F64), _prefix(emb[:2], F64), hards, CAPS[:2])[2]
    assert abs(losses[0] - ref[0]) <= 2 * LOGIT_REL * mx0         # before any update: the scorer's bound
    for k in range(1, 4):
        assert abs(losses[k] - ref[k]) <= 0.01 * (ref[0] - ref[k]), k
    # the live pipeline's operands are the trained ones: CaptionScorer reports the current loss
    sd64 = R.cast_sd(sd, F64)
    sd64.update(params)
    with torch.no_grad():
        want, _, mx = R.oracle_loss(sd64, _prefix(emb[:2], F64), hards, CAPS[:2])
    now = tr.loss_and_grads(e2, CAPS[:2])
    sc = CaptionScorer(pipe, 25).score_emb(e2, CAPS[:2]).cpu()
    live = -float(sc.sum_logprob.double().sum()) / int(sc.n_tokens.sum())
    print(f"after 4 steps: trainer {float(now.loss):.6f} scorer {live:.6f} float64 {float(want):.6f}")
    assert abs(live - float(now.loss)) <= 2 * LOGIT_REL * mx
    assert abs(live - float(want)) <= 2 * LOGIT_REL * mx + 0.01 * (ref[0] - float(want))
    # round trip: a pipeline built from the saved checkpoint captions id for id like the live one
    path = tr.save(str(tmp_path / "best.pth"))
    sd2 = safeload.load_state_dict(path)
    assert set(sd2) == set(sd)
    for k in R.KEYS:
        assert torch.equal(sd2[k], tr.master[k].cpu()) and not torch.equal(sd2[k], sd[k])
    caps_live = pipe.caption_emb(emb.to(cuda)).captions()
    caps_new = _pipe(sd2, F32, 3).caption_emb(emb.to(cuda)).captions()
    assert caps_live == caps_new


def test_bf16_training_decreases_the_loss(cuda, sd, emb, train_pipes, train_ref_run):
    from zsaac.train import MapperTrainer
    _, ref, _ = train_ref_run
    tr = MapperTrainer(train_pipes[BF16], sd, lr=1e-4, weight_decay=0.01)
    e2 = emb[:2].to(cuda)
    losses = [float(tr.step(e2, CAPS[:2])) for _ in range(4)]
    print("bf16 losses", [f"{v:.4f}" for v in losses], "ref", [f"{v:.4f}" for v in ref])
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert losses[0] - losses[3] >= 0.5 * (ref[0] - ref[3])


def test_noise_in_the_loop(cuda, sd, emb, train_pipes):
    from zsaac.train import MapperTrainer
    e2 = emb[:2].to(cuda)

    def run(seed):
        tr = MapperTrainer(train_pipes[F32], sd, lr=1e-4, noise_variance=0.016, seed=seed)
        return torch.stack([tr.step(e2, CAPS[:2]) for _ in range(2)]).cpu()
    a, b, c = run(3), run(3), run(4)
    clean = MapperTrainer(train_pipes[F32], sd).loss_and_grads(e2, CAPS[:2]).loss.cpu()
    print("noise losses", a.tolist(), c.tolist(), "clean", float(clean))
    assert torch.equal(a, b)
    assert not torch.equal(a, c) and float(a[0]) != float(clean)
