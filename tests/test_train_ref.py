"""CPU: the float64 restatements of tests/train_ref.py against torch.autograd on the forward
formulas, torch.optim.AdamW and tests/sample_ref.py's Philox known answers; the host side of
zsaac.train (schedule, checkpoint key set, refusals, the command line's flags and records).

The tests of the restatements alone (attention, LayerNorm, activations, the LM-head gradient,
column sums, AdamW, the Philox normals, the oracle) check the reference, not the feature: they
need nothing from zsaac.train or the new ops and pass without them.  The tests that fail without
the feature are the zsaac.train host tests below (schedule, state dict, refusals, command line)
and the GPU tests (tests/test_gpu_train_kernels.py, tests/test_gpu_train.py)."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sample_ref  # noqa: E402
import train_ref as R  # noqa: E402

F64 = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("B,L,lens,heads", [(1, 1, [1], 1), (3, 33, [1, 33, 17], 2),
                                            (2, 130, [130, 64], 2)])
def test_attention_bwd_is_autograd_of_the_forward(B, L, lens, heads):
    g = _g(L)
    qkv = torch.randn(B * L, 3 * heads * 64, generator=g, dtype=F64).requires_grad_(True)
    do = torch.randn(B * L, heads * 64, generator=g, dtype=F64)
    out = R.attention_fwd(qkv, B, L, lens, heads)
    (want,) = torch.autograd.grad((out * do).sum(), qkv)
    got = R.attention_bwd(qkv.detach(), do, B, L, lens, heads)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # rows >= len: poison is ignored, zeros come out
    q2, d2 = qkv.detach().clone().reshape(B, L, -1), do.clone().reshape(B, L, -1)
    for b in range(B):
        q2[b, lens[b]:] = math.nan
        d2[b, lens[b]:] = math.nan
    got2 = R.attention_bwd(q2.reshape(B * L, -1), d2.reshape(B * L, -1), B, L, lens, heads)
    assert torch.equal(got2, got)
    for b in range(B):
        assert bool((got2.reshape(B, L, -1)[b, lens[b]:] == 0).all())
    # round_to rounds the stored output only
    r = R.attention_bwd(qkv.detach(), do, B, L, lens, heads, round_to=torch.bfloat16)
    assert torch.equal(r, got.to(torch.bfloat16).to(F64))


@pytest.mark.parametrize("gain", [False, True])
def test_layernorm_bwd_is_autograd(gain):
    g = _g(3)
    M, C = 5, 32
    x = torch.randn(M, C, generator=g, dtype=F64).requires_grad_(True)
    x.data[2] = 0.75                                       # a constant row
    dy = torch.randn(M, C, generator=g, dtype=F64)
    w = torch.randn(C, generator=g, dtype=F64) if gain else None
    res = torch.randn(M, C, generator=g, dtype=F64)
    y = torch.nn.functional.layer_norm(x, (C,), w, None, 1e-5)
    (want,) = torch.autograd.grad((y * dy).sum(), x)
    got = R.layernorm_bwd(x.detach(), dy, g=w, res=res)
    assert float((got - (want + res)).abs().max()) <= 1e-9
    rows = [4, 1]
    gr = R.layernorm_bwd(x.detach(), dy[:2], g=w, rows=rows)
    y2 = torch.nn.functional.layer_norm(x, (C,), w, None, 1e-5)[rows]
    (want2,) = torch.autograd.grad((y2 * dy[:2]).sum(), x)
    assert float((gr - want2).abs().max()) <= 1e-9
    assert bool((gr[[0, 2, 3]] == 0).all())


def test_activation_backwards_are_autograd():
    u = torch.tensor([-30.0, -3.0, -0.5, 0.0, 0.7, 2.5, 30.0], dtype=F64).requires_grad_(True)
    dh = torch.linspace(-1, 2, 7, dtype=F64)
    (want,) = torch.autograd.grad((R.gelu_new(u) * dh).sum(), u)
    assert float((R.gelu_tanh_bwd(u.detach(), dh) - want).abs().max()) <= 1e-14
    from oracle import caption as OC
    assert torch.equal(OC.gelu_new(u.detach()), R.gelu_new(u.detach()))
    (want,) = torch.autograd.grad((torch.tanh(u) * dh).sum(), u)
    assert float((R.tanh_bwd(torch.tanh(u.detach()), dh) - want).abs().max()) <= 1e-14
    assert torch.equal(R.gelu_tanh_bwd(u.detach(), dh, round_to=torch.bfloat16),
                       R.gelu_tanh_bwd(u.detach(), dh).to(torch.bfloat16).to(F64))


def test_nll_grad_rows_is_autograd_of_the_mean_cross_entropy():
    g = _g(5)
    V, K, M = 50, 8, 6
    wte = torch.randn(V, K, generator=g, dtype=F64)
    hf = torch.randn(M, K, generator=g, dtype=F64).requires_grad_(True)
    tgt = torch.tensor([3, -1, 49, 0, -1, 7])
    cnt = torch.tensor([3, 1])
    ls = torch.log_softmax(hf @ wte.t(), -1)
    on = tgt >= 0
    loss = -ls[on].gather(1, tgt[on][:, None]).sum() / int(cnt.sum())
    (want,) = torch.autograd.grad(loss, hf)
    got = R.nll_grad_rows(R.softmax_mix(hf.detach(), wte), wte, tgt, cnt)
    assert float((got - want).abs().max()) <= 1e-14
    assert bool((got[~on] == 0).all())


def test_colsum_and_transpose_cast():
    g = _g(7)
    x = torch.randn(3, 70, generator=g)
    assert torch.equal(R.colsum(x), x.double().sum(0))
    t = R.transpose_cast(x, round_to=torch.bfloat16)
    assert t.shape == (70, 32) and bool((t[:, 3:] == 0).all())
    assert torch.equal(t[:, :3], x.to(torch.bfloat16).double().t())
    assert R.transpose_cast(torch.zeros(33, 5)).shape == (5, 64)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_matches_torch_over_three_steps(wd):
    g = _g(11)
    p0 = torch.randn(257, generator=g, dtype=F64)
    tp = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=1e-3, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in (1, 2, 3):
        grad = torch.randn(257, generator=g, dtype=F64)
        tp.grad = grad.clone()
        opt.step()
        p, m, v = R.adamw(p, grad, m, v, step, 1e-3, weight_decay=wd)
        assert float((p - tp.detach()).abs().max()) <= 1e-15


def test_philox_normals():
    # the words behind normals() are sample_ref's Philox (known answers there)
    for ctr, key, want in sample_ref.PHILOX_KAT:
        assert tuple(int(w) for w in sample_ref.philox4x32_10(ctr, key)) == want
    # row 0, step 0, column block 0 under seed 0 is the first known answer's counter and key
    w = sample_ref.PHILOX_KAT[0][2]
    u1, u2 = ((w[0] >> 8) + 1) * 2.0 ** -24, (w[1] >> 8) * 2.0 ** -24
    u3, u4 = ((w[2] >> 8) + 1) * 2.0 ** -24, (w[3] >> 8) * 2.0 ** -24
    want = [math.sqrt(-2 * math.log(u1)) * math.cos(2 * math.pi * u2),
            math.sqrt(-2 * math.log(u1)) * math.sin(2 * math.pi * u2),
            math.sqrt(-2 * math.log(u3)) * math.cos(2 * math.pi * u4),
            math.sqrt(-2 * math.log(u3)) * math.sin(2 * math.pi * u4)]
    n = R.normals(0, [0], 0, 4)
    assert np.allclose(n[0], want, rtol=0, atol=1e-14)
    # a row's noise depends on its id and the step, not on its slot; D need not be a multiple of 4
    a = R.normals(9, [5], 2, 1024)
    b = R.normals(9, [3, 4, 5], 2, 1024)
    assert np.array_equal(a[0], b[2]) and not np.array_equal(b[0], b[1])
    assert not np.array_equal(R.normals(9, [5], 3, 1024), a)
    assert not np.array_equal(R.normals(8, [5], 2, 1024), a)
    assert np.array_equal(R.normals(9, [5], 2, 30)[0], a[0, :30])
    big = R.normals(1, np.arange(70), 0, 1024).ravel()
    nn = big.size
    assert abs(big.mean()) <= 5 / math.sqrt(nn) and abs(big.var() - 1) <= 5 * math.sqrt(2 / nn)


def test_noise_inject_semantics():
    x = torch.randn(3, 32, generator=_g(2), dtype=F64) * 3
    assert torch.equal(R.noise_inject(x, 0.0), x)
    y = R.noise_inject(x, 0.016, seed=4, step=1)
    assert float((y.norm(dim=-1) - 1).abs().max()) <= 1e-14
    n = torch.from_numpy(R.normals(4, np.arange(3), 1, 32))
    want = torch.nn.functional.normalize(torch.nn.functional.normalize(x, dim=-1)
                                         + math.sqrt(0.016) * n, dim=-1)
    assert float((y - want).abs().max()) <= 1e-15


def test_linear_schedule():
    from zsaac.train import linear_schedule
    assert linear_schedule(0, 10, 100) == 0.0
    assert linear_schedule(9, 10, 100) == 0.9                 # the last warm-up step
    assert linear_schedule(10, 10, 100) == 1.0
    assert linear_schedule(55, 10, 100) == 0.5
    assert linear_schedule(100, 10, 100) == 0.0 and linear_schedule(120, 10, 100) == 0.0
    assert linear_schedule(0, 0, 10) == 1.0
    for s in (0, 3, 9, 10, 11, 99, 100):
        assert linear_schedule(s, 10, 100) == R.linear_schedule(s, 10, 100)
    sched = torch.optim.lr_scheduler.LambdaLR(
        torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=1.0),
        lambda s: linear_schedule(s, 4, 20))
    assert sched.get_last_lr()[0] == 0.0


def test_state_dict_has_the_reference_key_set():
    from zsaac import synthetic as S
    from zsaac.train import KEYS, trained_state_dict
    from zsaac._lib import ZsError
    keys = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                       "state_dict_keys.json")))["ClapCaption_prompt[mlp]"]
    sd = S.gpt2_state_dict()
    sd.update(S.mlp_mapper_state_dict(1))
    new = {k: torch.full_like(sd[k], 0.5) for k in KEYS}
    out = trained_state_dict(sd, new)
    assert set(out) == set(keys)
    for k, shape in keys.items():
        assert list(out[k].shape) == shape
        assert torch.equal(out[k], new[k] if k in KEYS else sd[k])
    assert KEYS == R.KEYS
    with pytest.raises(ZsError):
        trained_state_dict(sd, {k: new[k] for k in KEYS[:3]})
    with pytest.raises(ZsError):
        trained_state_dict(sd, dict(new, **{KEYS[1]: torch.zeros(7)}))


def test_trainer_refuses_host_tensors_and_the_transformer_mapper():
    from zsaac._lib import ZsError
    from zsaac.train import MapperTrainer
    fake = types.SimpleNamespace(cfg=types.SimpleNamespace(mapping_type="transformer"),
                                 dev=torch.device("cpu"))
    with pytest.raises(NotImplementedError):
        MapperTrainer(fake, {})
    fake.cfg.mapping_type = "mlp"
    with pytest.raises(ZsError, match="GPU"):
        MapperTrainer(fake, {})
    with pytest.raises(ZsError, match="device tensors"):
        MapperTrainer._check_emb(torch.zeros(2, 1024), 4)


def test_oracle_is_differentiable_and_training_decreases_the_loss():
    """The float64 oracle behind tests/test_gpu_train.py on a cut-down problem (one short clip):
    autograd reaches the four mapper tensors and the soft prefix, and two AdamW steps lower the
    loss."""
    from zsaac import synthetic as S
    sd = S.gpt2_state_dict()
    sd.update(S.mlp_mapper_state_dict(1))
    sd = R.cast_sd(sd, F64)
    prefix = torch.nn.functional.normalize(S.synthetic_clap_embeddings(1).double(), dim=-1)
    hards, caps = [[1858, 389, 13]], [[11, 22, 13]]
    loss, d_soft, grads, mx = R.oracle_grads(sd, prefix, hards, caps)
    assert mx > 0
    assert d_soft.shape == (1, 7680) and float(d_soft.abs().max()) > 0
    for k in R.KEYS:
        assert grads[k].shape == sd[k].shape and float(grads[k].abs().max()) > 0
    # d loss / d b2 is d_soft summed over the batch; d loss / d W2 = d_soft^T h
    assert float((grads[R.KEYS[3]] - d_soft.sum(0)).abs().max()) <= 1e-15
    h = torch.tanh(prefix @ sd[R.KEYS[0]].t() + sd[R.KEYS[1]])
    assert float((grads[R.KEYS[2]] - d_soft.t() @ h).abs().max()) <= 1e-14
    losses, _ = R.oracle_train(sd, prefix, hards, caps, 2, 1e-4, 0.01)
    assert abs(losses[0] - float(loss)) <= 1e-12 and losses[1] < losses[0]


def test_command_line_flags_and_records(tmp_path):
    """--ckpt_file and --data are required; a flag left out never overrides the checkpoint's
    params.json; records come out one per (embedding, caption), from several pickles per file."""
    import pickle
    from zsaac.train import _apply_flags, _parser, _records
    ap = _parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--data", "a.pkl"])                       # no --ckpt_file
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt_file", "best.pth"])               # no --data
    a = ap.parse_args(["--data", "a.pkl", "b.pkl", "--ckpt_file", "x/best.pth"])
    assert (a.bs, a.lr, a.weight_decay, a.noise_variance, a.seed) == (40, 1e-5, 0.0, 0.0, 0)
    assert a.data == ["a.pkl", "b.pkl"] and not a.use_audio_embedding and a.valdata == []
    params = {"normalize_prefix": True, "sound_effect_num": 5, "mapping_type": "mlp"}
    assert _apply_flags(params, a) == params
    b = ap.parse_args(["--data", "a.pkl", "--ckpt_file", "x", "--sound_effect_num", "0",
                       "--normalize_prefix", "--noise_variance", "0.016"])
    got = _apply_flags({"normalize_prefix": False, "sound_effect_num": 5}, b)
    assert got == {"normalize_prefix": True, "sound_effect_num": 0} and b.noise_variance == 0.016
    path = tmp_path / "train.pkl"
    recs = [{"text_embedding": np.arange(4, dtype=np.float32), "audio_embedding": np.ones(4, dtype=np.float32),
             "caption": ["a dog barks", "barking"]},
            {"text_embedding": np.zeros(4, dtype=np.float32), "audio_embedding": np.ones(4, dtype=np.float32),
             "caption": "rain"}]
    with open(path, "wb") as f:
        pickle.dump(recs[:1], f)                                 # a list of records, then one record
        pickle.dump(recs[1], f)
    out = _records([str(path)], "text_embedding")
    assert [r["caption"] for r in out] == ["a dog barks", "barking", "rain"]
    assert np.array_equal(out[1]["emb"], recs[0]["text_embedding"])
    assert np.array_equal(_records([str(path)], "audio_embedding")[2]["emb"], np.ones(4))
