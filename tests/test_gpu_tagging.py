"""The tagging head end to end on the GPU: AudioEncoder.events_logmel / encode_events, the
drop-in's forward_features and zsaac.tagging.AudioTagger, batch 2, htsat.npz's log-mel.

There is no whole-chain numeric bound against the golden here: the tokens come from the encoder
pass that tests/test_gpu_parity.py::test_encoder_from_logmel pins, the reference head ->
tagging_ref is pinned on the CPU (tests/test_tagging_ref.py), and tagging_ref -> the kernels is
what this file and tests/test_gpu_tagging_kernels.py pin: the head's outputs are compared with
tagging_ref applied to the engine's OWN final tokens."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tagging_ref as T  # noqa: E402
from test_gpu_encoder_kernels import _check, _check_bf16, _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
P = "audio_encoder.audio_enc."


def _sd():
    from zsaac import synthetic as S
    sd = S.htsat_state_dict(3)
    sd.update(S.audio_proj_state_dict(5))
    return sd


def _bn_logmel(golden, sd):
    from oracle import audio as A
    lm = torch.from_numpy(golden("htsat.npz")["logmel"])        # [2, 1, 1001, 64] (pre-bn0)
    return A.bn0(lm, dict(sd))                                  # [2, 1, 1001, 64]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_events_logmel(cuda, golden, dtype):
    from zsaac.encoder import AudioEncoder
    sd = _sd()
    enc = AudioEncoder(sd, "htsat", dtype, max_batch=2, device=cuda)
    assert enc._tagbuf is None and not enc._tagw            # nothing of the head before first use
    bn = _bn_logmel(golden, sd)[:, 0].to(cuda)
    emb0 = enc.encode_logmel(bn).clone()
    feat0 = enc.feat[:2].clone()
    out = enc.events_logmel(bn)
    torch.cuda.synchronize()
    assert _same_bits(out.feat, feat0) and _same_bits(out.emb, emb0)
    assert out.clip.shape == (2, 527) and out.frame.shape == (2, 32, 527)
    assert out.fine.shape == (2, 32, 768) and out.tokens.shape == (2, 64, 768)
    a = (out.tokens.cpu(), sd[P + "norm.weight"], sd[P + "norm.bias"], sd[P + "tscam_conv.weight"],
         sd[P + "tscam_conv.bias"])
    r64, r32 = T.head(*a), T.head(*a, dtype=F32)
    _check("fine", out.fine.cpu(), r64["fine"], r32["fine"])
    if dtype == F32:
        _check("frame", out.frame.cpu(), r64["frame"], r32["frame"])
        _check("clip", out.clip.cpu(), r64["clip"], r32["clip"])
    else:
        twin = T.head(*a, dtype=F32, rnd=BF16)
        _check_bf16("frame", out.frame.cpu(), r64["frame"], twin["frame"])
        _check_bf16("clip", out.clip.cpu(), r64["clip"], twin["clip"])
    # the embedding is ln_meanpool's: the mean over time of fine is the same quantity
    assert float((out.fine.mean(1) - out.feat).abs().max()) < 1e-4
    # encode after events: unchanged; a twin has its own head buffers and the same packed weight
    assert _same_bits(enc.encode_logmel(bn), emb0)
    tw = enc.twin()
    assert tw._tagbuf is None and tw._tagw is enc._tagw
    o2 = tw.events_logmel(bn)
    assert _same_bits(o2.clip.contiguous(), out.clip.contiguous()) and o2.frame.data_ptr() != out.frame.data_ptr()


def test_events_refused_without_the_head(cuda):
    from zsaac import synthetic as S
    from zsaac.encoder import AudioEncoder
    sd = {k: v for k, v in _sd().items() if "tscam_conv" not in k}
    enc = AudioEncoder(sd, "htsat", BF16, max_batch=1, device=cuda)
    wav = S.synthetic_waveforms(1).to(cuda)
    assert enc.encode(wav).shape == (1, 1024)                  # encode needs no head
    with pytest.raises(KeyError, match="tscam_conv"):
        enc.encode_events(wav)


def test_dropin_forward_features(cuda):
    from retrieval.models.ase_model import ASE
    from zsaac import synthetic as S
    cfg = {"audio_args": {"sr": 32000, "n_fft": 1024, "hop_length": 320, "f_min": 50, "f_max": 14000,
                          "n_mels": 64, "max_length": 10, "mono": True},
           "audio_encoder_args": {"type": "transformer", "pretrained": False, "freeze": False},
           "training": {"spec_augmentation": True}, "embed_size": 1024}
    ase = ASE(cfg)
    sd = ase.state_dict()
    sd.update(_sd())
    ase.load_state_dict(sd)
    ht = ase.to(cuda).eval().audio_encoder.audio_enc
    wav = S.synthetic_waveforms(2).to(cuda)
    emb = ht(wav)
    eng = ht._engine(2, 320000, wav.device)
    img = eng.img[:2].clone().unsqueeze(1)                     # the image forward() just folded
    assert _same_bits(ht.reshape_wav2img(eng.logmel[:2].clone().unsqueeze(1)), img)
    out = ht.forward_features(img)
    assert set(out) == {"framewise_output", "clipwise_output", "fine_grained_embedding", "embedding"}
    assert out["framewise_output"].shape == (2, 1024, 527) and out["clipwise_output"].shape == (2, 527)
    assert out["fine_grained_embedding"].shape == (2, 1024, 768) and out["embedding"].shape == (2, 768)
    assert all(v.dtype == F32 for v in out.values())
    assert _same_bits(out["embedding"], emb)
    tb = eng._tagbuf
    for key, t32 in (("framewise_output", tb["frame"][:2]), ("fine_grained_embedding", tb["fine"][:2])):
        assert torch.equal(out[key].view(2, 32, 32, -1), t32[:, :, None, :].expand(2, 32, 32, t32.shape[-1]))
    assert torch.equal(out["clipwise_output"], tb["clip"][:2, :527])


def test_audio_tagger(cuda):
    from zsaac import synthetic as S
    from zsaac.tagging import FRAME_SECONDS, AudioTagger
    names = [f"sound {i}" for i in range(527)]
    tg = AudioTagger(_sd(), names, dtype=BF16, batch=2, device=cuda)
    wav = S.synthetic_waveforms(2).to(cuda)
    ids, prob = tg.tag_wav(wav, k=5)
    ids, prob = ids.cpu().long(), prob.cpu()
    clip = tg.enc._tagbuf["clip"][:2, :527].cpu()
    v6, i6 = torch.topk(clip, 6, dim=1)
    assert torch.equal(prob, v6[:, :5])
    for b in range(2):
        for q in range(5):
            if (q == 0 or v6[b, q] != v6[b, q - 1]) and v6[b, q] != v6[b, q + 1]:
                assert int(ids[b, q]) == int(i6[b, q]), (b, q)
    # events: every run of the chosen classes' frame probabilities, found again on the host
    frame = tg.enc._tagbuf["frame"][:2].cpu()
    thr = float(frame[0, :, ids[0, 0]].median())
    ev = tg.events_wav(wav, k=5, threshold=thr, min_frames=2)
    want = []
    for b in range(2):
        for q in range(5):
            c = int(ids[b, q])
            want += [(b, c, names[c], s * FRAME_SECONDS, e * FRAME_SECONDS, pk)
                     for s, e, pk in T.segments(frame[b, :, c].tolist(), thr, 2)]
    assert ev == want and any(e[0] == 0 and e[1] == int(ids[0, 0]) for e in ev)
    assert all(0.0 <= e[3] < e[4] <= 10.24 + 1e-9 for e in ev)
