#!/usr/bin/env python3
"""Regenerates tests/golden/htsat_head.npz from the reference's own
``HTSAT_Swin_Transformer.forward_features`` (retrieval/models/htsat.py:830-894, imported from
/root/reference through tests/golden/_refshim.py and used as it is): the tagging head's four
outputs on htsat.npz's two log-mel clips under the seeded synthetic weights
``synthetic.htsat_state_dict(3)`` -- the weights and the input of htsat.npz, so ``embedding`` must
reproduce its ``embedding768`` exactly (asserted).

``framewise_output`` [2, 1024, 527] and ``fine_grained_embedding`` [2, 1024, 768] are each of 32
frames repeated 32 times (``interpolate``, htsat.py:31-44; asserted), so the file keeps the
32-frame form:
  tokens      [2, 64, 768] f32  the last stage's tokens, the input of ``norm`` (a forward
                                pre-hook on the reference's module; no arithmetic of this script)
  framewise32 [2, 32, 527] f32
  clipwise    [2, 527]     f32
  fine32      [2, 32, 64]  f32  the first 64 channels (the rest adds size, not coverage: every
                                channel runs the same formula)

    python tests/golden/make_htsat_head_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "zero-shot-aac_amd"))
import _refshim  # noqa: E402

_refshim.install()  # puts /root/reference first on sys.path

from zsaac import synthetic as S  # noqa: E402

FINE_CH = 64
MAX_BYTES = 588 * 1024


def audio_config():
    return {"audio_args": {"sr": 32000, "n_fft": 1024, "hop_length": 320, "f_min": 50,
                           "f_max": 14000, "n_mels": 64, "max_length": 10, "mono": True},
            "audio_encoder_args": {"type": "transformer", "model": "Cnn14", "pretrained": False,
                                   "freeze": False},
            "training": {"spec_augmentation": True, "dropout": 0.2}}


def main():
    from retrieval.models.audio_encoder import AudioEncoder  # the reference's module
    enc = AudioEncoder(audio_config())
    missing, unexpected = enc.load_state_dict(
        {k.replace("audio_encoder.", ""): v for k, v in S.htsat_state_dict(3).items()}, strict=False)
    assert not unexpected, unexpected
    assert all(("relative_position_index" in k) or ("attn_mask" in k) for k in missing), missing
    enc.eval()
    ht = enc.audio_enc
    seen = {}
    ht.norm.register_forward_pre_hook(lambda m, args: seen.__setitem__("tokens", args[0].detach().clone()))
    inner = ht.forward_features

    def recording(x):
        seen["out"] = inner(x)
        return seen["out"]
    ht.forward_features = recording

    g = dict(np.load(os.path.join(HERE, "htsat.npz")))
    with torch.no_grad():
        emb = enc(torch.from_numpy(g["logmel"]))
    out = seen["out"]
    diff = float((emb - torch.from_numpy(g["embedding768"])).abs().max())
    assert diff == 0.0 and torch.equal(out["embedding"], emb), diff
    tokens = seen["tokens"]
    frame, fine, clip = out["framewise_output"], out["fine_grained_embedding"], out["clipwise_output"]
    assert tokens.shape == (2, 64, 768) and frame.shape == (2, 1024, 527), (tokens.shape, frame.shape)
    assert fine.shape == (2, 1024, 768) and clip.shape == (2, 527), (fine.shape, clip.shape)
    frame32, fine32 = frame[:, ::32], fine[:, ::32]
    assert torch.equal(frame32.repeat_interleave(32, dim=1), frame), "framewise is not a x32 repeat"
    assert torch.equal(fine32.repeat_interleave(32, dim=1), fine), "fine-grained is not a x32 repeat"
    path = os.path.join(HERE, "htsat_head.npz")
    np.savez_compressed(path, tokens=tokens.numpy(), framewise32=frame32.contiguous().numpy(),
                        clipwise=clip.numpy(),
                        fine32=fine32[:, :, :FINE_CH].contiguous().numpy())
    size = os.path.getsize(path)
    print(f"embedding vs htsat.npz: {diff}; wrote {path} ({size} bytes)")
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
