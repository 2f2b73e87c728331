#!/usr/bin/env python3
"""Regenerates tests/golden/retrieval.npz from the reference's own ``a2t`` / ``t2a``
(retrieval/tools/utils.py:169-251, imported from /root/reference through tests/golden/_refshim.py
and used as they are) on seeded synthetic embeddings.

``sentence_transformers`` is absent here, so ``util.cos_sim`` is a stand-in of this script: rows
normalised to unit length, then one matmul -- what the library's function computes.

Embeddings: 40 clips x 5 captions, K = 128, "shared base + noise": a clip's audio row (repeated 5
times, the reference's layout) and its 5 caption rows share a base vector; the noise is chosen so
that R@1 lies between 20 % and 80 % in both directions.  The reference's ``np.argsort`` leaves the
order of ties unspecified, so the data must hold none: the smallest float64 gap of every
similarity row is asserted > 0, and the seed is the first one for which every gap that decides a
recorded number (a target's or the top-1's distance to every other value of its row) exceeds
1e-5, far above any float32 rounding of a K = 128 dot product.

    python tests/golden/make_retrieval_golden.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

_refshim.install()  # puts /root/reference first on sys.path

from retrieval.tools import utils as U  # noqa: E402  (the reference's module)

N_CLIPS, PER, K = 40, 5, 128
NOISE_AUDIO, NOISE_CAP = 1.0, 4.0
GAP = 1e-5


def cos_sim(a, b):
    a = torch.as_tensor(a).reshape(-1, a.shape[-1])
    b = torch.as_tensor(b).reshape(-1, b.shape[-1])
    a = a / a.norm(dim=1, keepdim=True).clamp(min=1e-12)
    b = b / b.norm(dim=1, keepdim=True).clamp(min=1e-12)
    return a @ b.t()


U.util = types.SimpleNamespace(cos_sim=cos_sim)


def embeddings(seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((N_CLIPS, K))
    audio = base + NOISE_AUDIO * rng.standard_normal((N_CLIPS, K))
    caps = np.repeat(base, PER, 0) + NOISE_CAP * rng.standard_normal((N_CLIPS * PER, K))
    audio /= np.linalg.norm(audio, axis=1, keepdims=True)
    caps /= np.linalg.norm(caps, axis=1, keepdims=True)
    return np.repeat(audio, PER, 0).astype(np.float32), caps.astype(np.float32)


def gaps(audio, caps):
    """(smallest gap of any row, smallest deciding gap) in float64, both directions."""
    a = audio[::PER].astype(np.float64)
    c = caps.astype(np.float64)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    row_min, dec_min = np.inf, np.inf
    for sim, tgt in ((a @ c.T, [list(range(PER * i, PER * i + PER)) for i in range(N_CLIPS)]),
                     (c @ a.T, [[j // PER] for j in range(N_CLIPS * PER)])):
        s = np.sort(sim, axis=1)
        row_min = min(row_min, float(np.diff(s, axis=1).min()))
        for m, cols in enumerate(tgt):
            for j in cols + [int(np.argmax(sim[m]))]:
                d = np.abs(sim[m] - sim[m, j])
                d[j] = np.inf
                dec_min = min(dec_min, float(d.min()))
    return row_min, dec_min


def main():
    for seed in range(10000):
        audio, caps = embeddings(seed)
        row_min, dec_min = gaps(audio, caps)
        if row_min > 0 and dec_min > GAP:
            break
    else:
        raise SystemExit("no seed without near-ties")
    assert row_min > 0
    ra = U.a2t(audio, caps, return_ranks=True)
    rt = U.t2a(audio, caps, return_ranks=True)
    print(f"seed {seed}: smallest row gap {row_min:.3e}, smallest deciding gap {dec_min:.3e}")
    print("a2t", ra[:7])
    print("t2a", rt[:7])
    assert 20.0 <= ra[0] <= 80.0 and 20.0 <= rt[0] <= 80.0, "R@1 outside 20 .. 80 %"
    path = os.path.join(HERE, "retrieval.npz")
    np.savez_compressed(path, audio_embs=audio, cap_embs=caps, seed=np.int64(seed),
                        a2t=np.asarray(ra[:7], dtype=np.float64), a2t_ranks=np.asarray(ra[7]),
                        a2t_top1=np.asarray(ra[8]),
                        t2a=np.asarray(rt[:7], dtype=np.float64), t2a_ranks=np.asarray(rt[7]),
                        t2a_top1=np.asarray(rt[8]))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
