"""Projection of embeddings onto a text memory bank (predict_prompt.py:23-56).

The caption model is trained on CLAP text embeddings and evaluated on audio embeddings; the
reference closes that gap by replacing an audio embedding ``q`` with a softmax-weighted mix of a
bank ``T`` of caption embeddings (``map2memory``)::

    w = softmax(100 * q @ T.T);  prefix = normalize(w @ T)

and builds ``T`` from its text-embedding pickles (``construct_support_memory``).  Its route
materialises the [M, N] logits, runs a separate softmax and reads the bank twice.  Here one fused
pass (zs_memory_project: online softmax, every bank tile fetched once for both products) writes
per-split partials and zs_memory_merge combines them; a bank given as several chunk tensors runs
one pass per chunk and the finished chunks re-enter the merge as ``(mix, lse, 1)``.

Device tensors, the current stream, no host synchronisation; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Iterable, List, Sequence, Union

import torch

from . import ops, safeload
from ._lib import ZsError
from .retrieval import _dtype, _prep

MAX_K = 1024


class SupportMemory:
    """A bank of text embeddings on the device, ready for ``project``.

    ``text_features``: one [N, K] tensor or a list of [N_i, K] chunk tensors (host or device).
    Rows are L2-normalised once in f32 (``normalize``; construct_support_memory does the same),
    padded with zero columns to K % 32 == 0 and cast to the compute dtype (``dtype``: f32 / bf16,
    default: the features' own dtype if it is one of the two, else f32)."""

    def __init__(self, text_features: Union[torch.Tensor, Sequence[torch.Tensor]], dtype=None,
                 device="cuda", normalize: bool = True):
        chunks = [text_features] if isinstance(text_features, torch.Tensor) else list(text_features)
        if not chunks or any(c.dim() != 2 or c.shape[0] == 0 for c in chunks):
            raise ZsError("SupportMemory: text_features is [N, K] or a list of such chunks, N > 0")
        self.K = int(chunks[0].shape[1])
        if any(c.shape[1] != self.K for c in chunks) or not 0 < self.K <= MAX_K:
            raise ZsError(f"SupportMemory: chunks share one K, 0 < K <= {MAX_K}")
        self.dtype = _dtype(chunks[0], dtype)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise ZsError("SupportMemory lives on the device (no CPU fallback)")
        self.chunks: List[torch.Tensor] = [_prep(c.to(self.dev), self.dtype, normalize) for c in chunks]
        self.Kp = int(self.chunks[0].shape[1])
        self.N = sum(int(c.shape[0]) for c in self.chunks)
        self.nsplit = [ops.memory_nsplit(int(c.shape[0]), self.Kp, self.dtype) for c in self.chunks]

    def project(self, emb: torch.Tensor, scale: float = 100.0, normalize: bool = True,
                return_lse: bool = False, nsplit=None):
        """emb [M, K] -> [M, K] f32: softmax(scale * emb @ T.T) @ T, rows L2-normalised with
        ``normalize``; with ``return_lse`` also lse [M] = log sum_n exp(scale * emb . T[n]).
        ``emb`` is used as given (not normalised), in the bank's compute dtype.  ``nsplit``
        overrides the split count of every chunk."""
        if not isinstance(emb, torch.Tensor) or not emb.is_cuda:
            raise ZsError("SupportMemory.project takes device tensors (no CPU fallback)")
        if emb.dim() != 2 or emb.shape[1] != self.K or emb.shape[0] == 0:
            raise ZsError(f"SupportMemory.project: emb is [M, {self.K}], M > 0")
        q = _prep(emb, self.dtype, False)
        M, Kp, dev = q.shape[0], self.Kp, q.device
        f32 = torch.float32
        nc = len(self.chunks)
        out = torch.empty(M, Kp, dtype=f32, device=dev)
        lse = torch.empty(M, dtype=f32, device=dev) if return_lse else None
        if nc > 1:
            cmix = torch.empty(M, nc, Kp, dtype=f32, device=dev)
            cml = torch.ones(M, nc, 2, dtype=f32, device=dev)
            clse = torch.empty(M, dtype=f32, device=dev)
        for i, bank in enumerate(self.chunks):
            ns = int(nsplit) if nsplit is not None else self.nsplit[i]
            pm = torch.empty(M, ns, Kp, dtype=f32, device=dev)
            pl = torch.empty(M, ns, 2, dtype=f32, device=dev)
            ops.memory_project(q, bank, scale, ns, pm, pl)
            if nc == 1:
                ops.memory_merge(pm, pl, M, ns, Kp, out, normalize, lse)
            else:                                  # the chunk as (mix, lse, 1)
                ops.memory_merge(pm, pl, M, ns, Kp, cmix[:, i], False, clse)
                cml[:, i, 0] = clse
        if nc > 1:
            ops.memory_merge(cmix, cml, M, nc, Kp, out, normalize, lse)
        res = out if Kp == self.K else out[:, :self.K].contiguous()
        return (res, lse) if return_lse else res


def map2memory(audio_embed: torch.Tensor, text_features) -> torch.Tensor:
    """predict_prompt.py:23-29, same name and argument order: normalize(softmax(100 * audio_embed
    @ text_features.T) @ text_features), [M, K] f32.  ``text_features`` is a SupportMemory (built
    once, the fast way) or the bank rows as stored (used as they are, like the reference)."""
    if not isinstance(audio_embed, torch.Tensor) or not audio_embed.is_cuda:
        raise ZsError("map2memory takes device tensors (no CPU fallback)")
    mem = text_features if isinstance(text_features, SupportMemory) else SupportMemory(
        text_features, dtype=torch.float32, device=audio_embed.device, normalize=False)
    x = audio_embed.reshape(-1, audio_embed.shape[-1])
    return mem.project(x, 100.0, True).view(*audio_embed.shape[:-1], mem.K)


def read_support_items(paths: Iterable[str], min_words: int = 8, max_words: int = 20) -> list:
    """The records construct_support_memory keeps (predict_prompt.py:30-48): every file is a
    stream of pickles; a list is taken whole, a single record only if its caption has
    min_words .. max_words whitespace-separated words."""
    items = []
    for p in paths:
        for obj in safeload.iter_pickles(p):
            if isinstance(obj, list):
                items.extend(obj)
            elif min_words <= len(str(obj["caption"]).split()) <= max_words:
                items.append(obj)
    return items


def construct_support_memory(paths: Iterable[str], min_words: int = 8, max_words: int = 20) -> torch.Tensor:
    """predict_prompt.py:30-56: the kept records' ``text_embedding`` rows concatenated, then
    L2-normalised; [N, K] f32 on the host (the reference divides by the bare norm)."""
    if isinstance(paths, (str, bytes)):
        paths = [paths]
    items = read_support_items(paths, min_words, max_words)
    if not items:
        raise ZsError("construct_support_memory: no record kept")
    rows = [safeload.as_tensor(it["text_embedding"]) for it in items]
    feats = torch.cat([r.reshape(-1, r.shape[-1]) for r in rows], dim=0)
    return feats / feats.norm(dim=-1, keepdim=True)
