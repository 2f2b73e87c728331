"""Teacher-forced scoring: log p(caption | clip) under the captioning model.

The converse of generation: given a clip and a caption, the log-probability of every caption
token -- the cross-entropy the reference trains on (train_prompt.py:133, over
ClapCaption_prompt.forward's logits, caption_model.py:297-313) -- for validation loss and
perplexity on reference captions, re-ranking candidates, teacher-forced accuracy and a continuous
bf16-vs-f32 measure.

Clip b with hard prompt ``hard[b][:H_b]`` (as prompt_kernel assembles it), ``n = prefix_length``
soft rows and caption ``cap[b][:T_b]`` is scored on the sequence generate2 / generate_beam
condition on (predict_prompt.py:129-148), not on the padded training layout:

    [wte(hard) ; soft ; wte(cap[:T_b - 1])]      positions 0 .. S_b - 1

token ``cap[b][t]`` being predicted from the row at position ``H_b + n - 1 + t``; temperature 1.
Per call: prompt assembly and mapper (as CaptionPipeline.begin_emb), zs_gpt2_score_embed,
the decoder's ragged prefill, ln_f of the scored rows only, zs_lmhead_nll (the LM head with the
softmax statistics and the target's logit taken in registers: no [rows, 50257] logits in memory)
and zs_nll_finalize.  Nothing synchronises with the host until a result is read.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from ._lib import ZsError
from .decoder import Gpt2Decoder

Captions = Union[Sequence[Sequence[int]], Tuple[torch.Tensor, torch.Tensor]]


@dataclass
class CaptionScores:
    token_logprob: torch.Tensor   # [B, Tmax] f32: log p(cap[b][t] | clip, cap[b][:t]); 0 for t >= T_b
    argmax_ids: torch.Tensor      # [B, Tmax] int32: the model's own pick there (ties -> lower id); -1 for t >= T_b
    sum_logprob: torch.Tensor     # [B] f32
    n_tokens: torch.Tensor        # [B] int32 (T_b)
    target_ids: torch.Tensor      # [B, Tmax] int32: cap[b][t]; -1 for t >= T_b
    status: Optional[torch.Tensor] = None   # [1] int32: ids / lengths the device had to correct

    def check(self) -> "CaptionScores":
        """Raises if the device met an id outside the vocabulary or a length outside its buffer
        (the first host synchronisation of a scoring call)."""
        if self.status is not None:
            bad = int(self.status.item())
            self.status = None
            if bad:
                raise ZsError(f"caption scoring: {bad} token id(s) outside the vocabulary or "
                              "length(s) outside the buffers")
        return self

    def mean_nll(self) -> torch.Tensor:
        """Per caption -sum_logprob / n_tokens; NaN for an empty caption."""
        self.check()
        n = self.n_tokens.to(torch.float32)
        return torch.where(n > 0, -self.sum_logprob / n.clamp(min=1), torch.full_like(n, math.nan))

    def perplexity(self) -> float:
        """exp(total NLL / total tokens) over every caption held (NaN without tokens)."""
        self.check()
        n = int(self.n_tokens.sum().item())
        if n == 0:
            return math.nan
        return math.exp(-float(self.sum_logprob.double().sum().item()) / n)

    def accuracy(self) -> float:
        """Teacher-forced accuracy: the share of caption tokens that are the model's argmax."""
        self.check()
        valid = self.target_ids >= 0
        n = int(valid.sum().item())
        if n == 0:
            return math.nan
        return int(((self.argmax_ids == self.target_ids) & valid).sum().item()) / n

    def cpu(self) -> "CaptionScores":
        self.check()
        return CaptionScores(self.token_logprob.cpu(), self.argmax_ids.cpu(), self.sum_logprob.cpu(),
                             self.n_tokens.cpu(), self.target_ids.cpu())

    @staticmethod
    def cat(parts: Sequence["CaptionScores"]) -> "CaptionScores":
        """The scores of several calls of one scorer as one corpus."""
        for p in parts:
            p.check()
        return CaptionScores(*(torch.cat([getattr(p, f) for p in parts]) for f in
                               ("token_logprob", "argmax_ids", "sum_logprob", "n_tokens",
                                "target_ids")))


def load_captions(captions: Captions, B: int, T: int, V: int, cap_ids: torch.Tensor,
                  cap_len: torch.Tensor):
    """captions -> cap_ids[:B] / cap_len[:B] (device buffers [>= B, T] / [>= B] int32).  Host data
    is checked here; device tensors by the kernel (CaptionScores.check)."""
    if (isinstance(captions, tuple) and len(captions) == 2
            and isinstance(captions[0], torch.Tensor)):
        ids, ln = captions
        if ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] > T or ln.numel() != B:
            raise ZsError(f"captions: ids [{B}, <= {T}] and len [{B}] expected, got "
                          f"{tuple(ids.shape)} and {tuple(ln.shape)}")
        if not ids.is_cuda:
            if ln.is_cuda:
                raise ZsError("captions: ids and len on the same side")
            lens = [int(v) for v in ln.reshape(-1).tolist()]
            if any(v < 0 or v > ids.shape[1] for v in lens):
                raise ZsError("captions: a length outside the id tensor")
            captions = [ids[b, :lens[b]].tolist() for b in range(B)]
        else:
            if ids.shape[1] < T:
                cap_ids[:B].zero_()
            cap_ids[:B, :ids.shape[1]].copy_(ids)
            cap_len[:B].copy_(ln.reshape(-1))
            return
    if len(captions) != B:
        raise ZsError(f"captions: {len(captions)} captions for {B} clips")
    ids = np.zeros((B, T), dtype=np.int32)
    ln = np.zeros(B, dtype=np.int32)
    for b, c in enumerate(captions):
        c = [int(t) for t in c]
        if len(c) > T:
            raise ZsError(f"caption {b}: {len(c)} tokens (max_caption_tokens {T})")
        if any(t < 0 or t >= V for t in c):
            raise ZsError(f"caption {b}: token id outside [0, {V})")
        ids[b, :len(c)] = c
        ln[b] = len(c)
    cap_ids[:B].copy_(torch.from_numpy(ids))
    cap_len[:B].copy_(torch.from_numpy(ln))


class CaptionScorer:
    """Scores captions of up to ``max_caption_tokens`` tokens for up to ``pipeline.cfg.batch``
    clips per call.  Shares the pipeline's packed GPT-2 weights, mapper and label tables (so it
    must not run concurrently with that pipeline on another stream); owns its decoder, KV cache
    and scoring buffers."""

    def __init__(self, pipeline, max_caption_tokens: int = 67):
        p, cfg = pipeline, pipeline.cfg
        if max_caption_tokens < 1:
            raise ZsError("CaptionScorer: max_caption_tokens >= 1")
        self.pipe, self.Tmax = p, int(max_caption_tokens)
        self.Smax = p.h_cap + cfg.prefix_length + self.Tmax - 1
        if self.Smax > 256:
            raise ZsError(f"CaptionScorer: {self.Smax} positions (hard prompt {p.h_cap} + prefix "
                          f"{cfg.prefix_length} + caption {self.Tmax} - 1) exceed zs_row_attention's 256")
        B, T, dev, w = cfg.batch, self.Tmax, p.dev, p.gpt
        self.dec = Gpt2Decoder(w, B, self.Smax, 1, use_graph=False)
        nblk = self.dec.nblk
        i32 = dict(device=dev, dtype=torch.int32)
        self.hard_ids = torch.zeros(B, p.h_cap, **i32)
        self.hard_len = torch.zeros(B, **i32)
        self.prefix = torch.empty(B, 1024, device=dev)
        self.cap_ids = torch.zeros(B, T, **i32)
        self.cap_len = torch.zeros(B, **i32)
        self.score_rows = torch.zeros(B, T, **i32)
        self.tgt = torch.zeros(B, T, **i32)
        self.status = torch.zeros(1, **i32)
        self.hf = torch.empty(B * T, w.wte.shape[1], device=dev, dtype=w.dtype)
        self.pstat = torch.empty(B * T, nblk, 2, device=dev)
        self.pval = torch.empty(B * T, nblk, device=dev)
        self.pidx = torch.empty(B * T, nblk, **i32)
        self.tgt_logit = torch.zeros(B * T, device=dev)
        self.logprob = torch.zeros(B, T, device=dev)
        self.argmax = torch.zeros(B, T, **i32)
        self.sum = torch.zeros(B, device=dev)
        self.cnt = torch.zeros(B, **i32)

    # ------------------------------------------------------------------ inputs
    def _load_captions(self, captions: Captions, B: int):
        load_captions(captions, B, self.Tmax, self.pipe.gpt.V, self.cap_ids, self.cap_len)

    # ------------------------------------------------------------------ scoring
    def score_wav(self, wav: torch.Tensor, captions: Captions) -> CaptionScores:
        return self.score_emb(self.pipe.encode(wav), captions)

    def score_emb(self, emb: torch.Tensor, captions: Captions) -> CaptionScores:
        """From CLAP audio embeddings [B, 1024]: the hard prompt is assembled on the device as
        for generation."""
        p, cfg, B = self.pipe, self.pipe.cfg, emb.shape[0]
        self._check_batch(B)
        ops.prompt_assemble(emb, p.labels, cfg.sound_effect_num, p.label_tok, p.label_len,
                            self.hard_ids[:B], self.hard_len[:B])
        return self._score(emb, self.hard_ids[:B], self.hard_len[:B], captions)

    def score_prompted(self, emb: torch.Tensor, hard_ids: torch.Tensor, hard_len: torch.Tensor,
                       captions: Captions) -> CaptionScores:
        """With given hard prompts (a CaptionBatch's hard_ids / hard_len; to re-rank beams repeat
        each clip's embedding and prompt once per beam)."""
        B = emb.shape[0]
        self._check_batch(B)
        if (hard_ids.dim() != 2 or hard_ids.shape[0] != B or hard_ids.shape[1] > self.pipe.h_cap
                or hard_len.numel() != B):
            raise ZsError(f"score_prompted: hard_ids [{B}, <= {self.pipe.h_cap}], hard_len [{B}]")
        if hard_ids.shape[1] < self.pipe.h_cap:
            self.hard_ids[:B].zero_()
        self.hard_ids[:B, :hard_ids.shape[1]].copy_(hard_ids)
        self.hard_len[:B].copy_(hard_len.reshape(-1))
        return self._score(emb, self.hard_ids[:B], self.hard_len[:B], captions)

    def _check_batch(self, B):
        if not 0 < B <= self.pipe.cfg.batch:
            raise ZsError(f"CaptionScorer: {B} clips (1 .. {self.pipe.cfg.batch})")

    def _score(self, emb, hard_ids, hard_len, captions) -> CaptionScores:
        p, cfg, dec, w = self.pipe, self.pipe.cfg, self.dec, self.pipe.gpt
        B, T, Smax = emb.shape[0], self.Tmax, self.Smax
        M = B * T
        self._load_captions(captions, B)
        self.status.zero_()
        prefix = self.prefix[:B]
        if cfg.normalize_prefix:
            ops.l2norm(emb, out=prefix)               # dataset.py:448-449
        else:
            prefix.copy_(emb)
        soft = p.mapper(prefix)
        tgt, rows = self.tgt[:B], self.score_rows[:B]
        ops.score_embed(hard_ids, hard_len, soft, p.mapper.soft_ld, cfg.prefix_length,
                        self.cap_ids[:B], self.cap_len[:B], w.wte, w.wpe, B, Smax, dec.x, dec.plen,
                        rows, tgt, self.status)
        dec.prefill(B, Smax)
        hf = self.hf[:M]
        ops.layernorm(dec.x, *w.lnf, out=hf, rows=rows.view(-1))
        ops.lmhead_nll(hf, w.wte, tgt, self.pstat, self.pval, self.pidx, self.tgt_logit)
        ops.nll_finalize(self.pstat, self.pval, self.pidx, tgt, self.tgt_logit, w.V, B, T,
                         self.logprob, self.argmax, self.sum, self.cnt)
        tg = tgt.clone()
        return CaptionScores(self.logprob[:B].clone(),
                             torch.where(tg >= 0, self.argmax[:B], torch.full_like(tg, -1)),
                             self.sum[:B].clone(), self.cnt[:B].clone(), tg, self.status.clone())


def beam_captions(batch) -> Tuple[List[List[int]], List[int]]:
    """A beam-search CaptionBatch's beams as a flat caption list (clip-major, the decoder's beam
    order) and the clip index of each: the inputs of a re-ranking score_prompted call."""
    ids, ln = batch.ids.cpu().numpy(), batch.lengths.cpu().numpy()
    caps, clip = [], []
    for c in range(ids.shape[0]):
        for i in range(ids.shape[1]):
            caps.append(ids[c, i, :int(ln[c, i])].tolist())
            clip.append(c)
    return caps, clip
