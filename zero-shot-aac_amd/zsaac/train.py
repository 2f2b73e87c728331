"""Training the MLP prefix mapper on the device, GPT-2 frozen (ClipCap's "only prefix" regime).

The loss is the one the reference trains on -- the teacher-forced cross-entropy of
train_prompt.py:133 over ClapCaption_prompt.forward (caption_model.py:297-313) -- on the sequence
CaptionScorer scores (``[wte(hard) ; soft ; wte(cap[:T-1])]``, the positions generation sees),
averaged over the batch's caption tokens.  One step:

    hard prompt (ops.prompt_assemble, from the un-noised embedding, dataset.py:365)
    prefix = l2norm(emb)  ->  noise_injection (utils.py:19-31, zs_noise_inject)
    soft = mapper(prefix) -> score_embed -> 12 blocks -> ln_f(scored rows) -> lmhead_nll ->
    nll_finalize -> zs_nll_loss                                    (CaptionScorer's sequence of ops)
    LM-head gradient without logits (memory_project / memory_merge over wte + zs_nll_grad_rows)
    -> ln_f / block backward (zs_layernorm_bwd, zs_gelu_tanh_bwd, zs_attention_bwd; every product
    zs_gemm on a transposed weight copy) -> d loss / d soft -> the four mapper gradients
    AdamW on f32 masters (zs_adamw), which also refreshes the operand copies pipeline.mapper reads

Three things differ from the reference on purpose: GPT-2 stays frozen (the reference's
``only_prefix`` merely calls gpt.eval(), caption_model.py:331-338, and updates GPT-2 too; GPT-2
weight gradients are the next step), the ragged scoring layout replaces the padded training layout
(whose wpe positions shift by the batch's longest hard prompt), and the mean runs over the
sum of T_b caption tokens (``ignore_index=0`` differs only for a caption holding token id 0).

No torch compute runs inside a step: torch supplies memory (allocation, memset, copies) and the
stream.  Nothing synchronises with the host until a result is read.  DESIGN.md §31.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import ZsError
from .decoder import D, HD, NH, NL
from .score import Captions, CaptionScorer, load_captions

KEYS = ("clap_project.model.0.weight", "clap_project.model.0.bias",
        "clap_project.model.2.weight", "clap_project.model.2.bias")


def linear_schedule(step: int, warmup_steps: int, total_steps: int) -> float:
    """get_linear_schedule_with_warmup's learning-rate factor (train_prompt.py:105-107) at
    ``step`` (the number of updates already made)."""
    if step < warmup_steps:
        return step / max(1, warmup_steps)
    return max(0.0, (total_steps - step) / max(1, total_steps - warmup_steps))


def trained_state_dict(sd: Dict[str, torch.Tensor], tensors: Dict[str, torch.Tensor]) -> Dict:
    """``sd`` (the reference's best.pth key set) with the four mapper tensors replaced."""
    if set(tensors) != set(KEYS):
        raise ZsError(f"trained_state_dict: the tensors {KEYS} expected")
    out = {k: v for k, v in sd.items()}
    for k in KEYS:
        if k not in sd or tuple(sd[k].shape) != tuple(tensors[k].shape):
            raise ZsError(f"trained_state_dict: {k} missing from the state dict or of another shape")
        out[k] = tensors[k].detach().to(device="cpu", dtype=sd[k].dtype).contiguous()
    return out


@dataclass
class TrainGrads:
    loss: torch.Tensor                 # [] f32, on the device
    n_tokens: torch.Tensor             # [B] int32: T_b
    d_soft: torch.Tensor               # [B, prefix_length * 768] f32
    grads: Dict[str, torch.Tensor]     # clap_project.model.{0,2}.{weight,bias}, f32


class MapperTrainer:
    """Trains ``pipeline``'s MLP mapper in place, up to ``pipeline.cfg.batch`` clips per step.
    ``sd`` supplies the f32 originals (the pipeline holds the operands in the model dtype only).
    Shares the pipeline's GPT-2 weights, mapper operands and label tables (so it must not run
    concurrently with that pipeline on another stream); owns its activations, its transposed
    weight copies and its optimiser state."""

    def __init__(self, pipeline, sd, lr: float = 1e-5, weight_decay: float = 0.0,
                 noise_variance: float = 0.0, seed: int = 0, max_caption_tokens: int = 25):
        p, cfg = pipeline, pipeline.cfg
        if cfg.mapping_type == "transformer":
            raise NotImplementedError("MapperTrainer: the Transformer mapper's backward is not "
                                      "built (MLP mapper only)")
        if cfg.mapping_type != "mlp":
            raise ZsError(f"MapperTrainer: mapping_type {cfg.mapping_type!r}")
        if torch.device(p.dev).type != "cuda":
            raise ZsError("MapperTrainer: the pipeline lives on a GPU (no CPU fallback)")
        if max_caption_tokens < 1 or noise_variance < 0:
            raise ZsError("MapperTrainer: max_caption_tokens >= 1, noise_variance >= 0")
        self.pipe, self.sd, self.Tmax = p, sd, int(max_caption_tokens)
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        self.noise_variance, self.seed = float(noise_variance), int(seed)
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self.Smax = p.h_cap + cfg.prefix_length + self.Tmax - 1
        if self.Smax > 256:
            raise ZsError(f"MapperTrainer: {self.Smax} positions exceed the attention kernels' 256")
        w, mp, dev = p.gpt, p.mapper, p.dev
        B, T, S = cfg.batch, self.Tmax, self.Smax
        M, Mr = B * S, B * T
        dt = w.dtype
        self.t = 0                                     # updates made
        f32 = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        # f32 masters, moments, gradients
        self.master = {k: sd[k].detach().to(**f32).contiguous().clone() for k in KEYS}
        for k, op in zip(KEYS, (mp.w0, mp.b0, mp.w2, mp.b2)):
            if tuple(self.master[k].shape) != tuple(op.shape):
                raise ZsError(f"MapperTrainer: {k} {tuple(self.master[k].shape)} does not match the "
                              f"pipeline's mapper {tuple(op.shape)}")
        # the operand copies the pipeline reads restart from the masters: both sides agree
        for k, op in zip(KEYS, (mp.w0, mp.b0, mp.w2, mp.b2)):
            ops.cast(self.master[k], op)
        self.m = {k: torch.zeros_like(v) for k, v in self.master.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.master.items()}
        self.grad = {k: torch.zeros_like(v) for k, v in self.master.items()}
        self.step_dev = torch.zeros(1, **i32)
        # GPT-2's weights transposed once (bf16: the LN-folded ones): dX = dY . W as zs_gemm
        self.wT = [{k: ly[k].t().contiguous() for k in ("attn_w", "proj_w", "fc_w", "mproj_w")}
                   for ly in w.layers]
        self.ln_g = [(None if w.folded else ly["ln1"][0], None if w.folded else ly["ln2"][0])
                     for ly in w.layers]
        H1, Do = mp.w0.shape[0], mp.out_dim
        self.w2T = torch.zeros(H1, -(-Do // 32) * 32, device=dev, dtype=dt)
        # inputs
        self.hard_ids = torch.zeros(B, p.h_cap, **i32)
        self.hard_len = torch.zeros(B, **i32)
        self.cap_ids = torch.zeros(B, T, **i32)
        self.cap_len = torch.zeros(B, **i32)
        self.score_rows = torch.zeros(B, T, **i32)
        self.tgt = torch.zeros(B, T, **i32)
        self.plen = torch.zeros(B, **i32)
        self.status = torch.zeros(1, **i32)
        # mapper activations
        self.prefix = torch.zeros(B, mp.in_dim, **f32)
        self.x_t = torch.zeros(B, mp.in_dim, device=dev, dtype=dt)
        self.h32 = torch.zeros(B, H1, **f32)
        self.h_t = torch.zeros(B, H1, device=dev, dtype=dt)
        self.soft = torch.zeros(B, Do, **f32)
        # GPT-2 activations kept for the backward pass (zeroed: padding rows must stay finite)
        self.xs = [torch.zeros(M, D, **f32) for _ in range(2 * NL + 1)]
        self.qkv = [torch.zeros(M, 3 * D, device=dev, dtype=dt) for _ in range(NL)]
        self.u = [torch.zeros(M, 4 * D, device=dev, dtype=dt) for _ in range(NL)]
        self.h = torch.zeros(M, D, device=dev, dtype=dt)
        self.att = torch.zeros(M, D, device=dev, dtype=dt)
        self.hid = torch.zeros(M, 4 * D, device=dev, dtype=dt)
        # LM head
        nblk = ops.lmhead_nblk(w.V)
        self.hf = torch.zeros(Mr, D, device=dev, dtype=dt)
        self.pstat = torch.zeros(Mr, nblk, 2, **f32)
        self.pval = torch.zeros(Mr, nblk, **f32)
        self.pidx = torch.zeros(Mr, nblk, **i32)
        self.tgt_logit = torch.zeros(Mr, **f32)
        self.logprob = torch.zeros(B, T, **f32)
        self.lse = torch.zeros(B, T, **f32)
        self.argmax = torch.zeros(B, T, **i32)
        self.sum = torch.zeros(B, **f32)
        self.cnt = torch.zeros(B, **i32)
        self.loss = torch.zeros(1, **f32)
        self.nsplit = ops.memory_nsplit(w.V, D, dt)
        self.part_mix = torch.zeros(Mr, self.nsplit, D, **f32)
        self.part_ml = torch.zeros(Mr, self.nsplit, 2, **f32)
        self.mix = torch.zeros(Mr, D, **f32)
        self.dhf = torch.zeros(Mr, D, **f32)
        # backward
        self.dx = torch.zeros(M, D, **f32)
        self.dxc = torch.zeros(M, D, device=dev, dtype=dt) if dt != torch.float32 else None
        self.dh = torch.zeros(M, D, **f32)
        self.dhid = torch.zeros(M, 4 * D, **f32)
        self.du = torch.zeros(M, 4 * D, device=dev, dtype=dt)
        self.datt = torch.zeros(M, D, device=dev, dtype=dt)
        self.dqkv = torch.zeros(M, 3 * D, device=dev, dtype=dt)
        self.d_soft = torch.zeros(B, Do, **f32)
        self.d_soft_c = torch.zeros(B, Do, device=dev, dtype=dt) if dt != torch.float32 else None
        self.dh1 = torch.zeros(B, H1, **f32)
        self.dpre = torch.zeros(B, H1, **f32)
        Bp = -(-B // 32) * 32
        self.tr = {n: torch.zeros(c * Bp, device=dev, dtype=dt)
                   for n, c in (("ds", Do), ("h", H1), ("dp", H1), ("x", mp.in_dim))}

    # ------------------------------------------------------------------ checks
    @staticmethod
    def _check_emb(emb, max_batch: int, in_dim: int = 1024):
        if not isinstance(emb, torch.Tensor) or not emb.is_cuda:
            raise ZsError("MapperTrainer: embeddings are device tensors (no CPU fallback)")
        if emb.dim() != 2 or emb.shape[1] != in_dim or emb.dtype != torch.float32:
            raise ZsError(f"MapperTrainer: emb is [B, {in_dim}] f32, got {tuple(emb.shape)} {emb.dtype}")
        if not 0 < emb.shape[0] <= max_batch:
            raise ZsError(f"MapperTrainer: {emb.shape[0]} clips (1 .. {max_batch})")

    def check(self) -> "MapperTrainer":
        """Raises if the device met a token id outside the vocabulary or a length outside its
        buffer since the last check (a host synchronisation)."""
        bad = int(self.status.item())
        self.status.zero_()
        if bad:
            raise ZsError(f"MapperTrainer: {bad} token id(s) outside the vocabulary or length(s) "
                          "outside the buffers")
        return self

    # ------------------------------------------------------------------ forward / backward
    def _cast(self, x, buf):
        """x as a GEMM operand of the model dtype (f32: x itself)."""
        if buf is None:
            return x
        return ops.cast(x, buf[:x.shape[0]])

    def _forward(self, B):
        p, cfg, w, mp = self.pipe, self.pipe.cfg, self.pipe.gpt, self.pipe.mapper
        S, T = self.Smax, self.Tmax
        M, Mr = B * S, B * T
        ops.cast(self.prefix[:B], self.x_t[:B])
        ops.gemm(self.x_t[:B], mp.w0, self.h32[:B], bias=mp.b0, act=ops.ACT_TANH)
        ops.cast(self.h32[:B], self.h_t[:B])
        ops.gemm(self.h_t[:B], mp.w2, self.soft[:B], bias=mp.b2)
        ops.score_embed(self.hard_ids[:B], self.hard_len[:B], self.soft[:B], mp.soft_ld,
                        cfg.prefix_length, self.cap_ids[:B], self.cap_len[:B], w.wte, w.wpe, B, S,
                        self.xs[0], self.plen, self.score_rows[:B], self.tgt[:B], self.status)
        h, att, hid = self.h[:M], self.att[:M], self.hid[:M]
        for l, ly in enumerate(w.layers):
            x0, x1, x2 = self.xs[2 * l][:M], self.xs[2 * l + 1][:M], self.xs[2 * l + 2][:M]
            qkv, u = self.qkv[l][:M], self.u[l][:M]
            ops.layernorm(x0, *ly["ln1"], out=h)
            ops.gemm(h, ly["attn_w"], qkv, bias=ly["attn_b"])
            ops.row_attention(qkv, 3 * D, qkv[:, D:], qkv[:, 2 * D:], 3 * D, B, S, NH, HD, True,
                              1.0 / math.sqrt(HD), att, D, lens=self.plen[:B])
            ops.gemm(att, ly["proj_w"], x1, bias=ly["proj_b"], residual=x0)
            ops.layernorm(x1, *ly["ln2"], out=h)
            ops.gemm(h, ly["fc_w"], u, bias=ly["fc_b"])                       # the pre-activation
            ops.gemm(h, ly["fc_w"], hid, bias=ly["fc_b"], act=ops.ACT_GELU_TANH)
            ops.gemm(hid, ly["mproj_w"], x2, bias=ly["mproj_b"], residual=x1)
        rows, tgt = self.score_rows[:B].view(-1), self.tgt[:B]
        hf = self.hf[:Mr]
        ops.layernorm(self.xs[2 * NL], *w.lnf, out=hf, rows=rows)
        ops.lmhead_nll(hf, w.wte, tgt, self.pstat, self.pval, self.pidx, self.tgt_logit)
        ops.nll_finalize(self.pstat, self.pval, self.pidx, tgt, self.tgt_logit, w.V, B, T,
                         self.logprob, self.argmax, self.sum, self.cnt, lse=self.lse)
        ops.nll_loss(self.sum[:B], self.cnt[:B], self.loss)

    def _backward(self, B):
        p, cfg, w, mp = self.pipe, self.pipe.cfg, self.pipe.gpt, self.pipe.mapper
        S, T = self.Smax, self.Tmax
        M, Mr = B * S, B * T
        rows, tgt = self.score_rows[:B].view(-1), self.tgt[:B].view(-1)
        # LM head: dhf = (softmax mix of wte - wte[target]) / tokens, no logits in memory
        ops.memory_project(self.hf[:Mr], w.wte, 1.0, self.nsplit, self.part_mix, self.part_ml)
        ops.memory_merge(self.part_mix, self.part_ml, Mr, self.nsplit, D, self.mix, normalize=False)
        ops.nll_grad_rows(self.mix[:Mr], w.wte, tgt, self.cnt[:B], self.dhf, M=Mr)
        dx, dh = self.dx[:M], self.dh[:M]
        dx.zero_()
        ops.layernorm_bwd(self.xs[2 * NL], self.dhf[:Mr], self.dx, g=w.lnf[0], rows=rows)
        for l in range(NL - 1, -1, -1):
            wT, (g1, g2) = self.wT[l], self.ln_g[l]
            x0, x1 = self.xs[2 * l][:M], self.xs[2 * l + 1][:M]
            ops.gemm(self._cast(dx, self.dxc), wT["mproj_w"], self.dhid[:M])
            ops.gelu_tanh_bwd(self.u[l][:M], self.dhid[:M], self.du[:M])
            ops.gemm(self.du[:M], wT["fc_w"], dh)
            ops.layernorm_bwd(x1, dh, dx, g=g2, residual=dx)
            ops.gemm(self._cast(dx, self.dxc), wT["proj_w"], self.datt[:M])
            ops.attention_bwd(self.qkv[l][:M], self.datt[:M], B, S, NH, self.dqkv[:M],
                              lens=self.plen[:B])
            ops.gemm(self.dqkv[:M], wT["attn_w"], dh)
            ops.layernorm_bwd(x0, dh, dx, g=g1, residual=dx)
        ds = self.d_soft[:B]
        ops.soft_grad_rows(self.dx, self.hard_len[:B], p.h_cap, cfg.prefix_length, B, S, ds)
        # mapper: soft = h W2^T + b2, h = tanh(x W0^T + b0)
        g = self.grad
        Bp = -(-B // 32) * 32
        tr = lambda n, src: ops.transpose_cast(src, self.tr[n][:src.shape[1] * Bp].view(src.shape[1], Bp))
        ops.colsum(ds, g[KEYS[3]])
        ops.gemm(tr("ds", ds), tr("h", self.h32[:B]), g[KEYS[2]])
        ops.transpose_cast(self.master[KEYS[2]], self.w2T)
        ops.gemm(self._cast(ds, self.d_soft_c), self.w2T, self.dh1[:B])
        ops.tanh_bwd(self.h32[:B], self.dh1[:B], self.dpre[:B])
        ops.colsum(self.dpre[:B], g[KEYS[1]])
        ops.gemm(tr("dp", self.dpre[:B]), tr("x", self.prefix[:B]), g[KEYS[0]])

    def _run(self, emb, captions, hard, noise, row_ids):
        p, cfg = self.pipe, self.pipe.cfg
        self._check_emb(emb, cfg.batch, p.mapper.in_dim)
        B = emb.shape[0]
        emb = emb.contiguous()
        if hard is None:
            ops.prompt_assemble(emb, p.labels, cfg.sound_effect_num, p.label_tok, p.label_len,
                                self.hard_ids[:B], self.hard_len[:B])
        else:
            hard_ids, hard_len = hard
            if (not hard_ids.is_cuda or hard_ids.dim() != 2 or hard_ids.shape[0] != B
                    or hard_ids.shape[1] > p.h_cap or hard_len.numel() != B):
                raise ZsError(f"MapperTrainer: hard = (ids [{B}, <= {p.h_cap}], len [{B}]) on the device")
            if hard_ids.shape[1] < p.h_cap:
                self.hard_ids[:B].zero_()
            self.hard_ids[:B, :hard_ids.shape[1]].copy_(hard_ids)
            self.hard_len[:B].copy_(hard_len.reshape(-1))
        load_captions(captions, B, self.Tmax, p.gpt.V, self.cap_ids, self.cap_len)
        prefix = self.prefix[:B]
        if cfg.normalize_prefix:
            ops.l2norm(emb, out=prefix)                   # dataset.py:448-449
        else:
            prefix.copy_(emb)
        if noise and self.noise_variance > 0:
            ops.noise_inject(prefix, prefix, self.noise_variance, seed=self.seed,
                             step_ctr=self.step_dev, row_id=row_ids)
        self._forward(B)
        self._backward(B)
        return B

    # ------------------------------------------------------------------ public
    def loss_and_grads(self, emb: torch.Tensor, captions: Captions,
                       hard: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                       noise: bool = False, row_ids: Optional[torch.Tensor] = None) -> TrainGrads:
        """The batch's loss, d loss / d soft and the four mapper gradients.  No update, and no
        noise unless ``noise`` (then this trainer's noise_variance / seed at its current step)."""
        B = self._run(emb, captions, hard, noise, row_ids)
        return TrainGrads(self.loss[0].clone(), self.cnt[:B].clone(), self.d_soft[:B].clone(),
                          {k: v.clone() for k, v in self.grad.items()})

    def step(self, emb: torch.Tensor, captions: Captions, lr: Optional[float] = None,
             hard: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
             row_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step (noise when noise_variance > 0) and AdamW update; returns the loss
        before the update, a device scalar.  ``row_ids`` [B] int32: the samples' logical ids for
        the noise (default: their slot in the batch)."""
        self._run(emb, captions, hard, True, row_ids)
        mp = self.pipe.mapper
        self.t += 1
        lr = self.lr if lr is None else float(lr)
        for i, (k, op) in enumerate(zip(KEYS, (mp.w0, mp.b0, mp.w2, mp.b2))):
            ops.adamw(self.master[k], self.grad[k], self.m[k], self.v[k], self.t, lr, *self.betas,
                      eps=self.eps, weight_decay=self.weight_decay, operand=op,
                      step_ctr=self.step_dev if i == 3 else None)
        return self.loss[0].clone()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's best.pth key set with the trained mapper tensors (f32 masters)."""
        return trained_state_dict(self.sd, self.master)

    def save(self, path: str) -> str:
        torch.save(self.state_dict(), path)
        return path


# ------------------------------------------------------------------------------ command line
def _records(paths: Sequence[str], key: str) -> List[Dict]:
    from . import safeload
    out = []
    for path in paths:
        for obj in safeload.iter_pickles(path):
            for it in (obj if isinstance(obj, (list, tuple)) else [obj]):
                caps = it.get("caption", [])
                for c in ([caps] if isinstance(caps, str) else caps):
                    out.append({"emb": it[key], "caption": c})
    return out


def _val_nll(pipe, scorer, tok, recs, T) -> float:
    from . import safeload
    from .predict import reference_ids
    tot, n, B = 0.0, 0, pipe.cfg.batch
    for c0 in range(0, len(recs), B):
        chunk = recs[c0:c0 + B]
        emb = safeload.stack_rows([r["emb"] for r in chunk]).to(pipe.dev)
        sc = scorer.score_emb(emb, [reference_ids(tok, r["caption"], T) for r in chunk]).cpu()
        tot -= float(sc.sum_logprob.double().sum())
        n += int(sc.n_tokens.sum())
    return tot / max(n, 1)


def _parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m zsaac.train", description=__doc__.split("\n")[0])
    ap.add_argument("--data", nargs="+", required=True, help="pickles of records with "
                    "text_embedding / audio_embedding and caption")
    ap.add_argument("--valdata", nargs="*", default=[])
    ap.add_argument("--out_dir", default="./checkpoints")
    ap.add_argument("--ckpt_file", required=True, help="the checkpoint to start from (best.pth); "
                    "required here (GPT-2 stays frozen and comes from it; the reference may start "
                    "without one)")
    ap.add_argument("--params", default=None, help="params.json of that checkpoint "
                    "(default: beside it)")
    ap.add_argument("--tokenizer", default=None, help="directory with GPT-2 vocab.json + merges.txt "
                    "(default: tokenizer/ beside the checkpoint)")
    ap.add_argument("--bs", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5000)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--weight_decay", type=float, default=0.0)
    ap.add_argument("--noise_variance", type=float, default=0.0)
    ap.add_argument("--normalize_prefix", action="store_true", default=None,
                    help="default: the checkpoint's params.json")
    ap.add_argument("--sound_effect_num", type=int, default=None,
                    help="default: the checkpoint's params.json")
    ap.add_argument("--use_audio_embedding", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    return ap


def _apply_flags(params: Dict, a) -> Dict:
    """The checkpoint's params.json with the flags that were given: a flag left out never
    overrides what the checkpoint was trained with."""
    out = dict(params)
    if a.normalize_prefix:
        out["normalize_prefix"] = True
    if a.sound_effect_num is not None:
        out["sound_effect_num"] = a.sound_effect_num
    return out


def main(argv=None) -> int:
    a = _parser().parse_args(argv)

    from . import predict, safeload
    from .pipeline import CaptionPipeline
    from .bpe import GPT2BPE
    pjson = a.params or os.path.join(os.path.dirname(a.ckpt_file), "params.json")
    params = _apply_flags(json.load(open(pjson)), a)
    tok = GPT2BPE.from_dir(a.tokenizer or os.path.join(os.path.dirname(a.ckpt_file), "tokenizer"))
    predict.check_template(tok)
    names, table = predict.load_labels(params["sound_effect"])
    sd = safeload.load_state_dict(a.ckpt_file)
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    cfg = predict.config_from_params(params, False, dtype, a.bs)
    pipe = CaptionPipeline(sd, None, table, predict.label_token_table(tok, names), cfg, device="cuda")
    T = 25
    trainer = MapperTrainer(pipe, sd, lr=a.lr, weight_decay=a.weight_decay,
                            noise_variance=a.noise_variance, seed=a.seed, max_caption_tokens=T)
    key = "audio_embedding" if a.use_audio_embedding else "text_embedding"
    recs = _records(a.data, key)
    val = _records(a.valdata, "audio_embedding") if a.valdata else []
    scorer = CaptionScorer(pipe, T) if val else None
    os.makedirs(a.out_dir, exist_ok=True)
    json.dump(dict({k: v for k, v in vars(a).items() if k not in ("data", "valdata")}, **params),
              open(os.path.join(a.out_dir, "params.json"), "w"), indent=1)
    steps_per_epoch = -(-len(recs) // a.bs)
    total = steps_per_epoch * a.epochs
    gen = torch.Generator().manual_seed(a.seed)
    ids_dev = torch.zeros(a.bs, device=pipe.dev, dtype=torch.int32)
    best = math.inf
    for epoch in range(a.epochs):
        order = torch.randperm(len(recs), generator=gen).tolist()
        losses = []
        for c0 in range(0, len(order), a.bs):
            idx = order[c0:c0 + a.bs]
            emb = safeload.stack_rows([recs[i]["emb"] for i in idx]).to(pipe.dev)
            caps = [predict.reference_ids(tok, recs[i]["caption"], T) for i in idx]
            ids_dev[:len(idx)].copy_(torch.tensor(idx, dtype=torch.int32))
            lr = a.lr * linear_schedule(trainer.t, a.warmup, total)
            losses.append(trainer.step(emb, caps, lr=lr, row_ids=ids_dev[:len(idx)]))
        trainer.check()
        train_loss = float(torch.stack(losses).mean()) if losses else math.nan
        trainer.save(os.path.join(a.out_dir, "last.pth"))
        metric = _val_nll(pipe, scorer, tok, val, T) if val else train_loss
        print(json.dumps({"epoch": epoch, "train_loss": train_loss,
                          "val_nll" if val else "metric": metric, "steps": trainer.t}))
        if metric < best:
            best = metric
            trainer.save(os.path.join(a.out_dir, "best.pth"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
