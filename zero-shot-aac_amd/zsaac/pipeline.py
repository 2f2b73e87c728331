"""End-to-end batched caption pipeline (the hot path of BASELINE.json ``north_star``):

  wav [B, 320000] --zs_logmel(+bn0)--> HTSAT/CNN14 --audio_proj, L2--> CLAP emb [B,1024]
  --zs_prompt_assemble--> hard prompt ids --normalize_prefix--> mapper --prefill_embed-->
  GPT-2 prefill (KV cache) --get_prefix_tokens--> greedy (generate2) or beam (generate_beam)
  --> token ids [B, <=67] (+ lengths), all on one GPU, one stream.

What the reference does per clip in Python (predict_prompt.py:129-148 over the dataset of
dataset/dataset.py:441-453 fed by data_handing/embeddings_generator.py:44-73) is done here for a
batch of clips.  Multi-GPU sharding and the token-id all-gather live in zsaac/dist.py.
"""
from __future__ import annotations

import copy
import dataclasses
import os
import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .decoder import Gpt2Decoder, Gpt2Weights, MlpMapper, build_mapper
from .encoder import AudioEncoder


@dataclass
class CaptionConfig:
    encoder: str = "htsat"            # "htsat" | "cnn14"
    mapping_type: str = "mlp"         # "mlp" | "transformer"
    dtype: torch.dtype = torch.bfloat16
    batch: int = 64
    sound_effect_num: int = 3
    normalize_prefix: bool = True
    prefix_length: int = 10
    entry_length: int = 67
    beam: int = 0                     # 0 -> greedy generate2, else generate_beam(beam_size)
    prefix_tokens: bool = True        # also compute get_prefix_tokens (predict_prompt.py:137)
    use_graph: bool = True
    compact_decode: bool = True       # greedy bf16: decode only the rows that have not stopped
    clip_length: int = 10             # TransformerMapper clip_length (params.json prefix_length_clip)
    mapper_layers: int = 8            # TransformerMapper num_layers (params.json num_layers)
    persist_decode: Optional[bool] = None   # greedy bf16 at <= 64 rows: the persistent decode
                                      # launch (zs_gpt2_decode_persist); None = env ZSAAC_PERSIST (on)
    encoder_batch: int = 64           # clips per encoder pass (the reference's eval batch size);
                                      # a larger ``batch`` is encoded in chunks of this size and
                                      # decoded together (clip results do not depend on it)


@dataclass
class CaptionBatch:
    ids: torch.Tensor          # greedy: [B, steps] int32; beam: [B, beam, steps]
    lengths: torch.Tensor      # greedy: [B] int32; beam: [B, beam] f32 seq_len
    scores: Optional[torch.Tensor]
    hard_ids: torch.Tensor     # [B, h_cap] int32 (0-padded)
    hard_len: torch.Tensor     # [B]
    plen: torch.Tensor         # [B] prompt length H + 10
    prefix_ids: Optional[torch.Tensor]   # [B, Pmax] int32 get_prefix_tokens ids
    clap_emb: torch.Tensor     # [B, 1024]

    def captions(self) -> List[List[int]]:
        """Per clip: the reference's output token list (beam: best beam first)."""
        if self.scores is None:
            ids, ln = self.ids.cpu().numpy(), self.lengths.cpu().numpy()
            return [ids[b, :ln[b]].tolist() for b in range(ids.shape[0])]
        return [beams[0] for beams in self.beams()]

    def beams(self) -> List[List[List[int]]]:
        ids = self.ids.cpu().numpy()
        ln = self.lengths.cpu().numpy()
        sc = self.scores.cpu().numpy()
        out = []
        for c in range(ids.shape[0]):
            avg = sc[c] / ln[c]                       # scores / seq_lengths (line 153)
            order = np.argsort(-avg, kind="stable")   # scores.argsort(descending=True)
            out.append([ids[c, i, :int(ln[c, i])].tolist() for i in order])
        return out

    def prefix_token_lists(self) -> List[List[int]]:
        pid, pl = self.prefix_ids.cpu().numpy(), self.plen.cpu().numpy()
        return [pid[b, :pl[b]].tolist() for b in range(pid.shape[0])]


@dataclass
class SampleBatch:
    """CaptionPipeline.sample_emb's result: n sampled captions per clip."""
    ids: torch.Tensor          # [B, n, steps] int32
    lengths: torch.Tensor      # [B, n] int32
    logprobs: torch.Tensor     # [B, n, steps] f32: log softmax (temperature 1) of each token, 0 past the end
    hard_ids: torch.Tensor     # [B, h_cap] int32 (0-padded)
    hard_len: torch.Tensor     # [B]
    plen: torch.Tensor         # [B]
    clap_emb: torch.Tensor     # [B, 1024]
    prefix_ids: Optional[torch.Tensor] = None   # [B, Pmax] int32 get_prefix_tokens ids
    logits: Optional[torch.Tensor] = None    # keep_logits: [steps, B * n, V]

    def samples(self) -> List[List[List[int]]]:
        ids, ln = self.ids.cpu().numpy(), self.lengths.cpu().numpy()
        return [[ids[b, j, :ln[b, j]].tolist() for j in range(ids.shape[1])]
                for b in range(ids.shape[0])]

    def prefix_token_lists(self) -> List[List[int]]:
        pid, pl = self.prefix_ids.cpu().numpy(), self.plen.cpu().numpy()
        return [pid[b, :pl[b]].tolist() for b in range(pid.shape[0])]

    def sum_logprob(self) -> torch.Tensor:
        """[B, n]: log p(caption | clip), what CaptionScorer reports for the same ids."""
        return self.logprobs.sum(-1)

    def mean_logprob(self) -> torch.Tensor:
        return self.sum_logprob() / self.lengths.clamp(min=1)


# token ids prompt_kernel (csrc/gpt2.hip) writes around the labels: "There", " are",
# " something", ",", " in", " this", " audio", "."
PROMPT_TEMPLATE_IDS = (1858, 389, 1223, 11, 287, 428, 6597, 13)


class CaptionPipeline:
    """Weights from reference-keyed state dicts; all buffers sized for ``cfg.batch`` clips."""

    def __init__(self, caption_sd, audio_sd, label_table: torch.Tensor,
                 label_tokens: Sequence[Sequence[int]], cfg: CaptionConfig = CaptionConfig(),
                 device="cuda"):
        self.cfg = cfg
        dev = torch.device(device)
        self.dev = dev
        B = cfg.batch
        eb = min(B, max(1, cfg.encoder_batch))
        self.encoder = AudioEncoder(audio_sd, cfg.encoder, cfg.dtype, eb, dev) if audio_sd else None
        self.mapper = build_mapper(caption_sd, cfg.mapping_type, dev, cfg.dtype, B,
                                   clip_length=cfg.clip_length, num_layers=cfg.mapper_layers)
        self.gpt = Gpt2Weights(caption_sd, dev, cfg.dtype)
        self._setup_tables(label_table, label_tokens)
        self._alloc()
        # get_prefix_tokens on the soft rows only when every id a hard prompt can hold (the
        # template tokens of prompt_kernel, gpt2.hip, and the label table's tokens) is its own
        # cosine argmax by a margin above the dtype's rounding (bf16 2e-2, f32 1e-4)
        cand = list(PROMPT_TEMPLATE_IDS) + [t for toks in label_tokens for t in toks]
        margin = 2e-2 if cfg.dtype == torch.bfloat16 else 1e-4
        self.hard_skip = cfg.prefix_tokens and self.decoder.hard_rows_safe(cand, margin)

    def twin(self) -> "CaptionPipeline":
        """A pipeline sharing every packed weight with this one but owning its activation
        buffers, KV cache, skinny-GEMM workspace and decode graphs — so it can run a different
        batch concurrently on another HIP stream (ConcurrentRunner)."""
        t = copy.copy(self)
        t.encoder = self.encoder.twin() if self.encoder is not None else None
        t.mapper = self.mapper.twin()
        t._alloc()
        return t

    def group_twin(self, k: int) -> "CaptionPipeline":
        """A twin sized for k eval batches (k x cfg.batch clips) whose begin (encode, prompt,
        mapper, get_prefix_tokens, prefill) runs for all of them at once (begin_group); each
        batch then takes step 0 and its persistent decode on a sub-decoder of its own whose KV
        cache rows are this twin's (Gpt2Decoder.share_rows).  Greedy bf16 / f32 decoding with
        the MLP mapper only."""
        assert not self.cfg.beam and isinstance(self.mapper, MlpMapper)
        sb = self.cfg.batch
        t = copy.copy(self)
        t.cfg = dataclasses.replace(self.cfg, batch=k * sb, encoder_batch=k * sb)
        t.encoder = self.encoder.twin(max_batch=k * sb) if self.encoder is not None else None
        t.mapper = self.mapper.twin()        # (called per eval batch: sb rows)
        t._alloc()
        t.sub_batch = sb
        t.soft_buf = torch.empty(k * sb, self.mapper.soft_ld, device=self.dev)
        t.subs = []
        for j in range(k):
            d = Gpt2Decoder(self.gpt, sb, self.Pmax, self.cfg.entry_length, max_prefill_rows=1,
                            use_graph=self.cfg.use_graph, topk=8, compact=self.cfg.compact_decode,
                            persist=self.cfg.persist_decode, alloc_kv=False)
            d.share_rows(t.decoder, j * sb)
            t.subs.append(d)
        return t

    def begin_group(self, emb: torch.Tensor, sizes: Optional[Sequence[int]] = None):
        """The begins of the consecutive eval batches of ``emb`` [<= k x sub_batch, 1024] at once
        (``sizes``: the batches' clip counts, each <= sub_batch; default: sub_batch each, the last
        ragged)
        (group_twin): prompt assembly, L2 norm, the mapper (one launch pair per eval batch, as a
        batch's own begin runs it), prefill_embed, get_prefix_tokens and the prefill over every
        row, then step 0 of each batch on its sub-decoder, persistent launches deferred
        (sub-decoder.launch_pending).  Every kernel's per-row arithmetic is independent of the
        rows it runs with (the tiled GEMMs accumulate k in order whatever the tile), so each
        batch's ids equal its own begin's (tests/test_gpu_persist.py)."""
        cfg, B, Pmax, sb = self.cfg, emb.shape[0], self.Pmax, self.sub_batch
        assert B <= cfg.batch
        if sizes is None:
            sizes = [min(sb, B - r) for r in range(0, B, sb)]
        sizes = [int(z) for z in sizes]
        assert sum(sizes) == B and len(sizes) <= len(self.subs) and all(0 < z <= sb for z in sizes)
        self._B, self._emb, self._sizes = B, emb, sizes
        self._offs = [sum(sizes[:j]) for j in range(len(sizes))]
        ops.prompt_assemble(emb, self.labels, cfg.sound_effect_num, self.label_tok, self.label_len,
                            self.hard_ids[:B], self.hard_len[:B])
        prefix = self.prefix[:B]
        if cfg.normalize_prefix:
            ops.l2norm(emb, out=prefix)               # dataset.py:448-449
        else:
            prefix.copy_(emb)
        soft = self.soft_buf[:B]
        for c0, z in zip(self._offs, sizes):      # the mapper per eval batch, as its own begin
            soft[c0:c0 + z].copy_(self.mapper(prefix[c0:c0 + z]))
        dec = self.decoder
        ops.prefill_embed(self.hard_ids[:B], self.hard_len[:B], soft, self.mapper.soft_ld,
                          cfg.prefix_length, self.gpt.wte, self.gpt.wpe, B, Pmax,
                          self.embed[:B * Pmax], dec.x, dec.plen, dec.last_row)
        if cfg.prefix_tokens:
            self.prefix_tokens(B, soft)
        dec.prefill(B, Pmax)
        for j, (r0, r) in enumerate(zip(self._offs, sizes)):
            d = self.subs[j]
            if d.kc[0].data_ptr() != dec.kc[0][r0:].data_ptr():
                d.share_rows(dec, r0)           # (batch j's rows start at r0 this time)
            d.greedy_begin_device(r)
            d.defer_launch = True
            try:
                d.greedy_begin_host(r)
            finally:
                d.defer_launch = False

    def sub_result(self, j: int) -> CaptionBatch:
        """Batch j of the last begin_group's outputs (views, valid until the next begin_group)."""
        Pmax = self.Pmax
        r0, r = self._offs[j], self._sizes[j]
        d = self.subs[j]
        pid = (self.prefix_ids[r0 * Pmax:(r0 + r) * Pmax].view(r, Pmax)
               if self.cfg.prefix_tokens else None)
        return CaptionBatch(d.out_ids[:r], d.out_len[:r], None, self.hard_ids[r0:r0 + r],
                            self.hard_len[r0:r0 + r], d.plen[:r], pid, self._emb[r0:r0 + r])

    def _alloc(self):
        cfg, dev, B = self.cfg, self.dev, self.cfg.batch
        beam = max(cfg.beam, 1)
        # beam: per-block top-`beam` lists suffice for the global top-beam (fewer candidates to
        # sort in the LM head's epilogue and to merge in beam_step)
        self.decoder = Gpt2Decoder(self.gpt, B * beam, self.Pmax, cfg.entry_length,
                                   max_prefill_rows=B, use_graph=cfg.use_graph,
                                   topk=cfg.beam if cfg.beam else 8,
                                   compact=cfg.compact_decode, persist=cfg.persist_decode)
        i32 = dict(device=dev, dtype=torch.int32)
        self.hard_ids = torch.zeros(B, self.h_cap, **i32)
        self.hard_len = torch.zeros(B, **i32)
        self.prefix = torch.empty(B, 1024, device=dev)
        self.embed = torch.empty(B * self.Pmax, 768, device=dev)
        self.prefix_ids = torch.zeros(B * self.Pmax, **i32)
        self.emb_buf = torch.empty(B, 1024, device=dev)
        self._sample_decs: Dict[int, Gpt2Decoder] = {}    # sample_decoder's, by samples per clip

    def _setup_tables(self, label_table, label_tokens):
        cfg, dev = self.cfg, self.dev
        self.labels = label_table.to(device=dev, dtype=torch.float32).contiguous()
        mt = max(len(t) for t in label_tokens)
        lt = np.zeros((len(label_tokens), mt), dtype=np.int32)
        for i, t in enumerate(label_tokens):
            lt[i, :len(t)] = t
        self.label_tok = torch.from_numpy(lt).to(dev)
        self.label_len = torch.tensor([len(t) for t in label_tokens], dtype=torch.int32, device=dev)
        k = cfg.sound_effect_num
        # longest possible hard prompt: "There are" + k labels + (k-1) commas + " in this audio."
        self.h_cap = 2 + k * mt + max(k - 1, 0) + 4 if k > 0 else 7
        self.Pmax = self.h_cap + cfg.prefix_length

    def encode(self, wav: torch.Tensor) -> torch.Tensor:
        """CLAP embeddings [B, 1024] of a waveform batch, encoder_batch clips per pass."""
        assert self.encoder is not None, "no audio encoder weights"
        B, eb = wav.shape[0], self.encoder.B
        if B <= eb:
            return self.encoder.encode(wav)
        for c0 in range(0, B, eb):
            c1 = min(B, c0 + eb)
            self.emb_buf[c0:c1].copy_(self.encoder.encode(wav[c0:c1]))
        return self.emb_buf[:B]

    def caption_wav(self, wav: torch.Tensor) -> CaptionBatch:
        return self.caption_emb(self.encode(wav))

    def caption_emb(self, emb: torch.Tensor) -> CaptionBatch:
        """From CLAP audio embeddings [B, 1024] (the pickle's ``audio_embedding``)."""
        self.begin_emb(emb)
        self.decoder.run_to_completion()
        return self.result()

    # ------------------------------------------------------------------ async (no host sync)
    def begin_wav(self, wav: torch.Tensor):
        self.begin_emb(self.encode(wav))

    def result(self) -> CaptionBatch:
        """Views of the current batch's outputs (valid until the next begin_*)."""
        B, cfg, dec = self._B, self.cfg, self.decoder
        assert B is not None, "result(): no begin_emb since the last sample_emb"
        if cfg.beam:
            R = B * cfg.beam
            ids = dec.out_ids[:R].view(B, cfg.beam, -1)
            ln, sc = dec.seq_len[:R].view(B, cfg.beam), dec.scores[:R].view(B, cfg.beam)
        else:
            ids, ln, sc = dec.out_ids[:B], dec.out_len[:B], None
        pid = self.prefix_ids[:B * self.Pmax].view(B, self.Pmax) if cfg.prefix_tokens else None
        return CaptionBatch(ids, ln, sc, self.hard_ids[:B], self.hard_len[:B], dec.plen[:B], pid,
                            self._emb)

    def prefix_tokens(self, B: int, soft: torch.Tensor):
        """get_prefix_tokens ids of the current batch into prefix_ids (after prefill_embed)."""
        n, Pmax, dec = self.cfg.prefix_length, self.Pmax, self.decoder
        if (self.hard_skip and self.mapper.soft_ld == n * 768 and soft.is_contiguous()
                and soft.dtype == torch.float32):
            dec.prefix_tokens_soft(soft.reshape(-1)[:B * n * 768].view(B * n, 768),
                                   self.hard_ids[:B], self.hard_len[:B], B, Pmax,
                                   self.prefix_ids[:B * Pmax])
        else:
            dec.prefix_tokens(self.embed[:B * Pmax], self.prefix_ids[:B * Pmax])

    def begin_emb(self, emb: torch.Tensor):
        """Enqueue prompt assembly, mapper, prefill, get_prefix_tokens and decode step 0 for a
        batch of CLAP embeddings, without any host synchronisation."""
        cfg, B, Pmax = self.cfg, emb.shape[0], self.Pmax
        self._B, self._emb = B, emb
        dec = self.decoder
        self._prompt_stage(emb, dec)
        if cfg.beam:
            dec.prefill(B, Pmax, row_stride=cfg.beam)
            dec.beam_begin(B, cfg.beam)
        else:
            dec.prefill(B, Pmax)
            dec.greedy_begin(B)

    def _prompt_stage(self, emb: torch.Tensor, dec: Gpt2Decoder):
        """Prompt assembly, mapper, the prompt rows into ``dec.x`` (with dec.plen /
        dec.last_row) and get_prefix_tokens: the begin up to the prefill, for the decoder that
        will run it."""
        cfg, B, Pmax = self.cfg, emb.shape[0], self.Pmax
        assert B <= cfg.batch
        ops.prompt_assemble(emb, self.labels, cfg.sound_effect_num, self.label_tok, self.label_len,
                            self.hard_ids[:B], self.hard_len[:B])
        prefix = self.prefix[:B]
        if cfg.normalize_prefix:
            ops.l2norm(emb, out=prefix)               # dataset.py:448-449
        else:
            prefix.copy_(emb)
        soft = self.mapper(prefix)
        ops.prefill_embed(self.hard_ids[:B], self.hard_len[:B], soft, self.mapper.soft_ld,
                          cfg.prefix_length, self.gpt.wte, self.gpt.wpe, B, Pmax,
                          self.embed[:B * Pmax], dec.x, dec.plen, dec.last_row)
        if cfg.prefix_tokens:
            self.prefix_tokens(B, soft)

    # ------------------------------------------------------------------ sampling
    def sample_decoder(self, n: int) -> Gpt2Decoder:
        """The stepwise decoder of batch * n rows that sample_emb runs on (built on first use;
        the greedy / beam decoder, its graphs and the persistent grid are not involved)."""
        decs = self._sample_decs
        if n not in decs:
            cfg = self.cfg
            decs[n] = Gpt2Decoder(self.gpt, cfg.batch * n, self.Pmax, cfg.entry_length,
                                  max_prefill_rows=cfg.batch, use_graph=False, compact=False,
                                  persist=False, grid=False)
        return decs[n]

    def sample_emb(self, emb: torch.Tensor, n: int, temperature: float = 1.0, top_k: int = 0,
                   top_p: float = 1.0, seed: int = 0, clip_offset: int = 0,
                   keep_logits: bool = False) -> "SampleBatch":
        """n sampled captions per clip from CLAP audio embeddings [B, 1024]: the greedy begin
        (prompt, mapper, prefill), then Gpt2Decoder.sample, on the current stream.  Clip b draws
        with the ids (clip_offset + b) * n + j: give each batch of a dataset its first clip's
        index and a clip's captions do not depend on the batching."""
        cfg, B, Pmax, dec = self.cfg, emb.shape[0], self.Pmax, self.sample_decoder(n)
        # the prompt stage rewrites the buffers a pending begin_emb's result() views (hard_ids,
        # prefix_ids): that batch is over
        self._B = self._emb = None
        self._prompt_stage(emb, dec)
        dec.prefill(B, Pmax, row_stride=n)
        out = dec.sample(B, n, self.Pmax, temperature, top_k, top_p, seed, clip_offset, keep_logits)
        ids, ln, lp = out[:3]
        pid = self.prefix_ids[:B * Pmax].view(B, Pmax) if cfg.prefix_tokens else None
        return SampleBatch(ids.view(B, n, -1), ln.view(B, n), lp.reshape(B, n, -1), self.hard_ids[:B],
                           self.hard_len[:B], dec.plen[:B], emb, pid, out[3] if keep_logits else None)

    def sample_wav(self, wav: torch.Tensor, n: int, **kw) -> "SampleBatch":
        return self.sample_emb(self.encode(wav), n, **kw)


def persist_grids(env: Optional[str] = None) -> List[int]:
    """The persistent-decode grid sizes (workgroups of 256 threads, ops.PERSIST_GRIDS) a runner
    may use, largest first: ``env`` or ZSAAC_PERSIST_GRIDS ("192,96,48"); with ``env`` None and
    ZSAAC_PERSIST_GRID set, that one size alone.  Every size gives the same ids (decode_grid.hip's
    canonical arithmetic), so the choice is a scheduling decision only."""
    if env is None:
        env = (os.environ["ZSAAC_PERSIST_GRID"] if "ZSAAC_PERSIST_GRID" in os.environ
               else os.environ.get("ZSAAC_PERSIST_GRIDS", DEFAULT_PERSIST_GRIDS))
    grids = sorted({int(t) for t in env.replace(" ", "").split(",") if t}, reverse=True)
    for g in grids:
        assert g in ops.PERSIST_GRIDS, f"persist grid {g} (one of {ops.PERSIST_GRIDS})"
    return grids


# largest first; the last is the throughput grid every batch can fall back to (192 stays
# available: alone it has the shortest step, but beside other grids 96 wins -- a 131-clip shard
# 3.47k vs 2.42k clips/s, the headline equal)
DEFAULT_PERSIST_GRIDS = "96,48"


def persist_budget(cus: int, staged: bool = False) -> int:
    """Workgroup slots the in-flight persistent grids may hold together: a grid workgroup takes
    half a CU (4 waves x <= 256 registers), so 2 x CUs is the chip.  The pipelined schedule's
    default, 1.5 x CUs (8 grids of 48), leaves a quarter of the slots to the begins' kernels:
    measured in one process (tools/headline_ab.py, 12 reps, encode-ahead 256, grids sized at
    launch): 5.73k clips/s against 5.33k at 2 x CUs and 4.71k at 1 x CUs.  ``staged``
    (begin_first: the begins have run before the grids) 2 x CUs less a sixteenth, ten grids of 48
    on 256 CUs (profiles/r6/begin_first_ab.txt: 448 / 480 / 512 slots 7.03k / 7.02k / 7.11k on
    the 1045-clip set, 480 / 512 6.96k / 6.81k on 1280 clips).  ZSAAC_PERSIST_BUDGET overrides."""
    dflt = 2 * cus - cus // 8 if staged else 3 * cus // 2
    return int(os.environ.get("ZSAAC_PERSIST_BUDGET", str(dflt)))


def choose_persist_grid(in_flight: int, to_begin: int, grids: List[int], budget: int) -> int:
    """Grid size of the persistent decode launch of the next batch to begin, given the workgroups
    of the grids already in flight and the batches still to begin (this one included): the
    largest grid that, beside the grids in flight and every other batch still to begin at the
    smallest size, fits the budget.  Then every later begin still has room for the smallest grid,
    so (with at most budget // smallest batches in flight) the grids in flight never exceed the
    budget and every persistent launch can be co-resident."""
    g_min = grids[-1]
    for g in grids:
        if in_flight + g + g_min * (to_begin - 1) <= budget:
            return g
    return g_min


_SPLIT_STREAMS = {}     # (device, CUs, begin CUs) -> (begin streams, grid streams)
# a staged run that sees no event complete for this long raises (with its state) instead of
# spinning: a persistent launch that cannot become co-resident gives up after ~2^22 polls (s)
STALL_S = float(os.environ.get("ZSAAC_RUNNER_STALL_S", "60"))
# the first wave of a staged run's grids, released by one gate, start STAGGER_US apart (each
# waits k x STAGGER_US after the gate on the GPU, zs_stream_spin): released together, one grid of
# ten sometimes found no room for all its workgroups until another ended -- a 1280-clip
# repetition 0.16 or 0.18 s at random; staggered by 300 us every repetition took 0.162-0.164 s
# (profiles/r6/begin_first_ab.txt, r6u; 100 us: 2 late grids in 8 repetitions; with begin groups
# of 2, 150 / 200 / 300 us: none in 8 each, 8.01k / 7.99k / 7.97k clips/s, r6ee)
STAGGER_US = int(os.environ.get("ZSAAC_STAGGER_US", "200"))


class SlotAccount:
    """What a run's persistent grids hold of the chip (host bookkeeping only): the workgroup
    slots of the grids in flight against ``budget``, which of the ``pool`` streams has a grid
    running on it, and -- the small-run path -- the workgroups launched exclusive (one CU each)
    against ``excl_cap`` CUs."""

    def __init__(self, grids: List[int], budget: int, pool: int, excl_cap: int = 0):
        self.grids, self.budget, self.pool, self.excl_cap = list(grids), budget, pool, excl_cap
        self.used = self.excl = 0
        self.busy = set()

    def admit(self, unlaunched: int) -> Optional[Tuple[int, int]]:
        """Takes room for the next batch's grid, ``unlaunched`` batches (it included) still to
        launch: (its size by choose_persist_grid, the index of a stream no grid is running on),
        or None while every stream is busy or that grid does not fit the budget."""
        if len(self.busy) >= self.pool:
            return None
        g = choose_persist_grid(self.used, unlaunched, self.grids, self.budget)
        if self.used + g > self.budget:
            return None
        k = next(k for k in range(self.pool) if k not in self.busy)
        self.used += g
        self.busy.add(k)
        return g, k

    def exclusive(self, g: int) -> bool:
        """Whether the grid just admitted takes one CU per workgroup (counted if so): while the
        exclusive workgroups in flight leave it the CUs (it shares CUs with normal grids only)."""
        if self.excl + g > self.excl_cap:
            return False
        self.excl += g
        return True

    def release(self, grid: int = 0, excl: int = 0, stream: Optional[int] = None):
        self.used -= grid
        self.excl -= excl
        self.busy.discard(stream)


@dataclass(eq=False)
class _InFlight:
    """A batch between its begin and its result copy (compared by identity)."""
    dec: Gpt2Decoder                  # decodes it: a pipeline's decoder or a group twin's sub-decoder
    result: Callable[[], CaptionBatch]    # views of its outputs
    batch: int
    owner: int                        # its pipeline's / group's index, as ``assign`` reports it
    stream: Optional[torch.cuda.Stream] = None    # its decode chunks and result copy run here
    begun: Optional[torch.cuda.Event] = None      # its begin's end (persistent launch deferred)
    k: Optional[int] = None           # the stream index the slot account gave its launch
    grid: int = 0                     # workgroups its launch holds (0: none, or it gave up)
    excl: int = 0                     # of those, exclusive ones
    join: Optional[torch.cuda.Stream] = None      # the launch's stream while ``stream`` has not joined it
    chunks: int = 0                   # decode chunks enqueued after the launch
    ev: Optional[torch.cuda.Event] = None         # finished_async's of the last enqueue: the event
    flag: Optional[torch.Tensor] = None           # and the pinned flags valid after it
    done: bool = False


class ConcurrentRunner:
    """Keeps several independent bs=`cfg.batch` batches in flight on one GPU; the host only
    polls events and a pinned all-done flag (no blocking syncs).  Three schedules, each a short
    driver (when begins are enqueued, which stream a grid takes, gating) around one launch
    (_launch), one poll (_poll), one slot account (SlotAccount) and one idle / watchdog / trace
    helper (_idle, _note):

    * pipelined (run): pipeline twins (shared weights, private buffers / KV cache / graphs),
      each on its own HIP stream; a batch's begin (encode .. step 0) is enqueued when a pipeline
      frees, its persistent decode grid when the begin has finished -- begins and grids share
      the chip.  Also the path of a run with no more batches than grids fit at once.
    * staged (begin_first; _run_staged): a begin on every free pipeline first, the decode grids
      launched in batch order as the budget frees, on a pool of budget / 48 streams, the first
      wave after the gating begins and released STAGGER_US apart.
    * grouped (begin_first with begin_group k, the bench's headline schedule; _run_grouped):
      staged with one begin per k consecutive batches on a group twin, each batch decoding on a
      sub-decoder that shares the twin's KV cache rows.

    Ids are the same under every schedule (tests/test_gpu_persist.py).  Results are copied out
    on the batch's stream before its pipeline takes the next batch."""

    def __init__(self, pipe: CaptionPipeline, n_inflight: int = 2, streams: Optional[list] = None,
                 grids: Optional[List[int]] = None, budget: Optional[int] = None,
                 encode_ahead: int = 0, begin_first: bool = False,
                 extra_pipes: int = 0, enc_stream=None, cu_split: int = 0,
                 begin_gate: int = 0, begin_group: int = 0, n_batches: int = 0):
        self.cus = torch.cuda.get_device_properties(pipe.dev).multi_processor_count
        # persistent grids (greedy bf16 at <= 64 rows; beam search never launches one), one size
        # per batch from `grids` (largest first, see choose_persist_grid)
        self.persist = pipe.decoder.persist and not pipe.cfg.beam
        self.grids = grids or (list(ops.PERSIST_GRIDS_F32) if getattr(pipe.decoder, "f32_grid", False)
                               else persist_grids())
        self.budget = budget or persist_budget(self.cus)
        # begin_first (persistent decode only): every pipeline begins its batch (prompt .. step 0)
        # at once, and the persistent launches follow as the budget frees, the first ones after
        # every first-round begin -- the begins run on the whole chip instead of beside the grids
        self.begin_first = bool(begin_first) and self.persist
        # begin_first: the first persistent launches wait for the first `begin_gate` begins (0:
        # every begin of the first round), so those begins run beside no decode grid
        self.begin_gate = int(begin_gate)
        # begin_group k > 0 (begin_first, greedy, MLP mapper): the begins of k consecutive eval
        # batches run as ONE begin of k x batch clips on a group twin (CaptionPipeline.group_twin:
        # encoder pass, prefill and get_prefix_tokens at k x the rows), each batch then decodes
        # on a sub-decoder sharing the twin's KV cache rows; n_batches sizes the group twins
        # warmup() prepares
        self.begin_group = (int(begin_group) if self.begin_first and not pipe.cfg.beam
                            and isinstance(pipe.mapper, MlpMapper) else 0)
        self.n_batches = int(n_batches)
        self.gpipes: List[CaptionPipeline] = []
        if self.persist and (not self.begin_first or self.begin_group):
            # persistent decode grids must be co-resident: at most budget // (smallest grid)
            n_inflight = max(1, min(n_inflight, self.budget // self.grids[-1]))
        self.n_inflight = n_inflight
        # extra_pipes: pipelines beyond the grids the budget holds, so the next batches' begins
        # (prefill etc.) run while every grid slot decodes and launch the moment one frees
        n_pipes = n_inflight + (max(0, int(extra_pipes)) if self.persist else 0)
        self.pipes = [pipe] + [pipe.twin() for _ in range(n_pipes - 1)]
        # encode_ahead > 0 (waveform inputs): one encoder twin sized for that many clips encodes
        # every batch's clips up front, in passes of up to encode_ahead clips (consecutive
        # batches), on a stream of its own; a batch's begin (mapper .. step 0) waits only for its
        # own pass.  The encoder then runs at its most efficient size and before the decode grids
        # fill the chip; captions do not depend on it (a clip's embedding is its own).
        self.encode_ahead = int(encode_ahead) if pipe.encoder is not None else 0
        self.enc = pipe.encoder.twin(max_batch=self.encode_ahead) if self.encode_ahead else None
        # dedicated streams on distinct hardware queues: pooled torch streams take their queue at
        # first use and can end up sharing one, which serializes the batches
        # (``streams``: reuse another runner's, at least as many -- tools/headline_ab.py)
        need = len(self.pipes)
        if self.begin_first:
            # begin_first keeps a pipeline per batch but only as many streams as grids can run at
            # once: every stream is a hardware queue, and a process holding more queues than the
            # scheduler maps at once gets its queues time-sliced (a stream per pipeline, 20 at
            # 1280 clips, slowed every later multi-stream run 5-27 %; a pool of 12 still cost C3
            # 9 % and C5's step 2.7 -> 3.8 ms, a pool of 10 nothing: profiles/r6/begin_first_ab.txt)
            cap = self.budget // self.grids[-1]
            need = cap if self.begin_group else min(need, cap)
        # cu_split > 0 (persistent decode, A/B option): the chip is split by CU masks -- the
        # pipelines' begins (prompt .. step 0, and a give-up's phase launches) on cu_split CUs,
        # the decode grids on the rest (each pipeline launches its grid on a second stream of
        # its own); the budget then holds the grids to two workgroups per grid CU
        self.cu_split = int(cu_split) if self.persist else 0
        self.gstreams = None
        if self.cu_split:
            key = (str(pipe.dev), self.cus, self.cu_split)
            have = _SPLIT_STREAMS.setdefault(key, ([], []))   # reused by later runners
            bmask, gmask = ops.cu_split_masks(self.cus, self.cu_split)
            if len(have[0]) < need:
                have[0].extend(ops.masked_streams(need - len(have[0]), pipe.dev, bmask))
                have[1].extend(ops.masked_streams(need - len(have[1]), pipe.dev, gmask))
            streams, self.gstreams = have[0][:need], have[1][:need]
            self.budget = min(self.budget, 2 * (self.cus - self.cu_split))
        streams = (list(streams[:need]) if streams is not None
                   else ops.dedicated_streams(need, pipe.dev, priority=-1))
        assert len(streams) == need, "ConcurrentRunner: too few streams given"
        self.streams = streams
        # the encoder running ahead yields to the begins and grids: a low-priority stream
        self.enc_stream = None
        if self.enc is not None:
            self.enc_stream = (enc_stream if enc_stream is not None
                               else ops.dedicated_streams(1, pipe.dev, priority=1)[0])

    def warmup(self, wav: torch.Tensor):
        """Runs one batch per pipeline (and per group twin) synchronously: captures every decode
        graph."""
        self._warm(wav, "wav")

    def warmup_emb(self, emb: torch.Tensor):
        self._warm(emb, "emb")

    def _warm(self, x: torch.Tensor, inputs: str):
        for i, p in enumerate(self.pipes):
            s = self.streams[i % len(self.streams)]
            s.wait_stream(torch.cuda.current_stream(p.dev))
            with torch.cuda.stream(s):
                (p.caption_wav if inputs == "wav" else p.caption_emb)(x)
                p.decoder.capture_buckets()
            s.synchronize()
        self._warm_groups(x, inputs)

    def decoders(self) -> List[Gpt2Decoder]:
        """Every decoder this runner steps: the pipelines' and the group twins' sub-decoders."""
        return [p.decoder for p in self.pipes] + [d for G in self.gpipes for d in G.subs]

    def _warm_groups(self, x: torch.Tensor, inputs: str):
        """begin_group: the group twins a run of n_batches needs, each run once (a full group of
        x's rows repeated) with its sub-decoders' persistent launches, synchronously."""
        k = self.begin_group
        if not k or not self.n_batches:
            return
        need = -(-self.n_batches // k)
        while len(self.gpipes) < need:
            self.gpipes.append(self.pipes[0].group_twin(k))
        sb = self.pipes[0].cfg.batch
        xs = x.repeat((-(-k * sb // x.shape[0]),) + (1,) * (x.dim() - 1))[:k * sb].contiguous()
        s = self.streams[0]
        s.wait_stream(torch.cuda.current_stream(self.pipes[0].dev))
        for G in self.gpipes:
            with torch.cuda.stream(s):
                G.begin_group(G.encode(xs) if inputs == "wav" else xs)
                for d in G.subs:
                    d.persist_grid = self.grids[-1]
                    d.persist_exclusive = False
                    d.launch_pending()
                    d.run_to_completion()
            s.synchronize()

    # ------------------------------------------------------------------ shared by the schedules
    def _start(self, n: int, keep, caller, slots: SlotAccount, schedule: str):
        """A run's bookkeeping, reset."""
        self.decode_steps = [0] * n      # per batch: decode steps actually enqueued
        self.assign = []                 # (pipeline / group index, batch index), in begin / launch order
        self.grid = [0] * n              # persistent grid size per batch (0: none)
        self.gave_up = 0                 # launches of this run that resumed stepwise
        self.trace = [] if os.environ.get("ZSAAC_RUNNER_TRACE") else None   # (kind, index, ms)
        self._results: List[Optional[CaptionBatch]] = [None] * n
        self._keep, self._caller, self._slots, self._schedule = keep, caller, slots, schedule
        self._t_run = self._t_prog = time.perf_counter()

    def _finish(self, streams, ahead=None) -> List[CaptionBatch]:
        """The end of a run: the caller's stream, which consumes the results, joins ``streams``."""
        for s in streams:
            self._caller.wait_stream(s)
        if ahead is not None:
            self._caller.wait_stream(self.enc_stream)
        results, self._results, self._keep = self._results, None, None
        return results

    def _note(self, kind: str, index: int):
        if self.trace is not None:
            self.trace.append((kind, index, round((time.perf_counter() - self._t_run) * 1e3, 2)))

    def _idle(self, progressed: bool, waiting, active):
        """The end of a driver's pass: after one that moved nothing, a short sleep, and a
        RuntimeError (with the run's state) once nothing has moved for STALL_S."""
        if progressed:
            self._t_prog = time.perf_counter()
            return
        time.sleep(20e-6)
        if time.perf_counter() - self._t_prog > STALL_S:
            sl = self._slots
            raise RuntimeError(
                f"ConcurrentRunner ({self._schedule}): no progress for {STALL_S} s; waiting "
                f"(batch, owner) {[(r.batch, r.owner) for r in waiting][:8]}, in flight (batch, "
                f"owner, chunks, stream, grid; no stream: begun, not launched) "
                f"{[(r.batch, r.owner, r.chunks, r.k, r.grid) for r in active]}, "
                f"{sl.used} of {sl.budget} slots, streams busy {sorted(sl.busy)} of {sl.pool}")

    def _begin(self, i, bi, batches, inputs, ahead, after=None):
        """Batch bi's begin on pipeline i's stream (``after``: an event it waits for first),
        enqueued kernel by kernel: replayed from a hipGraph per pipeline the headline measured
        5.75k vs 5.86k and 5.09k vs 5.30k clips/s (same box, medians of 5) -- the idle time
        between a begin's kernels beside the grids is waiting for CU resources, not host enqueue."""
        p, s = self.pipes[i], self.streams[i % len(self.streams)]
        with torch.cuda.stream(s):
            if after is not None:
                s.wait_event(after)
            if ahead is not None:
                s.wait_event(ahead.ready(bi))
                p.begin_emb(ahead.embs[bi])
            elif inputs == "wav":
                p.begin_emb(p.encode(batches[bi]))
            else:
                p.begin_emb(batches[bi])

    def _launch(self, r: _InFlight, g: int, s, waits=(), rank: Optional[int] = None,
                exclusive: bool = False):
        """Enqueues r's persistent launch, a grid of g workgroups, on stream s after the events
        ``waits``, held back rank x STAGGER_US (rank None: a launch outside the first wave)."""
        d = r.dec
        d.persist_grid, d.persist_exclusive = g, exclusive     # (never a value left over)
        r.grid, r.excl = g, g if exclusive else 0
        self.grid[r.batch] = g
        with torch.cuda.stream(s):
            for ev in waits:
                s.wait_event(ev)
            if rank is not None and STAGGER_US:
                ops.stream_spin(STAGGER_US * rank, s)
            d.launch_pending()
            r.ev, r.flag = d.finished_async()
        r.join = s if s is not r.stream else None
        self._note("launch", r.batch)

    def _launch_waiting(self, waiting: List[_InFlight], later: int, gate) -> List[_InFlight]:
        """The staged schedules' launches: the waiting batches in order while the slot account
        admits them (``later``: batches not begun yet), each on a stream no grid is running on,
        after its own begin and -- the first wave -- the gating begins' events, released in turn."""
        out = []
        while waiting:
            got = self._slots.admit(len(waiting) + later)
            if got is None:
                break
            r = waiting.pop(0)
            g, r.k = got
            r.stream = self.streams[r.k]
            self._launch(r, g, r.stream, [r.begun, *gate],
                         len(self._slots.busy) - 1 if gate else None)
            out.append(r)
        return out

    def _poll(self, r: _InFlight) -> bool:
        """Moves a launched batch on if its last enqueue has finished (else False): a launch that
        gave up resumes on the phase launches, a finished batch is copied out (r.done), any other
        takes its next chunk."""
        if not r.ev.query():
            return False
        d, s, flag = r.dec, r.stream, r.flag
        if r.join is not None:
            s.wait_stream(r.join)            # (cu_split: the grid ran on a stream of its own)
            r.join = None
        if int(flag[1]) < 0:
            # the persistent launch gave up waiting (its grid was not co-resident): finish this
            # batch on the per-step path from the state it started from
            self.gave_up += 1
            with torch.cuda.stream(s):
                d.resume_stepwise()
                d.step_chunk(None)
                r.ev, r.flag = d.finished_async()
            self._slots.release(r.grid, r.excl)
            r.grid = r.excl = 0
            r.chunks = 1
        elif int(flag[0]) or r.chunks >= d.n_chunks:
            d.note_persist_steps(int(flag[3]))
            self.decode_steps[r.batch] = (int(flag[3]) if not self.pipes[0].cfg.beam
                                          else 1 + r.chunks * d.chunk)
            self._note("done", r.batch)
            with torch.cuda.stream(s):
                out = self._results[r.batch] = _copy_batch(r.result(), self._caller)
                if self._keep is not None:
                    self._keep(out)
            self._slots.release(r.grid, r.excl, r.k)
            r.done = True
        else:
            with torch.cuda.stream(s):
                d.step_chunk(int(flag[2]))
                r.ev, r.flag = d.finished_async()
            r.chunks += 1
        return True

    # ------------------------------------------------------------------ the schedules
    def run(self, batches: Sequence[torch.Tensor], keep=None, inputs: str = "wav") -> List[CaptionBatch]:
        """Captions every batch (waveforms [B, n] or, with inputs="emb", CLAP embeddings
        [B, 1024]; B <= cfg.batch, ragged last batch allowed); returns CaptionBatch copies in
        input order.  ``keep`` optionally post-processes a result on its pipeline's stream; the
        completion order is timing-dependent, so it must not issue collectives (gather after
        run() instead, in input order — see bench.py)."""
        assert inputs in ("wav", "emb")
        self.bdec = None                 # (_run_grouped: batch -> the sub-decoder that decoded it)
        n = len(batches)
        caller = torch.cuda.current_stream(self.pipes[0].dev)
        for s in self.streams:           # inputs were produced on the caller's stream
            s.wait_stream(caller)
        staged = self.begin_first and n > self.budget // self.grids[-1]
        ahead = None
        if inputs == "wav" and self.enc is not None and not staged and n > len(self.pipes):
            # (a pipelined run that fits its pipelines at once begins sooner encoding per batch:
            # measured on a 131-clip shard, 37.5 vs 40 ms.  A staged run encodes on its begins'
            # streams: with the encoder's passes on their low-priority stream every repetition
            # took 2-32 s instead of 0.15 s -- profiles/r6/begin_first_ab.txt, r6i)
            ahead = _EncodeAhead(self, batches, caller)
        if staged and self.begin_group:
            return self._run_grouped(batches, keep, inputs, caller)
        if staged:
            # (more batches than grids the budget holds at once; fewer take the pipelined path
            # below, whose small-run form gives each batch an exclusive grid)
            return self._run_staged(batches, keep, inputs, caller, ahead)
        # a run that fits its pipelines at once (a small shard) has no later begins to leave room
        # for: its grids may fill the chip, and they take one CU per workgroup (exclusive
        # launches) while the CUs allow -- left to itself the dispatcher doubles workgroups up on
        # CUs while others idle (tools/placement.py: 3 grids of 96 covered 185 CUs, 103 twice)
        small = self.persist and n <= len(self.pipes)
        # (a pipeline decodes on its own stream: the account's stream index only counts it)
        slots = SlotAccount(self.grids, 2 * self.cus if small else self.budget, len(self.pipes),
                            excl_cap=self.cus if small else 0)
        self._start(n, keep, caller, slots, "pipelined")
        active = {}                      # pipeline index -> its batch
        nxt = 0
        while nxt < n or active:
            progressed = False
            if ahead is not None:
                ahead.pump()
            for i, (p, s) in enumerate(zip(self.pipes, self.streams)):
                r = active.get(i)
                if r is None:
                    if nxt == n:
                        continue
                    # persistent decode: the begin is enqueued now, the grid launch when the
                    # begin has finished (its size chosen then, from the grids in flight and
                    # the batches not yet launched: bigger grids once few batches remain; sized
                    # at the begin the headline ran 5.61k against 5.73k clips/s, budget 384,
                    # medians of 12: profiles/r5/headline_ab_budget_late.txt)
                    r = active[i] = _InFlight(p.decoder, p.result, nxt, i, s)
                    p.decoder.defer_launch = self.persist
                    try:
                        self._begin(i, nxt, batches, inputs, ahead)
                    finally:
                        p.decoder.defer_launch = False
                    if self.persist:
                        r.begun = torch.cuda.Event()
                        r.begun.record(s)
                    else:
                        with torch.cuda.stream(s):
                            r.ev, r.flag = p.decoder.finished_async()
                    self.assign.append((i, nxt))
                    self._note("begin", nxt)
                    nxt += 1
                    progressed = True
                    # one begin per pass over the pipelines, launches and completions before the
                    # next: a begin costs milliseconds of host enqueue, so beginning every idle
                    # pipeline in one pass delayed the first grids' launches until the last begin
                    # was enqueued (~43 ms into the headline, tools/timeline.py; the A/B
                    # among profiles/r5/headline_ab_*.txt)
                    break
                if r.ev is None:         # begun, its grid not launched yet
                    if not r.begun.query():
                        continue
                    got = slots.admit(n - nxt + sum(1 for a in active.values() if a.ev is None))
                    if got is None:
                        continue         # (extra pipelines: wait for a grid to finish)
                    g, r.k = got
                    gs = self.gstreams[i] if self.gstreams else s
                    if gs is not s:
                        gs.wait_stream(s)
                    self._launch(r, g, gs, exclusive=small and slots.exclusive(g))
                    progressed = True
                elif self._poll(r):
                    progressed = True
                    if r.done:
                        del active[i]
            self._idle(progressed, (), active.values())
        return self._finish(self.streams + (self.gstreams or []), ahead)

    def _run_staged(self, batches, keep, inputs, caller, ahead):
        """run() with begin_first: a begin on every free pipeline (persistent launches deferred),
        one begin per pass over the loop so finished batches and launches are handled between
        begins; launches in batch order while the grids in flight fit the budget, each on a
        stream no grid is running on, after its own begin and -- the first ones -- after the
        first `begin_gate` begins (0: every begin of the first round) have finished on the GPU.
        With a pipeline per batch every begin runs before (or beside few) decode grids and every
        later launch finds its batch begun.  With fewer, a pipeline's next begin waits for its
        last batch's result copy (which ran on the grid's stream, not the pipeline's)."""
        n, S = len(batches), len(self.streams)
        self._start(n, keep, caller, SlotAccount(self.grids, self.budget, S), "begin_first")
        free = list(range(len(self.pipes)))
        n_gate = min(n, len(free)) if self.begin_gate <= 0 else min(n, self.begin_gate)
        waiting, active, gate = [], [], []
        copied = {}                      # pipeline index -> the event after its last result copy
        nxt = 0
        while nxt < n or waiting or active:
            progressed = False
            if ahead is not None:
                ahead.pump()
            if nxt < n and free:
                i = free.pop(0)
                p = self.pipes[i]
                p.decoder.defer_launch = True
                try:
                    self._begin(i, nxt, batches, inputs, ahead, after=copied.pop(i, None))
                finally:
                    p.decoder.defer_launch = False
                r = _InFlight(p.decoder, p.result, nxt, i, begun=torch.cuda.Event())
                r.begun.record(self.streams[i % S])
                if len(gate) < n_gate:
                    gate.append(r.begun)
                waiting.append(r)
                self.assign.append((i, nxt))
                self._note("begin", nxt)
                nxt += 1
                progressed = True
            if len(gate) >= n_gate:
                launched = self._launch_waiting(waiting, n - nxt, gate)
                active += launched
                progressed = progressed or bool(launched)
                if active:
                    gate, n_gate = [], 0     # (launches after the first ones: no gate)
            for r in list(active):
                if not self._poll(r):
                    continue
                progressed = True
                if r.done:
                    active.remove(r)
                    free.append(r.owner)
                    if n > len(self.pipes):      # (pipelines take further batches)
                        copied[r.owner] = torch.cuda.Event()
                        copied[r.owner].record(r.stream)
            self._idle(progressed, waiting, active)
        return self._finish(self.streams, ahead)

    def _run_grouped(self, batches, keep, inputs, caller):
        """run() with begin_first and begin_group k: one begin per group of k consecutive eval
        batches (CaptionPipeline.begin_group on a group twin: the encoder pass, prefill and
        get_prefix_tokens at k x the rows), the groups' begins spread over the streams and all
        enqueued first; the decode grids then launch in batch order within the budget, each on
        a stream no grid is running on, after its group's begin -- the first ones after every
        group's begin has finished on the GPU."""
        n, k, S = len(batches), self.begin_group, len(self.streams)
        groups = [list(range(g, min(n, g + k))) for g in range(0, n, k)]
        while len(self.gpipes) < len(groups):
            self.gpipes.append(self.pipes[0].group_twin(k))
        self._start(n, keep, caller, SlotAccount(self.grids, self.budget, S), "begin_group")
        if self.trace is not None:       # (every run's: tools/sched_trace.py)
            self.traces = getattr(self, "traces", []) + [self.trace]
        gate = []           # every group's begin (gating on fewer brought the late grid back: r6w)
        for gi, bl in enumerate(groups):      # (on one stream: 5.3k instead of 7.3k clips/s)
            G, s = self.gpipes[gi], self.streams[gi % S]
            with torch.cuda.stream(s):
                x = _rows_span([batches[b] for b in bl])
                G.begin_group(G.encode(x) if inputs == "wav" else x,
                              [int(batches[b].shape[0]) for b in bl])
                ev = torch.cuda.Event()
                ev.record(s)
            gate.append(ev)
            self._note("begin_group", gi)
        waiting = [_InFlight(G.subs[j], lambda G=G, j=j: G.sub_result(j), b, gi, begun=gate[gi])
                   for gi, (G, bl) in enumerate(zip(self.gpipes, groups)) for j, b in enumerate(bl)]
        self.bdec = {r.batch: r.dec for r in waiting}
        active = []
        while waiting or active:
            launched = self._launch_waiting(waiting, 0, gate)
            self.assign += [(r.owner, r.batch) for r in launched]
            active += launched
            progressed = bool(launched)
            if active:
                gate = []
            for r in list(active):
                if self._poll(r):
                    progressed = True
                    if r.done:
                        active.remove(r)
            self._idle(progressed, waiting, active)
        return self._finish(self.streams)


class _EncodeAhead:
    """The encoder passes of every batch on the runner's encoder stream: consecutive batches
    grouped up to encode_ahead clips (one view when they are adjacent rows of one tensor, as the
    bench's are, else concatenated), enqueued one pass at a time (pump): a pass queued far ahead
    would hold the GPU ahead of the begins issued after it."""

    def __init__(self, runner, batches, caller):
        E = runner.encode_ahead
        self.enc, self.es, self.batches = runner.enc, runner.enc_stream, batches
        n = sum(int(b.shape[0]) for b in batches)
        self.emb = torch.empty(n, 1024, device=runner.pipes[0].dev)
        self.es.wait_stream(caller)
        self.passes, self.pass_of, self.embs = [], [], []
        i, c0 = 0, 0
        while i < len(batches):
            j, m = i, 0
            while j < len(batches) and m + int(batches[j].shape[0]) <= E:
                m += int(batches[j].shape[0])
                j += 1
            assert j > i, f"a batch of {batches[i].shape[0]} clips > encode_ahead {E}"
            self.passes.append((i, j, c0, m))
            for b in batches[i:j]:
                self.pass_of.append(len(self.passes) - 1)
                self.embs.append(self.emb[c0:c0 + int(b.shape[0])])
                c0 += int(b.shape[0])
            i = j
        self.events = []
        self.pump(force=1)

    def pump(self, force=0):
        """Enqueues the next pass when none is in flight (or until `force` passes are)."""
        while len(self.events) < len(self.passes):
            if len(self.events) >= force and self.events and not self.events[-1].query():
                return
            i, j, c0, m = self.passes[len(self.events)]
            with torch.cuda.stream(self.es):
                # (replayed from per-size hipGraphs, Encoder.encode_graphed: within the noise
                # of kernel-by-kernel enqueue, the A/B among profiles/r5/headline_ab_*.txt)
                self.emb[c0:c0 + m].copy_(self.enc.encode_graphed(_rows_span(self.batches[i:j])))
                ev = torch.cuda.Event()
                ev.record(self.es)
            self.events.append(ev)

    def ready(self, b):
        """The event batch b's begin waits for (its pass enqueued first if needed)."""
        k = self.pass_of[b]
        self.pump(force=k + 1)
        return self.events[k]


def _rows_span(ts: Sequence[torch.Tensor]) -> torch.Tensor:
    """The row-wise concatenation of 2-D tensors: a view when they are adjacent row ranges of one
    contiguous tensor, else a copy."""
    if len(ts) == 1:
        return ts[0]
    t0 = ts[0]
    adjacent = all(t.is_contiguous() and t.dtype == t0.dtype and t.shape[1:] == t0.shape[1:]
                   for t in ts)
    ptr = t0.data_ptr()
    for t in ts:
        adjacent = adjacent and t.data_ptr() == ptr
        ptr += t.numel() * t.element_size()
    if adjacent:
        rows = sum(int(t.shape[0]) for t in ts)
        return t0.as_strided((rows,) + tuple(t0.shape[1:]), t0.stride())
    return torch.cat(list(ts))


def _copy_batch(r: CaptionBatch, consumer=None) -> CaptionBatch:
    """Clones of a result, made on the current (pipeline) stream; ``consumer`` is the stream
    that will read and free them, recorded so the caching allocator does not recycle the blocks
    for the pipeline stream while consumer-stream kernels may still read them."""
    def c(t):
        if t is None:
            return None
        t = t.clone()
        if consumer is not None:
            t.record_stream(consumer)
        return t
    return CaptionBatch(c(r.ids), c(r.lengths), c(r.scores), c(r.hard_ids), c(r.hard_len),
                        c(r.plen), c(r.prefix_ids), c(r.clap_emb))
