"""Long recordings: tags, sound events, embeddings and captions over a file's whole duration.

Every other entry point that takes audio keeps the first 10 s (the reference's evaluation
behaviour: ``zsaac.extract``, ``zsaac.tagging``, ``CaptionPipeline.caption_wav``).  Here a
recording of any length is resampled ONCE on the device, straight into overlapping windows of
``T`` samples ``hop`` apart (zs_resample_windows: every window row is bit-equal to the same
outputs of the whole-file signal, so no window sees zeros where its neighbours' samples are);
the windows go through the HTSAT pass and the tagging head ``batch`` at a time like clips of
their own (``AudioEncoder.encode_events``); zs_window_stitch puts their outputs back onto one
time line per recording:

  time line   frame probabilities [F, 527], one frame per ``T / 32`` samples (0.3125 s): the
              mean of the windows that cover the frame
  tags        the recording's k most probable classes: the maximum over its windows of the
              clip probabilities (an event anywhere counts), device top-k
  events      ``tagging.segments`` on the time line of those classes: a run that crosses a
              window boundary is one event
  emb         the windows' embeddings weighted by their share of valid samples, summed and
              normalised; a recording of at most ``T`` samples keeps its one window's embedding,
              i.e. what ``EmbeddingExtractor.encode_files`` gives it, bit for bit

:func:`window_plan` and :func:`stitch_tables` are pure host functions.

``python -m zsaac.longform --ckpt CLAP.pt [--labels CSV] [--hop 5] [--k 5] [--threshold 0.5]
[--caption TEST_DIR [--per_window]] files...`` prints one JSON line per file.
"""
from __future__ import annotations

import json
import warnings
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import audio_io, ops
from .tagging import segments

FRAMES = 32                     # head frames per window


def _check_hop(T: int, hop: int) -> Tuple[int, int]:
    if T <= 0 or T % FRAMES:
        raise ValueError(f"window length {T}: a positive multiple of {FRAMES}")
    frame = T // FRAMES
    if hop % frame or not frame <= hop <= T:
        raise ValueError(f"hop {hop}: a multiple of the frame length {frame} in [{frame}, {T}]")
    return frame, hop // frame


def window_plan(n_out: int, T: int = 320000, hop: int = 160000) -> Tuple[int, int]:
    """(n_win, F) of a recording of ``n_out`` samples at the target rate: window w holds samples
    [w * hop, w * hop + T) (zero past ``n_out``), the last one more than ``T - hop`` valid ones;
    ``F`` time-line frames of ``T // 32`` samples, without those that lie wholly in the last
    window's padding.  An empty recording has no window."""
    frame, hop_f = _check_hop(T, hop)
    n_out = int(n_out)
    if n_out < 0:
        raise ValueError(f"n_out {n_out} < 0")
    if n_out == 0:
        return 0, 0
    n_win = 1 if n_out <= T else 1 + -(-(n_out - T) // hop)
    return n_win, min(-(-n_out // frame), (n_win - 1) * hop_f + FRAMES)


def stitch_tables(n_outs: Sequence[int], T: int = 320000, hop: int = 160000):
    """The tables of zs_window_stitch for recordings of ``n_outs`` samples, in order: plan [R, 4]
    int32 = (row0, n_win, frow0, F) and wgt [sum n_win] float32 = valid samples / T of every
    window row (host arrays)."""
    plan, wgt, row0, frow0 = [], [], 0, 0
    for n in n_outs:
        n_win, F = window_plan(n, T, hop)
        plan.append((row0, n_win, frow0, F))
        wgt += [min(T, int(n) - w * hop) / T for w in range(n_win)]
        row0, frow0 = row0 + n_win, frow0 + F
    if row0 >= 2 ** 31 or frow0 >= 2 ** 31:
        raise ValueError("more than 2^31 window rows or time-line frames in one group")
    return np.array(plan, np.int32).reshape(-1, 4), np.array(wgt, np.float32)


@dataclass
class LongResult:
    """One recording.  ``emb`` [1024] and ``window_emb`` [n_windows, 1024] are device tensors
    (``None`` for an empty recording, which has no window); ``tags`` [(id, name, prob)] best
    first; ``events`` [(id, name, onset_s, offset_s, peak)] by tag rank, then time; ``timeline``
    [F, 527] the frame probabilities, on the device (None without the head)."""
    file: Optional[str]
    seconds: float
    n_windows: int
    emb: Optional[torch.Tensor] = None
    tags: List[tuple] = field(default_factory=list)
    events: List[tuple] = field(default_factory=list)
    window_emb: Optional[torch.Tensor] = None
    timeline: Optional[torch.Tensor] = None

    def window_spans(self, T: int, hop: int, sr: int) -> List[Tuple[float, float]]:
        """(onset_s, offset_s) of every window, the last one ending with the recording."""
        return [(w * hop / sr, min(self.seconds, (w * hop + T) / sr)) for w in range(self.n_windows)]


class LongAudio:
    """``audio_sd``: the ASE audio-side state dict (``audio_encoder.*`` + ``audio_proj.*``).
    Built on one ``EmbeddingExtractor`` (``extractor``, made here if not given: the filter table
    and the reading pool's size are its) and its ``AudioEncoder`` (or ``encoder``).  A CNN14
    encoder has no tagging head: it gives embeddings only (``k=0``)."""

    def __init__(self, audio_sd, class_names: Optional[Sequence[str]] = None, dtype=torch.bfloat16,
                 batch=64, device="cuda", hop_seconds=5.0, encoder=None, extractor=None):
        from . import extract
        if extractor is None and encoder is None:
            kind = "htsat" if audio_sd["audio_proj.0.weight"].shape[1] == 768 else "cnn14"
            extractor = extract.EmbeddingExtractor(audio_sd, kind, dtype, batch, device)
        self.ex = extractor
        self.enc = encoder if encoder is not None else extractor.enc
        if self.enc.proj is None:
            raise ValueError("LongAudio needs the audio_proj weights (the 1024-d embedding)")
        self.device, self.B, self.T = self.enc.dev, self.enc.B, self.enc.T
        self.sr = extractor.sr if extractor is not None else 32000
        self.workers = extract.READ_WORKERS
        self.hop = int(round(hop_seconds * self.sr))
        self.frame, self.hop_f = _check_hop(self.T, self.hop)
        self.names = list(class_names) if class_names is not None else None
        self.group_windows = 4 * self.B          # windows resampled at once (a longer recording
        self._filter = None                       # is a group of its own)
        self._rows = None                         # [W, T] window rows, grown on demand

    def name(self, class_id: int) -> str:
        if self.names is not None and 0 <= class_id < len(self.names):
            return self.names[class_id]
        return f"class_{class_id}"

    def _resample_filter(self):
        if self.ex is not None:
            return self.ex._resample_filter()
        if self._filter is None:
            tab, nz, prec = audio_io.resample_filter("kaiser_best")
            self._filter = (torch.from_numpy(tab).to(self.device), nz, prec)
        return self._filter

    # ------------------------------------------------------------------ front: window rows
    def window_rows(self, items: Sequence):
        """``(frames, sr)`` pairs (whole recordings; frames [n] or [n, C], int16 or float) ->
        (rows [W, T] on the device, a view of an internal buffer; plan [R, 4], wgt [W] host
        tables in the items' order; n_out per item).  One upload and one zs_resample_windows per
        sample format."""
        recs = []
        for frames, sr in items:
            a = np.asarray(frames)
            if a.ndim == 1:
                a = a[:, None]
            if a.dtype != np.int16:
                a = a.astype(np.float32, copy=False)
            n_out, _ = audio_io.resample_plan(a.shape[0], sr, self.sr, self.T)
            recs.append((np.ascontiguousarray(a), int(sr), n_out))
        plan, wgt = stitch_tables([n for _, _, n in recs], self.T, self.hop)
        W = int(plan[:, 1].sum())
        if self._rows is None or self._rows.shape[0] < W:
            self._rows = None                     # release before growing
            self._rows = torch.empty(max(W, 1), self.T, device=self.device)
        table, nz, prec = self._resample_filter()
        # recordings of one sample format that follow each other share a call (rows are
        # recording-major, so a call's rows are contiguous)
        i = 0
        while i < len(recs):
            j = i
            while j < len(recs) and recs[j][0].dtype == recs[i][0].dtype:
                j += 1
            run = recs[i:j]
            if int(plan[i:j, 1].sum()):
                sizes = [a.size for a, _, _ in run]
                offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
                # each recording goes straight into its place of one device buffer (no host copy
                # of the whole group first)
                flat = torch.empty(max(sum(sizes), 1), device=self.device,
                                   dtype=torch.int16 if run[0][0].dtype == np.int16 else torch.float32)
                with warnings.catch_warnings():      # decoded files are read-only views of their bytes
                    warnings.simplefilter("ignore", UserWarning)
                    for (a, _, _), o in zip(run, offs):
                        if a.size:
                            flat[int(o):int(o) + a.size].copy_(torch.from_numpy(a.reshape(-1)), non_blocking=True)
                ops.resample_windows(flat, offs,
                                     [a.shape[0] for a, _, _ in run], [a.shape[1] for a, _, _ in run],
                                     [s for _, s, _ in run], [n for _, _, n in run], plan[i:j, 1],
                                     self.sr, self.T, self.hop, table, nz, prec,
                                     self._rows[int(plan[i, 0]):])
            i = j
        return self._rows[:W], plan, wgt, [n for _, _, n in recs]

    # ------------------------------------------------------------------ the windowed pass
    def _group(self, items, files, k, threshold, min_frames) -> List[LongResult]:
        rows, plan, wgt, n_outs = self.window_rows(items)
        res = [LongResult(f, n / self.sr, int(p[1])) for f, n, p in zip(files, n_outs, plan)]
        live = [r for r in range(len(items)) if plan[r, 1] > 0]
        if not live:
            return res
        W, dev, head = rows.shape[0], self.device, k > 0
        if head:
            tw, _ = self.enc._tag_setup()         # raises for CNN14 / a checkpoint without the head
            N = tw["n"]
            frame = torch.empty(W, FRAMES, N, device=dev)
            clip = torch.empty(W, N, device=dev)
        emb = torch.empty(W, 1024, device=dev)
        for c0 in range(0, W, self.B):            # a recording's windows may span passes
            c1 = min(W, c0 + self.B)
            if head:
                out = self.enc.encode_events(rows[c0:c1])
                frame[c0:c1].copy_(out.frame)
                clip[c0:c1].copy_(out.clip)
                emb[c0:c1].copy_(out.emb)
            else:
                emb[c0:c1].copy_(self.enc.encode(rows[c0:c1]))
        # empty recordings have no row and no frame: the stitch sees the live ones only
        lp = np.ascontiguousarray(plan[live])
        R, SF = len(live), int(lp[-1, 2] + lp[-1, 3])
        dplan, dwgt = torch.from_numpy(lp).to(dev), torch.from_numpy(wgt).to(dev)
        rec_emb = torch.empty(R, 1024, device=dev)
        if head:
            ldrc = (N + 7) // 8 * 8
            timeline = torch.empty(SF, N, device=dev)
            rec_clip = torch.empty(R, ldrc, device=dev)
            ops.window_stitch(dplan, lp, dwgt, self.hop_f, N, frame, clip, emb, timeline, rec_clip,
                              rec_emb)
            idx = torch.full((R, ldrc), 0x7fffffff, device=dev, dtype=torch.int32)
            idx[:, :N] = torch.arange(N, device=dev, dtype=torch.int32)
            top_v = torch.empty(R, k, device=dev)
            top_i = torch.empty(R, k, device=dev, dtype=torch.int32)
            ops.sim_topk_finalize(rec_clip, idx, R, ldrc // 8, 8, k, top_v, top_i)
            # the chosen classes' columns of every recording's frames: [sum F, k] leaves the device
            rec_of = torch.from_numpy(np.repeat(np.arange(R), lp[:, 3])).to(dev)
            sel = torch.gather(timeline, 1, top_i.long()[rec_of]).cpu()
            top_v, top_i = top_v.cpu(), top_i.cpu()
        else:
            ops.window_stitch(dplan, lp, dwgt, self.hop_f, 1, emb=emb, rec_emb=rec_emb)
        sec = self.frame / self.sr
        for q, r in enumerate(live):
            row0, n_win, frow0, F = (int(v) for v in lp[q])
            res[r].emb, res[r].window_emb = rec_emb[q], emb[row0:row0 + n_win]
            if not head:
                continue
            res[r].timeline = timeline[frow0:frow0 + F]
            for c in range(k):
                cid = int(top_i[q, c])
                res[r].tags.append((cid, self.name(cid), float(top_v[q, c])))
                for s, e, peak in segments(sel[frow0:frow0 + F, c].tolist(), threshold, min_frames):
                    res[r].events.append((cid, self.name(cid), s * sec, e * sec, peak))
        return res

    def _analyse(self, items, files, k, threshold, min_frames):
        if k and self.enc.kind != "htsat":
            raise NotImplementedError("tags / events need HTSAT's tagging head (CNN14 has none): "
                                      "k=0 gives the embeddings alone")
        if not 0 <= k <= 8:
            raise ValueError(f"k = {k}: 0 (embeddings only) .. 8")
        out, cur, nw = [], [], 0
        for it, f in zip(items, files):
            n = np.asarray(it[0]).shape[0]
            w = window_plan(audio_io.resample_plan(n, it[1], self.sr, self.T)[0], self.T, self.hop)[0]
            if cur and nw + w > self.group_windows:
                out += self._group([c[0] for c in cur], [c[1] for c in cur], k, threshold, min_frames)
                cur, nw = [], 0
            cur.append((it, f))
            nw += w
        if cur:
            out += self._group([c[0] for c in cur], [c[1] for c in cur], k, threshold, min_frames)
        return out

    def analyse_files(self, paths: Sequence[str], k: int = 5, threshold: float = 0.5,
                      min_frames: int = 1) -> List[LongResult]:
        """WAV files, read whole -> one :class:`LongResult` per file, in order."""
        paths = list(paths)
        if not paths:
            return []
        with ThreadPoolExecutor(max_workers=min(self.workers, len(paths))) as pool:
            items = list(pool.map(audio_io.read_wav, paths))
        return self._analyse(items, paths, k, threshold, min_frames)

    def analyse_clips(self, clips: Sequence, k: int = 5, threshold: float = 0.5,
                      min_frames: int = 1) -> List[LongResult]:
        """The same for 1-D sample arrays (numpy / torch) already at the encoder's rate."""
        items = [(torch.as_tensor(c, dtype=torch.float32).reshape(-1).numpy(), self.sr) for c in clips]
        return self._analyse(items, [None] * len(items), k, threshold, min_frames)

    # ------------------------------------------------------------------ captions
    def caption_files(self, pipe, tokenizer, paths: Sequence[str], per_window: bool = False,
                      **kw):
        """``analyse_files`` plus captions from ``pipe`` (a CaptionPipeline; ``tokenizer`` decodes
        its ids, None keeps the id lists): [(LongResult, caption, spans)] with ``caption`` of the
        recording's pooled embedding and, with ``per_window``, ``spans`` = [(onset_s, offset_s,
        caption)] of every window's own embedding (else None).  An empty recording has neither."""
        def dec(ids):
            return tokenizer.decode(ids).lower() if tokenizer is not None else list(ids)

        def captions(emb):
            caps, B = [], pipe.cfg.batch
            for c0 in range(0, emb.shape[0], B):
                caps += [dec(ids) for ids in pipe.caption_emb(emb[c0:c0 + B]).captions()]
            return caps
        res = self.analyse_files(paths, **kw)
        live = [r for r in res if r.n_windows]
        caps = captions(torch.stack([r.emb for r in live])) if live else []
        by_id = {id(r): c for r, c in zip(live, caps)}
        out = []
        for r in res:
            spans = None
            if per_window and r.n_windows:
                wc = captions(r.window_emb)
                spans = [(a, b, c) for (a, b), c in zip(r.window_spans(self.T, self.hop, self.sr), wc)]
            out.append((r, by_id.get(id(r)), spans))
        return out


# ------------------------------------------------------------------ python -m zsaac.longform
def main(argv=None) -> int:
    import argparse
    import os

    from . import safeload
    from .extract import _split_state_dict
    from .tagging import read_labels
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt", required=True, help="the CLAP checkpoint ({'model': ASE state dict})")
    ap.add_argument("--labels", default=None, help="class names: AudioSet's class_labels_indices.csv")
    ap.add_argument("--hop", type=float, default=5.0, help="seconds between windows (a multiple of 0.3125)")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--min_frames", type=int, default=1)
    ap.add_argument("--caption", default=None, metavar="TEST_DIR",
                    help="a trained caption model's directory (as zsaac.predict --test_dir)")
    ap.add_argument("--per_window", action="store_true", help="--caption: one caption per window too")
    ap.add_argument("--tokenizer", default=None, help="--caption: GPT-2 vocab.json + merges.txt directory")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="bf16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("files", nargs="+")
    args = ap.parse_args(argv)
    audio_sd, _ = _split_state_dict(safeload.load_state_dict(args.ckpt))
    dtype = torch.float32 if args.dtype == "f32" else torch.bfloat16
    la = LongAudio(audio_sd, read_labels(args.labels) if args.labels else None, dtype, args.batch,
                   args.device, hop_seconds=args.hop)
    kw = dict(k=args.k, threshold=args.threshold, min_frames=args.min_frames)
    if args.caption:
        from .bpe import GPT2BPE
        from .predict import build_pipeline, load_params
        tok = GPT2BPE.from_dir(args.tokenizer or os.path.join(args.caption, "tokenizer"))
        pipe, _ = build_pipeline(args.caption, load_params(args.caption), tok, False, dtype,
                                 args.batch, args.device)
        rows = la.caption_files(pipe, tok, args.files, args.per_window, **kw)
    else:
        rows = [(r, None, None) for r in la.analyse_files(args.files, **kw)]
    for r, cap, spans in rows:
        line = {"file": r.file, "seconds": round(r.seconds, 3), "windows": r.n_windows,
                "tags": [{"id": i, "name": nm, "prob": round(p, 6)} for i, nm, p in r.tags],
                "events": [{"id": i, "name": nm, "onset_s": round(on, 4), "offset_s": round(off, 4),
                            "peak": round(pk, 6)} for i, nm, on, off, pk in r.events]}
        if args.caption:
            line["caption"] = cap
            if spans is not None:
                line["window_captions"] = [{"onset_s": round(a, 3), "offset_s": round(b, 3),
                                            "caption": c} for a, b, c in spans]
        print(json.dumps(line))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
