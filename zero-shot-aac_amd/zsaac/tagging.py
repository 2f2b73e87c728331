"""Audio tagging and sound-event detection on the HTSAT checkpoint's own head.

``HTSAT_Swin_Transformer.forward_features`` (retrieval/models/htsat.py:830-894) returns, next to
the embedding every caption starts from, 527 AudioSet class probabilities per clip
(``clipwise_output``) and per time frame (``framewise_output``) from the trained ``tscam_conv``
head.  :class:`AudioTagger` runs that head on the HIP encoder (``AudioEncoder.encode_events``:
zs_tag_prep + zs_tag_conv after the usual pass) and turns it into "which sounds, and when":

  ``tag_wav``     the k most probable classes of each clip (device top-k, zs_sim_topk_finalize)
  ``events_wav``  for each clip's top-k classes, the maximal runs of frames whose probability is
                  at least ``threshold`` and that last at least ``min_frames`` frames, as
                  ``(clip, class_id, name, onset_s, offset_s, peak)``

One frame is 0.32 s: the head sees 1024 spectrogram frames (10.24 s at hop 320 / 32 kHz) as 32
time frames.  Only the [B, k, 32] slice of the frame probabilities travels to the host; the
run-finding (:func:`segments`) is a pure host function.

``python -m zsaac.tagging --ckpt CLAP.pt [--labels class_labels_indices.csv] [--k 5]
[--threshold 0.5] files...`` prints one JSON line per file.  Like the reference's evaluation it
looks at the first 10 s of a file; ``zsaac.longform`` covers a recording's whole duration.
"""
from __future__ import annotations

import csv
import json
from typing import List, Optional, Sequence, Tuple

import torch

FRAMES = 32
FRAME_SECONDS = 10.24 / FRAMES     # 1024 spectrogram frames x 320 samples / 32 kHz, over 32 frames


def segments(probs32, threshold: float, min_frames: int = 1) -> List[Tuple[int, int, float]]:
    """The maximal runs of consecutive frames with probability >= ``threshold`` that are at
    least ``min_frames`` long: ``[(first frame, one past the last frame, peak probability)]`` in
    time order.  ``probs32``: one class's per-frame probabilities (any sequence of numbers)."""
    p = [float(v) for v in probs32]
    out, start = [], -1
    for i in range(len(p) + 1):
        on = i < len(p) and p[i] >= threshold
        if on and start < 0:
            start = i
        elif not on and start >= 0:
            if i - start >= max(int(min_frames), 1):
                out.append((start, i, max(p[start:i])))
            start = -1
    return out


def read_labels(path: str) -> List[str]:
    """AudioSet's class_labels_indices.csv (columns index, mid, display_name) or a plain list of
    names, one per line -> names by class id."""
    with open(path, newline="", encoding="utf-8") as f:
        rows = [r for r in csv.reader(f) if r]
    if rows and [c.strip().lower() for c in rows[0]][:1] == ["index"]:
        col = [c.strip().lower() for c in rows[0]].index("display_name")
        return [r[col] for r in rows[1:]]
    return [r[-1] for r in rows]


class AudioTagger:
    """``audio_sd``: the ASE audio-side state dict (``audio_encoder.audio_enc.*`` with the
    ``tscam_conv`` head; ``audio_proj.*`` optional).  ``class_names``: names by class id
    (default ``class_<id>``).  Waveforms are [B <= batch, n_samples] f32 on the device."""

    def __init__(self, audio_sd, class_names: Optional[Sequence[str]] = None,
                 dtype=torch.bfloat16, batch=64, device="cuda", n_samples=320000, encoder=None):
        from .encoder import AudioEncoder
        self.enc = encoder if encoder is not None else AudioEncoder(
            audio_sd, "htsat", dtype, batch, device, n_samples=n_samples)
        self.names = list(class_names) if class_names is not None else None

    def name(self, class_id: int) -> str:
        if self.names is not None and 0 <= class_id < len(self.names):
            return self.names[class_id]
        return f"class_{class_id}"

    def tag_wav(self, wav: torch.Tensor, k: int = 5):
        """-> (ids [B, k] int32, probabilities [B, k] f32) on the device, best first, ties to the
        lower id (views of the encoder's buffers, valid until its next pass)."""
        self.enc.encode_events(wav)
        prob, ids = self.enc.tag_topk(wav.shape[0], k)
        return ids, prob

    def _events(self, out, B, k, threshold, min_frames):
        prob, ids = self.enc.tag_topk(B, k)
        # frame[b][:, ids[b][q]] for the k chosen classes only: [B, k, 32] leaves the device
        sel = torch.gather(out.frame, 2, ids.long()[:, None, :].expand(B, FRAMES, k))
        sel, ids = sel.permute(0, 2, 1).cpu(), ids.cpu()
        events = []
        for b in range(B):
            for q in range(k):
                cid = int(ids[b, q])
                for s, e, peak in segments(sel[b, q].tolist(), threshold, min_frames):
                    events.append((b, cid, self.name(cid), s * FRAME_SECONDS, e * FRAME_SECONDS,
                                   peak))
        return events, ids, prob.cpu()

    def events_wav(self, wav: torch.Tensor, k: int = 5, threshold: float = 0.5,
                   min_frames: int = 1):
        """For each clip's top-k classes, the maximal runs of frames with probability >=
        ``threshold`` and at least ``min_frames`` long: a list of
        ``(clip, class_id, name, onset_s, offset_s, peak)``, by clip, then class rank, then
        time."""
        out = self.enc.encode_events(wav)
        return self._events(out, wav.shape[0], k, threshold, min_frames)[0]


# ------------------------------------------------------------------ python -m zsaac.tagging
def main(argv=None) -> int:
    import argparse

    from . import safeload
    from .extract import EmbeddingExtractor, _split_state_dict
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt", required=True, help="the CLAP checkpoint ({'model': ASE state dict})")
    ap.add_argument("--labels", default=None, help="class names: AudioSet's class_labels_indices.csv")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--min_frames", type=int, default=1)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="bf16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("files", nargs="+")
    args = ap.parse_args(argv)
    audio_sd, _ = _split_state_dict(safeload.load_state_dict(args.ckpt))
    dtype = torch.float32 if args.dtype == "f32" else torch.bfloat16
    # reading, downmix, resampling and crop / pad are the extractor's (audio_io, zs_resample_pack)
    ex = EmbeddingExtractor(audio_sd, "htsat", dtype, args.batch, args.device)
    tagger = AudioTagger(None, read_labels(args.labels) if args.labels else None, encoder=ex.enc)
    for c0, items in ex._read_chunks(list(args.files)):
        wav = ex.pack_frames(items)
        out = ex.enc.encode_events(wav)
        events, ids, prob = tagger._events(out, len(items), args.k, args.threshold, args.min_frames)
        for b in range(len(items)):
            print(json.dumps({
                "file": args.files[c0 + b],
                "tags": [{"id": int(i), "name": tagger.name(int(i)), "prob": round(float(p), 6)}
                         for i, p in zip(ids[b], prob[b])],
                "events": [{"id": cid, "name": nm, "onset_s": round(on, 2), "offset_s": round(off, 2),
                            "peak": round(pk, 6)}
                           for (bb, cid, nm, on, off, pk) in events if bb == b]}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
