"""Batched embedding extraction: the reference's ``Extract_embeddings``
(data_handing/embeddings_generator.py:34-75) on the HIP encoder.

Per clip the reference decodes the audio file (``librosa.load(path, sr=32000, mono=True)``,
line 48: decode, downmix and, for a file at another rate, resampy's ``kaiser_best``), skips
empty clips, crops to the first ``max_length * sr`` samples or zero-pads to that length (lines
53-59), runs ``ASE.encode_audio`` on a batch of ONE and appends the record
``{"audio_embedding": [1, 1024] cpu tensor, "caption": captions, "text_embedding": 0,
"audio_id": id}`` (lines 70-71); with ``text_or_not`` one record per caption instead, with the
caption's string and its ``ASE.encode_text(text_preprocess(caption))`` (lines 64-69).  The
split's records are pickled to ``<out>/<split>/clap_embedding/ZS/data.pkl`` (lines 100-101).

Here a chunk's clips are packed on the device and encoded ``batch`` at a time.  Sample arrays
already at 32 kHz go through zs_pack_clips (the crop / pad); files go through
``audio_io.read_wav`` on a small thread pool and zs_resample_pack (downmix, resampling, crop /
pad in one launch per sample format; only the frames the kept 10 s need are uploaded).  Captions
are encoded in batches on the BERT text engine.  The records and the pickle have the reference's
format, so predict_prompt.py / zsaac.predict read them unchanged.

``python -m zsaac.extract --config extract_data.yaml --dataset_path D --out_path O`` is the
reference's ``main`` (lines 77-101).
"""
from __future__ import annotations

import csv
import json
import os
import pickle
import re
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import audio_io, ops
from .encoder import AudioEncoder

READ_WORKERS = 16      # most file-reading threads (never sized from the machine's core count)


def text_preprocess(sentence: str) -> str:
    """embeddings_generator.py:21-32: lower case, no space before punctuation, punctuation to
    spaces, double spaces collapsed once after each step."""
    sentence = sentence.lower()
    sentence = re.sub(r'\s([,.!?;:"](?:\s|$))', r'\1', sentence).replace('  ', ' ')
    sentence = re.sub('[(,.!?;:|*\")]', ' ', sentence).replace('  ', ' ')
    return sentence


def fit_plan(lengths: Sequence[int], max_samples: int):
    """Which clips are encoded (the reference skips empty ones) and how many samples of each
    are kept (crop to max_samples, the rest zero-padded)."""
    keep = [i for i, n in enumerate(lengths) if n > 0]
    return keep, [min(int(lengths[i]), max_samples) for i in keep]


def make_record(emb_row: torch.Tensor, caption, audio_id) -> dict:
    """One entry of the reference's data.pkl (embeddings_generator.py:70-71, text_or_not False)."""
    return {"audio_embedding": emb_row.detach().reshape(1, -1).float().cpu(), "caption": caption,
            "text_embedding": 0, "audio_id": audio_id}


class EmbeddingExtractor:
    """``Extract_embeddings`` for in-memory clips and for files.  ``audio_sd``: the ASE
    audio-side state dict (``audio_encoder.*`` + ``audio_proj.*``), ``kind`` "htsat" | "cnn14".
    ``text`` (an ``ASE`` with a text tower, or a ``zsaac.bert.BertTextEngine``) and ``tokenizer``
    (a BERT tokenizer; optional for an ASE that carries its own) enable ``text_or_not``."""

    def __init__(self, audio_sd, kind="htsat", dtype=torch.bfloat16, batch=64, device="cuda",
                 sr=32000, max_length=10, text=None, tokenizer=None, text_batch=256):
        self.sr, self.max_length = sr, max_length
        self.T = max_length * sr if max_length else 320000
        self.device = torch.device(device)
        self.enc = AudioEncoder(audio_sd, kind, dtype, batch, self.device, n_samples=self.T)
        self.B = batch
        self.wav = torch.empty(batch, self.T, device=self.device)
        self.text, self.tokenizer, self.text_batch = text, tokenizer, text_batch
        self._filter = None      # (device table, num_zeros, precision), built on first use
        self._stage = None       # second [batch, T] buffer: chunks that mix int16 and float32

    # ------------------------------------------------------------------ files
    def _resample_filter(self):
        if self._filter is None:
            tab, nz, prec = audio_io.resample_filter("kaiser_best")
            self._filter = (torch.from_numpy(tab).to(self.device), nz, prec)
        return self._filter

    def pack_frames(self, items: Sequence) -> torch.Tensor:
        """``(frames, sr)`` pairs (at most ``batch``; frames [n] or [n, C], int16 or float) ->
        wav [b, T] on the device, row i what ``librosa.load(file_i, sr=self.sr, mono=True)``
        cropped / padded to T gives (zs_resample_pack).  One upload and one launch for the int16
        clips, one for the float32 clips; only the frames the first T outputs read travel."""
        b = len(items)
        if not 0 < b <= self.B:
            raise ValueError(f"pack_frames takes 1..{self.B} clips, got {b}")
        groups = {}
        for i, (frames, sr) in enumerate(items):
            a = np.asarray(frames)
            if a.ndim == 1:
                a = a[:, None]
            if a.dtype != np.int16:
                a = a.astype(np.float32, copy=False)
            n_out, need = audio_io.resample_plan(a.shape[0], sr, self.sr, self.T)
            groups.setdefault(a.dtype == np.int16, []).append((i, a[:need], int(sr), n_out))
        table, nz, prec = self._resample_filter()
        mixed = len(groups) > 1
        if mixed and self._stage is None:
            self._stage = torch.empty_like(self.wav)
        dst, row, order = (self._stage if mixed else self.wav), 0, []
        for _, clips in sorted(groups.items()):
            sizes = [a.size for _, a, _, _ in clips]
            flat = np.concatenate([a.reshape(-1) for _, a, _, _ in clips]) if sum(sizes) else \
                np.zeros(1, clips[0][1].dtype)
            offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
            ops.resample_pack(torch.from_numpy(flat).to(self.device, non_blocking=True), offs,
                              [a.shape[0] for _, a, _, _ in clips],
                              [a.shape[1] for _, a, _, _ in clips], [s for _, _, s, _ in clips],
                              [n for _, _, _, n in clips], self.sr, self.T, table, nz, prec,
                              dst[row:])
            row += len(clips)
            order += [i for i, _, _, _ in clips]
        if mixed:                      # group order -> item order
            inv = torch.empty(b, dtype=torch.int64)
            inv[torch.tensor(order)] = torch.arange(b)
            torch.index_select(self._stage[:b], 0, inv.to(self.device), out=self.wav[:b])
        return self.wav[:b]

    def _encode_frames(self, items: Sequence) -> torch.Tensor:
        return self.enc.encode(self.pack_frames(items))

    def _read_chunks(self, paths: Sequence[str]):
        """Yields (first index, [(frames, sr), ...]) per ``batch`` files; the next chunk's files
        are read by the pool while the caller encodes the current one."""
        chunks = [paths[c0:c0 + self.B] for c0 in range(0, len(paths), self.B)]
        if not chunks:
            return
        with ThreadPoolExecutor(max_workers=min(READ_WORKERS, max(len(paths), 1))) as pool:
            nxt = [pool.submit(audio_io.read_wav, p) for p in chunks[0]]
            for ci in range(len(chunks)):
                cur = nxt
                nxt = [pool.submit(audio_io.read_wav, p) for p in chunks[ci + 1]] \
                    if ci + 1 < len(chunks) else []
                yield ci * self.B, [f.result() for f in cur]

    def encode_files(self, paths: Sequence[str]) -> torch.Tensor:
        """WAV files -> [n, 1024] device embeddings, in order (an empty file encodes silence;
        :meth:`extract_dataset` skips those like the reference)."""
        out = torch.empty(len(paths), 1024, device=self.device)
        for c0, items in self._read_chunks(list(paths)):
            out[c0:c0 + len(items)].copy_(self._encode_frames(items))
        return out

    # ------------------------------------------------------------------ text
    def encode_captions(self, texts: Sequence[str]) -> torch.Tensor:
        """``ASE.encode_text`` of already preprocessed strings, ``text_batch`` at a time ->
        [n, 1024] on the CPU."""
        if self.text is None:
            raise NotImplementedError("text embeddings need the BERT text encoder "
                                      "(retrieval/models/text_encoder.py): pass text= (an ASE with "
                                      "a text tower or a BertTextEngine) and tokenizer=")
        eng = self.text.text_engine() if hasattr(self.text, "text_engine") else self.text
        tok = self.tokenizer
        if tok is None and hasattr(self.text, "text_encoder"):
            tok = self.text.text_encoder.tokenizer
        if tok is None:
            raise NotImplementedError("text embeddings need a BERT tokenizer: pass tokenizer=")
        parts = [eng.encode_texts(tok, list(texts[c0:c0 + self.text_batch])).float().cpu()
                 for c0 in range(0, len(texts), self.text_batch)]
        return torch.cat(parts) if parts else torch.empty(0, 1024)

    def _records(self, emb: torch.Tensor, entries: Sequence[dict], text_or_not: bool) -> List[dict]:
        """The reference's records for the kept clips (``emb`` row j belongs to ``entries[j]``,
        an item of text.json's "audios")."""
        if not text_or_not:
            return [make_record(emb[j], e["captions"], e["audio_id"]) for j, e in enumerate(entries)]
        caps = [(j, c["caption"]) for j, e in enumerate(entries) for c in e["captions"]]
        temb = self.encode_captions([text_preprocess(c) for _, c in caps])
        recs = []
        for k, (j, c) in enumerate(caps):
            r = make_record(emb[j], c, entries[j]["audio_id"])
            r["text_embedding"] = temb[k].reshape(1, -1)
            recs.append(r)
        return recs

    def extract_dataset(self, data_path: str, text_or_not: bool = False) -> List[dict]:
        """``Extract_embeddings(model, data_path, text_or_not, config)``: ``wav.csv`` (tab
        separated ``audio_id``, ``file_name``) names the files, ``text.json["audios"]`` the clips
        and their captions, in the order of the records (lines 36-38); clips without samples are
        skipped (lines 51-52)."""
        if text_or_not and self.text is None:
            self.encode_captions([])        # raises: no text tower
        with open(os.path.join(data_path, "wav.csv"), newline="", encoding="utf-8") as f:
            files = {str(r["audio_id"]): r["file_name"] for r in csv.DictReader(f, delimiter="\t")}
        with open(os.path.join(data_path, "text.json"), encoding="utf-8") as f:
            entries = json.load(f)["audios"]
        paths = [files[str(e["audio_id"])] for e in entries]
        kept, embs = [], []
        for c0, items in self._read_chunks(paths):
            live = [j for j, (frames, _) in enumerate(items) if frames.shape[0] > 0]
            if live:
                embs.append(self._encode_frames([items[j] for j in live]).cpu())
                kept += [entries[c0 + j] for j in live]
        emb = torch.cat(embs) if embs else torch.empty(0, 1024)
        return self._records(emb, kept, text_or_not)

    # ------------------------------------------------------------------ sample arrays

    def encode_clips(self, clips: Sequence) -> torch.Tensor:
        """Ragged 1-D clips (numpy / torch, any length >= 1) -> [n, 1024] device embeddings, in
        order."""
        n = len(clips)
        out = torch.empty(n, 1024, device=self.device)
        for c0 in range(0, n, self.B):
            chunk = clips[c0:c0 + self.B]
            lens = [int(np.asarray(c).shape[-1]) if not torch.is_tensor(c) else int(c.shape[-1])
                    for c in chunk]
            flat = torch.cat([torch.as_tensor(c, dtype=torch.float32).reshape(-1) for c in chunk])
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            dflat = flat.to(self.device, non_blocking=True)
            b = len(chunk)
            ops.pack_clips(dflat, torch.from_numpy(offs).to(self.device),
                           torch.tensor(lens, dtype=torch.int32, device=self.device), self.T,
                           self.wav)
            out[c0:c0 + b].copy_(self.enc.encode(self.wav[:b]))
        return out

    def extract(self, clips: Sequence, audio_ids: Sequence, captions: Sequence,
                text_or_not: bool = False) -> List[dict]:
        """The records of ``Extract_embeddings`` (empty clips skipped, like the reference)."""
        if text_or_not and self.text is None:
            self.encode_captions([])        # raises: no text tower
        lengths = [int(torch.as_tensor(c).shape[-1]) for c in clips]
        keep, _ = fit_plan(lengths, self.T)
        emb = self.encode_clips([clips[i] for i in keep]).cpu()
        entries = [{"audio_id": audio_ids[i], "captions": captions[i]} for i in keep]
        return self._records(emb, entries, text_or_not)


def save_records(records: List[dict], out_path: str, split: Optional[str] = None) -> str:
    """Pickle the records where the reference writes them
    (``<out_path>/<split>/clap_embedding/ZS/data.pkl``, embeddings_generator.py:100-101); with
    ``split=None`` ``out_path`` is the file itself."""
    path = out_path if split is None else os.path.join(out_path, split, "clap_embedding", "ZS",
                                                        "data.pkl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(records, f)
    return path


# ------------------------------------------------------------------ python -m zsaac.extract
def _split_state_dict(sd):
    audio = {k: v for k, v in sd.items() if k.startswith("audio_encoder.") or k.startswith("audio_proj.")}
    text = {k: v for k, v in sd.items()
            if k.startswith("text_encoder.") or k.startswith("text_proj.") or k == "temp"}
    return audio, text


def main(argv=None) -> int:
    """embeddings_generator.py:77-101: the train split with text embeddings, val / test without;
    ``--config`` is the reference's extract_data.yaml (``audio_args.sr`` / ``max_length``,
    ``pretrain_path``: the CLAP checkpoint ``{"model": ASE state dict}``, ``device``)."""
    import argparse

    import yaml

    from . import safeload
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default="settings/extract_data.yaml", type=str, help="setting file")
    ap.add_argument("--dataset_path", type=str, required=True, help="<path>/<split>/{wav.csv,text.json}")
    ap.add_argument("--out_path", type=str, required=True, help="<path>/<split>/clap_embedding/ZS/data.pkl")
    ap.add_argument("--splits", type=str, default="train,val,test")
    ap.add_argument("--bert_vocab", type=str, default=None,
                    help="BERT vocab.txt (bert-base-uncased's); needed for the train split's text embeddings")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="bf16")
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args(argv)
    with open(args.config, encoding="utf-8") as f:
        config = yaml.safe_load(f)
    aa = config["audio_args"]
    device = config.get("device", "cuda")
    dtype = torch.float32 if args.dtype == "f32" else torch.bfloat16
    audio_sd, text_sd = _split_state_dict(safeload.load_state_dict(config["pretrain_path"]))
    kind = "htsat" if audio_sd["audio_proj.0.weight"].shape[1] == 768 else "cnn14"
    splits = [s for s in args.splits.split(",") if s]
    text = tokenizer = None
    if "train" in splits:
        if not args.bert_vocab:
            raise SystemExit("the train split carries text embeddings: --bert_vocab <vocab.txt>")
        from transformers import BertTokenizer

        from .bert import BertTextEngine
        with open(args.bert_vocab, encoding="utf-8") as f:
            vocab = {t.rstrip("\n"): i for i, t in enumerate(f)}
        tokenizer = BertTokenizer(vocab=vocab, do_lower_case=True)
        text = BertTextEngine(text_sd, device, dtype)
    ex = EmbeddingExtractor(audio_sd, kind, dtype, args.batch, device, sr=aa["sr"],
                            max_length=aa["max_length"], text=text, tokenizer=tokenizer)
    for split in splits:
        print(f"---Extract the embeddings of {split} set---")
        recs = ex.extract_dataset(os.path.join(args.dataset_path, split), split == "train")
        print(save_records(recs, args.out_path, split), len(recs), "records")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
