"""Audio-text retrieval metrics on the device.

The reference judges ASE by retrieval (``a2t`` / ``t2a``, retrieval/tools/utils.py:169-251, called
from ``validate``, retrieval/pretrain.py:262-284), classifies zero-shot by
``audio_emb @ text_embeds.t()`` (retrieval/zero_shot_classification.py:82-106) and gives every
caption its nearest captions of a bank (data_handing/embeddings_related_generator.py:19-28).  Its
route materialises the query x gallery similarity matrix and argsorts every row on the host.  Here
no such matrix exists:

* ``rank_targets``  zs_sim_rank: the rank of given gallery items (value descending, then index
  ascending) and their similarity, from the GEMM's registers;
* ``topk``          zs_lmhead_topk with the gallery as ``W`` (per-block lists) and
  zs_sim_topk_finalize (the row's global top-k).

Both take device tensors, run on the current stream and never synchronise with the host.
``metrics_from_ranks`` is the reference's arithmetic on the ranks, on the host in float64.

    python -m zsaac.retrieval RECORDS.pkl [--dtype bf16|f32]

reads the record pickle zsaac/extract.py writes and prints both metric lines of ``log_results``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import ZsError

# topk(): the [rows][nblk][k] value + index lists of one query chunk stay below this many bytes
TOPK_PARTIAL_BYTES = 256 << 20


def _prep(x: torch.Tensor, dtype, normalize: bool) -> torch.Tensor:
    """[R, K] device rows -> contiguous ``dtype`` rows with K a multiple of 32 (zero columns add
    nothing to a dot product); ``normalize``: zs_l2norm_rows in f32 first (cos_sim's own
    normalisation, util.cos_sim)."""
    if not x.is_cuda:
        raise ZsError("zsaac.retrieval takes device tensors (no CPU fallback)")
    if x.dim() != 2:
        raise ZsError("retrieval: embeddings are [rows, K]")
    K = x.shape[1]
    if normalize or K % 32:
        x = x.float().contiguous()
        if normalize:
            x = ops.l2norm(x)
        if K % 32:
            x = torch.nn.functional.pad(x, (0, 32 - K % 32))
    if x.dtype == dtype and x.is_contiguous():
        return x
    if dtype == torch.bfloat16 and x.dtype == torch.float32:
        return ops.cast(x.contiguous(), torch.empty(x.shape, dtype=dtype, device=x.device))
    return x.to(dtype).contiguous()


def _dtype(q, dtype):
    if dtype is None:
        dtype = q.dtype if q.dtype in (torch.float32, torch.bfloat16) else torch.float32
    if isinstance(dtype, str):
        dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype]
    return dtype


def rank_targets(q, g, tgt, dtype=None, normalize=False):
    """rank [M, T] int32 and tgt_sim [M, T] f32 of gallery items ``tgt`` [M, T] (or [M]) for
    queries q [M, K] against gallery g [N, K]: rank = the item's 0-based position in the row of
    similarities sorted by value descending, then index ascending; -1 for a target outside
    [0, N)."""
    dtype = _dtype(q, dtype)
    qq, gg = _prep(q, dtype, normalize), _prep(g, dtype, normalize)
    if not tgt.is_cuda:
        raise ZsError("zsaac.retrieval takes device tensors (no CPU fallback)")
    t2 = tgt.reshape(tgt.shape[0], -1).to(torch.int32).contiguous()
    rank = torch.empty(t2.shape, dtype=torch.int32, device=qq.device)
    sim = torch.empty(t2.shape, dtype=torch.float32, device=qq.device)
    ops.sim_rank(qq, gg, t2, sim, rank)
    return rank.view(tgt.shape), sim.view(tgt.shape)


def topk(q, g, k, dtype=None, normalize=False, partial_bytes=TOPK_PARTIAL_BYTES):
    """val [M, k] f32, idx [M, k] int32: the k most similar gallery rows of every query, value
    descending, then index ascending (1 <= k <= 8; with k > N the tail is (-inf, 0x7fffffff)).
    The queries go through in chunks whose partial lists stay under ``partial_bytes``."""
    if not 1 <= k <= 8:
        raise ZsError("retrieval.topk: 1 <= k <= 8")
    dtype = _dtype(q, dtype)
    qq, gg = _prep(q, dtype, normalize), _prep(g, dtype, normalize)
    M, N = qq.shape[0], gg.shape[0]
    nblk = ops.lmhead_nblk(N)
    rows = max(1, min(M, partial_bytes // (nblk * k * 8)))
    pv = torch.empty(rows, nblk, k, dtype=torch.float32, device=qq.device)
    pi = torch.empty(rows, nblk, k, dtype=torch.int32, device=qq.device)
    val = torch.empty(M, k, dtype=torch.float32, device=qq.device)
    idx = torch.empty(M, k, dtype=torch.int32, device=qq.device)
    for m0 in range(0, M, rows):
        m = min(rows, M - m0)
        ops.lmhead_topk(qq[m0:m0 + m], gg, k, None, pv, pi, M=m)
        ops.sim_topk_finalize(pv, pi, m, nblk, k, k, val[m0:m0 + m], idx[m0:m0 + m])
    return val, idx


# ------------------------------------------------------------------ metrics (host, float64)
def metrics_from_ranks(ranks, mode, return_ranks=False, top1=None):
    """The reference's metrics from 0-based ranks (retrieval/tools/utils.py:202-213, 240-251):
    ``(r1, r5, r10, r50, medr, meanr, mAP10)`` (+ ``ranks, top1`` with ``return_ranks``).

    mode "a2t": ranks [n_audio, per_audio], one row per clip -- the clip's rank is its group's
    best, AP@10 the precision over the group's positions below 10, divided by the group size.
    mode "t2a": ranks [n_query] -- mAP10 is the mean of 1 / (rank + 1) over the ranks below 10."""
    r = np.asarray(ranks, dtype=np.float64)
    if mode == "a2t":
        r = r.reshape(r.shape[0], -1)
        per = r.shape[1]
        best = r.min(axis=1)
        ap = np.zeros(r.shape[0])
        for i in range(r.shape[0]):
            pos = np.sort(r[i][r[i] < 10] + 1)
            if len(pos):
                ap[i] = np.sum(np.arange(1, len(pos) + 1) / pos) / per
        map10 = 100.0 * np.sum(ap) / len(best)
    elif mode == "t2a":
        best = r.reshape(-1)
        map10 = 100.0 * np.sum(1 / (best[best < 10] + 1)) / len(best)
    else:
        raise ValueError("metrics_from_ranks: mode 'a2t' or 't2a'")
    n = len(best)
    out = (100.0 * np.count_nonzero(best < 1) / n, 100.0 * np.count_nonzero(best < 5) / n,
           100.0 * np.count_nonzero(best < 10) / n, 100.0 * np.count_nonzero(best < 50) / n,
           np.floor(np.median(best)) + 1, best.mean() + 1, map10)
    if return_ranks:
        return out + (best, None if top1 is None else np.asarray(top1, dtype=np.float64))
    return out


def _dev(x, device=None):
    if isinstance(x, torch.Tensor):
        return x if x.is_cuda else x.to(device or "cuda")
    return torch.as_tensor(np.asarray(x)).to(device or "cuda")


def a2t(audio_embs, cap_embs, return_ranks=False, per_audio=5, dtype=None):
    """Audio-to-caption retrieval with the reference's arguments and layout
    (retrieval/tools/utils.py:169-213): audio rows repeated ``per_audio`` times, the query of clip
    i is row per_audio * i, its captions are rows per_audio * i .. per_audio * i + per_audio - 1."""
    if not 1 <= per_audio <= 8:
        raise ZsError("retrieval.a2t: 1 <= per_audio <= 8")
    a, c = _dev(audio_embs), _dev(cap_embs)
    n = a.shape[0] // per_audio
    q = a[0:n * per_audio:per_audio]
    tgt = (torch.arange(n, device=a.device, dtype=torch.int32)[:, None] * per_audio
           + torch.arange(per_audio, device=a.device, dtype=torch.int32)[None, :])
    rank, _ = rank_targets(q, c, tgt, dtype, normalize=True)
    top1 = topk(q, c, 1, dtype, normalize=True)[1][:, 0] if return_ranks else None
    return metrics_from_ranks(rank.cpu().numpy(), "a2t", return_ranks,
                              None if top1 is None else top1.cpu().numpy())


def t2a(audio_embs, cap_embs, return_ranks=False, per_audio=5, dtype=None):
    """Caption-to-audio retrieval (retrieval/tools/utils.py:216-251): every caption is a query,
    the gallery is every ``per_audio``-th audio row, caption j's target is clip j // per_audio."""
    a, c = _dev(audio_embs), _dev(cap_embs)
    n = a.shape[0] // per_audio
    g = a[0:n * per_audio:per_audio]
    q = c[:n * per_audio]
    tgt = (torch.arange(n * per_audio, device=a.device, dtype=torch.int32) // per_audio)[:, None]
    rank, _ = rank_targets(q, g, tgt, dtype, normalize=True)
    top1 = topk(q, g, 1, dtype, normalize=True)[1][:, 0] if return_ranks else None
    return metrics_from_ranks(rank.cpu().numpy()[:, 0], "t2a", return_ranks,
                              None if top1 is None else top1.cpu().numpy())


def evaluate(ase, audio_batches, texts, dtype=None):
    """``validate`` (retrieval/pretrain.py:262-284): ``audio_batches`` and ``texts`` are parallel
    iterables of device waveform batches and caption lists (5 consecutive rows per clip); the
    embeddings stay on the device.  -> {"t2a": [7 metrics], "a2t": [7 metrics]}."""
    ae, te = [], []
    for audio, text in zip(audio_batches, texts):
        ae.append(ase.encode_audio(audio).float())
        te.append(ase.encode_text(text).float())
    ae, te = torch.cat(ae, 0), torch.cat(te, 0)
    return {"t2a": list(t2a(ae, te, dtype=dtype)), "a2t": list(a2t(ae, te, dtype=dtype))}


def zero_shot_classify(audio_embs, class_embs, k=1, dtype=None):
    """ids [B, k] int32 and sims [B, k] f32 of the k best classes per clip
    (``audio_emb @ text_embeds.t()``, retrieval/zero_shot_classification.py:82-106)."""
    sims, ids = topk(audio_embs, class_embs, k, dtype)
    return ids, sims


def accuracy(ids, labels) -> float:
    """Top-1 accuracy in percent: ids [B, k] (column 0 is the prediction) against labels [B]."""
    ids = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    labels = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    return 100.0 * float(np.mean(ids.reshape(len(labels), -1)[:, 0] == labels.reshape(-1)))


def related(text_embs, bank, k=5, dtype=None):
    """idx [M, k] int32: the k captions of ``bank`` nearest to each row by cosine similarity, the
    selection of ``process_data`` (data_handing/embeddings_related_generator.py:19-28)."""
    return topk(text_embs, bank, k, dtype, normalize=True)[1]


# ------------------------------------------------------------------ command line
LINE = ("{}: r1: {:.2f}, r5: {:.2f}, r10: {:.2f}, r50: {:.2f}, medr: {:.2f}, meanr: {:.2f}, "
        "mAP10: {:.3f}")


def records_to_embeddings(records):
    """The record pickle of zsaac/extract.py (one record per clip, ``audio_embedding`` [1, K],
    ``text_embedding`` [n_captions, K]) -> the reference's layout: audio rows repeated once per
    caption, captions in order."""
    audio, text = [], []
    per = None
    for r in records:
        t = torch.as_tensor(np.asarray(r["text_embedding"]), dtype=torch.float32)
        if t.dim() != 2:
            raise ZsError(f"record {r.get('audio_id')!r} holds no text embeddings "
                          "(extract with text_or_not)")
        per = t.shape[0] if per is None else per
        if t.shape[0] != per:
            raise ZsError("records with different numbers of captions")
        a = torch.as_tensor(np.asarray(r["audio_embedding"]), dtype=torch.float32).reshape(1, -1)
        audio.append(a.expand(per, -1))
        text.append(t)
    return torch.cat(audio, 0), torch.cat(text, 0), per


def main(argv=None):
    import argparse
    import pickle
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("records")
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="f32")
    ap.add_argument("--name", default="records")
    a = ap.parse_args(argv)
    with open(a.records, "rb") as f:
        audio, text, per = records_to_embeddings(pickle.load(f))
    print(LINE.format(f"{a.name}: Caption to audio", *t2a(audio, text, per_audio=per, dtype=a.dtype)))
    print(LINE.format(f"{a.name}: Audio to caption", *a2t(audio, text, per_audio=per, dtype=a.dtype)))


if __name__ == "__main__":
    main()
