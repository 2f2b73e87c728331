"""Drop-in for the retrieval metrics of retrieval/tools/utils.py:169-251: ``a2t`` and ``t2a`` with
the reference's signatures and return tuples, on the device through zsaac.retrieval (zs_sim_rank;
no similarity matrix, no host argsort).  Inputs are numpy arrays or torch tensors in the
reference's layout: ``audio_embs`` [5 n, K] with every clip's row repeated 5 times, ``cap_embs``
[5 n, K] with a clip's 5 captions in consecutive rows.  Ties sort by value descending, then index
ascending (the reference's ``np.argsort(d)[::-1]`` leaves their order unspecified).

OUT OF SCOPE: the rest of that module (wandb logging, distributed init, seeding, AverageMeter).
"""
from zsaac import retrieval as _R


def a2t(audio_embs, cap_embs, return_ranks=False):
    # audio to caption retrieval
    return _R.a2t(audio_embs, cap_embs, return_ranks=return_ranks, per_audio=5)


def t2a(audio_embs, cap_embs, return_ranks=False):
    # caption to audio retrieval
    return _R.t2a(audio_embs, cap_embs, return_ranks=return_ranks, per_audio=5)
