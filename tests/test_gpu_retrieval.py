"""zsaac.retrieval and the drop-in retrieval.tools.utils on the device against the golden recorded
from the reference's own a2t / t2a (tests/golden/retrieval.npz) and tests/retrieval_ref.py.

f32: ranks, top-1 and the rank-derived tuples must equal the reference's (the golden holds no tie
and every deciding float64 gap exceeds twice the tolerance: asserted on the CPU in
tests/test_retrieval_ref.py); metrics to 1e-9.  bf16: the same against the references computed
from the bf16-rounded embeddings.  zero_shot_classify / related: exact data, exact answers."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("retrieval.npz")


def _check(out, want_tuple, want_ranks, want_top1):
    assert len(out) == 9
    assert np.array_equal(np.asarray(out[7], dtype=np.float64), want_ranks)
    assert np.array_equal(np.asarray(out[8], dtype=np.float64), want_top1)
    assert np.abs(np.asarray(out[:7], dtype=np.float64) - np.asarray(want_tuple)).max() <= 1e-9


@pytest.mark.parametrize("dirn", ["a2t", "t2a"])
def test_f32_reproduces_the_reference(cuda, gold, dirn):
    from retrieval.tools import utils as U
    from zsaac import retrieval
    a, c = gold["audio_embs"], gold["cap_embs"]
    want = (gold[dirn], gold[dirn + "_ranks"], gold[dirn + "_top1"])
    # host layer: device tensors; drop-in: numpy (the reference's callers) and torch
    _check(getattr(retrieval, dirn)(torch.from_numpy(a).to(cuda), torch.from_numpy(c).to(cuda),
                                    return_ranks=True), *want)
    _check(getattr(U, dirn)(a, c, return_ranks=True), *want)
    out = getattr(U, dirn)(torch.from_numpy(a), torch.from_numpy(c))
    assert len(out) == 7 and np.abs(np.asarray(out, dtype=np.float64) - gold[dirn]).max() <= 1e-9


@pytest.mark.parametrize("dirn", ["a2t", "t2a"])
def test_bf16_against_the_rounded_reference(cuda, gold, dirn):
    """rank_targets / topk on the bf16-rounded unit rows against the float64 count on the same
    rounded values (deciding gaps > 2 tau: exact), then the metric tuples from those ranks."""
    from zsaac import retrieval
    a, c = R.golden_operands(gold, "bf16")
    _, rank, top1, tgt = R.golden_expect(a, c)[dirn]
    q, g = (a[::5], c) if dirn == "a2t" else (c, a[::5])
    got, _ = retrieval.rank_targets(q.to(cuda), g.to(cuda), tgt.to(cuda))
    assert got.dtype == torch.int32
    assert torch.equal(got.cpu().long().reshape(rank.shape), rank)
    assert torch.equal(retrieval.topk(q.to(cuda), g.to(cuda), 1)[1][:, 0].cpu().long(), top1)
    want, best = R.metrics(rank, dirn)
    out = retrieval.metrics_from_ranks(got.cpu().numpy().reshape(rank.shape), dirn, True)
    assert np.array_equal(out[7], best)
    assert np.abs(np.asarray(out[:7], dtype=np.float64) - np.asarray(want)).max() <= 1e-9
    # end to end in bf16 (device normalisation, then the cast): the same unit, recall
    e2e = getattr(retrieval, dirn)(torch.from_numpy(gold["audio_embs"]).to(cuda),
                                   torch.from_numpy(gold["cap_embs"]).to(cuda), dtype="bf16")
    print(dirn, "bf16 end to end", e2e, "rounded reference", want)
    assert len(e2e) == 7


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_zero_shot_classify_and_related_exact(cuda, dt):
    from zsaac import retrieval
    c = R.exact_case(1000, 130, 1024, 5, "ints", dt=dt)       # ties across blocks included
    q, g = c["q"].contiguous().to(cuda), c["g"].contiguous().to(cuda)
    for k in (1, 5):
        ids, sims = retrieval.zero_shot_classify(q, g, k=k)
        wv, wi = R.topk(c["sim"], k)
        assert torch.equal(ids.cpu().long(), wi) and torch.equal(sims.cpu().double(), wv)
    labels = R.topk(c["sim"], 1)[1][:, 0].clone()
    labels[::2] = -1
    assert retrieval.accuracy(retrieval.zero_shot_classify(q, g)[0], labels) == pytest.approx(50.0)
    # related: cosine, so on rows of one length -- the grid rows scaled to a common norm would not
    # stay exact; use +-1 rows (norm sqrt(K) each, a power of two: the normalised products exact)
    gen = torch.Generator().manual_seed(3)
    bank = (torch.randint(0, 2, (300, 1024), generator=gen) * 2 - 1).float()
    text = bank[torch.randperm(300, generator=gen)[:70]].clone()
    text[:, :40] = 1.0
    sim = R.matmul(text, bank) / 1024.0
    want = R.topk(sim, 5)[1]
    dtype = R.DTS[dt]
    got = retrieval.related(text.to(dtype).to(cuda), bank.to(dtype).to(cuda), k=5)
    assert torch.equal(got.cpu().long(), want)
    # chunked queries (a cap of one row's lists) give the same answer
    v1, i1 = retrieval.topk(q, g, 5)
    v2, i2 = retrieval.topk(q, g, 5, partial_bytes=1)
    assert torch.equal(i1, i2) and torch.equal(v1, v2)


def test_evaluate_mirrors_validate(cuda, gold):
    """evaluate() walks parallel audio / text batches through encode_audio / encode_text and
    returns validate's dict; the towers are stood in for by the golden's rows (batches of 3, 1
    and 36 clips), so the result must be the golden's tuples."""
    from zsaac import retrieval
    a = torch.from_numpy(gold["audio_embs"]).to(cuda)
    c = torch.from_numpy(gold["cap_embs"]).to(cuda)

    class Towers:
        def encode_audio(self, rows):
            return a[rows]

        def encode_text(self, rows):
            return c[rows]

    n = a.shape[0]
    cuts = [0, 15, 20, n]
    batches = [torch.arange(lo, hi, device=cuda) for lo, hi in zip(cuts[:-1], cuts[1:])]
    out = retrieval.evaluate(Towers(), batches, batches)
    assert sorted(out) == ["a2t", "t2a"]
    for k in out:
        assert isinstance(out[k], list) and len(out[k]) == 7
        assert np.abs(np.asarray(out[k], dtype=np.float64) - gold[k]).max() <= 1e-9


def test_cli_on_a_record_pickle(cuda, gold, tmp_path):
    """python -m zsaac.retrieval on records in zsaac/extract.py's format prints log_results' two
    lines with the golden's numbers."""
    a, c = gold["audio_embs"], gold["cap_embs"]
    recs = [{"audio_embedding": torch.from_numpy(a[5 * i:5 * i + 1]), "caption": ["x"] * 5,
             "text_embedding": torch.from_numpy(c[5 * i:5 * i + 5]), "audio_id": f"clip{i}"}
            for i in range(a.shape[0] // 5)]
    path = tmp_path / "data.pkl"
    with open(path, "wb") as f:
        pickle.dump(recs, f)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "zero-shot-aac_amd"))
    r = subprocess.run([sys.executable, "-m", "zsaac.retrieval", str(path), "--dtype", "f32",
                        "--name", "golden"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    fmt = ("golden: {}: r1: {:.2f}, r5: {:.2f}, r10: {:.2f}, r50: {:.2f}, medr: {:.2f}, "
           "meanr: {:.2f}, mAP10: {:.3f}")
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == fmt.format("Caption to audio", *gold["t2a"])
    assert lines[-1] == fmt.format("Audio to caption", *gold["a2t"])
