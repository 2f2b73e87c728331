"""zsaac/memory.py and the harness's --memory on the GPU: map2memory against the reference formula
(float64, memory_ref's derived bound), make_preds with a memory bank against make_preds on records
whose embeddings were projected beforehand (exact: a row's projection does not depend on the rows
that share the launch), and the command line."""
import json
import os
import pickle
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memory_ref as MR  # noqa: E402
from test_gpu_harness import _make_test_dir  # noqa: E402

pytestmark = pytest.mark.gpu


def test_map2memory_matches_the_formula(cuda):
    from zsaac.memory import SupportMemory, map2memory
    M, N, K = 64, 2000, 1024
    g = torch.Generator().manual_seed(MR._seed("map2memory", M, N, K))
    q, T = MR.unit_rows(M, K, g), MR.unit_rows(N, K, g)
    for dt in ("f32", "bf16"):
        qs, Ts = q.to(MR.DTS[dt]), T.to(MR.DTS[dt])
        c = MR.project(qs, Ts, 100.0, dt)
        # the four lines of the reference, in float64 on the operands as stored
        w = (100.0 * (qs.double() @ Ts.double().T)).softmax(dim=-1)
        want = w @ Ts.double()
        want = want / want.norm(dim=-1, keepdim=True)
        assert torch.allclose(c["out"], want, rtol=1e-12, atol=1e-15)
        bank = Ts.to(cuda) if dt == "f32" else SupportMemory(Ts.to(cuda), device=cuda, normalize=False)
        got = map2memory(qs.to(cuda), bank)
        torch.cuda.synchronize()
        assert got.shape == (M, K) and got.dtype == torch.float32
        r = float(((got.cpu().double() - want).abs() / c["out_tol"]).max())
        print(f"map2memory {dt}: yardstick {c['yard']:.2e} tau {c['tau']:.2e} eps {c['eps']:.2e} "
              f"min ess {float(c['ess'].min()):.1f} |err|/bound {r:.3f}")
        assert r <= 1.0


def _memory_pickles(root, n=300, K=1024):
    """Two text-embedding files in the reference's format: a list, then a stream of records."""
    g = torch.Generator().manual_seed(9)
    rows = MR.unit_rows(n, K, g) * 3.0                   # not normalised: the loader does that
    recs = [{"caption": " ".join(["word"] * (8 + i % 13)), "text_embedding": rows[i:i + 1].clone(),
             "audio_id": f"t{i}"} for i in range(n)]
    p1, p2 = os.path.join(root, "mem_a.pkl"), os.path.join(root, "mem_b.pkl")
    with open(p1, "wb") as f:
        pickle.dump(recs[:200], f)
    with open(p2, "wb") as f:
        for r in recs[200:]:
            pickle.dump(r, f)
    return [p1, p2]


def test_make_preds_with_memory_equals_projected_records(cuda, golden, tmp_path):
    from zsaac import bpe, predict, safeload
    from zsaac.memory import SupportMemory, construct_support_memory
    root = str(tmp_path)
    _, _, _, clips = _make_test_dir(root, golden)
    paths = _memory_pickles(root)
    feats = construct_support_memory(paths)
    assert feats.shape == (300, 1024)
    mem = SupportMemory(feats, dtype=torch.float32, device=cuda)
    params = predict.load_params(root)
    tok = bpe.GPT2BPE.from_dir(os.path.join(root, "tokenizer"))
    pipe, _ = predict.build_pipeline(root, params, tok, False, torch.float32, 4, cuda)
    with_mem = predict.make_preds(pipe, tok, clips, memory=mem)
    emb = safeload.stack_rows([c["audio_embedding"] for c in clips]).to(cuda)
    proj = mem.project(emb).cpu()
    assert torch.allclose(proj.norm(dim=1), torch.ones(len(clips)), atol=1e-5)
    moved = [dict(c, audio_embedding=proj[i:i + 1].clone()) for i, c in enumerate(clips)]
    beforehand = predict.make_preds(pipe, tok, moved)
    assert with_mem[0] == beforehand[0] and with_mem[1] == beforehand[1]
    assert with_mem[2] == beforehand[2]
    plain = predict.make_preds(pipe, tok, clips)
    assert list(plain[0]) == list(with_mem[0])          # same clips, in order
    # the projection moved the embeddings (the prompts' labels come from them)
    assert float((proj - torch.nn.functional.normalize(emb.cpu(), dim=-1)).abs().max()) > 1e-2


def test_main_with_memory_writes_output(cuda, golden, tmp_path):
    from zsaac import predict
    root = str(tmp_path)
    _, _, _, clips = _make_test_dir(root, golden)
    paths = _memory_pickles(root)
    argv = ["--test_dir", root, "--test_data", os.path.join(root, "test.pkl"), "--dtype", "f32",
            "--batch", "4", "--memory", *paths, "--memory_scale", "100"]
    assert predict.main(argv) == 0
    out = json.load(open(os.path.join(root, "output.txt")))["predictions"]
    assert [p["filename"] for p in out] == [c["audio_id"] for c in clips]
    assert all(isinstance(p["caption"], str) and isinstance(p["prefix"], str) for p in out)


@pytest.mark.parametrize("other", ["--magic", "--score"])
def test_memory_with_magic_or_score_is_refused(cuda, tmp_path, other, capsys):
    from zsaac import predict
    argv = ["--test_dir", str(tmp_path), "--test_data", "x.pkl", "--memory", "m.pkl", other]
    with pytest.raises(SystemExit) as e:
        predict.main(argv)
    assert e.value.code == 2
    assert "--memory" in capsys.readouterr().err
