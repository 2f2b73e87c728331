"""GPU: bench.py as the command line runs it (a fresh process): a plain run prints the contract
line alone, times exactly --steps eval batches, and --dump-outputs writes that run's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("roofline", "roofline_decode_step", "stages", "clotho_1045", "strong_scaling_proxy",
             "f32_parity_mode", "throughput_mode", "c3_beam5", "c5_mistral", "id_agreement",
             "cpu_baseline")


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(cuda, tmp_path):
    steps, warmup, B = 3, 1, 64
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", str(warmup), "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    res = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert not [k for k in SECONDARY if k in res]
    assert res["steps"] == steps and res["warmup"] == warmup and res["unit"] == "clips/s"
    # one timed repetition of `steps` batches: ms_per_step is that region / steps
    reps = res["config"]["timed_reps_s"]
    assert len(reps) == 1
    assert res["ms_per_step"] == pytest.approx(reps[0] / steps * 1e3, rel=1e-3)
    assert res["value"] == pytest.approx(steps * B / reps[0], rel=1e-3)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {"ids", "lengths", "hard_ids", "hard_len", "plen", "prefix_ids", "clap_emb"} <= set(got)
    assert all(a.dtype == np.float32 and a.shape[0] == steps * B for a in got.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 10 ** 6
    ids, ln = got["ids"], got["lengths"]
    assert ids.shape[1] == 67 and ln.min() >= 1 and ln.max() <= 67
    inside = np.arange(ids.shape[1]) < ln[:, None]
    assert (ids[inside] >= 0).all() and (ids[inside] < 50257).all() and (ids[~inside] == -1).all()
    assert int(ln.sum()) == res["config"]["tokens_rank0"]
    assert got["clap_emb"].shape == (steps * B, 1024) and np.isfinite(got["clap_emb"]).all()
    # every clip has its own seed: no two embeddings alike
    assert len(np.unique(got["clap_emb"], axis=0)) == steps * B


@pytest.mark.gpu
def test_long_job_in_runs_equals_one_run(cuda, monkeypatch):
    """A job of more than RUN_BATCHES eval batches is taken in consecutive runs over the same
    buffers, clip c reading waveform c modulo RUN_BATCHES batches.  With RUN_BATCHES 4, each of
    the 3 runs of a 12-batch job is the run of a 4-batch job on the same waveforms (same
    kernels, same shapes, same schedule), so every field equals that job's bit for bit; against
    ONE staged run of the 12 batches the ids and lengths are equal, which is what the project
    holds across schedules (the encoder there runs 128 clips per pass, not 64, so its bf16
    embeddings need not be the same bits).  The line reports its runs."""
    dev = torch.device("cuda", 0)
    args = bench.parse([])
    pipe, _, _ = bench.build(args, dev)
    B, nb = 64, 12

    def job(n_batches, warmup):
        n = n_batches * B
        _, outs, _, info = bench.run_captions(args, 1, 0, dev, pipe, n, 0, [n], args.inflight,
                                              warmup)
        return outs, info
    staged, i1 = job(nb, 1)
    assert (i1["runs"], i1["batches_per_run"], len(staged)) == (1, nb, nb)
    monkeypatch.setattr(bench, "RUN_BATCHES", 4)
    one, i0 = job(4, 1)
    assert (i0["runs"], i0["batches_per_run"], len(one)) == (1, 4, 4)
    many, i2 = job(nb, 5)
    assert (i2["runs"], i2["batches_per_run"], len(many)) == (3, 4, nb)
    assert i2["persist_gave_up"] == 0 and sum(i2["persist_grids"].values()) == nb
    for i, o in enumerate(many):
        for f in ("ids", "lengths", "hard_ids", "hard_len", "plen", "prefix_ids", "clap_emb"):
            assert torch.equal(getattr(o, f), getattr(one[i % 4], f)), (i, f)
        assert torch.equal(o.ids, staged[i % 4].ids), i
        assert torch.equal(o.lengths, staged[i % 4].lengths), i
    assert i2["tokens_rank0"] == 3 * i0["tokens_rank0"]
