"""Host-side pieces of bench.py (no GPU): eval-batch splitting and the persistent decode
roofline's algorithmic byte count."""
import bench


def test_split_batches_reference_and_balanced():
    assert bench.split_batches(1045, 64)[-1] == (1024, 1045)
    assert len(bench.split_batches(1045, 64)) == 17
    assert bench.split_batches(131, 64) == [(0, 64), (64, 128), (128, 131)]
    bal = bench.split_batches(131, 64, parts=5)
    assert [b - a for a, b in bal] == [27, 26, 26, 26, 26]
    assert bal[0][0] == 0 and bal[-1][1] == 131
    # more parts than batches of 64 never exceeds B rows; fewer parts than needed keeps <= B
    assert all(b - a <= 64 for a, b in bench.split_batches(1045, 64, parts=5))
    assert bench.split_batches(3, 64, parts=5) == [(0, 1), (1, 2), (2, 3)]


def test_split_runs_bounded_and_in_order():
    """A job is one run up to RUN_BATCHES batches, beyond it consecutive near-equal runs."""
    R = bench.RUN_BATCHES
    for n in (1, 20, R, R + 1, 3 * R, 10 * R + 7):
        runs = bench.split_runs(list(range(n)))
        assert [b for r in runs for b in r] == list(range(n))
        assert len(runs) == -(-n // R) and max(map(len, runs)) - min(map(len, runs)) <= 1
        assert max(map(len, runs)) <= R


def test_persist_launch_bytes():
    row = 12 * 2 * 768 * 2
    # 2 rows, prompt 10 and 12, 3 steps (steps 1, 2 in the launch): step t at position
    # plen - 1 + t reads that many cached keys: 10 + 11 and 12 + 13
    got = bench.persist_launch_bytes(1000, [10, 12], 3)
    assert got == 2 * 1000 + row * ((10 + 11) + (12 + 13) + 2 * 2)
    assert bench.persist_launch_bytes(1000, [10], 1) == 0


def test_plain_run_options():
    """A plain run times the steps once and measures nothing else; --full is off by default."""
    a = bench.parse(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert (a.full, a.reps, a.dump_outputs, a.steps, a.warmup) == (False, None, None, 4, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_arrays(tmp_path, monkeypatch):
    """--dump-outputs: a row per clip across eval batches, entries past a row's length -1,
    float32 files, and above the size limit the same seeded rows of every array."""
    import numpy as np
    import torch
    from zsaac.pipeline import CaptionBatch

    def batch(n, first):
        ids = torch.arange(first, first + n * 6, dtype=torch.int32).view(n, 6)
        return CaptionBatch(ids=ids, lengths=torch.full((n,), 3, dtype=torch.int32), scores=None,
                            hard_ids=torch.ones(n, 4, dtype=torch.int32),
                            hard_len=torch.full((n,), 2, dtype=torch.int32),
                            plen=torch.full((n,), 5, dtype=torch.int32),
                            prefix_ids=torch.ones(n, 7, dtype=torch.int32),
                            clap_emb=torch.ones(n, 8).bfloat16())
    arr = bench.caption_arrays([batch(2, 0), batch(1, 100)])
    assert arr["ids"].tolist() == [[0, 1, 2, -1, -1, -1], [6, 7, 8, -1, -1, -1],
                                   [100, 101, 102, -1, -1, -1]]
    assert arr["lengths"].tolist() == [3, 3, 3] and arr["clap_emb"].shape == (3, 8)
    assert arr["hard_ids"][0].tolist() == [1, 1, -1, -1]
    assert arr["prefix_ids"][2].tolist() == [1, 1, 1, 1, 1, -1, -1]
    bench.dump_arrays(str(tmp_path / "all"), arr)
    got = {f.name: np.load(f) for f in (tmp_path / "all").iterdir()}
    assert sorted(got) == sorted(k + ".npy" for k in arr)
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["ids.npy"], arr["ids"])
    row = sum(v.nbytes // 3 for v in arr.values()) + 4
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * row + 256 * (len(arr) + 1))
    for d in ("s1", "s2"):
        bench.dump_arrays(str(tmp_path / d), arr)
    s1 = {f.name: np.load(f) for f in (tmp_path / "s1").iterdir()}
    rows = s1["rows.npy"].astype(int)
    assert len(rows) == 2
    assert sum(f.stat().st_size for f in (tmp_path / "s1").iterdir()) <= bench.DUMP_MAX_BYTES
    assert np.array_equal(s1["ids.npy"], arr["ids"][rows])
    assert all(np.array_equal(v, np.load(tmp_path / "s2" / k)) for k, v in s1.items())


def test_choose_persist_grid_keeps_grids_coresident():
    """ConcurrentRunner's persistent grid choice (zsaac.pipeline.choose_persist_grid), pure host
    logic: simulated begins and finishes in random order, grids of 192 / 96 / 48 half-CU
    workgroups within a budget of workgroup slots, budget // 48 pipelines -- the workgroups in
    flight never exceed the budget, a shard of two or three batches runs its first ones on the
    largest grid, and a long run of batches takes the smallest."""
    import random
    from zsaac.pipeline import choose_persist_grid, persist_grids
    for budget in (256, 384, 512):
        for spec in ("192,96,48", "96,48", "48", "192,48"):
            grids = persist_grids(spec)
            assert grids == sorted(grids, reverse=True)
            P = budget // grids[-1]
            rng = random.Random(0)
            for n in list(range(1, 24)) * 10:
                active, nxt, chosen = {}, 0, []
                while nxt < n or active:
                    free = [i for i in range(P) if i not in active]
                    if nxt < n and free and rng.random() < 0.7:
                        g = choose_persist_grid(sum(active.values()), n - nxt, grids, budget)
                        active[free[0]] = g
                        chosen.append(g)
                        nxt += 1
                        assert sum(active.values()) <= budget, (spec, n, chosen)
                    elif active:
                        del active[rng.choice(list(active))]
            assert choose_persist_grid(0, 17, grids, budget) == grids[-1]
    g = persist_grids("192,96,48")
    assert g == [192, 96, 48]
    assert choose_persist_grid(0, 2, g, 256) == 192         # 192 + one 48 beside it
    assert choose_persist_grid(0, 3, g, 256) == 96          # 96 + two 48s
    assert choose_persist_grid(96, 2, g, 256) == 96
    assert choose_persist_grid(0, 6, g, 512) == 192
    assert choose_persist_grid(0, 5, g, 256) == 48


def test_persist_grids_env(monkeypatch):
    """An explicit spec is never overridden by the environment (ZSAAC_PERSIST_GRID applies only
    when no spec is given)."""
    from zsaac.pipeline import persist_grids
    monkeypatch.setenv("ZSAAC_PERSIST_GRID", "96")
    assert persist_grids("192,48") == [192, 48]
    assert persist_grids() == [96]
    monkeypatch.delenv("ZSAAC_PERSIST_GRID")
    monkeypatch.setenv("ZSAAC_PERSIST_GRIDS", "48,96")
    assert persist_grids() == [96, 48]
