"""ConcurrentRunner's slot account (zsaac.pipeline.SlotAccount), pure host logic: seeded random
sequences of admit / release over the grid lists, budgets and stream pools the runner uses."""
import random

import pytest

from zsaac.pipeline import SlotAccount, choose_persist_grid

GRIDS = ([192, 96, 48], [96, 48], [48])


@pytest.mark.parametrize("pool", [2, 8, 10])
@pytest.mark.parametrize("budget", [384, 480, 96])
@pytest.mark.parametrize("grids", GRIDS, ids=lambda g: "-".join(map(str, g)))
def test_random_admit_release(grids, budget, pool):
    """Launches in order, finishes and give-ups (workgroups released before the stream) in random
    order: the workgroups in flight never exceed the budget, no busy stream is handed out again,
    admit refuses exactly when the pool is full or choose_persist_grid's size does not fit, every
    admitted size is choose_persist_grid's, and the account ends empty."""
    rng = random.Random(1000 * budget + 10 * pool + len(grids))
    for n in list(range(1, 41)) * 3:
        acc = SlotAccount(grids, budget, pool)
        held = {}                  # stream index -> workgroups its grid still holds
        launched = 0
        while launched < n or held:
            used = sum(held.values())
            assert (acc.used, acc.busy) == (used, set(held))
            what = rng.random()
            if launched < n and what < 0.6:
                want = choose_persist_grid(used, n - launched, grids, budget)
                got = acc.admit(n - launched)
                if len(held) >= pool or used + want > budget:
                    assert got is None, (n, launched, held)
                    assert (acc.used, acc.busy) == (used, set(held)), "a refusal took something"
                    continue
                assert got is not None, (n, launched, held)
                g, k = got
                assert g == want
                assert 0 <= k < pool and k not in held, (k, held)
                held[k] = g
                launched += 1
                assert sum(held.values()) <= budget
            elif held and what < 0.7:      # a give-up: the workgroups go, the stream stays busy
                k = rng.choice(sorted(held))
                acc.release(held[k])
                held[k] = 0
            elif held:                     # a finish
                k = rng.choice(sorted(held))
                acc.release(held.pop(k), stream=k)
        assert (acc.used, acc.excl, acc.busy) == (0, 0, set())


def test_headline_first_wave():
    """The headline's case (budget 480, grids 96 / 48, 20 batches, a pool of 10 streams): ten
    grids of 48, then nothing until a release."""
    acc = SlotAccount([96, 48], 480, 10)
    first = [acc.admit(20 - i) for i in range(10)]
    assert [g for g, _ in first] == [48] * 10
    assert sorted(k for _, k in first) == list(range(10))
    assert acc.admit(10) is None
    acc.release(48, stream=3)
    assert acc.admit(10) == (48, 3)
    assert acc.admit(9) is None


def test_exclusive_workgroups():
    """The small-run path: grids take a CU per workgroup while the exclusive workgroups in
    flight fit the CUs, and a release returns them; without a cap no grid is exclusive."""
    acc = SlotAccount([96, 48], 512, 3, excl_cap=256)
    took = []
    for left in (3, 2, 1):
        g, k = acc.admit(left)
        took.append((g, k, acc.exclusive(g)))
    assert [g for g, _, _ in took] == [96, 96, 96] and [e for _, _, e in took] == [True, True, False]
    assert acc.excl == 192
    for g, k, e in took:
        acc.release(g, g if e else 0, k)
    assert (acc.used, acc.excl, acc.busy) == (0, 0, set())
    acc = SlotAccount([48], 96, 2)
    g, _ = acc.admit(1)
    assert not acc.exclusive(g) and acc.excl == 0
