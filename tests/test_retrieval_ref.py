"""CPU: tests/retrieval_ref.py against the golden recorded from the reference's own a2t / t2a
(tests/golden/retrieval.npz), zsaac.retrieval.metrics_from_ranks against the same tuples, the
drop-in retrieval.tools.utils, and the input conditions of the GPU cases
(tests/test_gpu_retrieval_kernels.py, tests/test_gpu_retrieval.py): exact data really is exact,
the tie cases hold ties where they claim to, the brackets of the real-valued case are tight, and
each wrong rule of retrieval_ref.RULES would change the expected ranks of at least one case.  No
kernel -- and no deliberately wrong kernel -- runs here."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden):
    return golden("retrieval.npz")


@pytest.fixture(scope="module")
def exact():
    return [R.exact_case(*c) for c in R.EXACT_CASES]


# ------------------------------------------------------------------ the golden
@pytest.mark.parametrize("dirn", ["a2t", "t2a"])
def test_ref_reproduces_the_golden(gold, dirn):
    a, c = R.golden_operands(gold, "f32")
    sim, rank, top1, _ = R.golden_expect(a, c)[dirn]
    m, best = R.metrics(rank, dirn)
    assert np.array_equal(best, gold[dirn + "_ranks"])
    assert np.array_equal(top1.numpy().astype(np.float64), gold[dirn + "_top1"])
    assert np.allclose(m, gold[dirn], rtol=0, atol=1e-12)
    assert 20.0 <= gold[dirn][0] <= 80.0                     # R@1 neither trivial nor hopeless


@pytest.mark.parametrize("dirn", ["a2t", "t2a"])
def test_metrics_from_ranks_equal_the_golden(gold, dirn):
    from zsaac.retrieval import metrics_from_ranks
    a, c = R.golden_operands(gold, "f32")
    _, rank, top1, _ = R.golden_expect(a, c)[dirn]
    out = metrics_from_ranks(rank.numpy(), dirn, return_ranks=True, top1=top1.numpy())
    assert len(out) == 9
    assert np.abs(np.asarray(out[:7], dtype=np.float64) - gold[dirn]).max() <= 1e-12
    assert np.array_equal(out[7], gold[dirn + "_ranks"])
    assert np.array_equal(out[8], gold[dirn + "_top1"])
    assert len(metrics_from_ranks(rank.numpy(), dirn)) == 7


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_golden_has_no_deciding_near_tie(gold, dt):
    """Every float64 gap that decides a recorded number -- a target's or the top-1's distance to
    every other value of its row -- exceeds tau = 4 x the float32 yardstick + 1e-6 on the operands
    the device sees, so the GPU test may ask for exact ranks; no row holds an exact tie."""
    a, c = R.golden_operands(gold, dt)
    n = a.shape[0] // 5
    for q, g, dirn in ((a[::5], c, "a2t"), (c, a[::5], "t2a")):
        sim, yard, tau = R.yardstick(q, g)
        _, _, top1, tgt = R.golden_expect(a, c)[dirn]
        assert R.min_gap(sim) > 0
        dec = np.inf
        for m in range(sim.shape[0]):
            for j in [int(x) for x in tgt[m]] + [int(top1[m])]:
                d = (sim[m] - sim[m, j]).abs()
                d[j] = np.inf
                dec = min(dec, float(d.min()))
        print(f"{dt} {dirn}: yardstick {yard:.2e} tau {tau:.2e} smallest deciding gap {dec:.2e}")
        assert dec > 2 * tau
    assert n == 40


def test_dropin_utils_signatures():
    """retrieval.tools.utils is the reference's module path; a2t / t2a keep its parameter names."""
    from retrieval.tools import utils as U
    for f in (U.a2t, U.t2a):
        p = inspect.signature(f).parameters
        assert list(p) == ["audio_embs", "cap_embs", "return_ranks"]
        assert p["return_ranks"].default is False


def test_host_layer_refuses_host_tensors():
    from zsaac import retrieval
    from zsaac._lib import ZsError
    with pytest.raises(ZsError):
        retrieval.rank_targets(torch.zeros(2, 32), torch.zeros(3, 32),
                               torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(ZsError):
        retrieval.topk(torch.zeros(2, 32), torch.zeros(3, 32), 1)


# ------------------------------------------------------------------ conditions of the GPU cases
def test_exact_cases_are_exact(exact):
    """Largest |partial sum| < 2^24 in units of the data's grid (1 for integers, 1/64 for products
    of multiples of 1/8): every f32 accumulation is exact, whatever its order, and every operand
    is a bf16 value, so bf16 and f32 kernels owe the float64 similarities bit for bit."""
    for c, spec in zip(exact, R.EXACT_CASES):
        unit = 64.0 if spec[4] == "grid" else 1.0
        assert R.max_partial_sum(c["q"], c["g"]) * unit < 2 ** 24
        assert torch.equal(c["q"].to(R.BF16).float(), c["q"].float())
        assert torch.equal(c["g"].to(R.BF16).float(), c["g"].float())
        assert torch.equal(c["sim"].float().double(), c["sim"])
        bf = R.exact_case(*spec, dt="bf16")
        assert torch.equal(bf["sim"], c["sim"]) and torch.equal(bf["rank"], c["rank"])
        assert bool(torch.isnan(c["qbuf"][:, c["K"]:]).all()) and bool(torch.isnan(c["qbuf"][-1]).all())
        assert bool(torch.isnan(c["gbuf"][:, c["K"]:]).all()) and bool(torch.isnan(c["gbuf"][-1]).all())


def test_exact_cases_cover_the_edges(exact):
    seen = set()
    sizes = {"N": set(), "M": set(), "K": set(), "T": set()}
    for c in exact:
        N, tgt = c["N"], c["tgt"]
        for k in sizes:
            sizes[k].add(c[k])
        for name, col in (("0", 0), ("127", 127), ("128", 128), ("last", N - 1), ("-1", -1), ("N", N)):
            if bool((tgt == col).any()):
                seen.add(name)
        for m in range(c["M"]):
            row = [int(x) for x in tgt[m] if 0 <= int(x) < N]
            if len(set(row)) < len(row):
                seen.add("twice")
        bad = (tgt < 0) | (tgt >= N)
        assert bool((c["rank"][bad] == -1).all()) and bool((c["tsim"][bad] == 0).all())
        assert bool((c["rank"][~bad] >= 0).all())
    assert seen == {"0", "127", "128", "last", "-1", "N", "twice"}
    assert sizes == {"N": {3, 128, 129, 1000}, "M": {1, 64, 65, 130}, "K": {64, 96, 1024},
                     "T": {1, 5, 8}}
    eq = exact[[s[4] for s in R.EXACT_CASES].index("equal")]
    ok = (eq["tgt"] >= 0) & (eq["tgt"] < eq["N"])
    assert torch.equal(eq["rank"][ok], eq["tgt"][ok].long())   # all-equal gallery: rank = index
    # ranks across the whole range, ties in most rows (integer data, K = 1024)
    big = exact[3]
    assert int(big["rank"].max()) > 900 and 0 <= int(big["rank"][big["rank"] >= 0].min()) < 20


def _tie_sides(c, m, j):
    """Columns equal to sim[m][j]: (lower same block, higher same block, lower other, higher other)."""
    eq = torch.nonzero(c["sim"][m] == c["sim"][m, j]).flatten().tolist()
    blk = j // R.LM_BN
    return (any(n < j and n // R.LM_BN == blk for n in eq), any(n > j and n // R.LM_BN == blk for n in eq),
            any(n < j and n // R.LM_BN != blk for n in eq), any(n > j and n // R.LM_BN != blk for n in eq))


def test_tie_cases_hold_ties_on_both_sides(exact):
    n = 0
    for c in exact:
        if not c["ties"]:
            continue
        rows = [m for m in range(c["M"]) if int(c["tgt"][m, 0]) == R.TIE_J]
        assert rows
        for m in rows:
            assert _tie_sides(c, m, R.TIE_J) == (True, True, True, True)
        n += 1
    assert n >= 2
    d = R.real_case("f32", dups=True)
    assert _tie_sides(d, 0, R.TIE_J) == (True, True, True, True)
    assert torch.equal(d["tgt"][0].long(), torch.tensor([100, 390, 400, 410, 900]))


@pytest.mark.parametrize("rule", R.RULES)
def test_each_wrong_rule_changes_an_expected_rank(exact, rule):
    changed = [i for i, c in enumerate(exact)
               if not torch.equal(R.ranks(c["sim"], c["tgt"], rule)[0], c["rank"])]
    print(rule, "changes cases", changed)
    assert changed


def test_group_max_changes_the_golden_metrics(gold):
    a, c = R.golden_operands(gold, "f32")
    _, rank, _, _ = R.golden_expect(a, c)["a2t"]
    assert R.metrics(rank, "a2t", group_max=True)[0] != R.metrics(rank, "a2t")[0]
    assert not np.array_equal(R.metrics(rank, "a2t", group_max=True)[1], gold["a2t_ranks"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("dups", [False, True])
def test_real_case_brackets_are_tight(dt, dups):
    """tau is a few float32 roundings; a bracket holds the values within tau of the target, so it
    is one rank wide unless another similarity falls that close (about 1045 values over a range
    of ~0.3: a chance of ~1e-2 per pair) or is an exact copy (4 copies with ``dups``).  Cap: 4
    beyond the copies."""
    c = R.real_case(dt, dups)
    width = c["hi"] - c["lo"]
    print(f"{dt} dups={dups}: yardstick {c['yard']:.2e} tau {c['tau']:.2e} "
          f"widest bracket {int(width.max()) + 1}, "
          f"{100.0 * float((width > (4 if dups else 0)).float().mean()):.1f} % wider than one value")
    assert c["yard"] < 1e-6
    assert int(width.max()) + 1 <= R.REAL_WIDTH_CAP + (4 if dups else 0)
    assert int(width.min()) >= (4 if dups else 0)
    if not dups:
        assert 0.2 <= float((c["lo"] == 0).float().mean()) <= 0.9     # a spread of ranks


def test_scripted_partials_are_well_formed():
    for nblk, kpart in ((1, 8), (3, 8), (393, 8), (3, 1)):
        pv, pi = R.scripted_partials(2, nblk, kpart, seed=nblk)
        assert bool((pi[:, -1, 5:] == R.PAD_IDX).all()) and bool((pv[:, -1, 5:] == -R.INF).all())
        real = pi != R.PAD_IDX
        assert bool((pi[real] // R.LM_BN == torch.arange(nblk)[None, :, None].expand_as(pi)[real]).all())
        v, i = R.merge_partials(pv, pi, min(8, kpart))
        # ties across blocks exist and resolve to the lower index
        assert bool(((v[:, 1:] < v[:, :-1]) | ((v[:, 1:] == v[:, :-1]) & (i[:, 1:] >= i[:, :-1]))).all())
    pv, pi = R.scripted_partials(4, 393, 8, seed=393)
    v, i = R.merge_partials(pv, pi, 8)
    assert bool((v[:, 0] == v[:, 7]).any()) and bool((i[:, 0] // R.LM_BN != i[:, 7] // R.LM_BN).any())
