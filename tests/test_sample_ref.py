"""CPU: the float64 sampler of tests/sample_ref.py against known answers, and the input
conditions of the cases tests/test_gpu_sample_kernels.py runs (planted ties sit where intended;
at most 1/8 of any case's draws are indecisive)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as S  # noqa: E402


def test_philox_known_answers():
    for ctr, key, want in S.PHILOX_KAT:
        got = tuple(int(w) for w in S.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, [hex(g) for g in got])
    # vectorised over the counter's first word, and u inside (0, 1)
    w = S.philox4x32_10((np.arange(4), 0, 0, 0), (0, 0))[0]
    assert int(w[0]) == S.PHILOX_KAT[0][2][0] and len(set(w.tolist())) == 4
    u = S.uniform(S.SEED, np.arange(1000), 0)
    assert u.min() > 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.05
    assert not np.array_equal(u, S.uniform(S.SEED, np.arange(1000), 1))
    assert not np.array_equal(u, S.uniform(S.SEED + 1, np.arange(1000), 0))


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_is_mostly_decisive(name):
    """A condition on the inputs: over every setting of the case, at most 1/8 of the draws are
    indecisive -- in total and for each setting with at least 24 rows."""
    V, R, _ = S.CASES[name]
    total = bad = 0
    worst = 0.0
    for t, k, p in S.settings(name):
        recs = S.reference(name, t, k, p)
        n = sum(not r["decisive"] for r in recs)
        total += len(recs)
        bad += n
        worst = max(worst, n / len(recs))
        if R >= 24:
            assert n * 8 <= len(recs), (name, t, k, p, n)
    print(f"{name}: {bad} of {total} draws indecisive ({bad / total:.3%}); worst setting {worst:.3f}")
    assert bad * 8 <= total, (name, bad, total)


def test_planted_ties_sit_where_intended():
    x, V = S.case("planted")
    # row 0: the maxima are equal; top_k = 1 and a tiny top_p keep the lowest id of them
    assert all(x[0, i] == x[0, :V].max() for i in S.TIE_MAX_IDS)
    for t in S.TEMPERATURES:
        for k, p in ((1, 1.0), (0, 1e-6), (5, 1e-6)):
            r = S.reference("planted", t, k, p)[0]
            assert r["tok"] == min(S.TIE_MAX_IDS) and r["count"] == 1 and r["decisive"]
    # row 1: four larger, then four equal: top_k = 5 keeps the lowest id of the four
    o = np.sort(x[1, :V])[::-1]
    assert o[3] > o[4] == o[7] > o[8] and all(x[1, i] == o[4] for i in S.TIE_K_IDS)
    for t in S.TEMPERATURES:
        r = S.reference("planted", t, 5, 1.0)[1]
        assert sorted(np.nonzero(r["keep"])[0].tolist()) == sorted(S.TIE_K_TOP + (min(S.TIE_K_IDS),))
        assert r["k_gap"] == float("inf")
    # row 2: at T = 1, top_p = 0.8 the nucleus ends inside the seven equal tokens: six, by id
    r = S.reference("planted", 1.0, 0, 0.8)[2]
    assert sorted(np.nonzero(r["keep"])[0].tolist()) == sorted(S.TIE_P_IDS)[:6]
    assert r["p_gap"] > 4 * r["yard_p"] + 1e-6      # the cut itself is decisive
    # rows 3 and 5 hold -inf, which is never drawn; row 5's equal maxima sit beside -inf
    for row in (3, 5):
        assert np.isneginf(x[row, :V]).sum() >= V // 3
        for t, k, p in S.settings("planted"):
            r = S.reference("planted", t, k, p)[row]
            assert np.isfinite(x[row, r["tok"]]) and np.isfinite(r["logprob"])
    assert S.reference("planted", 1.0, 1, 1.0)[5]["tok"] == 401
    # row 4: the dominant token is drawn under every setting
    for t, k, p in S.settings("planted"):
        assert S.reference("planted", t, k, p)[4]["tok"] == S.DOMINANT_ID


@pytest.mark.parametrize("name", ["v5", "v64", "v1000", "planted"])
def test_top1_and_tiny_top_p_are_argmax(name):
    x, V = S.case(name)
    am = x[:, :V].argmax(1)       # numpy: the first maximum
    for t in S.TEMPERATURES:
        for k, p in ((1, 1.0), (1, 0.8), (0, 1e-6), (V + 3, 1e-6)):
            recs = S.reference(name, t, k, p)
            assert [r["tok"] for r in recs] == am.tolist()
            assert all(r["count"] == 1 for r in recs)


def test_plain_categorical_counts():
    """top_k = 0, top_p = 1: the draw is the inverse CDF at u.  Over 4096 row ids on one
    6-token row the counts equal the counts of searchsorted(cdf, u) on the same u exactly, and
    follow the probabilities."""
    x = np.float32([0.5, -1.0, 2.0, 0.0, -np.inf, 1.0])
    n = 4096
    rid = np.arange(n)
    recs = S.sample_rows(np.tile(x, (n, 1)), 6, 1.0, 0, 1.0, seed=11, step=2, row_id=rid)
    got = np.bincount([r["tok"] for r in recs], minlength=6)
    p = np.exp(x.astype(np.float64) - 2.0)
    cdf = np.cumsum(p)
    u = S.uniform(11, rid, 2)
    want = np.bincount(np.searchsorted(cdf, u * cdf[-1], side="right"), minlength=6)
    assert got.tolist() == want.tolist()
    assert got[4] == 0 and got.sum() == n
    expect = n * p / p.sum()
    assert np.abs(got - expect).max() < 5 * np.sqrt(expect.max())
    assert all(r["count"] == 6 and abs(r["mass"] - 1) < 1e-12 for r in recs)
    assert abs(recs[0]["logprob"] - np.log(p[recs[0]["tok"]] / p.sum())) < 1e-12
