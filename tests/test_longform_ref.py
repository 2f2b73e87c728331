"""CPU: zsaac.longform's window plan against tests/longform_ref.py and its invariants, the
reference stitch against its mutants on the GPU cases' own inputs, and tagging.segments on a
stitched time line."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_ref as L  # noqa: E402

HOP_F = (1, 5, 16, 32)


def _n_outs(T, hop):
    return [0, 1, T - 1, T, T + 1, T + hop, T + hop + 1, int(7.3 * T)]


@pytest.mark.parametrize("T", [320000, 1536])
@pytest.mark.parametrize("hop_f", HOP_F)
def test_plan_invariants(T, hop_f):
    from zsaac.longform import window_plan
    frame = T // 32
    hop = hop_f * frame
    for n_out in _n_outs(T, hop):
        n_win, F = window_plan(n_out, T, hop)
        assert (n_win, F) == L.window_plan(n_out, T, hop), (n_out, hop_f)
        if n_out == 0:
            assert (n_win, F) == (0, 0)
            continue
        assert n_win == (1 if n_out <= T else 1 + L.ceil_div(n_out - T, hop))
        # every output index lies in some window
        assert int(L.covered(n_out, T, hop).min()) >= 1, (n_out, hop_f)
        # the last window has more than T - hop valid samples (all of a short recording's)
        v_last = min(T, n_out - (n_win - 1) * hop)
        assert v_last > (T - hop if n_win > 1 else 0) and v_last >= 1
        # each time-line frame is covered by 1 .. ceil(32 / hop_f) windows and starts before the end
        cnt = np.array([sum(1 for w in range(n_win) if 0 <= f - w * hop_f < 32) for f in range(F)])
        assert cnt.min() >= 1 and cnt.max() <= L.ceil_div(32, hop_f), (n_out, hop_f)
        assert (F - 1) * frame < n_out and F <= (n_win - 1) * hop_f + 32
        # and no frame with a valid sample is left out
        assert F * frame >= n_out or F == (n_win - 1) * hop_f + 32


def test_plan_refuses_bad_hops():
    from zsaac.longform import window_plan
    for T, hop in ((320000, 0), (320000, 5000), (320000, 330000), (320000, 15000), (1000, 500)):
        with pytest.raises(ValueError):
            window_plan(10, T, hop)
    with pytest.raises(ValueError):
        window_plan(-1)


@pytest.mark.parametrize("hop_f", [32, 16, 5])
def test_stitch_tables_match_the_reference(hop_f):
    from zsaac.longform import stitch_tables
    c = L.stitch_case(hop_f, 17, 32)
    n_outs = c["n_outs"] + [0, 7]
    plan, wgt = stitch_tables(n_outs, c["T"], c["hop"])
    rp, rw = L.tables(n_outs, c["T"], c["hop"])
    assert plan.dtype == np.int32 and wgt.dtype == np.float32
    assert np.array_equal(plan, rp) and np.array_equal(wgt, rw.astype(np.float32))
    assert plan[3].tolist()[1::2] == [0, 0] and float(wgt[-1]) == np.float32(7 / c["T"])


@pytest.mark.parametrize("hop_f", [32, 16, 5])
@pytest.mark.parametrize("N,K", [(1, 32), (17, 32), (527, 1024)])
def test_reference_tells_mutants_apart(hop_f, N, K):
    """On the GPU stitch cases' own inputs every mutant is farther from the float64 reference
    than the GPU tolerance (4 x float32 yardstick + 1e-6) in the output it corrupts."""
    c = L.stitch_case(hop_f, N, K)
    a = (c["n_outs"], c["T"], c["hop"], c["frame"], c["clip"], c["emb"])
    ref = L.stitch(*a)
    twin = L.stitch(*a, dtype=np.float32)
    tols = [L.tolerance(r, t)[1] for r, t in zip(ref, twin)]
    assert all(t < 1e-4 for t in tols), tols
    which = {"late": 0, "nodiv": 0, "max_timeline": 0, "pad_kept": 0, "mean_clip": 1, "unweighted": 2}
    for m in L.MUTANTS:
        got = L.stitch(*a, mutant=m)
        if hop_f == 32 and m in ("nodiv", "max_timeline"):
            # windows that do not overlap: every frame has one term, nothing to divide or to pick
            assert np.array_equal(got[0], ref[0])
            continue
        i = which[m]
        n = min(got[i].shape[0], ref[i].shape[0])
        d = float(np.abs(got[i][:n] - ref[i][:n]).max())
        assert d > 100 * tols[i], (m, d, tols[i])
        for j in range(3):                         # and leaves the other outputs alone
            if j != i:
                assert np.array_equal(got[j], ref[j]), (m, j)


def test_segments_cross_a_window_boundary():
    """An event over time-line frames [14, 21) with hop_f = 16: window 0 sees it at its frames
    14..20, window 1 at its frames 0..4.  On the stitched line it is ONE segment; per window it
    would be two."""
    from zsaac.tagging import segments
    T, hop_f = 320, 16
    hop = hop_f * 10
    n_out = T + hop                                # 2 windows, 48 frames
    truth = np.full(48, 0.1)
    truth[14:21] = 0.9
    frame = np.stack([truth[0:32], truth[16:48]])[:, :, None].astype(np.float32)
    line = L.stitch([n_out], T, hop, frame=frame)[0][:, 0]
    assert line.shape == (48,) and np.allclose(line, truth)
    assert segments(line, 0.5) == [(14, 21, pytest.approx(0.9))]
    per_window = [segments(frame[w, :, 0], 0.5) for w in range(2)]
    assert [len(s) for s in per_window] == [1, 1] and per_window[1][0][:2] == (0, 5)
