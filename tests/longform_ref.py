"""Reference for zsaac.longform: the window plan, the window rows of zs_resample_windows and the
stitch of zs_window_stitch, restated in numpy independently of the package.

* :func:`window_plan` counts windows and time-line frames by walking them.
* :func:`window_rows` cuts the rows out of ``resample_ref.load_row`` of the whole recording
  (``T_big = (n_win - 1) * hop + T``), so a row is the whole-file signal's own samples.
* :func:`stitch` is the float64 reference; ``dtype=np.float32`` keeps the same order of
  operations in float32: the yardstick of tests/test_gpu_longform_kernels.py.  ``mutant`` names
  one deliberate mistake the reference must tell apart (tests/test_longform_ref.py).
* :func:`stitch_case` builds the inputs the GPU stitch cases and the mutant test share.
"""
import math

import numpy as np

import resample_ref as R

FRAMES = 32
MUTANTS = ("late", "nodiv", "max_timeline", "mean_clip", "pad_kept", "unweighted")


def window_plan(n_out, T, hop):
    """(n_win, F): windows start every ``hop`` samples until one reaches the end; a time-line
    frame counts if it starts before the end and inside some window."""
    if n_out == 0:
        return 0, 0
    frame = T // FRAMES
    n_win = 1
    while (n_win - 1) * hop + T < n_out:
        n_win += 1
    span = (n_win - 1) * (hop // frame) + FRAMES
    return n_win, sum(1 for f in range(span) if f * frame < n_out)


def tables(n_outs, T, hop, pad_kept=False):
    """plan [R, 4] (row0, n_win, frow0, F) and wgt [W] (valid samples / T) as float64."""
    plan, wgt, row0, frow0 = [], [], 0, 0
    for n in n_outs:
        n_win, F = window_plan(n, T, hop)
        if pad_kept and n_win:
            F = (n_win - 1) * (hop // (T // FRAMES)) + FRAMES
        plan.append((row0, n_win, frow0, F))
        wgt += [min(T, n - w * hop) / T for w in range(n_win)]
        row0, frow0 = row0 + n_win, frow0 + F
    return np.array(plan, np.int64).reshape(-1, 4), np.array(wgt, np.float64)


def window_rows(frames, sr_in, sr_out, T, hop, dtype=np.float64):
    """The [n_win, T] rows of one recording: slices of the whole-file row, zero past its end."""
    n_win, _ = window_plan(R.n_out(np.asarray(frames).shape[0], sr_in, sr_out), T, hop)
    T_big = (n_win - 1) * hop + T
    return np.stack([R.load_row(frames, sr_in, sr_out, T_big, w * hop, w * hop + T, dtype=dtype)
                     for w in range(n_win)]) if n_win else np.zeros((0, T), dtype)


def stitch(n_outs, T, hop, frame=None, clip=None, emb=None, dtype=np.float64, mutant=None):
    """-> (timeline [sum F, N], rec_clip [R, N], rec_emb [R, K]); an absent input gives None.
    Sums run in ascending window order in ``dtype``."""
    assert mutant is None or mutant in MUTANTS
    hop_f = hop // (T // FRAMES)
    plan, wgt = tables(n_outs, T, hop, pad_kept=mutant == "pad_kept")
    shift = 1 if mutant == "late" else 0
    timeline = rec_clip = rec_emb = None
    if frame is not None:
        fr = np.asarray(frame).astype(dtype)
        timeline = np.zeros((int(plan[:, 3].sum()), fr.shape[2]), dtype)
        for row0, n_win, frow0, F in plan:
            for f in range(F):
                terms = [fr[row0 + w, f - w * hop_f - shift] for w in range(n_win)
                         if 0 <= f - w * hop_f - shift < FRAMES]
                if not terms:                      # only a mutant leaves a frame uncovered
                    continue
                if mutant == "max_timeline":
                    timeline[frow0 + f] = np.max(terms, axis=0)
                    continue
                s = terms[0].copy()
                for t in terms[1:]:
                    s = (s + t).astype(dtype)
                if len(terms) > 1 and mutant != "nodiv":
                    s = (s / dtype(len(terms))).astype(dtype)
                timeline[frow0 + f] = s
    if clip is not None:
        cl = np.asarray(clip).astype(dtype)
        rec_clip = np.stack([(cl[r0:r0 + nw].mean(0) if mutant == "mean_clip" else cl[r0:r0 + nw].max(0))
                             for r0, nw, _, _ in plan]).astype(dtype)
    if emb is not None:
        em = np.asarray(emb).astype(dtype)
        rec_emb = np.zeros((len(plan), em.shape[1]), dtype)
        for r, (r0, nw, _, _) in enumerate(plan):
            if nw == 1:
                rec_emb[r] = em[r0]
                continue
            s = np.zeros(em.shape[1], dtype)
            for w in range(nw):
                g = dtype(1.0) if mutant == "unweighted" else dtype(wgt[r0 + w])
                s = (s + (g * em[r0 + w]).astype(dtype)).astype(dtype)
            norm = np.sqrt(np.sum(s * s, dtype=dtype), dtype=dtype)
            rec_emb[r] = s / max(norm, dtype(1e-12))
    return timeline, rec_clip, rec_emb


def stitch_case(hop_f, N, K, T=320, seed=0):
    """Three recordings with 1, 3 and 4 windows: the first shorter than a window (padded frames
    even alone), the second ending exactly with its last window, the third mid-window.
    -> dict(n_outs, T, hop, frame [8, 32, N], clip [8, N], emb [8, K]) float32, probabilities in
    (0, 1), unit embedding rows."""
    frame_len = T // FRAMES
    hop = hop_f * frame_len
    n_outs = [int(0.6 * T), T + 2 * hop, T + 2 * hop + max(hop // 2 - 3, 1)]
    assert [window_plan(n, T, hop)[0] for n in n_outs] == [1, 3, 4]
    rng = np.random.default_rng(1000 * hop_f + 10 * N + K + seed)
    W = 8
    emb = rng.standard_normal((W, K)).astype(np.float32)
    emb /= np.linalg.norm(emb.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    return dict(n_outs=n_outs, T=T, hop=hop, frame=rng.uniform(0, 1, (W, FRAMES, N)).astype(np.float32),
                clip=rng.uniform(0, 1, (W, N)).astype(np.float32), emb=emb)


def tolerance(ref64, ref32):
    """The project's bound for an f32 kernel that sums in the reference's order or another:
    4 x the float32 restatement's own error + 1e-6 (max norm)."""
    yard = float(np.abs(np.asarray(ref32, np.float64) - ref64).max(initial=0.0))
    return yard, 4 * yard + 1e-6


def covered(n_out, T, hop):
    """How many windows hold each output index [n_out] (uint16)."""
    n_win, _ = window_plan(n_out, T, hop)
    c = np.zeros(n_out, np.uint16)
    for w in range(n_win):
        c[w * hop:w * hop + T] += 1
    return c


def ceil_div(a, b):
    return int(math.ceil(a / b))
