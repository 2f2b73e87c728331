"""zs_resample_windows (csrc/frontend.hip) and zs_window_stitch (csrc/longform.hip) against
tests/longform_ref.py, through the raw ABI and through ops.

Resampling: every window row is BIT-EQUAL to the same outputs of zs_resample_pack run on the
same buffer with T_big = (n_win - 1) * hop + T, and meets the criterion of
tests/test_gpu_resample.py against the float64 reference (max error over a row at most 2 x the
float32 restatement's own error on that row, plus 1e-7); padding is exactly +0.

Stitch: within 4 x float32 yardstick + 1e-6 of the float64 reference (max norm); entries with
one term, the one-window embedding and every clip maximum are bit-equal to their inputs.

Outputs are sentinel-filled with a guard row behind them; padding columns of the inputs hold
NaN, those of the outputs must keep the sentinel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_ref as L  # noqa: E402
import resample_ref as R  # noqa: E402
from gpu_helpers import Out  # noqa: E402
from test_gpu_resample import _call, _group, _table  # noqa: E402

pytestmark = pytest.mark.gpu
SR, T, SENT = 32000, 1536, -7.0

# (sr_in, channels, frames, int16?)
RECS = [(44100, 2, 9000, True),                        # 6530 outputs: several windows, a partial last one
        (48000, 1, 700, True),                         # 466 outputs < T: one window
        (16000, 1, 2500, False),                       # upsampling
        (32000, 3, 4000, False),                       # bypass
        (44100, 2, 0, False)]                          # empty: n_win = 0, writes no row


@pytest.fixture(scope="module")
def recs():
    """The two format groups (flat buffers with odd offsets and poisoned gaps) and, per
    recording, the whole-file float64 / float32 reference rows, computed once."""
    rng = np.random.default_rng(77)
    groups = []
    for int16 in (True, False):
        clips = [c for c in RECS if c[3] == int16]
        flat, offs, frames = _group(clips, int16, rng)
        n_out = [R.n_out(f.shape[0], c[0], SR) for c, f in zip(clips, frames)]
        big = [n + 2 * T for n in n_out]
        groups.append(dict(
            clips=clips, flat=flat, offs=offs, frames=frames, n_out=n_out,
            ref64=[R.load_row(f, c[0], SR, b) for c, f, b in zip(clips, frames, big)],
            ref32=[R.load_row(f, c[0], SR, b, dtype=np.float32) for c, f, b in zip(clips, frames, big)]))
    assert all(int(o) % 2 == 1 for g in groups for o in g["offs"])
    return groups


def _meta(g, hop):
    from zsaac.longform import window_plan
    i32 = lambda v: np.array(v, np.int32)  # noqa: E731
    return (i32([f.shape[0] for f in g["frames"]]), i32([c[1] for c in g["clips"]]),
            i32([c[0] for c in g["clips"]]), i32(g["n_out"]),
            i32([window_plan(n, T, hop)[0] for n in g["n_out"]]))


def _windows(cuda, g, hop, through_ops, tab, nz, prec):
    from zsaac import ops
    nf, ch, sr, no, nw = _meta(g, hop)
    rows = int(nw.sum())
    out = Out(cuda, (rows, T), torch.float32, SENT)
    fd = torch.from_numpy(g["flat"]).to(cuda)
    if through_ops:
        ops.resample_windows(fd, g["offs"], nf, ch, sr, no, nw, SR, T, hop, tab, nz, prec, out.t)
    else:
        _call("zs_resample_windows", fd.data_ptr(), int(g["flat"].dtype == np.int16), g["offs"].ctypes.data,
              nf.ctypes.data, ch.ctypes.data, sr.ctypes.data, no.ctypes.data, nw.ctypes.data, len(nf),
              SR, T, hop, tab.data_ptr(), nz, prec, out.t.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), nw


def _pack(cuda, g, T_big, tab, nz, prec):
    nf, ch, sr, no, _ = _meta(g, T)
    out = Out(cuda, (len(nf), T_big), torch.float32, SENT)
    fd = torch.from_numpy(g["flat"]).to(cuda)
    _call("zs_resample_pack", fd.data_ptr(), int(g["flat"].dtype == np.int16), g["offs"].ctypes.data,
          nf.ctypes.data, ch.ctypes.data, sr.ctypes.data, no.ctypes.data, len(nf), SR, T_big,
          tab.data_ptr(), nz, prec, out.t.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_row(name, got, ref64, ref32, sr_in, n_valid):
    """tests/test_gpu_resample.py::_check_row for a row of any length."""
    n = got.shape[0]
    assert not got[n_valid:].any() and not np.signbit(got[n_valid:]).any(), f"{name}: padding is not exactly +0"
    if sr_in == SR:
        assert np.array_equal(got, ref32), f"{name}: bypass is not the channel mean, bit for bit"
        return
    yard = float(np.abs(ref32.astype(np.float64) - ref64).max(initial=0.0))
    err = float(np.abs(got.astype(np.float64) - ref64).max(initial=0.0))
    tol = 2 * yard + 1e-7
    assert np.isfinite(got).all() and err <= tol, f"{name}: error {err:.3e} > {tol:.3e} (yardstick {yard:.3e})"
    assert n == ref64.shape[0]


@pytest.mark.parametrize("hop", [48, 768, 1536])
def test_window_rows(cuda, recs, hop):
    tab, nz, prec = _table(cuda)
    worst = 0.0
    for g in recs:
        got, nw = _windows(cuda, g, hop, False, tab, nz, prec)
        assert np.array_equal(_windows(cuda, g, hop, True, tab, nz, prec)[0], got), "ops != raw call"
        T_big = int(max((nw.max() - 1) * hop + T, T))
        pack = _pack(cuda, g, T_big, tab, nz, prec)
        row = 0
        for r, (c, n_out) in enumerate(zip(g["clips"], g["n_out"])):
            assert nw[r] == L.window_plan(n_out, T, hop)[0]
            for w in range(nw[r]):
                name = f"hop {hop}: {c[0]} Hz x{c[1]} window {w}"
                a, nv = w * hop, max(0, min(T, n_out - w * hop))
                assert np.array_equal(got[row].view(np.int32), pack[r, a:a + T].view(np.int32)), \
                    f"{name}: not bit-equal to zs_resample_pack's outputs [{a}, {a + T})"
                _check_row(name, got[row], g["ref64"][r][a:a + T], g["ref32"][r][a:a + T], c[0], nv)
                worst = max(worst, float(np.abs(got[row] - g["ref64"][r][a:a + T]).max()))
                row += 1
        assert row == got.shape[0]
    print(f"hop {hop}: worst |gpu - float64| {worst:.3e}")
    assert T % 1024 != 0                               # the row is no multiple of the kernel's tile


def test_reference_rows_are_slices(recs):
    """longform_ref.window_rows (load_row per window) is the whole-file reference row cut up."""
    g = recs[0]
    rows = L.window_rows(g["frames"][0], g["clips"][0][0], SR, T, 768)
    assert rows.shape == (L.window_plan(g["n_out"][0], T, 768)[0], T) and rows.shape[0] > 2
    for w in range(rows.shape[0]):
        assert np.array_equal(rows[w], g["ref64"][0][w * 768:w * 768 + T])


def test_late_window(cuda):
    """10 s at 44.1 kHz, T = 4096, hop = 300000: window 1 starts at output 300000, where
    t * sr_in is far beyond 2^31.  It meets the criterion and is bit-equal to zs_resample_pack
    at T = 320000 on the overlap."""
    Tl, hop, sr_in, n, Tp = 4096, 300000, 44100, 441000, 320000
    x = np.random.default_rng(7).uniform(-1, 1, (n, 1)).astype(np.float32)
    tab, nz, prec = _table(cuda)
    fd = torch.from_numpy(x.reshape(-1)).to(cuda)
    no = R.n_out(n, sr_in, SR)
    assert no in (Tp - 1, Tp) and hop * sr_in > 2 ** 33
    a = [np.array([v], dt) for v, dt in ((0, np.int64), (n, np.int32), (1, np.int32), (sr_in, np.int32),
                                         (no, np.int32))]
    out = Out(cuda, (2, Tl), torch.float32, SENT)
    nw = np.array([2], np.int32)                       # windows at outputs 0 and 300000
    _call("zs_resample_windows", fd.data_ptr(), 0, *[v.ctypes.data for v in a], nw.ctypes.data, 1, SR, Tl,
          hop, tab.data_ptr(), nz, prec, out.t.data_ptr())
    pack = Out(cuda, (1, Tp), torch.float32, SENT)
    _call("zs_resample_pack", fd.data_ptr(), 0, *[v.ctypes.data for v in a], 1, SR, Tp, tab.data_ptr(),
          nz, prec, pack.t.data_ptr())
    torch.cuda.synchronize()
    got, pk = out.cpu().numpy(), pack.cpu().numpy()[0]
    for w, t0 in ((0, 0), (1, hop)):
        assert np.array_equal(got[w].view(np.int32), pk[t0:t0 + Tl].view(np.int32)), w
        r64 = R.load_row(x, sr_in, SR, Tp, t0, t0 + Tl)
        r32 = R.load_row(x, sr_in, SR, Tp, t0, t0 + Tl, dtype=np.float32)
        _check_row(f"late window {w}", got[w], r64, r32, sr_in, min(Tl, no - t0))


def test_resample_windows_refuses(cuda):
    """Everything zs_resample_pack refuses, and: hop <= 0, n_win < 0, a window without a valid
    output, a last input index beyond an int, more window rows than an int: -1 with a message
    before any launch, the sentinel-filled output untouched."""
    from zsaac import _lib
    tab, nz, prec = _table(cuda)
    out = Out(cuda, (4, 64), torch.float32, SENT)
    fd = torch.zeros(256, device=cuda)
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    BIG = 2 ** 31 - 2

    def run(fmt=0, ch=(1, 1), sr=(44100, 16000), no=(36, 100), nw=(1, 2), R_=2, hop=64, frames=fd.data_ptr()):
        a = [np.array(v, dt) for v, dt in (([0, 100], np.int64), ([50, 50], np.int32), (ch, np.int32),
                                           (sr, np.int32), (no, np.int32), (nw, np.int32))]
        return lib.zs_resample_windows(frames, fmt, *[v.ctypes.data for v in a], R_, SR, 64, hop,
                                       tab.data_ptr(), nz, prec, out.t.data_ptr(), st)
    for kw, word in ((dict(fmt=2), "fmt"), (dict(ch=(1, 0)), "channels"), (dict(ch=(9, 1)), "channels"),
                     (dict(sr=(44100, 256001)), "factor of 8"), (dict(sr=(3999, 44100)), "factor of 8"),
                     (dict(frames=None), "NULL"), (dict(R_=0), "R > 0"),
                     (dict(hop=0), "hop > 0"), (dict(hop=-64), "hop > 0"),
                     (dict(nw=(1, -1)), "n_win"), (dict(nw=(1, 3)), "no valid output"),
                     (dict(nw=(2, 2)), "no valid output"),
                     (dict(sr=(64000, 16000), no=(BIG, 100)), "does not fit an int"),
                     (dict(sr=(32000, 32000), no=(BIG, BIG), nw=(2 ** 30, 2 ** 30), hop=1), "sum n_win")):
        assert run(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENT).all())
    assert run() == 0                                  # the same call with good arguments runs
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[:3] != SENT).all()) and bool((got[3] == SENT).all())


# ------------------------------------------------------------------ zs_window_stitch
def _stitch_gpu(cuda, c, N, K, ldf, rows=slice(0, 8), recs_=slice(0, 3), through_ops=False):
    """Runs the stitch on recordings ``recs_`` of case ``c`` (their window rows ``rows``).
    -> (timeline [SF, N], rec_clip [R, ldrc], rec_emb [R, K], plan) as numpy; checks the poisoned
    padding and the guards."""
    from zsaac import ops
    from zsaac.longform import stitch_tables
    n_outs = c["n_outs"][recs_]
    plan, wgt = stitch_tables(n_outs, c["T"], c["hop"])
    Rn, W, SF = len(n_outs), int(plan[:, 1].sum()), int(plan[:, 3].sum())
    hop_f = c["hop"] // (c["T"] // 32)
    ldc, lde, ldt, ldrc, ldre = N + 3, K + 8, ldf, (N + 7) // 8 * 8 + 8, K + 4
    nan = float("nan")
    frame = torch.full((W, 32, ldf), nan, device=cuda)
    frame[:, :, :N] = torch.from_numpy(c["frame"][rows]).to(cuda)
    clip = torch.full((W, ldc), nan, device=cuda)
    clip[:, :N] = torch.from_numpy(c["clip"][rows]).to(cuda)
    emb = torch.full((W, lde), nan, device=cuda)
    emb[:, :K] = torch.from_numpy(c["emb"][rows]).to(cuda)
    tl = Out(cuda, (SF, ldt), torch.float32, SENT)
    rc = Out(cuda, (Rn, ldrc), torch.float32, SENT)
    re = Out(cuda, (Rn, ldre), torch.float32, SENT)
    dplan, dwgt = torch.from_numpy(plan).to(cuda), torch.from_numpy(wgt).to(cuda)
    if through_ops:
        ops.window_stitch(dplan, plan, dwgt, hop_f, N, frame, clip, emb[:, :K], tl.t, rc.t, re.t[:, :K])
    else:
        _call("zs_window_stitch", dplan.data_ptr(), dwgt.data_ptr(), Rn, hop_f, N, frame.data_ptr(), ldf,
              clip.data_ptr(), ldc, emb.data_ptr(), lde, K, tl.t.data_ptr(), ldt, rc.t.data_ptr(), ldrc,
              re.t.data_ptr(), ldre)
    torch.cuda.synchronize()
    t, r, e = tl.cpu().numpy(), rc.cpu().numpy(), re.cpu().numpy()
    assert (t[:, N:] == SENT).all() and (e[:, K:] == SENT).all(), "padding columns written"
    assert np.isneginf(r[:, N:]).all(), "rec_clip padding is not -inf"
    return t[:, :N], r, e[:, :K], plan


@pytest.mark.parametrize("N", [1, 17, 527])
@pytest.mark.parametrize("hop_f", [32, 16, 5])
def test_stitch(cuda, hop_f, N):
    for K in (32, 1024):
        c = L.stitch_case(hop_f, N, K)
        a = (c["n_outs"], c["T"], c["hop"], c["frame"], c["clip"], c["emb"])
        ref, twin = L.stitch(*a), L.stitch(*a, dtype=np.float32)
        for ldf in (N, 528):
            tag = f"hop_f {hop_f} N {N} K {K} ldf {ldf}"
            t, r, e, plan = _stitch_gpu(cuda, c, N, K, ldf)
            for name, got, r64, r32 in (("timeline", t, ref[0], twin[0]), ("rec_clip", r[:, :N], ref[1], twin[1]),
                                        ("rec_emb", e, ref[2], twin[2])):
                yard, tol = L.tolerance(r64, r32)
                err = float(np.abs(got.astype(np.float64) - r64).max())
                print(f"{tag} {name}: error {err:.3e}, yardstick {yard:.3e}, tolerance {tol:.3e}")
                assert got.shape == r64.shape and np.isfinite(got).all() and err <= tol, (tag, name, err, tol)
            # a max has no rounding; one term and one window are copies
            assert np.array_equal(r[:, :N], twin[1]), tag
            assert np.array_equal(e[0].view(np.int32), c["emb"][0].view(np.int32)), tag
            ones = 0
            for row0, n_win, frow0, F in plan:
                for f in range(F):
                    ws = [w for w in range(n_win) if 0 <= f - w * hop_f < 32]
                    assert 1 <= len(ws) <= -(-32 // hop_f)
                    if len(ws) == 1:
                        src = c["frame"][row0 + ws[0], f - ws[0] * hop_f]
                        assert np.array_equal(t[frow0 + f].view(np.int32), src.view(np.int32)), (tag, f)
                        ones += 1
            assert ones > 0
            # recording 1 alone == recording 1 as the second of three, bit for bit
            t1, r1, e1, p1 = _stitch_gpu(cuda, c, N, K, ldf, rows=slice(1, 4), recs_=slice(1, 2))
            f0, F = int(plan[1, 2]), int(plan[1, 3])
            assert p1.tolist() == [[0, 3, 0, F]]
            assert np.array_equal(t1.view(np.int32), t[f0:f0 + F].view(np.int32)), tag
            assert np.array_equal(r1.view(np.int32), r[1:2].view(np.int32)), tag
            assert np.array_equal(e1.view(np.int32), e[1:2].view(np.int32)), tag
            # ops.window_stitch launches the same kernels on the same arguments
            to, ro, eo, _ = _stitch_gpu(cuda, c, N, K, ldf, through_ops=True)
            assert np.array_equal(to, t) and np.array_equal(ro, r) and np.array_equal(eo, e), tag
    assert c["n_outs"][2] < c["T"] + 3 * c["hop"]      # the last recording ends mid-window


def test_stitch_refuses(cuda):
    """Each refusal of include/zsaac.h: -1 with a message before any launch, outputs untouched."""
    from zsaac import _lib
    from zsaac.longform import stitch_tables
    N, K = 17, 32
    c = L.stitch_case(16, N, K)
    plan, wgt = stitch_tables(c["n_outs"], c["T"], c["hop"])
    dplan, dwgt = torch.from_numpy(plan).to(cuda), torch.from_numpy(wgt).to(cuda)
    frame = torch.from_numpy(c["frame"]).to(cuda)
    clip, emb = torch.from_numpy(c["clip"]).to(cuda), torch.from_numpy(c["emb"]).to(cuda)
    SF = int(plan[:, 3].sum())
    tl = Out(cuda, (SF, N), torch.float32, SENT)
    rc = Out(cuda, (3, 24), torch.float32, SENT)
    re = Out(cuda, (3, 4096), torch.float32, SENT)
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    P = dict(plan=dplan.data_ptr(), wgt=dwgt.data_ptr(), R=3, hop_f=16, N=N, frame=frame.data_ptr(), ldf=N,
             clip=clip.data_ptr(), ldc=N, emb=emb.data_ptr(), lde=K, K=K, timeline=tl.t.data_ptr(), ldt=N,
             rec_clip=rc.t.data_ptr(), ldrc=24, rec_emb=re.t.data_ptr(), ldre=4096)

    def run(**kw):
        a = dict(P, **kw)
        return lib.zs_window_stitch(*[a[k] for k in P], st)
    bad = [dict(R=0), dict(R=-1), dict(hop_f=0), dict(hop_f=33), dict(N=0), dict(ldf=N - 1), dict(ldt=N - 1),
           dict(ldc=N - 1), dict(ldrc=N - 1), dict(lde=K - 1), dict(ldre=K - 1), dict(K=48, lde=64),
           dict(K=2080, lde=4096), dict(K=0), dict(plan=None), dict(wgt=None), dict(frame=None),
           dict(clip=None), dict(emb=None), dict(timeline=None, rec_clip=None, rec_emb=None)]
    for kw in bad:
        assert run(**kw) == -1, kw
        assert "zs_window_stitch" in _lib.last_error(), kw
    torch.cuda.synchronize()
    assert bool((tl.cpu() == SENT).all()) and bool((rc.cpu() == SENT).all()) and bool((re.cpu() == SENT).all())
    # an input without its output is fine, and so is every single pair
    assert run() == 0 and run(timeline=None) == 0 and run(rec_clip=None, clip=None, rec_emb=None) == 0
    torch.cuda.synchronize()
    assert bool((tl.cpu() != SENT).all())
