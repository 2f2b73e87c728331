"""zs_resample_pack (csrc/frontend.hip) against tests/resample_ref.py, through the raw ABI and
through ops.resample_pack.

Criterion for every resampled output: max |gpu - float64 reference| over a clip is at most
2 x max |float32 restatement - float64 reference| on the same clip, plus 1e-7 -- the project's
customary factor over the reference's own arithmetic at the kernel's precision (the kernel sums
in another order and scales by the ratio after the sum).  Every output is compared; padding is
exactly 0; a clip already at the target rate is bit-equal to the channel mean.

The output has a guard row behind it and is filled with a sentinel.  In the flat frame buffers
float32 clips are separated by NaN and int16 clips by runs of +-32767, at odd offsets, so a read
outside a clip shows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402
from gpu_helpers import Out  # noqa: E402

pytestmark = pytest.mark.gpu
SR, T, SENT = 32000, 4096, -7.0

# (sr_in, channels, frames, int16?)                      what the clip is there for
CLIPS = [(44100, 1, 6000, True),                       # crop: 4353 outputs > T
         (11025, 1, 900, True),
         (44100, 1, 50, True),                         # shorter than a wing: both clamps at once
         (48000, 2, 1000, True),                       # int16 downmix
         (48000, 2, 3000, False),                      # pad
         (16000, 1, 1500, False),                      # upsampling
         (22050, 3, 2000, False),
         (11025, 1, 700, False),
         (96000, 2, 9000, False),
         (32000, 2, 3000, False),                      # bypass, padded
         (32000, 8, 5000, False),                      # bypass, cropped, numpy's 8-way pairwise mean
         (16000, 1, 1, False),                         # 1 frame -> 2 outputs
         (44100, 1, 50, False),                        # both clamps at once
         (44100, 1, 1, False),                         # n_out = 0: a zero row
         (44100, 2, 0, False),                         # no frames: a zero row
         (252000, 1, 21000, False)]                    # 7.875 : 1, the widest LDS span


def _call(name, *args):
    from zsaac._lib import call
    return call(name, *args, torch.cuda.current_stream().cuda_stream)


def _table(cuda):
    from zsaac import audio_io
    tab, nz, prec = audio_io.resample_filter("kaiser_best")
    return torch.from_numpy(tab).to(cuda), nz, prec


def _group(clips, int16, rng):
    """One flat buffer of the group's clips with a gap in front of each (odd offsets) and one
    behind the last; -> (flat, offsets, frames per clip)."""
    parts, offs, frames, pos = [], [], [], 0
    for k, (sr, ch, n, _) in enumerate(clips):
        gap = 2 * k + 1 + (pos % 2)                    # makes the clip's offset odd
        if int16:
            parts.append((32767 * (1 - 2 * (np.arange(gap) % 2))).astype(np.int16))
            x = rng.integers(-32768, 32768, (n, ch)).astype(np.int16)
        else:
            parts.append(np.full(gap, np.nan, np.float32))
            x = rng.uniform(-1, 1, (n, ch)).astype(np.float32)
        pos += gap
        assert pos % 2 == 1
        offs.append(pos)
        frames.append(x)
        parts.append(x.reshape(-1))
        pos += x.size
    parts.append(parts[0][:1])
    return np.concatenate(parts), np.array(offs, np.int64), frames


def _meta(clips, frames):
    return (np.array([f.shape[0] for f in frames], np.int32), np.array([c[1] for c in clips], np.int32),
            np.array([c[0] for c in clips], np.int32),
            np.array([R.n_out(f.shape[0], c[0], SR) for c, f in zip(clips, frames)], np.int32))


@pytest.fixture(scope="module")
def batch():
    """The mixed batch and its references, computed once: per group the flat buffer and the
    metadata, per clip the float64 row and the float32 yardstick row."""
    rng = np.random.default_rng(2024)
    groups = []
    for int16 in (True, False):
        clips = [c for c in CLIPS if c[3] == int16]
        flat, offs, frames = _group(clips, int16, rng)
        groups.append(dict(clips=clips, flat=flat, offs=offs, frames=frames, meta=_meta(clips, frames)))
    for g in groups:
        g["ref64"] = [R.load_row(f, c[0], SR, T) for c, f in zip(g["clips"], g["frames"])]
        g["ref32"] = [R.load_row(f, c[0], SR, T, dtype=np.float32) for c, f in zip(g["clips"], g["frames"])]
    return groups


def _check_row(name, got, ref64, ref32, sr_in, n_valid):
    got = got.numpy()
    assert not got[n_valid:].any() and np.array_equal(np.signbit(got[n_valid:]), np.zeros(T - n_valid, bool)), \
        f"{name}: padding is not exactly 0"
    if sr_in == SR:
        assert np.array_equal(got, ref32), f"{name}: bypass is not the channel mean, bit for bit"
        return 0.0
    yard = float(np.abs(ref32.astype(np.float64) - ref64).max(initial=0.0))
    err = float(np.abs(got.astype(np.float64) - ref64).max(initial=0.0))
    tol = 2 * yard + 1e-7
    print(f"{name}: error {err:.3e}, yardstick {yard:.3e}, tolerance {tol:.3e}")
    assert np.isfinite(got).all() and err <= tol, f"{name}: error {err:.3e} > {tol:.3e} (yardstick {yard:.3e})"
    return err


def _run(cuda, batch, through_ops):
    from zsaac import ops
    tab, nz, prec = _table(cuda)
    B = sum(len(g["clips"]) for g in batch)
    out = Out(cuda, (B, T), torch.float32, SENT)
    row, keep = 0, []
    for g in batch:
        fd = torch.from_numpy(g["flat"]).to(cuda)
        nf, ch, sr, no = g["meta"]
        keep.append(fd)
        if through_ops:
            ops.resample_pack(fd, g["offs"], nf, ch, sr, no, SR, T, tab, nz, prec, out.t[row:])
        else:
            _call("zs_resample_pack", fd.data_ptr(), int(g["flat"].dtype == np.int16), g["offs"].ctypes.data,
                  nf.ctypes.data, ch.ctypes.data, sr.ctypes.data, no.ctypes.data, len(nf), SR, T,
                  tab.data_ptr(), nz, prec, out.t[row:].data_ptr())
        row += len(nf)
    torch.cuda.synchronize()
    return out.cpu()


def test_mixed_batch_abi(cuda, batch):
    """Every clip of the mixed batch through the raw entry point: the criterion of the module
    docstring on every output, zero padding, bit-exact bypass, the guard row untouched."""
    got = _run(cuda, batch, False)
    row = 0
    for g in batch:
        for c, f, r64, r32 in zip(g["clips"], g["frames"], g["ref64"], g["ref32"]):
            name = f"{c[0]} Hz x{c[1]} {'s16' if c[3] else 'f32'} {c[2]} frames"
            _check_row(name, got[row], r64, r32, c[0], min(R.n_out(c[2], c[0], SR), T))
            row += 1
    # the cases the batch is built for are in it
    n_outs = [R.n_out(c[2], c[0], SR) for c in CLIPS]
    assert max(n_outs) > T and 0 in n_outs and any(c[2] < 64 * c[0] / SR and c[2] > 1 for c in CLIPS)
    assert all(int(o) % 2 == 1 for g in batch for o in g["offs"])


def test_mixed_batch_ops(cuda, batch):
    """ops.resample_pack launches the same kernel on the same arguments: bit-equal rows."""
    assert torch.equal(_run(cuda, batch, True), _run(cuda, batch, False))


def test_late_outputs(cuda):
    """A 10 s clip at 44.1 kHz, T = 320000: t * sr_in passes 2^31 near t = 48700 and a float32
    time register has 5 fractional bits left at the end.  Outputs [48000, 50000) and the last
    4096 meet the criterion (the reference computed for those ranges only); the row is finite."""
    Tl, sr_in, n = 320000, 44100, 441000
    x = np.random.default_rng(7).uniform(-1, 1, (n, 1)).astype(np.float32)
    tab, nz, prec = _table(cuda)
    out = Out(cuda, (1, Tl), torch.float32, SENT)
    fd = torch.from_numpy(x.reshape(-1)).to(cuda)
    no = R.n_out(n, sr_in, SR)
    assert no in (Tl - 1, Tl)
    a = [np.array([v], dt) for v, dt in ((0, np.int64), (n, np.int32), (1, np.int32), (sr_in, np.int32), (no, np.int32))]
    _call("zs_resample_pack", fd.data_ptr(), 0, *[v.ctypes.data for v in a], 1, SR, Tl, tab.data_ptr(),
          nz, prec, out.t.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu()[0].numpy()
    assert np.isfinite(got).all() and not got[no:].any()
    for t0, t1 in ((48000, 50000), (Tl - 4096, Tl)):
        r64 = R.load_row(x, sr_in, SR, Tl, t0, t1)
        r32 = R.load_row(x, sr_in, SR, Tl, t0, t1, dtype=np.float32)
        yard = float(np.abs(r32.astype(np.float64) - r64).max())
        err = float(np.abs(got[t0:t1].astype(np.float64) - r64).max())
        print(f"late [{t0}, {t1}): error {err:.3e}, yardstick {yard:.3e}, tolerance {2 * yard + 1e-7:.3e}")
        assert err <= 2 * yard + 1e-7, (t0, t1, err, yard)
    assert (48000 * sr_in < 2 ** 31 < 50000 * sr_in)


def test_prefix_upload_is_enough(cuda):
    """audio_io.resample_plan: a 30 s stereo int16 clip's first T outputs computed from its
    first ``frames_needed`` frames equal those computed from the whole clip, bit for bit."""
    from zsaac import audio_io
    sr_in, n = 44100, 3 * T
    x = np.random.default_rng(8).integers(-32768, 32768, (n, 2)).astype(np.int16)
    n_out, need = audio_io.resample_plan(n, sr_in, SR, T)
    assert n_out > T and need < n
    tab, nz, prec = _table(cuda)
    rows = []
    for frames in (x, x[:need]):
        out = Out(cuda, (1, T), torch.float32, SENT)
        fd = torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).to(cuda)
        a = [np.array([v], dt) for v, dt in ((0, np.int64), (frames.shape[0], np.int32), (2, np.int32),
                                             (sr_in, np.int32), (n_out, np.int32))]
        _call("zs_resample_pack", fd.data_ptr(), 1, *[v.ctypes.data for v in a], 1, SR, T, tab.data_ptr(),
              nz, prec, out.t.data_ptr())
        torch.cuda.synchronize()
        rows.append(out.cpu())
    assert torch.equal(rows[0], rows[1])


def test_host_checks_refuse(cuda):
    """A bad fmt, channels = 0 and sr_in > 8 sr_out (and the other way round, a NULL buffer,
    B = 0) return -1 with a message before any launch: the sentinel-filled output stays as it is."""
    from zsaac import _lib
    tab, nz, prec = _table(cuda)
    out = Out(cuda, (2, 64), torch.float32, SENT)
    fd = torch.zeros(256, device=cuda)
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream

    def run(fmt=0, ch=(1, 1), sr=(44100, 16000), B=2, frames=fd.data_ptr()):
        a = [np.array(v, dt) for v, dt in (([0, 100], np.int64), ([50, 50], np.int32), (ch, np.int32),
                                           (sr, np.int32), ([10, 10], np.int32))]
        return lib.zs_resample_pack(frames, fmt, *[v.ctypes.data for v in a], B, SR, 64, tab.data_ptr(),
                                    nz, prec, out.t.data_ptr(), st)
    for kw, word in ((dict(fmt=2), "fmt"), (dict(ch=(1, 0)), "channels"), (dict(ch=(9, 1)), "channels"),
                     (dict(sr=(44100, 256001)), "factor of 8"), (dict(sr=(3999, 44100)), "factor of 8"),
                     (dict(frames=None), "NULL"), (dict(B=0), "B > 0")):
        assert run(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENT).all())
    assert run() == 0                                  # the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool((out.cpu() != SENT).all())
