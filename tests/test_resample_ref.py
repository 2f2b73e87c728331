"""CPU: the numpy restatement of librosa.load's resampler (tests/resample_ref.py) is anchored,
since librosa / resampy cannot be run here: the vectorised form equals a literal transcription
of resampy's resample_f loop, the table has resampy's shape, and a resampled sine is the sine at
the new rate.  The package's own table builder (zsaac.audio_io.resample_filter) is held to the
same table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402

SR_OUT = 32000


@pytest.mark.parametrize("sr_in", [44100, 48000, 16000, 11025])
def test_vectorised_equals_scalar_transcription(sr_in):
    x = np.random.default_rng(sr_in).uniform(-1, 1, 400)
    ref = R.resample_scalar(x, sr_in, SR_OUT)
    got = R.resample(x, sr_in, SR_OUT)
    assert got.shape == ref.shape and ref.shape[0] == int(400 * (float(SR_OUT) / sr_in))
    err = float(np.abs(got - ref).max())
    print(f"{sr_in} -> {SR_OUT}: vectorised vs scalar {err:.3e}")
    assert err <= 1e-12
    # any range of outputs on its own equals that range of the whole
    assert np.array_equal(R.resample(x, sr_in, SR_OUT, 37, 113), got[37:113])


def test_short_clip_both_clamps():
    """A clip shorter than one wing: both loop bounds bind on every output."""
    x = np.random.default_rng(5).uniform(-1, 1, 50)
    assert 50 < 64 / (SR_OUT / 44100)
    assert float(np.abs(R.resample(x, 44100, SR_OUT) - R.resample_scalar(x, 44100, SR_OUT)).max()) <= 1e-12


def test_table():
    win, delta = R.filter_table()
    assert win.shape == (32769,) and delta.shape == (32769,)
    assert win[0] == R.ROLLOFF and delta[-1] == 0.0
    assert np.array_equal(delta[:-1], win[1:] - win[:-1])
    from zsaac import audio_io
    tab, nz, prec = audio_io.resample_filter("kaiser_best")
    assert (nz, prec) == (64, 9) and tab.shape == (32769, 2) and tab.dtype == np.float32
    assert np.array_equal(tab[:, 0], win.astype(np.float32))
    assert np.array_equal(tab[:, 1], delta.astype(np.float32))
    with pytest.raises(ValueError):
        audio_io.resample_filter("kaiser_fast")


@pytest.mark.parametrize("sr_in,bound", [(44100, 1e-3), (48000, 1e-3), (16000, 1e-6), (22050, 1e-6)])
def test_sine_is_the_sine_at_the_new_rate(sr_in, bound):
    """10 s of a 0.5-amplitude 1 kHz sine: away from the edges the resampled signal is the same
    sine sampled at 32 kHz.  Downsampling carries the gain error of resampy's truncated table
    step (int(scale * 512) / (scale * 512)); upsampling does not."""
    f0, amp = 1000.0, 0.5
    x = amp * np.sin(2 * np.pi * f0 * np.arange(10 * sr_in) / sr_in)
    y = R.resample(x, sr_in, SR_OUT)
    assert y.shape[0] == R.n_out(x.shape[0], sr_in, SR_OUT)
    t = np.arange(y.shape[0])
    ideal = amp * np.sin(2 * np.pi * f0 * t / SR_OUT)
    err = float(np.abs(y - ideal)[2000:-2000].max())
    print(f"{sr_in} -> {SR_OUT}: sine error {err:.3e} (bound {bound:g})")
    assert err <= bound


def test_f32_twin_is_close_and_not_identical():
    """The float32 twin (the GPU tests' yardstick) deviates from float64 by float32 rounding only."""
    x = np.random.default_rng(3).uniform(-1, 1, 3000).astype(np.float32)
    for sr_in in (44100, 16000):
        d = float(np.abs(R.resample(x, sr_in, SR_OUT, dtype=np.float32).astype(np.float64)
                         - R.resample(x, sr_in, SR_OUT)).max())
        print(f"{sr_in}: float32 twin vs float64 {d:.3e}")
        assert 0 < d < 1e-5


def test_downmix_is_numpy_mean():
    rng = np.random.default_rng(4)
    for C in range(1, 9):
        x = rng.uniform(-1, 1, (64, C)).astype(np.float32)
        assert np.array_equal(R.downmix(x), np.mean(x.T, axis=0))       # librosa.to_mono's view
    s = rng.integers(-32768, 32768, (64, 2)).astype(np.int16)
    assert np.array_equal(R.downmix(s), ((s[:, 0] / 32768.0 + s[:, 1] / 32768.0) / 2).astype(np.float32))


def test_load_row_crop_pad_bypass():
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, (300, 2)).astype(np.float32)
    row = R.load_row(x, 44100, SR_OUT, 1000)
    nv = R.n_out(300, 44100, SR_OUT)
    assert np.array_equal(row[:nv], R.resample(R.downmix(x), 44100, SR_OUT)) and not row[nv:].any()
    assert np.array_equal(R.load_row(x, 44100, SR_OUT, 100), row[:100])
    assert np.array_equal(R.load_row(x, 44100, SR_OUT, 1000, 90, 260), row[90:260])
    by = R.load_row(x, SR_OUT, SR_OUT, 400, dtype=np.float32)
    assert np.array_equal(by[:300], R.downmix(x)) and not by[300:].any()
