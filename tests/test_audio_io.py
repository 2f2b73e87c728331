"""CPU: zsaac.audio_io -- the WAV decoder against files written by stdlib ``wave`` and by hand
(what ``wave`` cannot write: float, EXTENSIBLE, extra chunks, wrong sizes), soundfile's sample
conversions, and resample_plan against resampy's length formula and the resampler's reach."""
import os
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402

from zsaac import audio_io  # noqa: E402


def _ints(rng, bits, n, ch):
    if bits == 8:
        return rng.integers(0, 256, (n, ch))
    x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), (n, ch))
    x[0, 0], x[1, 0] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1       # both ends of the range
    return x


def _expected(x, bits):
    """soundfile's float32 of integer PCM (PCM16 stays int16 here)."""
    if bits == 8:
        return ((x.astype(np.float64) - 128) / 128).astype(np.float32)
    if bits == 16:
        return x.astype(np.int16)
    return (x.astype(np.float64) / 2.0 ** (bits - 1)).astype(np.float32)


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_read_wav_stdlib_pcm(tmp_path, bits, ch):
    rng = np.random.default_rng(bits + ch)
    x = _ints(rng, bits, 101, ch)
    path = str(tmp_path / f"pcm{bits}_{ch}.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(ch)
        w.setsampwidth(bits // 8)
        w.setframerate(44100)
        w.writeframes(R.sample_bytes(x, {8: "u8", 16: "s16", 24: "s24", 32: "s32"}[bits]))
    got, sr = audio_io.read_wav(path)
    exp = _expected(x, bits)
    assert sr == 44100 and got.shape == (101, ch) and got.dtype == exp.dtype
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("kind,bits", [("f32", 32), ("f64", 64)])
def test_read_wav_float(tmp_path, kind, bits):
    x = np.random.default_rng(bits).uniform(-1, 1, (77, 2))
    path = str(tmp_path / f"{kind}.wav")
    R.wav_file(path, R.sample_bytes(x, kind), 3, bits, 2, 48000)
    got, sr = audio_io.read_wav(path)
    assert sr == 48000 and got.dtype == np.float32 and np.array_equal(got, x.astype(np.float32))


def test_read_wav_extensible_chunks_and_wrong_sizes(tmp_path):
    rng = np.random.default_rng(9)
    s = _ints(rng, 16, 33, 3)
    # EXTENSIBLE PCM16, a LIST chunk and an odd-sized chunk before data, a chunk after it
    p1 = str(tmp_path / "ext_pcm.wav")
    R.wav_file(p1, R.sample_bytes(s, "s16"), 1, 16, 3, 22050, extensible=True,
               before=[(b"LIST", b"INFOISFT\x05\x00\x00\x00abcd\x00\x00"), (b"odd ", b"xyz")],
               after=[(b"cue ", b"\0" * 4)])
    got, sr = audio_io.read_wav(p1)
    assert sr == 22050 and got.dtype == np.int16 and np.array_equal(got, s)
    # EXTENSIBLE float32 whose data size says 0 (a streamed writer never went back)
    f = rng.uniform(-1, 1, (20, 1))
    p2 = str(tmp_path / "ext_f32.wav")
    R.wav_file(p2, R.sample_bytes(f, "f32"), 3, 32, 1, 96000, extensible=True, data_size=0)
    got, sr = audio_io.read_wav(p2)
    assert sr == 96000 and np.array_equal(got, f.astype(np.float32))
    # a data size larger than the file: clamped to the file (whole frames only)
    p3 = str(tmp_path / "long.wav")
    R.wav_file(p3, R.sample_bytes(s, "s16") + b"\x01", 1, 16, 3, 8000, data_size=1 << 30)
    got, sr = audio_io.read_wav(p3)
    assert sr == 8000 and np.array_equal(got, s)


def test_non_wav_raises(tmp_path):
    for name, body, word in (("a.flac", b"fLaC" + b"\0" * 64, "FLAC"), ("b.mp3", b"ID3\x04" + b"\0" * 64, "MP3"),
                             ("c.ogg", b"OggS" + b"\0" * 64, "Ogg"), ("d.bin", b"\x01\x02", "not a RIFF/WAVE")):
        p = tmp_path / name
        p.write_bytes(body)
        with pytest.raises(ValueError, match=word):
            audio_io.read_wav(str(p))
    # a WAV of a codec that is not decoded (tag 2: ADPCM) names its tag
    p = str(tmp_path / "adpcm.wav")
    R.wav_file(p, b"\0" * 64, 2, 4, 1, 8000)
    with pytest.raises(ValueError, match="0x2"):
        audio_io.read_wav(p)


def test_resample_pack_host_checks_need_no_gpu():
    """zs_resample_pack validates its host arrays before it touches the device: bad arguments
    come back as -1 with a message on a machine without a GPU too (pointers are never read)."""
    from zsaac import _lib
    lib = _lib.lib()
    dummy = np.zeros(16, np.float32).ctypes.data

    def run(fmt=0, ch=1, sr=44100, B=1, T=64, prec=9):
        a = [np.array([v], dt) for v, dt in ((0, np.int64), (50, np.int32), (ch, np.int32),
                                             (sr, np.int32), (10, np.int32))]
        return lib.zs_resample_pack(dummy, fmt, *[v.ctypes.data for v in a], B, 32000, T, dummy, 64,
                                    prec, dummy, None)
    for kw, word in ((dict(fmt=-1), "fmt"), (dict(ch=0), "channels"), (dict(sr=256001), "factor of 8"),
                     (dict(sr=0), "sr_in"), (dict(T=0), "T > 0"), (dict(sr=200000, prec=2), "step 0")):
        assert run(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())


def test_resample_plan_lengths():
    """n_out is resampy's int(n * (sr_out / sr_in)) in float64, for every length and rate."""
    for sr_in in (8000, 11025, 16000, 22050, 44100, 48000, 96000, 192000, 32000):
        for n in list(range(0, 40)) + [441, 4410, 44100, 441000, 661500, 1323000, 999983]:
            n_out, need = audio_io.resample_plan(n, sr_in, 32000, 320000)
            assert n_out == R.n_out(n, sr_in, 32000), (sr_in, n)
            assert 0 <= need <= n
    assert audio_io.resample_plan(1323000, 44100, 32000, 320000)[1] < 441000 + 200   # 30 s uploads ~10 s


@pytest.mark.parametrize("sr_in", [44100, 48000, 96000, 16000, 252000])
def test_resample_plan_reach(sr_in):
    """The first T outputs of a file computed from its first ``frames_needed`` frames equal those
    computed from the whole file, and one frame fewer would not do at the last output."""
    T = 300
    x = np.random.default_rng(sr_in).uniform(-1, 1, 8 * T * 9)
    n_out, need = audio_io.resample_plan(x.shape[0], sr_in, 32000, T)
    assert need < x.shape[0] and n_out > T
    whole = R.resample(x, sr_in, 32000, 0, T)
    assert np.array_equal(R.resample(x[:need], sr_in, 32000, 0, T), whole)
    # the reach is tight to within the slack of the formula: the ceil over T (up to
    # sr_in / sr_out + 1 frames), the + 1, and one tap between the longest and the shortest wing
    short = R.resample(x[:need - (sr_in // 32000 + 5)], sr_in, 32000, 0, T)
    assert not np.array_equal(short, whole)
