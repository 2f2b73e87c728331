"""Reference for zs_resample_pack and zsaac.audio_io: ``librosa.load(path, sr, mono=True)`` of
librosa 0.9.2 (data_handing/embeddings_generator.py:48) restated in numpy -- soundfile's sample
conversion, ``to_mono`` (np.mean over the channels in float32) and resampy's ``resample_f`` with
the ``kaiser_best`` table -- followed by the crop / pad of lines 53-59.  librosa, resampy and
soundfile are not installed here, so tests/test_resample_ref.py anchors the restatement instead:
against a literal scalar transcription of resample_f and against the ideal band-limited answer
for a sine.

* :func:`resample` is vectorised over the outputs and computes any range ``[t0, t1)``, so late
  outputs are cheap.  ``dtype=np.float64`` is the reference; ``dtype=np.float32`` keeps the same
  loop order with the table, the weights and the accumulator in float32: the reference's
  arithmetic at the kernel's precision, the yardstick of tests/test_gpu_resample.py.  Times are
  float64 in both, as in resampy.
* :func:`resample_scalar` is the loop of resampy's resample_f, line for line.
* :func:`wav_file` writes RIFF/WAVE files byte by byte (float, EXTENSIBLE, extra chunks, wrong
  sizes: what stdlib ``wave`` cannot write).
"""
import struct

import numpy as np

NUM_ZEROS, PRECISION = 64, 9
ROLLOFF, BETA = 0.9475937167399596, 14.769656459379492   # resampy's kaiser_best


def filter_table(num_zeros=NUM_ZEROS, precision=PRECISION, rolloff=ROLLOFF, beta=BETA):
    """resampy.filters.sinc_window + the deltas of resampy.core.resample: (win, delta) float64,
    ``(num_zeros << precision) + 1`` entries, the last delta 0."""
    nb = 2 ** precision
    n = nb * num_zeros
    win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, n + 1)) * np.kaiser(2 * n + 1, beta)[n:]
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return win, delta


_TABLE = {}


def _table():
    if "t" not in _TABLE:
        _TABLE["t"] = filter_table()
    return _TABLE["t"]


def n_out(n_frames, sr_in, sr_out):
    """resampy.resample's output length (librosa's fix_length to the ceil only appends a zero)."""
    if sr_in == sr_out:
        return int(n_frames)
    return int(n_frames * (float(sr_out) / sr_in))


def to_float(frames):
    """soundfile's float32 view of decoded samples: int16 / 32768, float32 as is."""
    frames = np.asarray(frames)
    if frames.dtype == np.int16:
        return frames.astype(np.float32) / np.float32(32768.0)
    return frames.astype(np.float32)


def downmix(frames):
    """librosa.to_mono of soundfile's [n, C] frames: np.mean over the channels in float32."""
    x = to_float(frames)
    return x if x.ndim == 1 else np.mean(x, axis=1, dtype=np.float32)


def resample(x, sr_in, sr_out, t0=0, t1=None, dtype=np.float64, table=None, precision=PRECISION):
    """Outputs [t0, t1) of resampy's resample_f(x, sr_in -> sr_out) for mono ``x``."""
    win, delta = table if table is not None else _table()
    nb = 2 ** precision
    ratio = float(sr_out) / sr_in
    if ratio < 1:                       # resampy scales the table (float64) before the loop
        win, delta = win * ratio, delta * ratio
    win, delta = win.astype(dtype), delta.astype(dtype)
    x = np.asarray(x).astype(dtype)
    n_orig = x.shape[0]
    t1 = n_out(n_orig, sr_in, sr_out) if t1 is None else t1
    scale = min(1.0, ratio)
    time_increment = 1.0 / ratio
    step = int(scale * nb)
    nwin = win.shape[0]
    time = np.arange(t0, t1, dtype=np.int64) * time_increment           # float64
    n = time.astype(np.int64)
    y = np.zeros(time.shape[0], dtype=dtype)

    def wing(frac, count, pick):
        index_frac = frac * nb
        off = index_frac.astype(np.int64)
        eta = (index_frac - off).astype(dtype)
        cmax = np.minimum(count, (nwin - off) // step)
        for i in range(int(cmax.max(initial=0))):
            m = i < cmax
            idx = off[m] + i * step
            w = win[idx] + eta[m] * delta[idx]
            y[m] += w * x[pick(n[m], i)]

    frac = scale * (time - n)
    wing(frac, n + 1, lambda nn, i: nn - i)
    wing(scale - frac, n_orig - n - 1, lambda nn, k: nn + k + 1)
    return y


def resample_scalar(x, sr_in, sr_out, table=None, precision=PRECISION):
    """resampy.interpn.resample_f, one channel, transcribed loop for loop (float64)."""
    interp_win, interp_delta = table if table is not None else _table()
    num_table = 2 ** precision
    sample_ratio = float(sr_out) / sr_in
    if sample_ratio < 1:
        interp_win = interp_win * sample_ratio
        interp_delta = interp_delta * sample_ratio
    x = np.asarray(x, dtype=np.float64)
    y = np.zeros(int(x.shape[0] * sample_ratio), dtype=np.float64)
    scale = min(1.0, sample_ratio)
    time_increment = 1.0 / sample_ratio
    index_step = int(scale * num_table)
    nwin = interp_win.shape[0]
    n_orig = x.shape[0]
    for t in range(y.shape[0]):
        time_register = t * time_increment
        n = int(time_register)
        frac = scale * (time_register - n)
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        i_max = min(n + 1, (nwin - offset) // index_step)
        for i in range(i_max):
            weight = interp_win[offset + i * index_step] + eta * interp_delta[offset + i * index_step]
            y[t] += weight * x[n - i]
        frac = scale - frac
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        k_max = min(n_orig - n - 1, (nwin - offset) // index_step)
        for k in range(k_max):
            weight = interp_win[offset + k * index_step] + eta * interp_delta[offset + k * index_step]
            y[t] += weight * x[n + k + 1]
    return y


def load_row(frames, sr_in, sr_out, T, t0=0, t1=None, dtype=np.float64):
    """Elements [t0, t1) of the row zs_resample_pack writes for one clip: librosa.load's mono
    signal at sr_out, cropped to T or zero-padded (embeddings_generator.py:53-59)."""
    t1 = T if t1 is None else t1
    mono = downmix(frames)
    row = np.zeros(t1 - t0, dtype=dtype)
    nv = min(n_out(mono.shape[0], sr_in, sr_out), T)
    hi = min(nv, t1)
    if hi > t0:
        if sr_in == sr_out:
            row[:hi - t0] = mono[t0:hi]
        else:
            row[:hi - t0] = resample(mono, sr_in, sr_out, t0, hi, dtype)
    return row


# ------------------------------------------------------------------ WAV files, byte by byte
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def sample_bytes(frames, kind):
    """Interleaved frames [n, C] -> little-endian sample bytes: 'u8' | 's16' | 's24' | 's32'
    (integers given as integers) | 'f32' | 'f64'."""
    a = np.asarray(frames)
    if kind == "u8":
        return a.astype(np.uint8).tobytes()
    if kind == "s16":
        return a.astype("<i2").tobytes()
    if kind == "s32":
        return a.astype("<i4").tobytes()
    if kind == "s24":
        v = a.astype(np.int64).reshape(-1) & 0xFFFFFF
        return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).tobytes()
    return a.astype("<f4" if kind == "f32" else "<f8").tobytes()


def wav_file(path, payload, tag, bits, channels, sr, extensible=False, before=(), after=(),
             data_size=None):
    """Write a RIFF/WAVE file: ``fmt `` (16 bytes, or the 40-byte EXTENSIBLE form carrying
    ``tag`` in its sub-format GUID), the chunks ``before`` [(id, bytes)], ``data`` (its size
    field ``data_size`` if given, else the payload's), the chunks ``after``.  Odd-sized chunks
    get their pad byte."""
    align = channels * bits // 8
    if extensible:
        fmt = struct.pack("<HHIIHH", 0xFFFE, channels, sr, sr * align, align, bits)
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + _GUID_TAIL
    else:
        fmt = struct.pack("<HHIIHH", tag, channels, sr, sr * align, align, bits)

    def chunk(cid, body, size=None):
        return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")
    body = b"WAVE" + chunk(b"fmt ", fmt)
    for cid, b in before:
        body += chunk(cid, b)
    body += chunk(b"data", payload, data_size)
    for cid, b in after:
        body += chunk(cid, b)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
