"""Host side of the file path of ``Extract_embeddings``
(data_handing/embeddings_generator.py:48): what ``librosa.load(path, sr=32000, mono=True)`` does
before the device takes over.

* :func:`read_wav` decodes a RIFF/WAVE file to interleaved frames ``[n, C]`` as soundfile
  delivers them (PCM16 stays int16: it is uploaded as is and converted on the device, exactly).
  FLAC / MP3 / OGG are out of scope (no decoder here): they raise ``ValueError``.
* :func:`resample_filter` builds resampy's half-filter table (``kaiser_best``, the default
  ``res_type`` of librosa 0.9.2) in float64 and returns it as the interleaved ``(win, delta)``
  float32 table ``zs_resample_pack`` reads.
* :func:`resample_plan` says how many outputs a file has at the target rate and how many of
  its frames the first ``T`` of them read, so a 30 s clip uploads a little over 10 s.

Downmix, resampling, crop and pad run on the device (``ops.resample_pack``).
"""
from __future__ import annotations

import struct
from typing import Tuple

import numpy as np

# resampy's filters.py: (num_zeros, precision, rolloff, beta) of the windowed sinc it ships
FILTERS = {"kaiser_best": (64, 9, 0.9475937167399596, 14.769656459379492)}

_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE
# the tail of KSDATAFORMAT_SUBTYPE_PCM / _IEEE_FLOAT: the first two bytes are the format tag
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def half_window(num_zeros: int, precision: int, rolloff: float, beta: float) -> np.ndarray:
    """resampy.filters.sinc_window's half filter in float64: ``nb * num_zeros + 1`` taps."""
    n = (1 << precision) * num_zeros
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True)) * taper


def resample_filter(name: str = "kaiser_best"):
    """-> (table [n + 1, 2] float32: (win[i], win[i+1] - win[i]), the last delta 0; num_zeros;
    precision).  The deltas are taken in float64 and rounded once, as resampy holds them."""
    if name not in FILTERS:
        raise ValueError(f"resample filter {name!r}: only {sorted(FILTERS)} is wired in")
    num_zeros, precision, rolloff, beta = FILTERS[name]
    win = half_window(num_zeros, precision, rolloff, beta)
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return np.stack([win, delta], axis=1).astype(np.float32), num_zeros, precision


def resample_plan(n_frames: int, sr_in: int, sr_out: int, T: int, name: str = "kaiser_best"
                  ) -> Tuple[int, int]:
    """(n_out, frames_needed): resampy's output length ``int(n_frames * (sr_out / sr_in))`` of the
    whole file (float64, as resampy computes it; librosa's fix_length to the ceil only appends a
    zero), and how many leading frames the first ``T`` outputs read: the sample left of output
    T - 1 plus one wing of ``ceil(num_zeros / scale)`` taps plus one."""
    n_frames, sr_in, sr_out = int(n_frames), int(sr_in), int(sr_out)
    if sr_in == sr_out:
        return n_frames, min(n_frames, T)
    n_out = int(n_frames * (float(sr_out) / sr_in))
    num_zeros, precision = FILTERS[name][:2]
    nb = 1 << precision
    step = nb * sr_out // sr_in if sr_out < sr_in else nb      # int(scale * nb)
    if step < 1:
        raise ValueError(f"{sr_in} Hz -> {sr_out} Hz: beyond what the {name} table resolves")
    wing = (nb * num_zeros + 1) // step                          # most taps of one wing
    need = -(-T * sr_in // sr_out) + wing + 1
    return n_out, min(n_frames, need)


def _fmt_error(path, what):
    return ValueError(f"{path}: {what}")


def read_wav(path: str) -> Tuple[np.ndarray, int]:
    """A RIFF/WAVE file -> (frames [n, C], sample rate).  Format tags 1 (PCM 8 / 16 / 24 / 32
    bit), 3 (IEEE float 32 / 64) and 0xFFFE (EXTENSIBLE with either sub-format); chunks other
    than ``fmt `` and ``data`` are skipped, odd chunk sizes are padded, a ``data`` size of 0 or
    past the end of the file is clamped to the file (streamed writers leave both).  PCM16 is
    returned as int16; everything else as float32 by soundfile's rules (u8 ``(x - 128) / 128``,
    s24 ``/ 2**23``, s32 ``/ 2**31``, f64 rounded to f32).  Anything else raises ValueError
    naming what it found."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        magic = data[:4]
        kind = {b"fLaC": "FLAC", b"OggS": "Ogg", b"ID3\x03": "MP3", b"ID3\x04": "MP3",
                b"RF64": "RF64", b"FORM": "AIFF"}.get(magic, None)
        if kind is None and len(data) >= 2 and data[0] == 0xFF and (data[1] & 0xE0) == 0xE0:
            kind = "MP3"
        raise _fmt_error(path, f"not a RIFF/WAVE file ({kind or repr(magic)}); only WAV is decoded here")
    pos, fmt, body = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        start = pos + 8
        if cid == b"fmt ":
            if size < 16 or start + 16 > len(data):
                raise _fmt_error(path, "truncated fmt chunk")
            tag, ch, sr, _, align, bits = struct.unpack_from("<HHIIHH", data, start)
            if tag == _EXTENSIBLE:
                if size < 40 or start + 40 > len(data):
                    raise _fmt_error(path, "WAVE_FORMAT_EXTENSIBLE without its sub-format")
                sub = data[start + 24:start + 40]
                if sub[2:] != _GUID_TAIL:
                    raise _fmt_error(path, f"WAVE_FORMAT_EXTENSIBLE sub-format {sub.hex()} (PCM and IEEE float only)")
                tag = struct.unpack_from("<H", sub)[0]
            fmt = (tag, ch, sr, align, bits)
        elif cid == b"data":
            if fmt is None:
                raise _fmt_error(path, "data chunk before fmt chunk")
            if size == 0 or start + size > len(data):
                size = len(data) - start
            body = data[start:start + size]
            break
        pos = start + size + (size & 1)
    if fmt is None or body is None:
        raise _fmt_error(path, "no fmt / data chunk")
    tag, ch, sr, align, bits = fmt
    if ch < 1 or sr < 1:
        raise _fmt_error(path, f"{ch} channels at {sr} Hz")
    if tag == _PCM and bits in (8, 16, 24, 32):
        kind = "pcm"
    elif tag == _FLOAT and bits in (32, 64):
        kind = "float"
    else:
        raise _fmt_error(path, f"WAVE format tag {tag:#x} with {bits} bits (PCM 8/16/24/32, float 32/64 only)")
    bps = bits // 8
    n = len(body) // (bps * ch)
    raw = np.frombuffer(body, dtype=np.uint8, count=n * ch * bps)
    if kind == "float":
        x = raw.view("<f4" if bits == 32 else "<f8").astype(np.float32)
    elif bits == 16:
        x = raw.view("<i2").astype(np.int16, copy=False)
    elif bits == 8:
        x = (raw.astype(np.float32) - 128.0) / 128.0
    elif bits == 32:
        x = (raw.view("<i4").astype(np.float64) / 2.0 ** 31).astype(np.float32)
    else:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = v - ((v & 0x800000) << 1)
        x = (v.astype(np.float32) / np.float32(2.0 ** 23)).astype(np.float32)
    return x.reshape(n, ch), int(sr)
