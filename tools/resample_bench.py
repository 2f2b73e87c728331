#!/usr/bin/env python3
"""What the file path of Extract_embeddings costs next to the encoder.

    kernel : zs_resample_pack on 64 mono PCM16 clips, 44.1 kHz -> 32 kHz, T = 320000 (each clip
             the prefix audio_io.resample_plan uploads); per-call time against its byte floor
             (frames read + rows written, at HBM_GBPS) and against its multiply-add count
    encode : the bf16 HTSAT encoder pass (AudioEncoder.encode) on the 64 packed rows
    files  : EmbeddingExtractor.encode_files on 64 synthetic 30 s stereo PCM16 files at
             44.1 kHz written to a temporary directory: clips / s, second pass (page cache warm)

Each step runs in a child process of its own under a time limit; a step that fails or runs out
of time ends the run (nothing further is started on the device).

    python tools/resample_bench.py [out.txt]
"""
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zero-shot-aac_amd"))

B, SR_IN, SR, T = 64, 44100, 32000, 320000
HBM_GBPS = 6300.0           # what a streaming kernel reaches on an MI355X
STEPS = [("kernel", 120), ("encode", 240), ("files", 300)]
ROUNDS, REPS = 5, 10


def _window(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _times(fn, reps=REPS):
    _window(fn, 2)
    return [_window(fn, reps) for _ in range(ROUNDS)]


def _fmt(ts):
    return f"{min(ts):8.3f} / {statistics.median(ts):8.3f} / {max(ts):8.3f} ms (min / median / max of {ROUNDS} windows)"


def step_kernel():
    import numpy as np
    import torch
    from zsaac import audio_io, ops
    dev = torch.device("cuda", 0)
    tab, nz, prec = audio_io.resample_filter("kaiser_best")
    table = torch.from_numpy(tab).to(dev)
    n_out, need = audio_io.resample_plan(30 * SR_IN, SR_IN, SR, T)
    rng = np.random.default_rng(0)
    flat = torch.from_numpy(rng.integers(-32768, 32768, B * need).astype(np.int16)).to(dev)
    offs = np.arange(B, dtype=np.int64) * need
    out = torch.empty(B, T, device=dev)
    meta = ([need] * B, [1] * B, [SR_IN] * B, [n_out] * B)

    def run():
        ops.resample_pack(flat, offs, *meta, SR, T, table, nz, prec, out)
    ts = _times(run)
    med = statistics.median(ts)
    byts = B * need * 2 + B * T * 4
    floor_ms = byts / (HBM_GBPS * 1e9) * 1e3
    nb = 1 << prec
    taps = 2 * ((nb * nz + 1) // (nb * SR // SR_IN))
    macs = B * T * taps
    print(f"kernel  zs_resample_pack {B} clips {SR_IN} -> {SR}, T {T}, {need} frames each: {_fmt(ts)}")
    print(f"kernel  byte floor {floor_ms:.3f} ms ({byts / 1e6:.1f} MB at {HBM_GBPS:.0f} GB/s): "
          f"{med / floor_ms:.1f} x the floor; {macs / 1e9:.2f} G taps (2 FMA + 1 table load each), "
          f"{macs / med / 1e9:.2f} T taps/s")


def step_encode():
    import torch
    from zsaac import synthetic as S
    from zsaac.encoder import AudioEncoder
    dev = torch.device("cuda", 0)
    asd = S.htsat_state_dict(3)
    asd.update(S.audio_proj_state_dict(5))
    enc = AudioEncoder(asd, "htsat", torch.bfloat16, B, dev, n_samples=T)
    wav = (torch.rand(B, T, device=dev) * 2 - 1) * 0.1
    ts = _times(lambda: enc.encode(wav), reps=5)
    print(f"encode  AudioEncoder.encode bf16 HTSAT, {B} clips x {T} samples: {_fmt(ts)}")


def step_files():
    import wave

    import numpy as np
    import torch
    from zsaac import synthetic as S
    from zsaac.extract import EmbeddingExtractor
    dev = torch.device("cuda", 0)
    asd = S.htsat_state_dict(3)
    asd.update(S.audio_proj_state_dict(5))
    ex = EmbeddingExtractor(asd, "htsat", torch.bfloat16, batch=B, device=dev)
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(B):
            p = os.path.join(d, f"{i}.wav")
            with wave.open(p, "wb") as w:
                w.setnchannels(2)
                w.setsampwidth(2)
                w.setframerate(SR_IN)
                w.writeframes(rng.integers(-8000, 8000, (30 * SR_IN, 2)).astype("<i2").tobytes())
            paths.append(p)
        ex.encode_files(paths[:4])
        torch.cuda.synchronize()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            ex.encode_files(paths)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
    w = statistics.median(walls)
    print(f"files   encode_files, {B} files of 30 s stereo PCM16 at {SR_IN} Hz: "
          f"{min(walls):.3f} / {w:.3f} / {max(walls):.3f} s wall (3 passes), {B / w:.1f} clips / s")


def main(out_path=None):
    lines = []
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                            "--step", name], capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"step {name} ended with status {r.returncode}: stopping")
            return r.returncode
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("".join(lines))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        {"kernel": step_kernel, "encode": step_encode, "files": step_files}[sys.argv[2]]()
    else:
        raise SystemExit(main(sys.argv[1] if len(sys.argv) > 1 else None))
