"""zsaac.longform end to end on the GPU: synthetic HTSAT weights (as tests/test_gpu_tagging.py),
f32 and bf16, batch 4.

The kernels are pinned in tests/test_gpu_longform_kernels.py; here the engine's plumbing is: the
window rows are the recording's own samples, every window goes through encode_events as a clip
of its own would, the stitched results are longform_ref.stitch of exactly those outputs, and a
recording of at most 10 s keeps what the 10 s entry points give it, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_ref as L  # noqa: E402
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
SR, T, HOP = 32000, 320000, 160000
NAMES = [f"sound {i}" for i in range(527)]


def _sd():
    from zsaac import synthetic as S
    sd = S.htsat_state_dict(3)
    sd.update(S.audio_proj_state_dict(5))
    return sd


@pytest.fixture(scope="module", params=[F32, BF16], ids=["f32", "bf16"])
def la(request, cuda):
    from zsaac.longform import LongAudio
    return LongAudio(_sd(), NAMES, dtype=request.param, batch=4, device=cuda)


@pytest.fixture(scope="module")
def pipe(cuda):
    """The tiny caption model of tests/test_gpu_harness.py (synthetic GPT-2 + MLP mapper), f32."""
    from zsaac import synthetic as S
    from zsaac.pipeline import CaptionConfig, CaptionPipeline
    csd = S.gpt2_state_dict(seed=0, std=0.1, emb_std=0.1, stop_boost=2.0)
    csd.update(S.mlp_mapper_state_dict(1))
    return CaptionPipeline(csd, None, S.label_table(), S.label_token_table(),
                           CaptionConfig(dtype=F32, batch=4, entry_length=8), device=cuda)


def _recording(seconds, seed):
    """Noise with a 1 kHz tone burst of 1.5 s planted at 17 s (where the recording is that long)."""
    n = int(seconds * SR)
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32) * 0.05
    a, b = 17 * SR, min(n, int(18.5 * SR))
    if b > a:
        x[a:b] += 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(b - a) / SR).astype(np.float32)
    return x


def _host_windows(x, n_win):
    w = np.zeros((n_win, T), np.float32)
    for i in range(n_win):
        seg = x[i * HOP:i * HOP + T]
        w[i, :seg.shape[0]] = seg
    return w


def _keep(out):
    return out.frame.clone(), out.clip.clone(), out.emb.clone()


def test_long_recording(la, cuda):
    """Case A, 23.7 s at 32 kHz given as samples: 4 windows, 76 time-line frames.  The synthetic
    head (random weights of std 0.01) does not respond to the planted tone selectively, so the
    events are asserted through the time line's values: the stitched line equals the reference
    stitch of the windows' own head outputs, the events are tagging.segments of exactly that
    line, and with the threshold at the top class's median probability more frames pass it than
    lie before 10.24 s -- an event past the 10 s crop must be reported."""
    from zsaac.tagging import segments
    x = _recording(23.7, 1)
    assert L.window_plan(x.shape[0], T, HOP) == (4, 76)
    rows, plan, wgt, n_outs = la.window_rows([(x, SR)])
    assert plan.tolist() == [[0, 4, 0, 76]] and n_outs == [x.shape[0]]
    host = torch.from_numpy(_host_windows(x, 4)).to(cuda)
    assert torch.equal(rows, host), "window rows are not the recording's own samples"
    f1, c1, e1 = _keep(la.enc.encode_events(rows))
    f2, c2, e2 = _keep(la.enc.encode_events(host))
    assert torch.equal(f1, f2) and torch.equal(c1, c2) and torch.equal(e1, e2)
    # the threshold comes from the reference stitch of those outputs
    a = ([x.shape[0]], T, HOP, f1.cpu().numpy(), c1.cpu().numpy(), e1.cpu().numpy())
    ref, twin = L.stitch(*a), L.stitch(*a, dtype=np.float32)
    top = int(np.argmax(twin[1][0]))
    thr = float(np.median(twin[0][:, top]))
    res = la.analyse_clips([x], k=5, threshold=thr, min_frames=1)[0]
    torch.cuda.synchronize()
    assert (res.n_windows, res.file) == (4, None) and abs(res.seconds - 23.7) < 1e-9
    assert torch.equal(res.window_emb, e1)
    got = (res.timeline.cpu().numpy(), None, res.emb.cpu().numpy()[None])
    assert got[0].shape == (76, 527)
    for name, i in (("timeline", 0), ("rec_emb", 2)):
        yard, tol = L.tolerance(ref[i], twin[i])
        err = float(np.abs(got[i].astype(np.float64) - ref[i]).max())
        print(f"{name}: error {err:.3e}, yardstick {yard:.3e}, tolerance {tol:.3e}")
        assert err <= tol, (name, err, tol)
    # tags: the maximum over the windows of the clip probabilities, best first
    assert [t[0] for t in res.tags][0] == top and res.tags[0][1] == NAMES[top]
    assert [t[2] for t in res.tags] == sorted(twin[1][0].tolist(), reverse=True)[:5]
    # events: segments of the device time line of the chosen classes, in seconds of T / 32 / sr
    line = res.timeline.cpu()
    want = [(cid, NAMES[cid], s * 0.3125, e * 0.3125, pk) for cid, _, _ in res.tags
            for s, e, pk in segments(line[:, cid].tolist(), thr, 1)]
    assert res.events == want
    late = [e for e in res.events if e[0] == top and e[3] > 10.24]
    assert late and all(e[3] <= 76 * 0.3125 + 1e-9 for e in res.events), res.events[:4]
    assert sum(1 for v in line[:, top].tolist() if v >= thr) > 33


def test_short_recording_keeps_the_clip_results(la, cuda):
    """Case B, 7 s: one window.  emb is EmbeddingExtractor.encode_clips' bit for bit, the time
    line's 23 rows are encode_events' frame rows, the tags are AudioTagger.tag_wav's."""
    from zsaac.tagging import AudioTagger
    x = _recording(7.0, 2)
    res = la.analyse_clips([x], k=5)[0]
    torch.cuda.synchronize()
    emb, line, wemb = res.emb.clone(), res.timeline.clone(), res.window_emb.clone()
    assert res.n_windows == 1 and line.shape == (23, 527)
    assert torch.equal(emb, la.ex.encode_clips([x])[0]) and torch.equal(wemb[0], emb)
    wav = torch.from_numpy(_host_windows(x, 1)).to(cuda)
    out = la.enc.encode_events(wav)
    assert torch.equal(line, out.frame[0, :23])
    ids, prob = AudioTagger(None, NAMES, encoder=la.enc).tag_wav(wav, k=5)
    assert [t[0] for t in res.tags] == ids[0].tolist() and [t[2] for t in res.tags] == prob[0].tolist()
    assert all(e[3] <= 23 * 0.3125 + 1e-9 for e in res.events)


def test_file_and_captions(la, pipe, cuda, tmp_path):
    """Cases C and D: a 12 s 44.1 kHz stereo int16 WAV gives 2 windows, window 0's row is
    pack_frames' row bit for bit; caption_files' caption is pipe.caption_emb of the recording's
    embedding, per_window gives one span per window at the planned times.  A 26 s file and an empty one
    share the call: 7 windows at batch 4 are two encoder passes, and the second file's windows
    span both."""
    from zsaac import audio_io
    rng = np.random.default_rng(3)
    paths = []
    for name, secs in (("a.wav", 12.0), ("b.wav", 26.0), ("empty.wav", 0.0)):
        fr = rng.integers(-8000, 8000, (int(secs * 44100), 2)).astype(np.int16)
        paths.append(str(tmp_path / name))
        R.wav_file(paths[-1], R.sample_bytes(fr, "s16"), 1, 16, 2, 44100)
    item = audio_io.read_wav(paths[0])
    rows, plan, _, n_outs = la.window_rows([item])
    n_a = R.n_out(item[0].shape[0], 44100, SR)           # 384000, or one less by float64 rounding
    assert n_outs == [n_a] and n_a in (383999, 384000) and plan.tolist() == [[0, 2, 0, 39]]
    row0, tail = rows[0].clone(), rows[1].clone()
    assert torch.equal(row0, la.ex.pack_frames([item])[0])
    assert bool((tail[n_a - HOP:] == 0).all()) and bool((tail[:1000] != 0).any())
    out = la.caption_files(pipe, None, paths, per_window=True, k=3)
    assert [r.n_windows for r, _, _ in out] == [2, 5, 0] and [r.file for r, _, _ in out] == paths
    (ra, cap, spans), (rb, capb, spb), (re_, cape, spe) = out
    assert ra.seconds == n_a / SR and len(ra.tags) == 3
    by_hand = pipe.caption_emb(torch.stack([ra.emb, rb.emb])).captions()
    assert [cap, capb] == by_hand
    assert [(a, b) for a, b, _ in spans] == [(0.0, 10.0), (5.0, ra.seconds)]
    assert [c for _, _, c in spans] == pipe.caption_emb(ra.window_emb).captions()
    assert len(spb) == 5 and spb[-1][:2] == (20.0, rb.seconds) and rb.seconds > 25.9
    assert (re_.emb, re_.tags, re_.events, cape, spe) == (None, [], [], None, None)
    assert abs(float(ra.emb.norm()) - 1.0) < 1e-5       # the pooled embedding is a unit vector


def test_cnn14_has_no_head(la):
    """A CNN14 encoder gives embeddings only: asking for tags raises before any launch."""
    kind = la.enc.kind
    try:
        la.enc.kind = "cnn14"
        with pytest.raises(NotImplementedError, match="tagging head"):
            la.analyse_clips([np.zeros(1000, np.float32)], k=5)
    finally:
        la.enc.kind = kind
    with pytest.raises(ValueError):
        la.analyse_clips([np.zeros(1000, np.float32)], k=9)
