"""GPU: Extract_embeddings from files (data_handing/embeddings_generator.py:34-75) --
EmbeddingExtractor.encode_files / pack_frames / extract_dataset on synthetic encoder weights and
WAV files written into a temporary directory."""
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SR, T = 32000, 320000


def _write_pcm16(path, x, sr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[1])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(x.astype("<i2").tobytes())


@pytest.fixture(scope="module")
def extractor(cuda):
    from zsaac import synthetic as S
    from zsaac.extract import EmbeddingExtractor
    asd = S.htsat_state_dict(3)
    asd.update(S.audio_proj_state_dict(5))
    return EmbeddingExtractor(asd, "htsat", torch.bfloat16, batch=4, device=cuda)


def _clap(cuda, layers=2):
    from retrieval.models.ase_model import ASE
    from zsaac import synthetic as S
    vocab = {t: i for i, t in enumerate(S.bert_vocab())}
    cfg = {"audio_args": {"sr": 32000, "n_fft": 1024, "hop_length": 320, "f_min": 50,
                          "f_max": 14000, "n_mels": 64, "max_length": 10, "mono": True},
           "audio_encoder_args": {"type": "transformer", "model": "Cnn14", "pretrained": False,
                                  "freeze": False},
           "embed_size": 1024, "temp": 0.07,
           "text_encoder_args": {"type": "bert-base-uncased", "freeze": False, "vocab": vocab,
                                 "vocab_size": len(S.bert_vocab()), "num_layers": layers}}
    clap = ASE(cfg)
    missing, unexpected = clap.load_state_dict(S.bert_state_dict(layers=layers), strict=False)
    assert not unexpected and all(m.startswith("audio") for m in missing)
    clap.zs_dtype = torch.float32
    return clap.to(cuda).eval()


def test_encode_files_at_the_target_rate_is_encode_clips(extractor, tmp_path):
    """A 32 kHz mono PCM16 file: librosa.load neither resamples nor downmixes, so encode_files
    equals encode_clips of samples / 32768 bit for bit (one cropped, one padded clip)."""
    rng = np.random.default_rng(1)
    xs = [rng.integers(-8000, 8000, (n, 1)).astype(np.int16) for n in (400000, 90000)]
    paths = []
    for i, x in enumerate(xs):
        paths.append(str(tmp_path / f"c{i}.wav"))
        _write_pcm16(paths[-1], x, SR)
    got = extractor.encode_files(paths).cpu()
    ref = extractor.encode_clips([x[:, 0].astype(np.float32) / np.float32(32768.0) for x in xs]).cpu()
    assert got.shape == (2, 1024) and torch.equal(got, ref)


def test_pack_frames_stereo_44k1(extractor, tmp_path):
    """A 44.1 kHz stereo PCM16 file next to a float32 one (a mixed chunk: two launches and the
    reorder): each row meets the criterion of tests/test_gpu_resample.py against librosa.load's
    restatement, on every one of its 320000 elements."""
    from zsaac import audio_io
    rng = np.random.default_rng(2)
    x = rng.integers(-32768, 32768, (70000, 2)).astype(np.int16)
    p = str(tmp_path / "st.wav")
    _write_pcm16(p, x, 44100)
    frames, sr = audio_io.read_wav(p)
    assert sr == 44100 and frames.dtype == np.int16 and np.array_equal(frames, x)
    f = rng.uniform(-1, 1, (30000, 1)).astype(np.float32)
    got = extractor.pack_frames([(f, 48000), (frames, sr)]).cpu().numpy()
    for name, row, src, s in (("48 k f32", got[0], f, 48000), ("44.1 k stereo s16", got[1], x, 44100)):
        r64 = R.load_row(src, s, SR, T)
        r32 = R.load_row(src, s, SR, T, dtype=np.float32)
        yard = float(np.abs(r32.astype(np.float64) - r64).max())
        err = float(np.abs(row.astype(np.float64) - r64).max())
        print(f"pack_frames {name}: error {err:.3e}, yardstick {yard:.3e}, tolerance {2 * yard + 1e-7:.3e}")
        assert err <= 2 * yard + 1e-7
        assert not row[R.n_out(src.shape[0], s, SR):].any()


def _dataset(root, rng):
    """wav.csv + text.json + files: a 44.1 kHz stereo clip, an empty clip, a 16 kHz mono clip."""
    clips = {"a": (rng.integers(-9000, 9000, (50000, 2)).astype(np.int16), 44100),
             "empty": (np.zeros((0, 1), np.int16), 44100),
             "c": (rng.integers(-9000, 9000, (20000, 1)).astype(np.int16), 16000)}
    with open(os.path.join(root, "wav.csv"), "w") as f:
        f.write("audio_id\tfile_name\n")
        for k, (x, sr) in clips.items():
            p = os.path.join(root, k + ".wav")
            _write_pcm16(p, x, sr)
            f.write(f"{k}\t{p}\n")
    audios = [{"audio_id": "c", "captions": [{"caption": "A dog , barks."}, {"caption": "w1 w2 in this audio!"}]},
              {"audio_id": "empty", "captions": [{"caption": "nothing"}]},
              {"audio_id": "a", "captions": [{"caption": "There are sounds"}]}]
    with open(os.path.join(root, "text.json"), "w") as f:
        json.dump({"audios": audios}, f)
    return clips, audios


def test_extract_dataset_records(extractor, tmp_path):
    """text_or_not False: the reference's record keys, the order of text.json, the empty clip
    skipped, each embedding the encoder's on the packed row; without a text tower text_or_not
    raises."""
    clips, audios = _dataset(str(tmp_path), np.random.default_rng(3))
    recs = extractor.extract_dataset(str(tmp_path), False)
    assert [r["audio_id"] for r in recs] == ["c", "a"]
    for r, e in zip(recs, (audios[0], audios[2])):
        assert list(r.keys()) == ["audio_embedding", "caption", "text_embedding", "audio_id"]
        assert r["caption"] == e["captions"] and r["text_embedding"] == 0
        assert r["audio_embedding"].shape == (1, 1024) and r["audio_embedding"].device.type == "cpu"
    direct = extractor.enc.encode(extractor.pack_frames([clips["c"], clips["a"]])).cpu()
    assert torch.equal(torch.cat([r["audio_embedding"] for r in recs]), direct)
    with pytest.raises(NotImplementedError):
        extractor.extract_dataset(str(tmp_path), True)


def test_extract_dataset_with_text(extractor, cuda, tmp_path):
    """text_or_not True with a small synthetic BERT: one record per caption with the caption's
    string and ASE.encode_text([text_preprocess(caption)]) as [1, 1024] on the CPU.  The batch
    and the single text differ only in the shapes the float32 GEMMs run at (summation order):
    unit-norm embeddings, so 1e-5 per component is some 30 float32 steps of the largest."""
    from zsaac.extract import text_preprocess
    assert text_preprocess("A dog , barks.") == "a dog barks "
    clips, audios = _dataset(str(tmp_path), np.random.default_rng(3))
    clap = _clap(cuda)
    extractor.text, extractor.tokenizer = clap, None
    try:
        recs = extractor.extract_dataset(str(tmp_path), True)
    finally:
        extractor.text = None
    assert [(r["audio_id"], r["caption"]) for r in recs] == [
        ("c", "A dog , barks."), ("c", "w1 w2 in this audio!"), ("a", "There are sounds")]
    assert torch.equal(recs[0]["audio_embedding"], recs[1]["audio_embedding"])
    for r in recs:
        assert list(r.keys()) == ["audio_embedding", "caption", "text_embedding", "audio_id"]
        ref = clap.encode_text([text_preprocess(r["caption"])]).cpu()
        te = r["text_embedding"]
        assert te.shape == (1, 1024) and te.device.type == "cpu" and te.dtype == torch.float32
        d = float((te - ref).abs().max())
        print(f"text embedding of {r['caption']!r}: batch vs single {d:.3e}")
        assert d <= 1e-5
