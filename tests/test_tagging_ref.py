"""CPU: tests/tagging_ref.py against the reference's own tagging head, and the conditions the GPU
cases of tests/test_gpu_tagging_kernels.py rely on.

* The float64 reference, fed the golden's tokens (tests/golden/htsat_head.npz: the reference's
  ``forward_features`` on htsat.npz's clips), reproduces its framewise / clipwise / fine-grained
  outputs under encoder_ref.tolerance -- this pins tok(), the zero padding and the mean before
  the sigmoid to the real reference.
* On the GPU cases' own inputs each mutant of tagging_ref.MUTANTS differs from the reference by
  more than the case's tolerance, in f32 and in bf16 mode, so a kernel that makes that error
  fails its GPU case.
* segments() and the top-k order; the host-side packing of the conv weight.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tagging_ref as T  # noqa: E402

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


@pytest.fixture(scope="module")
def head_golden(golden):
    return {k: torch.from_numpy(v) for k, v in golden("htsat_head.npz").items()}


@pytest.fixture(scope="module")
def head_weights():
    from zsaac import synthetic as S
    sd = S.htsat_state_dict(3)
    p = "audio_encoder.audio_enc."
    return (sd[p + "norm.weight"], sd[p + "norm.bias"], sd[p + "tscam_conv.weight"],
            sd[p + "tscam_conv.bias"])


def test_reference_reproduces_the_golden(head_golden, head_weights):
    g = head_golden
    assert g["tokens"].shape == (2, 64, 768) and g["framewise32"].shape == (2, 32, 527)
    assert g["clipwise"].shape == (2, 527) and g["fine32"].shape == (2, 32, 64)
    r64 = T.head(g["tokens"], *head_weights)
    r32 = T.head(g["tokens"], *head_weights, dtype=F32)
    for name, got, key, cut in (("framewise", g["framewise32"], "frame", None),
                                ("clipwise", g["clipwise"], "clip", None),
                                ("fine", g["fine32"], "fine", 64)):
        ref64, ref32 = r64[key][..., :cut], r32[key][..., :cut]
        yard, tol = T.tolerance(ref64, ref32)
        err = (got.double() - ref64).abs()
        print(f"{name}: golden vs float64 reference {float(err.max()):.3e}, yardstick {yard:.3e}")
        assert bool((err <= tol).all()), (name, float(err.max()), yard)
    # the golden is not degenerate: probabilities move across classes and across time
    assert float(g["framewise32"].std()) > 1e-3 and float(g["clipwise"].std()) > 1e-3
    assert float(g["framewise32"].std(1).max()) > 1e-4


def test_golden_tells_the_mutants(head_golden, head_weights):
    """The real weights and tokens, too, tell every index mutant from the reference."""
    g = head_golden
    r64 = T.head(g["tokens"], *head_weights)
    r32 = T.head(g["tokens"], *head_weights, dtype=F32)
    for mut in ("pad_group", "bin_swap", "tap_rev", "tau_4t_g"):
        m = T.head(g["tokens"], *head_weights, mut=mut)
        _, tol = T.tolerance(r64["frame"], r32["frame"])
        assert bool(((m["frame"] - r64["frame"]).abs() > tol).any()), mut


def _affected(mut):
    """The outputs a mutant must move.  tau_4t_g only permutes the frames and keeps frames 0 and
    31 in place, so the time sum -- and with it clip -- is unchanged: it shows in frame and fine.
    tap_rev moves the time sum only through the two edge frames (a 1/32 effect, below the bf16
    rule's bound at some shapes): it is held to frame."""
    return {"mean_sigmoid": ("clip",), "fine_bf16": ("fine",), "tau_4t_g": ("frame", "fine"),
            "tap_rev": ("frame",)}.get(mut, ("frame", "clip"))


@pytest.mark.parametrize("B,C,N", T.CASES)
def test_gpu_cases_tell_the_mutants(B, C, N):
    c = T.case(B, C, N)
    a = (c["x"], c["lnw"], c["lnb"], c["W"], c["bias"])
    r64, r32, twin = T.case_refs(B, C, N)
    for mut in T.MUTANTS:
        m = T.head(*a, mut=mut)
        for key in _affected(mut):
            d = (m[key] - r64[key]).abs()
            _, tol32 = T.tolerance(r64[key], r32[key])
            assert bool((d > tol32).any()), (mut, key, "f32", float(d.max()))
            if key == "fine":
                continue          # fine is held to the f32 rule in both modes
            _, tolbf = T.tolerance_bf16(r64[key], twin[key])
            assert float(d.max()) > tolbf, (mut, key, "bf16", float(d.max()), tolbf)


@pytest.mark.parametrize("B,C,N", T.CASES)
def test_gpu_cases_are_not_degenerate(B, C, N):
    r64, r32, twin = T.case_refs(B, C, N)
    z = r64["z"]
    assert 0.5 < float(z.std()) < 4.0, float(z.std())            # sigmoid neither flat nor saturated
    f = r64["frame"]
    assert float(((f > 0.02) & (f < 0.98)).double().mean()) > 0.8
    # the yardsticks are real: plain f32 and the bf16 roundings both move the result
    assert 0 < float((r32["z"].double() - z).abs().max()) < 1e-4
    assert 1e-4 < float((twin["z"].double() - z).abs().max()) < 0.2


def test_duplicate_rows_case_ties():
    c = T.dup_case()
    r = T.head(c["x"], c["lnw"], c["lnb"], c["W"], c["bias"])
    assert torch.equal(r["clip"][:, 3], r["clip"][:, 140]) and torch.equal(r["frame"][..., 20], r["frame"][..., 21])
    # make the tied classes the row's best, so the order among equals decides the list
    v = r["clip"].clone()
    v[:, [3, 140]] = 2.0
    v[:, [20, 21]] = 1.5
    _, idx = T.topk(v, 5)
    assert idx[:, :4].tolist() == [[3, 140, 20, 21]] * 2


def test_topk_order():
    v = torch.tensor([[0.1, 0.7, 0.7, 0.2, 0.7, 0.0], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]])
    vals, idx = T.topk(v, 4)
    assert idx.tolist() == [[1, 2, 4, 3], [0, 1, 2, 3]]
    assert vals[0].tolist() == pytest.approx([0.7, 0.7, 0.7, 0.2])
    vals, idx = T.topk(v[:, :2], 3)                 # a row shorter than k: padding comes last
    assert idx[0].tolist() == [1, 0, 0x7fffffff] and math.isinf(float(vals[0, 2]))
    # torch.topk agrees wherever the values differ
    g = torch.Generator().manual_seed(5)
    w = torch.rand(3, 50, generator=g)
    assert torch.equal(T.topk(w, 8)[1], torch.topk(w, 8, dim=1).indices)


def test_segments():
    from zsaac.tagging import FRAME_SECONDS, segments
    assert FRAME_SECONDS == pytest.approx(0.32) and T.FRAME_SECONDS == 0.32
    assert segments([], 0.5) == [] and segments([0.1] * 32, 0.5) == []
    p = [0.0] * 32
    p[0] = p[1] = 0.9                               # a run touching frame 0
    p[1] = 0.95
    p[10] = 0.5                                     # exactly at the threshold: in
    p[11] = 0.49999
    p[29] = p[30] = p[31] = 0.6                     # a run touching frame 31
    p[30] = 0.8
    assert segments(p, 0.5) == [(0, 2, 0.95), (10, 11, 0.5), (29, 32, 0.8)]
    assert segments(p, 0.5, min_frames=2) == [(0, 2, 0.95), (29, 32, 0.8)]
    assert segments(p, 0.5, min_frames=3) == [(29, 32, 0.8)]
    assert segments(p, 0.5, min_frames=4) == []
    assert segments([0.7] * 32, 0.5) == [(0, 32, 0.7)]
    assert segments(torch.tensor(p), 0.5) == [(s, e, pytest.approx(pk)) for s, e, pk in T.segments(p, 0.5)]
    g = torch.Generator().manual_seed(9)
    for _ in range(20):
        q = torch.rand(32, generator=g).tolist()
        for mf in (1, 2, 3):
            assert segments(q, 0.4, mf) == T.segments(q, 0.4, mf)


def test_pack_tscam_layout():
    """encoder.pack_tscam: column (c * 3 + d) * C + ch of row k is W[k][ch][c][d]; rows past N
    are zero; fragment (nt, ks), lane l, element j is row 16 nt + l % 16, column 32 ks + 8 (l //
    16) + j."""
    from zsaac.encoder import pack_tscam
    N, C = 17, 32
    W = torch.arange(N * C * 6, dtype=torch.float32).reshape(N, C, 2, 3)
    p = pack_tscam(W)
    assert p.shape == (2, 6, 4, 16, 8)
    m = torch.zeros(32, 6 * C)
    m[:N] = T.weight_matrix(W)
    flat = p.reshape(2, 6, 64, 8)
    for nt, ks, l, j in ((0, 0, 0, 0), (1, 5, 63, 7), (0, 3, 17, 2), (1, 2, 0, 5), (1, 0, 1, 0)):
        assert float(flat[nt, ks, l, j]) == float(m[16 * nt + l % 16, 32 * ks + 8 * (l // 16) + j])
    assert float(m[3, (1 * 3 + 2) * C + 9]) == float(W[3, 9, 1, 2])
    assert float(flat[1, :, 1:16].abs().max()) == 0.0 and float(flat[1, :, 17:32].abs().max()) == 0.0


def test_encode_events_refusals():
    """cnn14 has no such head; a checkpoint without tscam_conv.* is refused by the head's setup
    alone (checked on the methods' host code, no device needed)."""
    from zsaac.encoder import AudioEncoder
    e = AudioEncoder.__new__(AudioEncoder)
    e.kind, e._tagw, e._tagbuf, e._tscam = "cnn14", {}, None, (None, None)
    with pytest.raises(NotImplementedError):
        e._tag_setup()
    e.kind = "htsat"
    with pytest.raises(KeyError, match="tscam_conv"):
        e._tag_setup()
