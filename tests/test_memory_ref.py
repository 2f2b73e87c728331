"""CPU: tests/memory_ref.py against the four-line formula, the input conditions of the GPU cases,
construct_support_memory's reading rule on temporary pickle streams, and the argument refusals of
the zs_memory_* exports (they run on the host before any launch, so no GPU is needed)."""
import math
import os
import pickle
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memory_ref as MR  # noqa: E402

F64 = torch.float64


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_reference_equals_the_formula(dt):
    c = MR.spread_case(5, 333, 1024, dt)
    q, T = c["q"].to(F64), c["b"].to(F64)
    w = (c["scale"] * (q @ T.T)).softmax(dim=-1)
    mix = w @ T
    out = mix / mix.norm(dim=-1, keepdim=True)
    assert torch.allclose(c["w"], w, rtol=1e-12, atol=1e-300)
    assert torch.allclose(c["mix"], mix, rtol=1e-12, atol=1e-15)
    assert torch.allclose(c["out"], out, rtol=1e-12, atol=1e-15)
    assert torch.allclose(c["lse"], torch.logsumexp(c["scale"] * (q @ T.T), dim=-1), rtol=1e-13, atol=0)
    assert torch.allclose(c["ess"], 1.0 / (w * w).sum(-1), rtol=1e-12, atol=0)
    assert torch.allclose(c["A"], w @ T.abs(), rtol=1e-12, atol=1e-15)
    # the buffers are NaN outside the views
    assert bool(torch.isnan(c["qbuf"][-1]).all()) and bool(torch.isnan(c["bbuf"][:, -8:]).all())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_tolerances_are_the_derived_ones(dt):
    c = MR.spread_case(3, 63, 32, dt)
    eps_p = 2.0 ** -8 if dt == "bf16" else 0.0
    assert c["tau"] == 4.0 * c["yard"] + 1e-6
    eps = math.expm1(2.0 * c["scale"] * c["tau"]) + eps_p + 2.0 ** -20
    assert c["eps"] == eps
    assert torch.equal(c["mix_tol"], 2.0 * eps * c["A"] + 1e-6)
    assert c["lse_tol"] == c["scale"] * c["tau"] + eps_p + 1e-6
    assert torch.equal(c["out_tol"], c["mix_tol"] / c["norm"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_spread_cases_keep_their_support(dt):
    """Every row of the spread cases with N >= 256 mixes at least ESS_MIN bank rows (float64)."""
    seen = 0
    for M, N, K in MR.SPREAD_CASES:
        c = MR.spread_case(M, N, K, dt)
        assert c["scale"] == 1.5 * math.sqrt(K)
        assert torch.allclose(c["b"].to(F64).norm(dim=1), torch.ones(N, dtype=F64), atol=1e-2)
        if N >= 256:
            seen += 1
            print(f"{dt} {M}x{N}x{K}: min ess {float(c['ess'].min()):.1f}")
            assert float(c["ess"].min()) >= MR.ESS_MIN
    assert seen == 4


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_ref_scale_case_is_as_planted(dt):
    c = MR.ref_scale_case(dt)
    M, N, K = MR.REF_CASE
    q, b = c["q"].to(F64), c["b"].to(F64)
    cos = q @ b.T
    assert abs(float(cos[0, N - 1]) - 0.95) < 1e-2 and abs(float(cos[1, 0]) - 0.95) < 1e-2
    assert abs(float(cos[2, N // 2]) - 0.6) < 1e-2
    # row 0: everything before the last bank row is weighted by less than e^-80 against it
    z = c["scale"] * cos
    assert float(z[0, N - 1] - z[0, :N - 1].max()) > 80.0
    assert float(z[1, 0] - z[1, 1:].max()) > 80.0
    assert float(c["w"][0, N - 1]) == 1.0 and float(c["w"][1, 0]) == 1.0      # to float64 precision
    assert float(c["w"][2, N // 2]) > 0.99


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N", MR.EXACT_NS)
def test_exact_case_is_exact(N, dt):
    c = MR.exact_case(N, dt)
    assert torch.equal(c["b"].float() * 8, (c["b"].float() * 8).round())
    assert float(c["b"].float().abs().max()) <= 2.0
    assert torch.equal(c["mix"].to(torch.float32), c["mean"])
    assert torch.allclose(c["lse"], torch.full_like(c["lse"], math.log(N)), rtol=1e-15, atol=0)
    # every column sum is exact in f32 in any order: |sum| <= 2 N in steps of 1/8
    assert 2 * N * 8 < 2 ** 24


def test_merge_reference_against_the_whole():
    """Partials cut from one softmax merge back to it (float64), empty splits included."""
    g = torch.Generator().manual_seed(3)
    z = torch.randn(4, 90, generator=g, dtype=F64) * 20
    b = torch.randn(90, 32, generator=g, dtype=F64)
    cuts = [(0, 40), (40, 40), (40, 77), (77, 90)]
    pm = torch.zeros(4, len(cuts), 32, dtype=F64)
    pl = torch.zeros(4, len(cuts), 2, dtype=F64)
    for s, (lo, hi) in enumerate(cuts):
        if lo == hi:
            pl[:, s, 0] = -MR.INF
            continue
        m = z[:, lo:hi].max(dim=1).values
        e = torch.exp(z[:, lo:hi] - m[:, None])
        pm[:, s], pl[:, s, 0], pl[:, s, 1] = e @ b[lo:hi], m, e.sum(1)
    mix, lse = MR.merge(pm, pl)
    assert not bool(torch.isnan(mix).any())
    assert torch.allclose(mix, z.softmax(-1) @ b, rtol=1e-12, atol=1e-14)
    assert torch.allclose(lse, torch.logsumexp(z, -1), rtol=1e-13, atol=0)
    a, ml = MR.scripted_partials(6, 7, 32, 1)
    assert bool((ml[0, :, 1] > 0).sum() == 1) and bool(torch.isinf(ml[:, 1::3, 0]).all())
    mix, lse = MR.merge(a, ml)
    assert bool(torch.isfinite(mix).all()) and bool(torch.isfinite(lse).all())


# ------------------------------------------------------------------ construct_support_memory
def _rec(words, val, K=8):
    return {"caption": " ".join(["w"] * words), "text_embedding": torch.full((1, K), float(val)),
            "audio_id": f"id{val}"}


def test_construct_support_memory_reading_rule(tmp_path):
    from zsaac.memory import construct_support_memory, read_support_items
    p1, p2 = str(tmp_path / "a.pkl"), str(tmp_path / "b.pkl")
    with open(p1, "wb") as f:      # a stream: single records at the word-count edges, then a list
        for words, val in ((7, 1), (8, 2), (20, 3), (21, 4)):
            pickle.dump(_rec(words, val), f)
        pickle.dump([_rec(2, 5), _rec(40, 6)], f)       # a list is taken whole
    with open(p2, "wb") as f:
        pickle.dump([_rec(9, 7)], f)
        pickle.dump(_rec(12, 8), f)
    items = read_support_items([p1, p2])
    assert [it["audio_id"] for it in items] == ["id2", "id3", "id5", "id6", "id7", "id8"]
    feats = construct_support_memory([p1, p2])
    assert feats.shape == (6, 8) and feats.dtype == torch.float32
    assert torch.allclose(feats, torch.full((6, 8), 1.0 / math.sqrt(8.0)))
    # other limits, one path as a string
    assert [it["audio_id"] for it in read_support_items([p1], 7, 21)] == ["id1", "id2", "id3", "id4",
                                                                          "id5", "id6"]
    assert construct_support_memory(p2).shape == (2, 8)
    # rows with several embeddings per record are concatenated
    with open(p2, "wb") as f:
        pickle.dump([{"caption": "x", "text_embedding": torch.ones(3, 8)}], f)
    assert construct_support_memory([p2]).shape == (3, 8)


def test_construct_support_memory_refuses_code(tmp_path):
    from zsaac.memory import construct_support_memory
    p = str(tmp_path / "evil.pkl")
    with open(p, "wb") as f:
        pickle.dump(os.path.join, f)
    with pytest.raises(pickle.UnpicklingError):
        construct_support_memory([p])


# ------------------------------------------------------------------ host-side refusals
def test_abi_refusals_need_no_gpu():
    from zsaac import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    buf = (torch.zeros(4096 + 16).data_ptr() + 15) // 16 * 16      # never dereferenced
    ok = dict(M=4, N=64, K=64, dt=0, ldq=64, ldb=64, ns=2)

    def project(**kw):
        a = dict(ok, **kw)
        return lib.zs_memory_project(a["M"], a["N"], a["K"], a["dt"], buf, a["ldq"], buf, a["ldb"],
                                     100.0, a["ns"], buf, buf, None)
    for kw, word in ((dict(K=30, ldq=32, ldb=32), "K % 32"), (dict(K=1056, ldq=1056, ldb=1056), "K % 32"),
                     (dict(ldb=32), "ldq / ldb"), (dict(N=0), "M, N > 0"), (dict(M=0), "M, N > 0"),
                     (dict(ldq=68), "ldq / ldb"), (dict(dt=2), "dtype"), (dict(ns=0), "nsplit")):
        assert project(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert lib.zs_memory_project(4, 64, 64, 0, None, 64, buf, 64, 100.0, 2, buf, buf, None) == -1
    assert "null" in _lib.last_error()
    assert lib.zs_memory_project(4, 64, 64, 0, buf + 4, 64, buf, 64, 100.0, 2, buf, buf, None) == -1
    assert "aligned" in _lib.last_error()
    assert lib.zs_memory_merge(buf, buf, 4, 2, 30, 1, buf, 32, None, None) == -1
    assert lib.zs_memory_merge(buf, buf, 4, 2, 64, 1, buf, 32, None, None) == -1
    assert "ldo" in _lib.last_error()
    assert lib.zs_memory_merge(buf, buf, 0, 2, 64, 1, buf, 64, None, None) == -1
    assert lib.zs_memory_merge(buf, None, 4, 2, 64, 1, buf, 64, None, None) == -1
    # the split count is a function of (N, K, dtype) alone
    assert lib.zs_memory_nsplit(1, 32, 0) == 1 and lib.zs_memory_nsplit(333, 1024, 1) == 1
    assert lib.zs_memory_nsplit(4099, 1024, 1) == 9
    assert lib.zs_memory_nsplit(1 << 20, 1024, 1) == lib.zs_memory_nsplit(1 << 16, 1024, 0) == 128
    assert lib.zs_memory_nsplit(0, 1024, 1) == -1 and lib.zs_memory_nsplit(64, 30, 1) == -1


def test_host_layer_refuses_cpu_tensors():
    from zsaac import memory, ops
    from zsaac._lib import ZsError
    t = torch.zeros(4, 32)
    with pytest.raises(ZsError):
        memory.SupportMemory(t, device="cpu")
    mem = memory.SupportMemory.__new__(memory.SupportMemory)       # no device needed for the check
    mem.K = 32
    with pytest.raises(ZsError):
        mem.project(t)
    with pytest.raises(ZsError):
        memory.map2memory(t, t)
    with pytest.raises(ZsError):
        ops.memory_project(t, t, 100.0, 1, torch.zeros(4, 1, 32), torch.zeros(4, 1, 2))
    with pytest.raises(ZsError):
        ops.memory_merge(torch.zeros(4, 1, 32), torch.zeros(4, 1, 2), 4, 1, 32, torch.zeros(4, 32))
