"""The GEMM family op by op on the GPU against the plain float64 references of tests/gemm_ref.py:
zs_gemm on every route (lean tiles, gemm_big_kernel, the gemm_fast_kernel ring in bf16 and f32,
split-K, the register-staged gemm_kernel<T>, the rows kernel, the skinny kernel), zs_gemm_ln,
zs_gemm_ln_f32 and zs_lmhead_topk_t.

Every operand is a view of a strided buffer with NaN in its padding columns and in one extra row
(nothing outside the operand may reach a result); every output is a gpu_helpers.Out, sentinel
filled with a guard row, and in a strided output the padding columns must still hold the sentinel
afterwards.  The comparison runs on the CPU under the project's rule (mistral_ref.tolerance):
yardstick = the float32 formula's largest deviation from float64 on the case's own data,
tolerance 4 x yardstick + 1e-6 against the float64 value before the output rounding; a bf16
output adds 2^-8 |ref| elementwise (its own rounding).  Integer-valued
operands (|v| <= 3) must come out exactly.  tests/test_gemm_ref.py shows on the CPU that these
cases tell each arithmetic error of gemm_ref.MUTANTS from the reference.  Each test prints
error / yardstick per case (pytest -s).

Knobs are set through ``knobs`` below only; it restores the previous values on the way out."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402
from gpu_helpers import Out, offset  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SENT = R.OUT_SENTINEL

# zs_tune_set has no getter: the first change of a knob starts from the library's default
# (gemm_ref.KNOB_DEFAULTS, checked against csrc by tests/test_gemm_ref.py), later ones from what
# this file set last; every other test file restores its knobs to the same defaults.
_KNOBS = dict(R.KNOB_DEFAULTS)


@contextlib.contextmanager
def knobs(**kw):
    from zsaac._lib import call
    old = {k: _KNOBS[k] for k in kw}
    try:
        for k, v in kw.items():
            call("zs_tune_set", k.encode(), v)
            _KNOBS[k] = v
        yield
    finally:
        for k, v in old.items():
            call("zs_tune_set", k.encode(), v)
            _KNOBS[k] = v


def _act(name):
    return R.ACTS.index(name)


# ------------------------------------------------------------------ running one strided case
def _outbuf(dev, c):
    """The output view [M, N] inside a sentinel-filled Out of [M][ldo] (+ guard row), at the
    layout's element offset; alias: the residual's values placed in it."""
    M, N = c["M"], c["N"]
    ldo, off = R.out_layout(N, c["layout"], c["out_dtype"])
    o = Out(dev, (M, ldo), c["out_dtype"], SENT)
    view = o.buf.as_strided((M, N), (ldo, 1), off)
    if c["alias"]:
        view.copy_(c["res"].to(dev))
    return o, view, ldo, off


def _collect(o, M, N, ldo, off):
    """-> the [M, N] result in float64; asserts the padding and the guard row kept the sentinel."""
    full = o.buf.cpu().double()
    mask = torch.zeros(full.numel(), dtype=torch.bool)
    mask.as_strided((M, N), (ldo, 1), off).fill_(True)
    assert bool((full[~mask] == SENT).all()), "write outside the output (padding / guard row)"
    return full.as_strided((M, N), (ldo, 1), off).clone()


def _epi_args(dev, c, view):
    bias = None
    if c["bias"] is not None:
        bias = offset(c["bias"], dev) if c["bias_off"] else c["bias"].to(dev)
    res = None
    if c["alias"]:
        res = view
    elif c["rbuf"] is not None:
        res = c["rbuf"].to(dev)[:c["M"], :c["N"]]
    return bias, res


def _compare(label, got, ref, yard, tol):
    err = (got - ref).abs()
    bad = ~(err <= tol)
    worst = float((err / tol).nan_to_num(nan=float("inf")).max())
    print(f"{label}: err {float(err.nan_to_num(nan=float('inf')).max()):.3e} yardstick {yard:.3e} "
          f"err/tol {worst:.3f}")
    assert not bool(bad.any()), (label, int(bad.sum()), float(err[bad].max()), yard)
    return worst


def _run_gemm(dev, label, c, split_k=1, ws=None):
    from zsaac import ops
    a = c["abuf"].to(dev)[:c["M"], :c["K"]]
    w = c["wbuf"].to(dev)[:c["N"], :c["K"]]
    o, view, ldo, off = _outbuf(dev, c)
    bias, res = _epi_args(dev, c, view)
    if split_k > 1 and ws is None:
        ws = torch.full((split_k * c["M"] * c["N"] + 8,), float("nan"), device=dev)
    ops.gemm(a, w, view, bias=bias, residual=res, act=_act(c["act"]), split_k=split_k, workspace=ws)
    got = _collect(o, c["M"], c["N"], ldo, off)
    ref, yard, tol = R.gemm_expect(c)
    worst = _compare(label + ("/bf16out" if c["out_dtype"] == BF16 else "/f32out"), got, ref, yard, tol)
    if c["out_dtype"] == BF16:
        worst = 0.0          # (by construction up to 1: the output's own rounding is the tolerance)
    if c["kind"] == "ints" and c["act"] in ("none", "relu"):
        # integer operands: exact, and a bf16 output is the exact value rounded once
        assert torch.equal(got, R._round(ref, c["out_dtype"] if c["out_dtype"] == BF16 else None)), label
    return worst


def _sweep(dev, route, split_k=None, ws=None, extra=()):
    """The route's two 12-epilogue sweeps (ragged N, N % 8 == 0), an M = 1 case and integer
    operands with a plain and with a full epilogue."""
    M, Nr, Na, K, dt, sk = R.SWEEPS[route]
    sk = sk if split_k is None else split_k
    worst = 0.0
    for aligned in (False, True):
        for label, c in R.sweep(route, aligned):
            worst = max(worst, _run_gemm(dev, label, c, sk, ws))
    for i, (m, n, kind) in enumerate(((1, Nr, "randn"), (1, Na, "randn"), (M, Nr, "ints"),
                                      (M, Na, "ints")) + tuple(extra)):
        epi = R.EPILOGUES[(0, 3, 0, 3)[i % 4]] if kind == "ints" else R.EPILOGUES[(2, 1)[i % 2]]
        c = R.gemm_case(m, n, K, dt, epi, R._seed(route, "x", i), kind=kind)
        worst = max(worst, _run_gemm(dev, f"{route}/M{m}N{n}/{kind}", c, sk, ws))
    print(f"{route}: closest f32-output case err/tol {worst:.3f}")


# ------------------------------------------------------------------ 1. lean tiles
# fast_tile 100 + t -> (BM, BN, NS, BK_); 102 takes 128 x 64 at M >= N, else 64 x 128; 104 falls
# through to the 64 x 64 4-stage tile
LEAN = {101: (128, 128, 2, 64), 102: (128, 64, 3, 64), 103: (64, 64, 2, 128), 104: (64, 64, 4, 64),
        105: (256, 128, 2, 64), 106: (128, 256, 2, 64), 107: (256, 256, 2, 64),
        108: (256, 128, 3, 64), 109: (128, 256, 3, 64), 110: (256, 128, 3, 64),
        111: (128, 128, 3, 64), 112: (128, 128, 4, 64), 113: (128, 96, 2, 64)}


def _pipeline_edges(dev, name, BM, BN, NS, BK, dt=BF16, swap=False, split_k=1):
    """nk = K / BK_ = 1 .. NS + 1 k tiles (which counted waits of the ring run) at two tiles plus
    a ragged remainder in M and N (an nv < 8 column tail), epilogues rotating through the table."""
    M, N = BM + 5, BN + 6
    if swap:
        M, N = BN + 5, BM + 6
    for nk in range(1, NS + 2):
        for j in range(2):
            i = (2 * nk + j + NS) % len(R.EPILOGUES)
            c = R.gemm_case(M, N, nk * BK, dt, R.EPILOGUES[i], R._seed(name, nk, j),
                            kind="ints" if j and R.EPILOGUES[i][4] in ("none", "relu") else "randn")
            _run_gemm(dev, f"{name}/nk{nk}/e{i}", c, split_k)


@pytest.mark.parametrize("tile", sorted(LEAN))
def test_gemm_lean_tile_pipeline_edges(cuda, tile):
    BM, BN, NS, BK = LEAN[tile]
    with knobs(fast_tile=tile):
        _pipeline_edges(cuda, f"lean{tile}", BM, BN, NS, BK)
        if tile == 102:
            _pipeline_edges(cuda, "lean102t", BM, BN, NS, BK, swap=True)


@pytest.mark.parametrize("route,kn", [("lean104", dict(fast_tile=104)), ("lean101", dict(fast_tile=101)),
                                      ("lean113", dict(fast_tile=113))])
def test_gemm_lean_epilogues(cuda, route, kn):
    """epi_slab at WN = 32, 64 and 96 over the whole epilogue table."""
    with knobs(**kn):
        _sweep(cuda, route)


@pytest.mark.parametrize("kn,M,N,K", [(dict(lean96=1), 6144 - 3, 768, 64),
                                      (dict(lean8w=1), 4096 - 3, 4096 - 2, 64),
                                      (dict(lean128_ns=4), 2048 - 3, 1024 + 6, 320),
                                      (dict(), 2048 - 3, 1024 + 6, 256)],
                         ids=["lean96", "lean8w", "lean128_ns4", "lean128_ns3"])
def test_gemm_lean_auto_knobs(cuda, kn, M, N, K):
    """The dispatch conditions the forced tiles bypass: lean96 and lean8w (their grid thresholds
    need 384 / 1024 tiles: K = 64 keeps them small), lean128_ns 4 and the default 3-stage 8-wave
    tile (128 <= n128 < 256)."""
    with knobs(**kn):
        c = R.gemm_case(M, N, K, BF16, R.EPILOGUES[7 if "lean8w" in kn else 1], R._seed("auto", M, N))
        _run_gemm(cuda, f"lean-auto{kn}/{M}x{N}x{K}", c)


# ------------------------------------------------------------------ 2. gemm_big_kernel
def test_gemm_big_tile(cuda):
    with knobs(fast_tile=18):
        for nk in (1, 2, 3, 4):
            for j in range(3):
                i = (3 * nk + j) % len(R.EPILOGUES)
                c = R.gemm_case(261, 262, 64 * nk, BF16, R.EPILOGUES[i], R._seed("big", nk, j))
                _run_gemm(cuda, f"big18/nk{nk}/e{i}", c)
        _sweep(cuda, "big18")


# ------------------------------------------------------------------ 3. the gemm_fast_kernel ring
RING = {1: (256, 256, 4, 32), 2: (256, 128, 4, 32), 3: (128, 256, 4, 32), 4: (128, 128, 2, 64),
        5: (128, 128, 4, 32), 6: (256, 256, 2, 64), 7: (128, 128, 6, 32), 8: (128, 64, 3, 64),
        9: (64, 128, 3, 64), 10: (128, 128, 3, 64), 11: (128, 128, 2, 32), 12: (128, 128, 3, 32),
        13: (64, 64, 2, 64), 14: (128, 128, 4, 64), 15: (256, 128, 2, 64), 16: (128, 256, 2, 64),
        17: (64, 64, 2, 128)}


@pytest.mark.parametrize("tile", sorted(RING))
def test_gemm_ring_tile_pipeline_edges(cuda, tile):
    BM, BN, NS, BK = RING[tile]
    with knobs(fast_tile=tile):
        _pipeline_edges(cuda, f"ring{tile}", BM, BN, NS, BK)


def test_gemm_ring_epilogues_and_short_k(cuda):
    """gemm_lean 0 sends bf16 to gemm_fast_kernel; K % 64 != 0 does so with the lean tiles on."""
    with knobs(gemm_lean=0):
        _sweep(cuda, "ring")
        with knobs(fast_xcd=0):
            _sweep(cuda, "ring")
    for K in (32, 96, 160):
        for j in range(3):
            i = (K // 32 + 4 * j) % len(R.EPILOGUES)
            c = R.gemm_case(69, 70, K, BF16, R.EPILOGUES[i], R._seed("shortk", K, j))
            _run_gemm(cuda, f"ring/K{K}/e{i}", c)


@pytest.mark.parametrize("dt", [BF16, F32])
def test_gemm_split_k(cuda, dt):
    """Ring slabs + splitk_reduce_kernel at split_k 2 and 3: N % 4 != 0 (the scalar workspace
    store), a short last split (K = 160: 64 + 64 + 32 and 96 + 64); the workspace starts as NaN."""
    route = "splitk" if dt == BF16 else "splitk_f32"
    for sk in (2, 3):
        _sweep(cuda, route, split_k=sk)
    for K, sk in ((256, 2), (384, 3), (192, 3)):       # even splits; 128-deep k steps at 256 / 2
        c = R.gemm_case(133, 134, K, dt, R.EPILOGUES[4], R._seed("sk", K, sk))
        _run_gemm(cuda, f"splitk/K{K}/s{sk}", c, sk)


@pytest.mark.parametrize("persist", [1, 0])
def test_gemm_ring_persistent_loop(cuda, persist):
    """More 64 x 64 tiles than launch_fast's 256 x per_cu (2) workgroups: the persistent loop
    with its cross-tile prefetch, ragged last tile row and column (so a next tile with and
    without a full prefetch), in one slab and with split_k 3; fast_persist 0 = one workgroup per
    tile on the same problems."""
    with knobs(gemm_lean=0, fast_persist=persist):
        c = R.gemm_case(2112 - 10, 1024 - 2, 128, BF16, R.EPILOGUES[1], 71)     # 33 x 16 = 528 tiles
        _run_gemm(cuda, f"persist{persist}/2102x1022x128", c)
        c = R.gemm_case(704 - 10, 1024 - 2, 192, BF16, R.EPILOGUES[2], 72)      # 11 x 16 x 3 = 528
        _run_gemm(cuda, f"persist{persist}/694x1022x192/s3", c, 3)
        with knobs(fast_xcd=0):
            c = R.gemm_case(2112 - 10, 1024 - 2, 64, BF16, R.EPILOGUES[5], 73)
            _run_gemm(cuda, f"persist{persist}/xcd0", c)


# ------------------------------------------------------------------ 4. f32 on the ring
def test_gemm_f32_ring_epilogues(cuda):
    _sweep(cuda, "ring_f32")
    with knobs(f32_tile=0):
        _sweep(cuda, "ring_f32")


# (M, N) by the block-count thresholds of dispatch_fast_f32: 16 x 16 tiles of 128 x 128 (>= 256),
# 16 x 16 of 128 x 64 and of 64 x 128 (128 x 128 would give 128), and a small grid (64 x 64)
F32_SHAPES = {"128x128": (1930, 2040), "128x64": (1930, 1000), "64x128": (1000, 1930), "64x64": (133, 134)}


@pytest.mark.parametrize("shape", sorted(F32_SHAPES))
def test_gemm_f32_ring_tiles(cuda, shape):
    """The four default shapes (f32_tile 8) and round 4's (f32_tile 0); on the full grid also the
    forced variants 1-7, 10 and 11 (11 takes its 256 x 128 tile from 16 x 16 of those up).  One
    reference per shape, shared by the variants."""
    from zsaac import ops
    M, N = F32_SHAPES[shape]
    tiles = (8, 0) if shape != "128x128" else (8, 0, 1, 2, 3, 4, 5, 6, 7, 10, 11)
    for K in (96, 128):
        c = R.gemm_case(M, N, K, F32, R.EPILOGUES[9 if K == 96 else 2], R._seed("f32", shape, K))
        ref, yard, tol = R.gemm_expect(c)
        a = c["abuf"].to(cuda)[:M, :K]
        w = c["wbuf"].to(cuda)[:N, :K]
        for t in tiles:
            with knobs(f32_tile=t):
                o, view, ldo, off = _outbuf(cuda, c)
                bias, res = _epi_args(cuda, c, view)
                ops.gemm(a, w, view, bias=bias, residual=res, act=_act(c["act"]), split_k=1)
                _compare(f"f32/{shape}/K{K}/tile{t}", _collect(o, M, N, ldo, off), ref, yard, tol)
    if shape == "128x128":
        c = R.gemm_case(3850, 2040, 64, F32, R.EPILOGUES[0], 74, kind="ints")   # 16 x 16 of 256 x 128
        with knobs(f32_tile=11):
            _run_gemm(cuda, "f32/256x128/tile11", c)


# ------------------------------------------------------------------ 5. register-staged gemm_kernel<T>
@pytest.mark.parametrize("dt", [BF16, F32])
def test_gemm_register_staged(cuda, dt):
    """gemm_fast 0 / f32_fast 0: the three tile shapes dispatch_gemm reaches (64 x 64 at M <= 64,
    128 x 64, 128 x 128 at N >= 2048; its 64 x 128 needs M <= 64 and M > 64 at once) and split-K."""
    with knobs(gemm_fast=0, f32_fast=0):
        _sweep(cuda, "staged" if dt == BF16 else "staged_f32")
        for j, (M, N, K, sk) in enumerate(((40, 150, 96, 1), (64, 70, 160, 1), (130, 2054, 64, 1),
                                           (130, 150, 160, 3), (40, 70, 160, 2), (133, 2054, 96, 2))):
            c = R.gemm_case(M, N, K, dt, R.EPILOGUES[(5 * j + 2) % 12], R._seed("staged", j, M))
            _run_gemm(cuda, f"staged/{M}x{N}x{K}/s{sk}", c, sk)


# ------------------------------------------------------------------ 6. the rows kernel
ROWS_KS = (256, 512, 768, 1024, 1536, 2048, 3072, 3840, 4096)


def test_gemm_rows_epilogues(cuda):
    _sweep(cuda, "rows", extra=((15, 1002, "randn"), (16, 1000, "randn"), (64, 1002, "randn")))
    with knobs(rows_wide=1):                     # 32-column tiles below N = 1536
        _sweep(cuda, "rows")


@pytest.mark.parametrize("K", ROWS_KS)
def test_gemm_rows_plan(cuda, K):
    """Every K of rows_plan (S = 2, 4, 6, 8, 12 at 4 waves; 8, 12, 15, 16 at 8 waves) at N on both
    sides of 1536 (16- / 32-column tiles) and a ragged N; M = 1, 15, 16, 17, 64; and a row's bits
    do not depend on M."""
    from zsaac import ops
    for j, (M, N) in enumerate(((17, 1530), (64, 1544), (1, 1000), (15, 1002), (16, 1000))):
        c = R.gemm_case(M, N, K, BF16, R.EPILOGUES[(K // 256 + 5 * j) % 12], R._seed("rows", K, j),
                        lda=K + 8 * (j % 2), ldw=K + 8 * (j % 3 == 1))
        _run_gemm(cuda, f"rows/K{K}/{M}x{N}", c, 0)
    with knobs(rows_wide=1):
        c = R.gemm_case(17, 1002, K, BF16, R.EPILOGUES[2], R._seed("rowsw", K))
        _run_gemm(cuda, f"rows_wide/K{K}", c, 0)
    c = R.gemm_case(64, 1000, K, BF16, R.EPILOGUES[0], R._seed("rowsM", K))
    a = c["a"].contiguous().to(cuda)
    w = c["w"].contiguous().to(cuda)
    o64, o1 = Out(cuda, (64, 1000), F32, SENT), Out(cuda, (1, 1000), F32, SENT)
    ops.gemm(a, w, o64.t)
    ops.gemm(a[:1], w, o1.t)
    assert torch.equal(o64.cpu()[0], o1.cpu()[0])


def test_gemm_rows_uncovered_k_falls_through(cuda):
    """K = 640 is in no plan: auto mode goes on to the tiled kernel (no workspace) or the skinny
    kernel (workspace given) and is still right."""
    from zsaac import ops
    for j, M in enumerate((1, 17, 64)):
        c = R.gemm_case(M, 1002, 640, BF16, R.EPILOGUES[2 + j], R._seed("k640", M))
        _run_gemm(cuda, f"k640/tiled/M{M}", c, 0)
        ws = ops.skinny_workspace(cuda, [(M, 1002, 640)])
        _run_gemm(cuda, f"k640/skinny/M{M}", c, 0, ws)


# ------------------------------------------------------------------ 7. the skinny kernel
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("dt", [BF16, F32])
def test_gemm_skinny(cuda, dt, mode):
    """gemm_rows 0, a private zeroed workspace, both slab modes: the epilogue table; row blocks at
    M = 1, 64, 65, 200, 256; K with one split (64) and several; bf16 above 64 rows takes the
    skinny kernel only for K >= 2048 on a small grid."""
    from zsaac import ops
    route = "skinny" if dt == BF16 else "skinny_f32"
    with knobs(gemm_rows=0, skinny_mode=mode):
        shapes = [(m, 70, k) for m in (1, 64, 65, 200, 256) for k in (64, 256, 2048)]
        ws = ops.skinny_workspace(cuda, shapes + [(R.SWEEPS[route][0], 72, 256)])
        assert ws is not None
        _sweep(cuda, route, ws=ws)
        for j, M in enumerate((1, 64, 65, 200, 256)):
            for K in ((64, 256) if dt == F32 or M <= 64 else (2048,)):
                c = R.gemm_case(M, 70, K, dt, R.EPILOGUES[(3 * j + K // 64) % 12], R._seed("sk", M, K),
                                lda=K + 8, ldw=K + 16)
                _run_gemm(cuda, f"skinny/M{M}/K{K}", c, 0, ws)
        # the counters re-arm: two shapes back to back on the one workspace, twice
        c1 = R.gemm_case(64, 134, 256, dt, R.EPILOGUES[2], 81)
        c2 = R.gemm_case(33, 70, 512, dt, R.EPILOGUES[9], 82)
        for rep in range(2):
            _run_gemm(cuda, f"skinny/rearm{rep}/a", c1, 0, ws)
            _run_gemm(cuda, f"skinny/rearm{rep}/b", c2, 0, ws)
        assert bool((ws.view(torch.int32)[:R.SK_MAX_TILES] == 0).all())    # every tile counter re-armed


# ------------------------------------------------------------------ 8. host refusals
def test_gemm_host_refusals(cuda):
    """Each returns an error before any launch: the sentinel-filled output is untouched."""
    from zsaac._lib import ZS_BF16, ZS_F32, ZsError, call
    o = Out(cuda, (8, 64), F32, SENT)
    a = torch.zeros(9, 72, device=cuda, dtype=BF16)
    w = torch.zeros(65, 72, device=cuda, dtype=BF16)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()      # noqa: E731

    def gemm(M=8, N=64, K=64, dt=ZS_BF16, A=P(a), lda=72, W=P(w), ldw=72, split_k=1, ws=None):
        call("zs_gemm", M, N, K, dt, A, lda, W, ldw, None, None, 0, P(o.t), 64, ZS_F32, 0, split_k,
             ws, st)

    bad = dict(k48=dict(K=48), lda=dict(lda=68), ldw=dict(ldw=76), lda_short=dict(lda=56),
               ldw_short=dict(ldw=56), a_mis=dict(A=P(a) + 4),
               w_mis=dict(W=P(w) + 8), split=dict(split_k=2), dtype=dict(dt=7), neg_m=dict(M=-1),
               neg_split=dict(split_k=-1))
    for name, kw in bad.items():
        with pytest.raises(ZsError):
            gemm(**kw)
        torch.cuda.synchronize()
        assert bool((o.cpu() == SENT).all()), name
    gemm(M=0)                                    # nothing to do is not an error
    assert bool((o.cpu() == SENT).all())
    x = torch.zeros(8, 768, device=cuda)
    wl = torch.zeros(64, 768, device=cuda, dtype=BF16)
    for kw in (dict(M=65), dict(K=640), dict(ldx=770), dict(ldw=772), dict(ldx=764), dict(ldw=760)):
        args = dict(M=8, K=768, ldx=768, ldw=768)
        args.update(kw)
        with pytest.raises(ZsError):
            call("zs_gemm_ln", args["M"], 64, args["K"], P(x), args["ldx"], None, None, 1e-5, P(wl),
                 args["ldw"], None, None, 0, P(o.t), 64, ZS_F32, 0, st)
    wf = torch.zeros(64, 768, device=cuda)
    for kw in (dict(M=65), dict(K=640), dict(ldx=770), dict(ldw=770), dict(ldx=764), dict(ldw=764)):
        args = dict(M=8, K=768, ldx=768, ldw=768)
        args.update(kw)
        with pytest.raises(ZsError):
            call("zs_gemm_ln_f32", args["M"], 64, args["K"], P(x), args["ldx"], None, None, 1e-5,
                 P(wf), args["ldw"], None, None, 0, P(o.t), 64, 0, st)
    pv, pi = Out(cuda, (8, 1, 5), F32, SENT), Out(cuda, (8, 1, 5), torch.int32, -7)
    for kw in (dict(topk=9), dict(topk=0), dict(lda=68), dict(lda=56), dict(K=48), dict(temp=0.0),
               dict(row_norm=1, temp=0.5), dict(A=P(a) + 4), dict(dt=7)):
        args = dict(K=64, A=P(a), lda=72, topk=5, row_norm=0, temp=1.0, dt=ZS_BF16)
        args.update(kw)
        with pytest.raises(ZsError):
            call("zs_lmhead_topk_t", 8, args["K"], 65, args["dt"], args["A"], args["lda"], P(w),
                 args["topk"], args["row_norm"], float(args["temp"]), None, P(pv.t), P(pi.t), st)
    torch.cuda.synchronize()
    assert bool((o.cpu() == SENT).all()) and bool((pv.cpu() == SENT).all()) and bool((pi.cpu() == -7).all())


# ------------------------------------------------------------------ zs_gemm_ln, zs_gemm_ln_f32
def _run_ln(dev, s, f32):
    from zsaac import ops
    c = R.ln_build(s, F32 if f32 else BF16)
    M, N, K = s["M"], s["N"], s["K"]
    x = c["xbuf"].to(dev)[:M, :K]
    w = c["w"].to(dev)
    o, view, ldo, off = _outbuf(dev, c)
    bias, res = _epi_args(dev, c, view)
    lw = c["ln_w"].to(dev) if c["ln_w"] is not None else None
    lb = c["ln_b"].to(dev) if c["ln_b"] is not None else None
    with knobs(**s["knobs"]):
        (ops.gemm_ln_f32 if f32 else ops.gemm_ln)(x, lw, lb, w, view, bias=bias, residual=res,
                                                  act=_act(c["act"]), eps=c["eps"])
    got = _collect(o, M, N, ldo, off)
    if f32 and not s["affine"]:                  # no LayerNorm at all: a plain GEMM of x
        args = (c["x"], c["w"], c["bias"], c["res"], c["act"], F32)
        ref = R.gemm(*args, dtype=F64).double()
        yard, tol = R.tolerance(ref, R.gemm(*args, dtype=F32), c["out_dtype"] == BF16)
    else:
        # zs_gemm_ln rounds the normalised rows to bf16: the float32 twin with the same rounding
        # is the yardstick
        ref, yard, tol = R.ln_expect(c, None if f32 else BF16)
    label = s["id"] + f"/M{M}" + ("/bf16out" if c["out_dtype"] == BF16 else "/f32out")
    if not f32:
        print(f"{label}: largest rounding-tie allowance {float(R.ln_flip_allowance(c).max()):.3e}")
    return _compare(label, got, ref, yard, tol)


@pytest.mark.parametrize("spec", R.ln_specs(), ids=lambda s: s["id"])
def test_gemm_ln(cuda, spec):
    _run_ln(cuda, spec, False)
    for M in R.LN_MS:                            # every row count on every tile / mode
        if M != spec["M"]:
            _run_ln(cuda, dict(spec, M=M, seed=spec["seed"] + M), False)


@pytest.mark.parametrize("spec", R.ln_f32_specs(), ids=lambda s: s["id"])
def test_gemm_ln_f32(cuda, spec):
    _run_ln(cuda, spec, True)
    for M in R.LN_MS:
        if M != spec["M"]:
            _run_ln(cuda, dict(spec, M=M, seed=spec["seed"] + M), True)


@pytest.mark.parametrize("affine", [True, False], ids=["aff", "norm"])
def test_gemm_ln_epilogues(cuda, affine):
    """gemm_rows_kernel's LN instantiations (LNM 1 / 2) over the whole epilogue table, ragged and
    aligned N: bf16 and f32 output, every activation (the decode step's ln_2 -> c_fc is gelu_new
    with bf16 output), every layout, bias and residual form."""
    worst = 0.0
    for s in R.ln_epi_specs(affine):
        r = _run_ln(cuda, s, False)
        worst = max(worst, r if s["epi"][2] == F32 else 0.0)
    print(f"ln-epi-{'aff' if affine else 'norm'}: closest f32-output case err/tol {worst:.3f}")


def test_gemm_ln_f32_epilogues(cuda):
    """gemm_rows_f32_kernel's own epilogue over every f32-output row of the table, ragged N."""
    for i, epi in enumerate(R.F32_EPIS):
        for ln, K in ((True, 768), (False, 1024)):
            _run_ln(cuda, dict(id=f"lnf32-epi{i}-K{K}", M=17, N=70, K=K, affine=ln, epi=epi,
                               ldx=K + 4, knobs={}, seed=500 + i), True)


def test_gemm_ln_row_independent_of_m(cuda):
    from zsaac import ops
    c = R.ln_case(64, 202, 768, BF16, R.EPILOGUES[0], 91)
    x, w = c["x"].contiguous().to(cuda), c["w"].to(cuda)
    lw, lb = c["ln_w"].to(cuda), c["ln_b"].to(cuda)
    o64, o1 = Out(cuda, (64, 202), F32, SENT), Out(cuda, (1, 202), F32, SENT)
    ops.gemm_ln(x, lw, lb, w, o64.t)
    ops.gemm_ln(x[:1], lw, lb, w, o1.t)
    assert torch.equal(o64.cpu()[0], o1.cpu()[0])


# ------------------------------------------------------------------ zs_lmhead_topk_t
def _run_lmhead(dev, s, c=None, rows=None):
    """-> (stat, val, idx) on the CPU; rows: a row gather of A (the permutation test)."""
    from zsaac import ops
    c = c or R.lm_build(s)
    M, V, K, topk = s["M"], s["V"], s["K"], s["topk"]
    nblk = ops.lmhead_nblk(V)
    assert nblk == (V + 127) // 128
    abuf = c["abuf"]
    if rows is not None:
        abuf = torch.cat([abuf[rows], abuf[-1:]])
        M = len(rows)
    a = abuf.to(dev)[:M, :K]
    w = c["wbuf"].to(dev)[:V]
    ps = Out(dev, (M, nblk, 2), F32, SENT)
    pv = Out(dev, (M, nblk, topk), F32, SENT)
    pi = Out(dev, (M, nblk, topk), torch.int32, -7)
    with knobs(**s["knobs"]):
        ops.lmhead_topk(a, w, topk, ps.t if s["stat"] else None, pv.t, pi.t, row_norm=s["row_norm"],
                        temperature=s["temp"])
    return ps.cpu(), pv.cpu(), pi.cpu()


@pytest.mark.parametrize("spec", R.lm_specs(), ids=lambda s: s["id"])
def test_lmhead_topk(cuda, spec):
    s = spec
    c = R.lm_build(s)
    stat, val, idx = _run_lmhead(cuda, s, c)
    r64 = R.lmhead(c["a"], c["w"], s["topk"], s["row_norm"], s["temp"])
    r32 = R.lmhead(c["a"], c["w"], s["topk"], s["row_norm"], s["temp"], dtype=F32)
    # every (row, block) written; indices and order exact; padding entries as documented
    assert not bool((idx == -7).any()) and not bool((val == SENT).any())
    assert torch.equal(idx.long(), r64["idx"]), s["id"]
    pad = r64["idx"] == R.PAD_IDX
    assert bool((val[pad] == -R.INF).all())
    assert bool(pad.any()) == (s["V"] % 128 != 0 and s["V"] % 128 < s["topk"])
    yard, tol = R.tolerance(r64["val"][~pad], r32["val"][~pad])
    _compare(s["id"] + "/val", val.double()[~pad], r64["val"][~pad], yard, tol)
    if not s["row_norm"] and s["temp"] == 1.0:   # exact logits: exact values
        assert torch.equal(val.double()[~pad], r64["val"][~pad])
    if not s["stat"]:
        assert bool((stat == SENT).all())        # part_stat NULL: nothing written
        return
    assert not bool((stat == SENT).any())
    tols = R.lm_stat_tolerance(r64, r32)       # (the sum-exp rule: see there)
    _compare(s["id"] + "/max", stat.double()[..., 0], r64["stat"][..., 0], *tols["max"])
    _compare(s["id"] + "/sumexp", stat.double()[..., 1], r64["stat"][..., 1], *tols["sumexp"])
    g = stat.double()[..., 0].max(-1)[0]
    lse = g + torch.log((stat.double()[..., 1] * torch.exp(stat.double()[..., 0] - g[:, None])).sum(-1))
    _compare(s["id"] + "/lse", lse, r64["lse"], *tols["lse"])


@pytest.mark.parametrize("mode", R.LM_MODES)
def test_lmhead_rows_permute_and_repeat(cuda, mode):
    """A row's results do not depend on its position in the launch or on the row count: bitwise."""
    s = dict(R.lm_named("V1000-M130-K96-f32_ring-k8-grid"), mode=mode, stat=True, kind="randn")
    s["knobs"] = dict(f32_fast=0 if mode == "f32_tile" else 1)
    c = R.lm_build(s)
    base = _run_lmhead(cuda, s, c)
    g = torch.Generator().manual_seed(9)
    for n in (130, 97, 65):      # (all on the 128-row kernel, as the 130 rows)
        rows = torch.randint(0, 130, (n,), generator=g)
        got = _run_lmhead(cuda, s, c, rows)
        for b, t in zip(base, got):
            assert torch.equal(b[rows], t), (mode, n)
