"""zs_memory_project / zs_memory_merge (csrc/memory.hip) against tests/memory_ref.py.  Operands are
NaN-padded views of [rows + 1][ld] buffers (a padding column or the extra row read shows as NaN),
outputs and partials are sentinel-filled with a guard row behind them.

Tolerances are memory_ref's derived ones (yardstick -> tau -> eps); every test prints the
yardstick, tau and the measured error over its bound.  lse is checked everywhere: it is the sharp
detector of a lost or doubled tile.  Exact data (scale 0, multiples of 1/8) must give the exact
column mean; rows must not depend on the launch; runs must be bit-identical."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memory_ref as MR  # noqa: E402
from gpu_helpers import Out  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32
SENT = -7.5
DTYPES = ["f32", "bf16"]


def _ops():
    from zsaac import ops
    return ops


def _views(dev, c, rows=None):
    M, K = c["q"].shape
    N = c["b"].shape[0]
    q = c["qbuf"].to(dev)[:M, :K]
    return (q if rows is None else q[rows[0]:rows[1]]), c["bbuf"].to(dev)[:N, :K]


def _project(dev, q, b, scale, nsplit=None, normalize=False):
    """zs_memory_project + zs_memory_merge into sentinel-filled buffers -> (out, lse) on the CPU."""
    ops = _ops()
    M, K = q.shape
    ns = nsplit if nsplit is not None else ops.memory_nsplit(b.shape[0], K, q.dtype)
    pm, pl = Out(dev, (M, ns, K), F32, SENT), Out(dev, (M, ns, 2), F32, SENT)
    out, lse = Out(dev, (M, K), F32, SENT), Out(dev, (M,), F32, SENT)
    ops.memory_project(q, b, scale, ns, pm.t, pl.t)
    ops.memory_merge(pm.t, pl.t, M, ns, K, out.t, normalize, lse.t)
    torch.cuda.synchronize()
    pm.cpu(), pl.cpu()                                  # guard rows
    return out.cpu(), lse.cpu()


def _check(tag, c, mix, lse, rows=slice(None), normalized=False):
    """Prints the figures, then asserts the derived bounds; -> the two error/bound ratios."""
    want, tol = (c["out"], c["out_tol"]) if normalized else (c["mix"], c["mix_tol"])
    assert not bool(torch.isnan(mix).any()) and not bool(torch.isnan(lse).any()), tag
    r_mix = float(((mix.double() - want[rows]).abs() / tol[rows]).max())
    r_lse = float((lse.double() - c["lse"][rows]).abs().max()) / c["lse_tol"]
    print(f"{tag}: yardstick {c['yard']:.2e} tau {c['tau']:.2e} eps {c['eps']:.2e} "
          f"|mix err|/bound {r_mix:.3f} |lse err|/bound {r_lse:.3f}")
    assert r_mix <= 1.0 and r_lse <= 1.0, tag
    return r_mix, r_lse


@pytest.fixture(scope="module")
def spread():
    return {(spec, dt): MR.spread_case(*spec, dt) for spec in MR.SPREAD_CASES for dt in DTYPES}


@pytest.fixture(scope="module")
def ref100():
    return {dt: MR.ref_scale_case(dt) for dt in DTYPES}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("spec", MR.SPREAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_spread(cuda, spread, spec, dt):
    c = spread[(spec, dt)]
    q, b = _views(cuda, c)
    mix, lse = _project(cuda, q, b, c["scale"])
    _check(f"{dt} {spec}", c, mix, lse)
    out, lse2 = _project(cuda, q, b, c["scale"], normalize=True)
    _check(f"{dt} {spec} normalised", c, out, lse2, normalized=True)
    assert torch.equal(lse, lse2)
    assert torch.allclose(out.norm(dim=1), torch.ones(spec[0]), atol=1e-5)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("spec", MR.VARIANT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_other_register_variants(cuda, spec, dt):
    """K = 512 and 672: the kernel instantiations with 2 and 3 column units per wave."""
    c = MR.spread_case(*spec, dt)
    q, b = _views(cuda, c)
    for ns in (None, 3):
        mix, lse = _project(cuda, q, b, c["scale"], nsplit=ns)
        _check(f"{dt} {spec} nsplit {ns}", c, mix, lse)


@pytest.mark.parametrize("dt", DTYPES)
def test_reference_scale_100(cuda, ref100, dt):
    """Scale 100 with planted near-copies: the accumulators are rescaled by about e^-90 when the
    copy comes last, and every later weight underflows when it comes first."""
    c = ref100[dt]
    q, b = _views(cuda, c)
    for ns in (None, 3):
        mix, lse = _project(cuda, q, b, c["scale"], nsplit=ns)
        _check(f"{dt} scale 100 nsplit {ns}", c, mix, lse)
    out, _ = _project(cuda, q, b, c["scale"], normalize=True)
    _check(f"{dt} scale 100 normalised", c, out, lse, normalized=True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", MR.EXACT_NS)
def test_exact_mean(cuda, N, dt):
    c = MR.exact_case(N, dt)
    q, b = _views(cuda, c)
    for ns in (None, 3):
        mix, lse = _project(cuda, q, b, 0.0, nsplit=ns)
        assert torch.equal(mix, c["mean"]), f"nsplit {ns}"
        want = torch.full_like(lse, math.log(N))
        ulp = float(torch.nextafter(want[0], want[0] + 1) - want[0])
        assert float((lse - want).abs().max()) <= ulp, f"nsplit {ns}"


@pytest.mark.parametrize("dt", DTYPES)
def test_explicit_splits_and_empty_splits(cuda, spread, dt):
    """nsplit 1, 2, 7 and more splits than bank rows (empty splits): all within the bound, no NaN."""
    for spec in ((5, 333, 1024), (3, 63, 32)):
        c = spread[(spec, dt)]
        q, b = _views(cuda, c)
        for ns in (1, 2, 7, spec[1] + 5):
            mix, lse = _project(cuda, q, b, c["scale"], nsplit=ns)
            _check(f"{dt} {spec} nsplit {ns}", c, mix, lse)


@pytest.mark.parametrize("dt", DTYPES)
def test_rows_do_not_depend_on_the_launch(cuda, spread, dt):
    """Bitwise: two runs with the default split count are equal; row m of the M = 130 launch
    equals the same query launched alone, and as part of another row range."""
    for spec in ((130, 257, 64), (64, 4099, 1024)):
        c = spread[(spec, dt)]
        q, b = _views(cuda, c)
        one, two = _project(cuda, q, b, c["scale"]), _project(cuda, q, b, c["scale"])
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
        M = spec[0]
        for lo, hi in ((M - 1, M), (37, 38), (0, 1), (30, 63)):
            qs, _ = _views(cuda, c, (lo, hi))
            part = _project(cuda, qs, b, c["scale"])
            assert torch.equal(part[0], one[0][lo:hi]) and torch.equal(part[1], one[1][lo:hi]), (lo, hi)


@pytest.mark.parametrize("dt", DTYPES)
def test_chunked_bank_agrees(cuda, spread, dt):
    """The bank as three uneven chunks through SupportMemory (each chunk merged, then re-entered
    as (mix, lse, 1)) against the float64 reference of the whole bank."""
    from zsaac.memory import SupportMemory
    spec = (64, 4099, 1024)
    c = spread[(spec, dt)]
    q, b = _views(cuda, c)
    b = b.contiguous()
    cuts = (0, 100, 3001, 4099)
    mem3 = SupportMemory([b[lo:hi] for lo, hi in zip(cuts, cuts[1:])], device=cuda, normalize=False)
    mem1 = SupportMemory(b, device=cuda, normalize=False)
    assert mem3.dtype == mem1.dtype == MR.DTS[dt] and mem3.N == spec[1]
    mix3, lse3 = mem3.project(q.contiguous(), c["scale"], normalize=False, return_lse=True)
    mix1, lse1 = mem1.project(q.contiguous(), c["scale"], normalize=False, return_lse=True)
    torch.cuda.synchronize()
    _check(f"{dt} three chunks", c, mix3.cpu(), lse3.cpu())
    _check(f"{dt} one tensor", c, mix1.cpu(), lse1.cpu())
    single = _project(cuda, q, b, c["scale"])
    assert torch.equal(mix1.cpu(), single[0]) and torch.equal(lse1.cpu(), single[1])


def test_merge_scripted_partials(cuda):
    """zs_memory_merge alone on hand-scripted partials (maxima 120 apart, empty splits, a row with
    one non-empty split) against float64: f32 weights and a sum over nsplit terms."""
    for M, ns, K in ((6, 7, 32), (3, 130, 1024), (2, 1, 96)):
        a, ml = MR.scripted_partials(M, ns, K, 11 + ns)
        want_mix, want_lse = MR.merge(a, ml)
        bound = 8 * 2.0 ** -23 * ns ** 0.5 + 2.0 ** -20      # rounding of ns weighted f32 terms
        wt = torch.where(torch.isinf(ml[..., 0]), torch.zeros(M, ns),
                         torch.exp(ml[..., 0] - ml[..., 0].max(1, keepdim=True).values)).double()
        size = (a.abs().double() * wt[..., None]).sum(1) / (ml[..., 1].double() * wt).sum(1)[:, None]
        for normalize in (False, True):
            out, lse = Out(cuda, (M, K), F32, SENT), Out(cuda, (M,), F32, SENT)
            _ops().memory_merge(a.to(cuda), ml.to(cuda), M, ns, K, out.t, normalize, lse.t)
            torch.cuda.synchronize()
            got, gl = out.cpu().double(), lse.cpu().double()
            assert not bool(torch.isnan(got).any())
            norm = want_mix.norm(dim=1, keepdim=True)
            want, tol = (want_mix / norm, (bound * size + 1e-7) / norm) if normalize else \
                (want_mix, bound * size + 1e-7)
            r = float(((got - want).abs() / tol).max())
            rl = float(((gl - want_lse).abs() / (want_lse.abs() * 2.0 ** -22 + bound)).max())
            print(f"merge {M}x{ns}x{K} normalize {normalize}: err/bound {r:.3f} lse {rl:.3f}")
            assert r <= 1.0 and rl <= 1.0
