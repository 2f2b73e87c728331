"""Plain CPU reference of the memory-bank projection (zs_memory_project / zs_memory_merge of
csrc/memory.hip, zsaac/memory.py), written from its definition, and the cases the GPU tests run.

    z = scale * q b^T,  lse = log sum_n exp z,  w = exp(z - lse),  mix = w b

in float64 on the operands as stored (bf16 cases use the bf16-rounded values).  Besides the
results it returns A = w |b| (the size of what is summed into each output element), the
effective support ess = 1 / sum w^2 of every row, and the project's yardstick
(retrieval_ref.yardstick: the float32 dot product chunked by 16 against float64, tau = 4 yard +
1e-6).  The tolerances follow from those, not from what the kernel gives:

    a dot product off by tau moves z by |scale| tau, so a weight by a factor within
    exp(+-|scale| tau) and, after the division by the equally perturbed sum, within
    exp(+-2 |scale| tau);  bf16 banks round the weights to bf16 (relative 2^-9, eps_p = 2^-8
    covers numerator and denominator);  2^-20 for the f32 accumulation and exp:
        eps = expm1(2 |scale| tau) + eps_p + 2^-20
        |mix - mix64| <= 2 eps A + 1e-6          elementwise
        |lse - lse64| <= |scale| tau + eps_p + 1e-6
    the normalised output: the same bound divided by ||mix64||.

Nothing here reads the original project.
"""
from __future__ import annotations

import math

import torch

from gemm_ref import BF16, F32, F64, INF, NAN, strided  # noqa: F401
from retrieval_ref import yardstick

DTS = {"f32": F32, "bf16": BF16}
EPS_P = {"f32": 0.0, "bf16": 2.0 ** -8}

# (M, N, K) of the spread cases: scale = 1.5 sqrt(K), unit-norm Gaussian rows
SPREAD_CASES = ((5, 333, 1024), (70, 1000, 96), (130, 257, 64), (64, 4099, 1024), (1, 1, 32),
                (3, 63, 32))
# the kernel's other register variants (columns per wave 64 and 96: K in 257 .. 768) and a K whose
# 16-byte chunks per row are no power of two (672: 84 bf16 / 168 f32 chunks), more than one row
# block and a ragged last tile
VARIANT_CASES = ((33, 130, 512), (7, 95, 672))
ESS_MIN = 8.0       # asserted on the CPU for every row of the spread cases with N >= 256
REF_SCALE = 100.0   # map2memory's scale
REF_CASE = (5, 333, 1024)
EXACT_NS = (256, 320)
EXACT_MK = (3, 64)


def _seed(*parts):
    s = 0
    for p in parts:
        s = (s * 1000003 + (sum(map(ord, p)) if isinstance(p, str) else int(p))) % (2 ** 31 - 1)
    return s


def project(q, b, scale, dt):
    """The float64 reference and the tolerances for operands q [M, K], b [N, K] of storage type
    ``dt`` ("f32" / "bf16").  -> dict(lse, w, mix, out (normalised mix), A, ess, norm, yard, tau,
    eps, mix_tol [M, K], lse_tol, out_tol [M, K])."""
    s64, yard, tau = yardstick(q, b)
    z = scale * s64
    mx = z.max(dim=1, keepdim=True).values
    e = torch.exp(z - mx)
    den = e.sum(dim=1, keepdim=True)
    w = e / den
    lse = (mx + torch.log(den))[:, 0]
    b64 = b.to(F64)
    mix = w @ b64
    A = w @ b64.abs()
    norm = mix.norm(dim=1, keepdim=True)
    eps = math.expm1(2.0 * abs(scale) * tau) + EPS_P[dt] + 2.0 ** -20
    mix_tol = 2.0 * eps * A + 1e-6
    return dict(lse=lse, w=w, mix=mix, out=mix / norm.clamp(min=1e-12), A=A, norm=norm,
                ess=1.0 / (w * w).sum(dim=1), yard=yard, tau=tau, eps=eps, mix_tol=mix_tol,
                lse_tol=abs(scale) * tau + EPS_P[dt] + 1e-6, out_tol=mix_tol / norm)


def unit_rows(R, K, gen):
    x = torch.randn(R, K, generator=gen, dtype=F64)
    return (x / x.norm(dim=1, keepdim=True)).to(F32)


def _pack(q, b, dt, scale, pad=8):
    """Operands of storage type ``dt`` in NaN-padded [rows + 1][K + pad] buffers + reference."""
    K = q.shape[1]
    qbuf, qv = strided(q.to(DTS[dt]), K + pad)
    bbuf, bv = strided(b.to(DTS[dt]), K + pad)
    c = project(qv, bv, scale, dt)
    c.update(qbuf=qbuf, q=qv, bbuf=bbuf, b=bv, scale=scale, dt=dt)
    return c


def spread_case(M, N, K, dt):
    # seed series 6: the smallest effective support over the N >= 256 cases is 14.7 (K = 64 with
    # scale 12 is the tight one; tests/test_memory_ref.py asserts >= ESS_MIN)
    g = torch.Generator().manual_seed(_seed("spread", M, N, K, 6))
    return _pack(unit_rows(M, K, g), unit_rows(N, K, g), dt, 1.5 * math.sqrt(K))


def planted(q_row, cos, gen):
    """A unit row at cosine ``cos`` to the unit row q_row."""
    n = torch.randn(q_row.shape, generator=gen, dtype=F64)
    qd = q_row.to(F64)
    n = n - (n @ qd) * qd
    n = n / n.norm()
    return (cos * qd + math.sqrt(1.0 - cos * cos) * n).to(F32)


def ref_scale_case(dt):
    """map2memory's scale 100 at REF_CASE.  Row 0's near-copy (cosine 0.95) is the LAST bank row
    (everything accumulated before it is rescaled by about e^-90); row 1's near-copy is bank row 0
    (every later weight underflows against it); row 2 has a 0.6 copy mid-bank."""
    M, N, K = REF_CASE
    g = torch.Generator().manual_seed(_seed("ref100", M, N, K))
    q, b = unit_rows(M, K, g), unit_rows(N, K, g)
    b[N - 1] = planted(q[0], 0.95, g)
    b[0] = planted(q[1], 0.95, g)
    b[N // 2] = planted(q[2], 0.6, g)
    return _pack(q, b, dt, REF_SCALE)


def exact_case(N, dt):
    """scale 0, entries multiples of 1/8 in [-2, 2]: every weight is 1 / N, every column sum is
    exact in f32, so mix is the correctly rounded column mean and lse = log N."""
    M, K = EXACT_MK
    g = torch.Generator().manual_seed(_seed("exact", N))
    q = torch.randint(-16, 17, (M, K), generator=g).to(F32) / 8
    b = torch.randint(-16, 17, (N, K), generator=g).to(F32) / 8
    c = _pack(q, b, dt, 0.0)
    c["mean"] = (c["b"].to(F64).sum(dim=0) / N).to(F32).repeat(M, 1)
    return c


# ------------------------------------------------------------------ scripted partials
def scripted_partials(M, nsplit, K, seed):
    """part_mix [M][nsplit][K], part_ml [M][nsplit][2] as zs_memory_project writes them: maxima
    spread over +-60 (weights from 1 down to underflow), positive sums, and empty splits
    (0, -inf, 0) at every third position; row 0 keeps a single non-empty split."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, nsplit, K, generator=g)
    m = (torch.rand(M, nsplit, generator=g) * 120.0 - 60.0)
    l = torch.rand(M, nsplit, generator=g) * 30.0 + 1.0
    empty = torch.zeros(M, nsplit, dtype=torch.bool)
    empty[:, 1::3] = True
    empty[0, :] = True
    empty[0, nsplit // 2] = False
    a[empty] = 0.0
    m[empty] = -INF
    l[empty] = 0.0
    return a, torch.stack([m, l], dim=2).contiguous()


def merge(part_mix, part_ml):
    """The merge in float64 -> (mix [M, K], lse [M])."""
    a, m, l = part_mix.to(F64), part_ml[..., 0].to(F64), part_ml[..., 1].to(F64)
    top = m.max(dim=1, keepdim=True).values
    wt = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - top))
    L = (l * wt).sum(dim=1)
    mix = (a * wt[..., None]).sum(dim=1) / L[:, None]
    return mix, top[:, 0] + torch.log(L)
