"""Plain CPU references of the GPT-2 / mapper / cross attention kernels of csrc/attn.hip
(zs_row_attention, zs_row_attention_kv, zs_kv_write, zs_decode_attention,
zs_decode_attention_map, zs_cross_attention), one function per op.

Pure torch on the CPU; every float is computed in ``dtype``: float64 is the reference, float32
the yardstick (the same formula in the kernel's precision; its distance from the float64 run on a
case's own data is what plain float32 arithmetic costs there).  ``round_to`` rounds to the
storage type where a kernel stores its output.  Nothing here reads a golden or the original
project.  tests/test_attn_ref.py ties these functions to independent formulations and to
oracle/caption.py's attention, and asserts the input conditions of the GPU cases;
tests/test_gpu_attn_kernels.py compares the kernels with them.

The functions work on the kernels' own layouts: q / k / v as 2-D row views whose row stride is
the kernel's ld argument (a packed q|k|v buffer or separate ones), caches
[row][head][Lmax][head dim], kvrow [R][Lmax], rowmap / cpos per compact slot.

``mut`` names one deliberate, in-bounds arithmetic error of a kernel (MUTANTS; "name:a:b" carries
the keys per phase and the slice count).  It is only ever set by tests/test_attn_ref.py, which
shows on the CPU that the inputs of the GPU cases tell each of them from the reference by more
than twice the case's tolerance.

The second half builds the inputs both test files share.
"""
from __future__ import annotations

import functools
import math

import torch

I32 = torch.int32
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NAN = float("nan")

MUTANTS = ("strict", "stale_new", "clamp_dup", "no_rescale", "drop_slice", "kvrow_self",
           "kvrow_row0", "scale1", "head_shift", "noncausal", "causal_strict", "len_ignored",
           "batch0_keys", "hd_trunc")

# zs_tune_set knobs of attn.hip and their initial values (checked against the g_* initialisers by
# tests/test_attn_ref.py); the GPU tests restore every knob they touch to these
KNOB_DEFAULTS = dict(small_attn=1, small_rmax=128, beam_xcd=5, decode_attn5=6, attn_split=3,
                     row_mfma=1)


def _round(v, round_to):
    return v if round_to is None else v.to(round_to).to(v.dtype)


def _mut(mut):
    name, *a = mut.split(":")
    return name, [int(x) for x in a]


def tolerance(ref64, ref32, bf16=False):
    """The project's rule (mistral_ref.tolerance): yardstick = the float32 formula's largest
    deviation from float64 on this data, tolerance 4 x yardstick + 1e-6; a bf16 output adds one
    bf16 step of the reference elementwise (2^-8 |ref|).  -> (yardstick, tolerance tensor)."""
    yard = float((ref32.double() - ref64).abs().max())
    tol = torch.full_like(ref64, 4.0 * yard + 1e-6)
    if bf16:
        tol = tol + ref64.abs() * 2.0 ** -8
    return yard, tol


def _softmax_v(sc, v, p_round=None):
    """softmax(sc) v with the max subtracted: sc [..., n], v [..., n, d].  ``p_round``: the
    unnormalised probabilities are rounded before P.V, the sum is taken of the unrounded ones."""
    e = torch.exp(sc - sc.max(-1, keepdim=True).values)
    return (_round(e, p_round).unsqueeze(-2) @ v).squeeze(-2) / e.sum(-1, keepdim=True)


# ------------------------------------------------------------------ the ops
def row_attention(q, ldq, k, v, ldkv, B, L, lens, heads, hd, causal, scale, p_round=None,
                  dtype=F64, round_to=None, mut=""):
    """Dense attention per (batch row, head): query i of row b against keys j < lens[b] (and
    j <= i when causal) of the same row, softmax(scale q k^T) v.  q [B*L, >= heads*hd] with row
    stride ldq, k / v likewise with ldkv.  Query rows i >= lens[b] are computed like the others
    (causal: over the lens[b] keys).  ``p_round`` = BF16 models the MFMA kernel, which rounds the
    unnormalised probabilities to bf16 before P.V.  -> [B*L, heads*hd]."""
    assert q.stride(0) == ldq and k.stride(0) == ldkv and v.stride(0) == ldkv
    E = heads * hd
    name, _ = _mut(mut)
    qh = q[:, :E].to(dtype).reshape(B, L, heads, hd).transpose(1, 2)          # [B, H, L, hd]
    kh = k[:, :E].to(dtype).reshape(B, L, heads, hd).transpose(1, 2)
    vh = v[:, :E].to(dtype).reshape(B, L, heads, hd).transpose(1, 2)
    if name == "head_shift":
        kh = kh.roll(-1, 1)
    if name == "scale1":
        scale = 1.0
    if name == "noncausal":
        causal = False
    out = torch.zeros(B, heads, L, hd, dtype=dtype)
    i = torch.arange(L)
    for b in range(B):
        n = L if lens is None or name == "len_ignored" else int(lens[b])
        sc = (qh[b] @ kh[b, :, :n].transpose(-1, -2)) * scale                   # [H, L, n]
        if causal:
            mask = i[:n][None] < i[:, None] if name == "causal_strict" else i[:n][None] <= i[:, None]
            sc = sc.masked_fill(~mask, -float("inf"))
            if name == "causal_strict":
                sc[:, 0, 0] = 0.0                 # row 0 has no key left: keep it finite
        out[b] = _softmax_v(sc, vh[b, :, None, :n], p_round)
    return _round(out.transpose(1, 2).reshape(B * L, E), round_to)


def kv_write(qkv, R, n, D, heads, pos0, row_stride, kc, vc):
    """k / v of qkv row r * n + i (columns D..2D and 2D..3D) into cache row r * row_stride,
    position (pos0[r] or 0) + i.  A pure copy in the storage type.  -> (kc, vc) afterwards."""
    hd = D // heads
    kc, vc = kc.clone(), vc.clone()
    for r in range(R):
        p0 = int(pos0[r]) if pos0 is not None else 0
        rows = qkv[r * n:(r + 1) * n]
        kc[r * row_stride, :, p0:p0 + n] = rows[:, D:2 * D].reshape(n, heads, hd).transpose(0, 1)
        vc[r * row_stride, :, p0:p0 + n] = rows[:, 2 * D:3 * D].reshape(n, heads, hd).transpose(0, 1)
    return kc, vc


def decode_attention(qkv, R, D, heads, kc, vc, Lmax, pos, kvrow=None, rowmap=None, cpos=None,
                     nphys=None, dtype=F64, round_to=None, mut=""):
    """One decode step of R slots, head dim 64, scale 1/8.  Slot c is physical row r = rowmap[c]
    (c without rowmap) at position p = cpos[c] (pos[r] without cpos): its query against the
    cached keys j < p of row kvrow[r][j] (row r without kvrow), as the cache was before the call,
    and key p = the slot's own new k / v, which is also written to cache row r, position p.
    Padding slots (rowmap[c] >= nphys) give zero rows and write nothing.
    -> (out [R, D], kc, vc afterwards)."""
    HD = 64
    name, arg = _mut(mut)
    x = qkv.to(dtype)
    k0, v0 = kc.to(dtype), vc.to(dtype)
    kc, vc = kc.clone(), vc.clone()
    out = torch.zeros(R, heads, HD, dtype=dtype)
    scale = 1.0 if name == "scale1" else 0.125
    hsrc = (torch.arange(heads) + 1) % heads if name == "head_shift" else torch.arange(heads)
    for c in range(R):
        r = int(rowmap[c]) if rowmap is not None else c
        if nphys is not None and r >= nphys:
            continue
        p = min(int(cpos[c]) if cpos is not None else int(pos[r]), Lmax - 1)
        qv = x[c, :D].view(heads, HD)
        kn, vn = x[c, D:2 * D].view(heads, HD), x[c, 2 * D:].view(heads, HD)
        kc[r, :, p] = qkv[c, D:2 * D].view(heads, HD)
        vc[r, :, p] = qkv[c, 2 * D:].view(heads, HD)
        j = torch.arange(p)
        if kvrow is None or name == "kvrow_self":
            src = torch.full((p,), r)
        else:
            src = kvrow[0 if name == "kvrow_row0" else r, :p].long()
        K, V = k0[src, :, j].transpose(0, 1), v0[src, :, j].transpose(0, 1)      # [H, p, 64]
        if name == "stale_new":
            kn, vn = k0[r, :, p], v0[r, :, p]
        if name != "strict":
            K, V = torch.cat((K, kn[:, None]), 1), torch.cat((V, vn[:, None]), 1)
        if name == "clamp_dup" and p > 0:
            K, V = torch.cat((K, K[:, p - 1:p]), 1), torch.cat((V, V[:, p - 1:p]), 1)
        if K.shape[1] == 0:
            continue
        K = K[hsrc]
        sc = torch.einsum("hd,hnd->hn", qv * scale, K)
        if name == "drop_slice":
            kpp, split = arg
            keep = (torch.arange(sc.shape[1]) // kpp) % split != split - 1
            sc, V = sc[:, keep], V[:, keep]
        if name == "no_rescale":
            kpp = arg[0]
            m = torch.full((heads, 1), -float("inf"), dtype=dtype)
            s = torch.zeros(heads, 1, dtype=dtype)
            o = torch.zeros(heads, HD, dtype=dtype)
            for b0 in range(0, sc.shape[1], kpp):
                m = torch.maximum(m, sc[:, b0:b0 + kpp].max(-1, keepdim=True).values)
                e = torch.exp(sc[:, b0:b0 + kpp] - m)
                s = s + e.sum(-1, keepdim=True)
                o = o + (e.unsqueeze(1) @ V[:, b0:b0 + kpp]).squeeze(1)
            out[c] = o / s
        else:
            out[c] = _softmax_v(sc, V)
    return _round(out.reshape(R, D), round_to), kc, vc


def cross_attention(q, ldq, k, v, ldkv, B, Lq, Lk, heads, hd, scale, dtype=F64, round_to=None,
                    mut=""):
    """nn.MultiheadAttention's core: query row b * Lq + i, head h against the Lk keys of batch
    row b, softmax(scale q k^T) v.  -> [B*Lq, heads*hd]."""
    assert q.stride(0) == ldq and k.stride(0) == ldkv and v.stride(0) == ldkv
    E = heads * hd
    name, _ = _mut(mut)
    qh = q[:, :E].to(dtype).reshape(B, Lq, heads, hd).transpose(1, 2)
    kh = k[:, :E].to(dtype).reshape(B, Lk, heads, hd).transpose(1, 2)
    vh = v[:, :E].to(dtype).reshape(B, Lk, heads, hd).transpose(1, 2)
    if name == "scale1":
        scale = 1.0
    if name == "batch0_keys":
        kh = kh[:1].expand(B, -1, -1, -1)
    nd = 64 * (hd // 64) if name == "hd_trunc" else hd
    sc = (qh[..., :nd] @ kh[..., :nd].transpose(-1, -2)) * scale                # [B, H, Lq, Lk]
    out = _softmax_v(sc, vh[:, :, None])
    return _round(out.transpose(1, 2).reshape(B * Lq, E), round_to)


# ------------------------------------------------------------------ shared inputs
DATA = ["flat", "rising", "hot"]
HOT = 92.0                    # exp(88.73) is the largest finite float32
PHASES = [16, 32, 64, 128]    # keys per phase of decode_attn6_kernel's instantiations
SPLITS = [(32, 2), (64, 2), (32, 4)]
DEC_LMAX = 136
DEC_POS = [0, 1, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, 135]
DEC_HEADS = [12, 6, 5]
LONG_LMAX = 520
LONG_POS = [0, 63, 64, 511, 512, 513, 519]
EDGE_LMAX = 512               # the largest Lmax decode_attn4_kernel serves (136,768 B of LDS)
EDGE_POS = [0, 254, 255, 256, 257, 511]       # both sides of its 256-thread score loop's stride
BEAM_POS = [16, 31, 32, 33, 64, 65, 128, 135]      # one per clip of the 40-row beam case
MAP_NPHYS, MAP_HEADS = 24, 6
MAP_ACTIVE = list(range(1, MAP_NPHYS, 3))           # rows 1, 4, ..., 22
MAP_POS = [0, 16, 17, 32, 64, 65, 128, 135]         # of the active rows
# the plans of attn.hip's decode_plan, as (small_attn, attn_split, decode_attn5)
DEC_PLANS = [(1, 0, 6), (1, 1, 6), (1, 3, 6), (1, 4, 6), (0, 3, 6), (0, 3, 4), (0, 3, 3), (0, 3, 2)]
ROW_L = {64: [1, 27, 64, 65, 130, 256], 96: [20, 65]}
ROW_HEADS = {64: 3, 96: 2}
MFMA_L = [1, 5, 16, 17, 27, 31, 32]
MASKED = 1e4                  # k / v rows j >= lens[b]: finite, as in production
KVW_CASES = [(given, n, rs) for given in (False, True) for n in (1, 3) for rs in (1, 5)]
KVW_R, KVW_HEADS, KVW_LMAX = 3, 3, 9
CROSS_HEADS = 4
CROSS_HD = [256, 100, 64, 24]
CROSS_SHAPES = [(B, Lq, Lk) for B in (1, 3) for Lq in (1, 2) for Lk in (1, 3, 5, 64)]


def gen(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 1000003
    return torch.Generator().manual_seed(s)


def _unit(heads, hd, g):
    """One direction per head with entries +-1/sqrt(hd)."""
    return (torch.randint(0, 2, (heads, hd), generator=g).float() * 2 - 1) / hd ** 0.5


def _hot(hd, scale):
    """The common component of "hot" q and k elements: hd c^2 scale >= HOT, c a multiple of 1/16
    (exact in bf16)."""
    return math.ceil(16.0 * (HOT / (hd * scale)) ** 0.5) / 16.0


def _q(data, n, hd, scale, u):
    """Query noise n [.., heads, hd] -> queries; see _k."""
    if data == "flat":
        return n * (scale * hd ** 0.5) ** -0.5
    if data == "hot":
        return _hot(hd, scale) + 0.15 * n
    return u / scale + 0.1 * n


def _k(data, n, hd, scale, u, jpos):
    """Key noise n [nk, heads, hd] -> keys whose scaled scores against _q's queries are: "flat"
    unit-variance; "hot" about HOT with a spread of about 0.7; "rising" about the key's position
    jpos[nk] along the per-head direction u (one more per key, noise 0.1)."""
    if data == "flat":
        return n * (scale * hd ** 0.5) ** -0.5
    if data == "hot":
        return _hot(hd, scale) + 0.15 * n
    return jpos.float()[:, None, None] * u + 0.1 * n


@functools.lru_cache(maxsize=None)
def decode_case(data, dt, heads, form="ragged"):
    """A decode step in storage type ``dt``.  Forms: "ragged" (one row per position of DEC_POS,
    Lmax 136), "long" (LONG_POS, Lmax 520), "edge" (EDGE_POS, Lmax 512), "beam40" / "beam10" (8 / 2 clips x 5 beams, a clip's
    rows share a position of BEAM_POS and kvrow stays within the clip), "map" (24 physical rows,
    the active ones at MAP_POS).  Cache slots j >= pos[r] hold NaN; every kvrow entry is a valid
    row.  -> dict(qkv [R, 3D], kc, vc [R, heads, Lmax, 64], pos, kvrow | None, R, D, Lmax)."""
    g = gen(data, dt, heads, form)
    Lmax = {"long": LONG_LMAX, "edge": EDGE_LMAX}.get(form, DEC_LMAX)
    if form == "ragged":
        pos = list(DEC_POS)
    elif form == "long":
        pos = list(LONG_POS)
    elif form == "edge":
        pos = list(EDGE_POS)
    elif form == "map":
        pos = [int(x) for x in torch.randint(0, Lmax, (MAP_NPHYS,), generator=g)]
        for r, p in zip(MAP_ACTIVE, MAP_POS):
            pos[r] = p
    else:
        nclip = int(form[4:]) // 5
        pos = [p for p in BEAM_POS[:nclip] for _ in range(5)]
    R, D = len(pos), 64 * heads
    u = _unit(heads, 64, g)
    q = _q(data, torch.randn(R, heads, 64, generator=g), 64, 0.125, u)
    kk = _k(data, torch.randn(R * Lmax, heads, 64, generator=g), 64, 0.125, u,
            torch.arange(Lmax).repeat(R))
    kn = _k(data, torch.randn(R, heads, 64, generator=g), 64, 0.125, u, torch.tensor(pos))
    v = torch.randn(R * Lmax + R, heads, 64, generator=g)
    qkv = torch.cat((q.reshape(R, D), kn.reshape(R, D), v[R * Lmax:].reshape(R, D)), 1).to(dt)
    kc = kk.view(R, Lmax, heads, 64).transpose(1, 2).contiguous().to(dt)
    vc = v[:R * Lmax].view(R, Lmax, heads, 64).transpose(1, 2).contiguous().to(dt)
    for r, p in enumerate(pos):
        kc[r, :, p:] = NAN
        vc[r, :, p:] = NAN
    kvrow = None
    if form.startswith("beam"):
        clip = torch.arange(R) // 5
        kvrow = (clip[:, None] * 5 + torch.randint(0, 5, (R, Lmax), generator=g)).to(I32)
    return dict(qkv=qkv, kc=kc, vc=vc, pos=torch.tensor(pos, dtype=I32), kvrow=kvrow, R=R, D=D,
                Lmax=Lmax, heads=heads)


def decode_scores(c):
    """The scaled float64 scores of a decode case per slot: list of [heads, p + 1]."""
    x, k0 = c["qkv"].double(), c["kc"].double()
    D, H = c["D"], c["heads"]
    out = []
    for r in range(c["R"]):
        p = int(c["pos"][r])
        src = c["kvrow"][r, :p].long() if c["kvrow"] is not None else torch.full((p,), r)
        K = torch.cat((k0[src, :, torch.arange(p)].transpose(0, 1), x[r, D:2 * D].view(H, 1, 64)), 1)
        out.append(torch.einsum("hd,hnd->hn", x[r, :D].view(H, 64), K) * 0.125)
    return out


def map_case(with_cpos):
    """zs_decode_attention_map over the "map" decode case (bf16, "flat"): the strided active rows
    followed by three padding slots (rowmap >= nphys) whose qkv rows hold NaN.  With cpos the
    positions come from it and ``pos`` holds other (in-range) values.
    -> dict(c = the physical case, qkv_c, rowmap, cpos | None, pos, Rb)."""
    c = decode_case("flat", BF16, MAP_HEADS, "map")
    na = len(MAP_ACTIVE)
    rowmap = torch.tensor(MAP_ACTIVE + [MAP_NPHYS, MAP_NPHYS + 7, MAP_NPHYS], dtype=I32)
    Rb = rowmap.numel()
    qkv_c = torch.full((Rb, 3 * c["D"]), NAN, dtype=BF16)
    qkv_c[:na] = c["qkv"][MAP_ACTIVE]
    cpos, pos = None, c["pos"]
    if with_cpos:
        cpos = torch.zeros(Rb, dtype=I32)
        cpos[:na] = c["pos"][MAP_ACTIVE]
        pos = (c["pos"] + 1) % c["Lmax"]
    return dict(c=c, qkv_c=qkv_c, rowmap=rowmap, cpos=cpos, pos=pos.to(I32), Rb=Rb)


def row_lens(B, L):
    return torch.tensor([L, max(L - 5, 1), min(3, L), 1, L][:B], dtype=I32)


@functools.lru_cache(maxsize=None)
def row_case(data, dt, hd, heads, B, L, packed, ldo_pad=8):
    """q / k / v rows of B sequences of L in ``dt``: packed = the three column blocks of one
    [B*L, 3E] buffer (ldq = ldkv = 3E), else q [B*L, E] and k | v the halves of [B*L, 2E].  k and
    v rows j >= lens[b] hold +-MASKED.  -> dict(q, k, v, ldq, ldkv, ldo, lens, E)."""
    g = gen(data, dt, hd, heads, B, L, packed)
    E = heads * hd
    scale = hd ** -0.5
    u = _unit(heads, hd, g)
    q = _q(data, torch.randn(B * L, heads, hd, generator=g), hd, scale, u)
    k = _k(data, torch.randn(B * L, heads, hd, generator=g), hd, scale, u, torch.arange(L).repeat(B))
    v = torch.randn(B * L, heads, hd, generator=g)
    lens = row_lens(B, L)
    for b in range(B):
        sgn = torch.randint(0, 2, (L - int(lens[b]), heads, hd), generator=g).float() * 2 - 1
        k[b * L + int(lens[b]):(b + 1) * L] = MASKED * sgn
        v[b * L + int(lens[b]):(b + 1) * L] = -MASKED * sgn
    q, k, v = (t.reshape(B * L, E).to(dt) for t in (q, k, v))
    if packed:
        buf = torch.cat((q, k, v), 1).contiguous()
        q, k, v = buf[:, :E], buf[:, E:2 * E], buf[:, 2 * E:]
    else:
        kv = torch.cat((k, v), 1).contiguous()
        q, k, v = q.contiguous(), kv[:, :E], kv[:, E:]
    return dict(q=q, k=k, v=v, ldq=q.stride(0), ldkv=k.stride(0), ldo=E + ldo_pad, lens=lens, E=E,
                scale=scale, B=B, L=L, heads=heads, hd=hd)


def kvw_case(dt, given, n, row_stride):
    """zs_kv_write: 3 rows x n tokens, 3 heads of 64 (R n D is no multiple of the 256-thread
    block), Lmax 9, pos0 NULL or {0, 5, 6 - n + ... } with pos0 + n <= Lmax."""
    g = gen(dt, given, n, row_stride)
    D = 64 * KVW_HEADS
    qkv = torch.randn(KVW_R * n, 3 * D, generator=g).to(dt)
    pos0 = torch.tensor([0, 5, KVW_LMAX - n], dtype=I32) if given else None
    return dict(qkv=qkv, pos0=pos0, D=D, shape=(KVW_R * row_stride, KVW_HEADS, KVW_LMAX, 64))


@functools.lru_cache(maxsize=None)
def cross_case(data, dt, hd, B, Lq, Lk):
    """q [B*Lq, E + 8] (the 8 columns past E hold NaN), k | v the two halves of one [B*Lk, 2E]
    buffer, as models/caption_model.py passes them; scale hd^-0.5."""
    g = gen(data, dt, hd, B, Lq, Lk)
    E = CROSS_HEADS * hd
    scale = hd ** -0.5
    q = _q(data, torch.randn(B * Lq, CROSS_HEADS, hd, generator=g), hd, scale, None)
    k = _k(data, torch.randn(B * Lk, CROSS_HEADS, hd, generator=g), hd, scale, None, None)
    v = torch.randn(B * Lk, E, generator=g)
    qb = torch.full((B * Lq, E + 8), NAN).to(dt)
    qb[:, :E] = q.reshape(B * Lq, E).to(dt)
    kv = torch.cat((k.reshape(B * Lk, E), v), 1).to(dt).contiguous()
    return dict(q=qb[:, :E], k=kv[:, :E], v=kv[:, E:], ldq=E + 8, ldkv=2 * E, ldo=E + 8, E=E,
                scale=scale)
