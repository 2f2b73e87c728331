"""Float64 reference of zs_sample_rows (include/zsaac.h): Philox4x32-10, the sampler itself
(temperature -> top-k -> top-p -> draw, gpt2_prefix_eval.py:196-206 for the temperature and the
nucleus rule, HF's processor order) and, per draw, how decisive it is.

A draw is three comparisons that rounding can turn: which tokens the top-k cut keeps, where the
nucleus ends, and which token's running mass first exceeds u * mass.  Each has a gap:
  k_gap  z of the last kept minus z of the first dropped token at the top-k cut (inf when top-k
         is off, or when the two logits are EQUAL: a tie goes to the lower id in any arithmetic)
  p_gap  the distance of top_p * mass from the nearest "mass before rank i", i >= 1 (inf when
         top-p is off)
  o_gap  z of the nucleus' last token minus z of the first token behind it (inf when top-p is
         off or drops nothing, or when the two logits are equal).  The order of two tokens by
         p = exp(z - max z) is their order by z in any arithmetic whose division, subtraction and
         exponential are monotone; what another arithmetic can do is make two close z, z - max z
         or p EQUAL, and then take the lower id first.  Rounding moves z by at most yard_z and
         z - max z by at most twice that, so this gap is measured in z
  d_gap  the distance of u * mass from the nearest value of the id-order running mass
and each is measured against a yardstick: the same formula evaluated in float32, as its largest
deviation from float64 on the row's own data (the rule of
tests/test_gpu_magic_kernels.py::_check):
  yard_z  z = x / T                                              (for k_gap and o_gap)
  yard_p  the running sums of p = exp(z - max z) over the tokens the top-k cut keeps, in the
          nucleus' order, and top_p times their total            (for p_gap)
  yard_d  the running sums of p over the tokens finally kept, in id order, and u times their
          total                                                  (for d_gap)
with the float64 evaluation's order and kept sets in both (what is summed is the same; only the
arithmetic differs).  A draw is decisive when every gap exceeds 4 x yardstick + 1e-6; only then must an implementation in another
arithmetic return the same token and the same number of kept tokens.

The masses are in units of the row's largest probability (p = exp(z - max z) <= 1), as the kernel
holds them."""
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# Known-answer vectors of Philox4x32-10 (Random123, kat_vectors): (counter, key, output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(ctr, key):
    """ctr: 4 and key: 2 arrays (or ints) of 32-bit words -> 4 uint64 arrays of 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in key]
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m]
        k = [(k[0] + np.uint64(W0)) & m, (k[1] + np.uint64(W1)) & m]
    return c


def uniform(seed, row_id, step):
    """u = (w + 0.5) * 2^-32, w = word 0 of Philox(key = seed, counter = (row_id, step, 0, 0))."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rid = np.asarray(row_id, dtype=np.int64) & MASK
    z = np.zeros_like(rid)
    w = philox4x32_10((rid, z + (int(step) & MASK), z, z), (z + (seed & MASK), z + (seed >> 32)))[0]
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def _probs(x, temperature, dt):
    x = x.astype(dt)
    z = x / dt(temperature)
    with np.errstate(invalid="ignore"):
        p = np.where(np.isneginf(z), dt(0), np.exp(z - z.max()))
    return z, p.astype(dt)


def logprob_of(x, tok, dt=np.float64):
    """log softmax(x)[tok] at temperature 1, unfiltered."""
    x = x.astype(dt)
    mx = x.max()
    with np.errstate(invalid="ignore"):
        s = np.where(np.isneginf(x), dt(0), np.exp(x - mx)).sum(dtype=dt)
    return dt(x[tok] - mx) - np.log(s)


def sample_row(x, temperature, top_k, top_p, u, dt=np.float64):
    """One row.  Returns a dict: tok, count, mass (kept share of softmax(z)), logprob, the three
    gaps, and `keep` (bool [V])."""
    V = len(x)
    ids = np.arange(V)
    z, p = _probs(x, temperature, dt)
    z32, p32 = _probs(x, temperature, np.float32)
    fin = np.isfinite(z)
    yard_z = float(np.abs(z32[fin].astype(np.float64) - z[fin].astype(np.float64)).max()) if fin.any() else 0.0
    yard_p = 0.0
    inf = float("inf")
    keep = np.ones(V, dtype=bool)
    k_gap = inf
    if 0 < top_k < V:
        o = np.lexsort((ids, -z))
        keep[:] = False
        keep[o[:top_k]] = True
        a, b = o[top_k - 1], o[top_k]
        k_gap = inf if x[a] == x[b] else float(z[a] - z[b])
    p_gap = o_gap = inf
    if top_p < 1:
        kid = ids[keep]
        o = kid[np.lexsort((kid, -p[kid]))]
        ps = p[o]
        cs = np.cumsum(ps)
        before = np.concatenate([np.zeros(1, dt), cs[:-1]])
        P = dt(top_p) * cs[-1]
        cs32 = np.cumsum(p32[o])
        yard_p = max(float(np.abs(cs32.astype(np.float64) - cs).max()),
                     abs(float(np.float32(top_p) * cs32[-1]) - float(P)))
        ok = before <= P
        ok[0] = True
        n = int(ok.sum())
        assert ok[:n].all()
        keep[:] = False
        keep[o[:n]] = True
        if len(o) > 1:
            p_gap = float(np.abs(before[1:] - P).min())
        if n < len(o) and x[o[n - 1]] != x[o[n]]:
            o_gap = float(z[o[n - 1]] - z[o[n]])
    pk = np.where(keep, p, dt(0))
    cdf = np.cumsum(pk)
    M = cdf[-1]
    target = dt(u) * M
    hit = np.nonzero(keep & (cdf > target))[0]
    tok = int(hit[0]) if len(hit) else int(ids[keep][-1])
    d_gap = float(min(np.abs(cdf - target).min(), abs(target)))
    cdf32 = np.cumsum(np.where(keep, p32, np.float32(0)))
    yard_d = max(float(np.abs(cdf32.astype(np.float64) - cdf).max()),
                 abs(float(np.float32(u) * cdf32[-1]) - float(target)))
    return dict(tok=tok, count=int(keep.sum()), mass=float(M / p.sum(dtype=dt)),
                logprob=float(logprob_of(x, tok, dt)), k_gap=k_gap, p_gap=p_gap, o_gap=o_gap, d_gap=d_gap,
                yard_z=yard_z, yard_p=yard_p, yard_d=yard_d, keep=keep)


def decisive(rec):
    yz = 4 * rec["yard_z"] + 1e-6
    return (rec["k_gap"] > yz and rec["o_gap"] > yz and rec["p_gap"] > 4 * rec["yard_p"] + 1e-6
            and rec["d_gap"] > 4 * rec["yard_d"] + 1e-6)


def sample_rows(logits, V, temperature, top_k, top_p, seed, step, row_id=None):
    """The rows of ``logits`` [R, >= V] (numpy f32).  Returns a list of records (sample_row's,
    plus `decisive` and the float32 evaluation's logprob / mass as
    `logprob32` / `mass32`: the yardsticks of those two outputs)."""
    R = logits.shape[0]
    rid = np.arange(R) if row_id is None else np.asarray(row_id)
    us = uniform(seed, rid, step)
    out = []
    for r in range(R):
        x = np.ascontiguousarray(logits[r, :V])
        rec = sample_row(x, temperature, top_k, top_p, us[r])
        r32 = sample_row(x, temperature, top_k, top_p, us[r], dt=np.float32)
        rec.update(u=float(us[r]), decisive=decisive(rec),
                   logprob32=float(logprob_of(x, rec["tok"], np.float32)), mass32=r32["mass"],
                   count32=r32["count"])
        out.append(rec)
    return out


# ---------------------------------------------------------------------------- the cases
TEMPERATURES = (0.7, 1.0, 2.0)
TOP_PS = (1.0, 0.8, 1e-6)
SEED, STEP = 0x1234567890ABCDEF, 3
POISON = 1e30    # the padding columns ld > V hold this (an implementation that read them would
                 # draw them: they dominate every row)


def top_ks(V):
    return (0, 1, 5, V + 3)


# name -> (V, R, ld).  v1000 has an odd row stride (rows that do not start on 16 bytes); the two
# vocabulary sizes of the decoders run at R = 3.  The kernel holds ceil(V / 4096) float4 per lane
# in variants of 1 / 2 / 4 / 8 / 13 / 16: v4096 fills the first, v4097 is the first size of the
# second, v10000 takes the third, v32000 / v50257 the fourth and fifth, v65536 fills the last.  The spread of the random rows grows with V so
# that a few tokens carry most of a row's mass (as an LM head's do): the draws then sit well
# inside a token's share of the running mass.
CASES = {
    "v1": (1, 3, 4),
    "v5": (5, 70, 8),
    "v64": (64, 1, 64),
    "v1000": (1000, 70, 1003),
    "v4096": (4096, 3, 4096),
    "v4097": (4097, 3, 4100),
    "v10000": (10000, 3, 10000),
    "v32000": (32000, 3, 32000),
    "v50257": (50257, 3, 50272),
    "v65536": (65536, 2, 65536),
    "planted": (1000, 6, 1000),
}
SPREAD = {"v1": 1.0, "v5": 2.0, "v64": 3.0, "v1000": 4.0, "v4096": 5.0, "v4097": 5.0,
          "v10000": 5.0, "v32000": 6.0, "v50257": 6.0, "v65536": 8.0}

# planted rows (V = 1000; a wave of the kernel owns 256 consecutive ids, so the planted ids span
# several waves)
TIE_MAX_IDS = (300, 7, 999)             # row 0: three equal maxima -> the lowest id wins top_k = 1
TIE_K_IDS = (3, 299, 300, 998)          # row 1: ranks 3 .. 6 equal, four larger: top_k = 5 keeps
TIE_K_TOP = (10, 500, 700, 900)         #        ids 3 and 299 of them (by id), not 300 and 998
TIE_P_IDS = (5, 260, 261, 600, 777, 800, 999)   # row 2: seven equal tokens of 0.135 each; at
#                                         T = 1, top_p = 0.8 the nucleus ends inside them (6 of 7)
DOMINANT_ID = 513                       # row 4: one token 30 above the rest


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits [R, ld] numpy f32 with the padding columns poisoned, V)."""
    V, R, ld = CASES[name]
    g = np.random.default_rng(sum(map(ord, name)))
    x = np.full((R, ld), POISON, dtype=np.float32)
    if name != "planted":
        x[:, :V] = (g.standard_normal((R, V)) * SPREAD[name]).astype(np.float32)
    else:
        base = (g.standard_normal((R, V)) * 0.5).astype(np.float32)
        x[:, :V] = base
        x[0, list(TIE_MAX_IDS)] = 6.0
        x[1, list(TIE_K_TOP)] = np.float32([9.0, 8.5, 8.0, 7.5])
        x[1, list(TIE_K_IDS)] = 6.0
        # row 2: 7 e^a / (7 e^a + sum of the rest) = 0.945
        rest = np.exp(base[2].astype(np.float64))
        rest[list(TIE_P_IDS)] = 0.0
        x[2, list(TIE_P_IDS)] = np.float32(np.log(0.945 / 0.055 * rest.sum() / 7.0))
        x[3, :V] = (g.standard_normal(V) * 3.0).astype(np.float32)     # row 3: a third is -inf
        x[3, 1:V:3] = -np.inf
        x[4, :V] = base[4]
        x[4, DOMINANT_ID] = 30.0
        x[5, :V] = (g.standard_normal(V) * 4.0).astype(np.float32)     # row 5: -inf and a tie of
        x[5, 0:V:2] = -np.inf                                          # maxima next to it
        x[5, [401, 403]] = 20.0
    x.setflags(write=False)
    return x, V


@functools.lru_cache(maxsize=None)
def reference(name, temperature, top_k, top_p):
    x, V = case(name)
    return sample_rows(x, V, temperature, top_k, top_p, SEED, STEP)


def settings(name):
    V = CASES[name][0]
    return [(t, k, p) for t in TEMPERATURES for k in top_ks(V) for p in TOP_PS]
