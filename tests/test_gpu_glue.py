"""The GPT-2 decode glue kernels (csrc/gpt2.hip) one by one against tests/glue_ref.py, at the
shapes and edges where they can go wrong: exact ties, the unaligned / odd-D / k != 3 paths of the
label choice, truncated prompts, every beam width and block count of beam_step.

Every output is filled with a sentinel and allocated with a guard row behind it; the guard must
come back unchanged.  Ids, lengths, flags, maps and embeddings are compared with torch.equal;
only the beam scores carry a tolerance (see test_beam_step).  The input conditions of the
float-valued cases (selection margins >= 1e-3, the situations each beam scenario must contain)
are asserted on the CPU in tests/test_glue_ref.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ref as G  # noqa: E402
from gpu_helpers import Out, offset as _offset  # noqa: E402

pytestmark = pytest.mark.gpu
I32 = torch.int32


def _ops():
    from zsaac import ops
    return ops


# ------------------------------------------------------------------ label choice + prompt
def _run_labels(dev, emb, labels, k, ltok, llen, h_cap, with_chosen=True):
    ops = _ops()
    B = emb.shape[0]
    hard = Out(dev, (B, h_cap), I32, -7)
    hlen = Out(dev, (B,), I32, -7)
    chosen = Out(dev, (B, max(k, 1)), I32, -7) if with_chosen else None
    ops.prompt_assemble(emb, labels, k, ltok.to(dev), llen.to(dev), hard.t, hlen.t,
                        chosen=chosen.t if chosen else None)
    torch.cuda.synchronize()
    ch = chosen.cpu().reshape(-1)[:B * k].view(B, k) if chosen else None
    return hard.cpu(), hlen.cpu(), ch


@pytest.mark.parametrize("variant,L,k", G.LABEL_CASES)
def test_label_choice_exact_ties(cuda, variant, L, k):
    """Small-integer data: every similarity is exact in f32 and a column-swapped twin row ties
    exactly; the kernels must give glue_ref.label_select's (value desc, index asc).  That every
    case's answer depends on the data is asserted in test_glue_ref.py."""
    ops = _ops()
    D = G.LABEL_D[variant]
    emb, labels = G.label_case(variant, L, k)
    want = G.label_select(emb, labels, k)
    d_emb = _offset(emb, cuda) if variant == "d1024_emb_off" else emb.to(cuda)
    d_lab = _offset(labels, cuda) if variant == "d1024_labels_off" else labels.to(cuda)
    assert d_emb.data_ptr() % 16 == (4 if variant == "d1024_emb_off" else 0)
    ltok = torch.arange(L * 2, dtype=I32).view(L, 2) + 100
    llen = torch.full((L,), 2, dtype=I32)
    h_cap = 6 + 3 * max(k, 1)
    hard, hlen, chosen = _run_labels(cuda, d_emb, d_lab, k, ltok, llen, h_cap)
    assert torch.equal(chosen, want)
    ids, lens = G.prompt_ids(want, ltok, llen, h_cap)
    assert torch.equal(hard, ids) and torch.equal(hlen, lens)
    if k >= 1:
        rows = Out(cuda, (5, k, D), torch.float32, -7.0)
        idx = Out(cuda, (5, k), I32, -7)
        ops.label_topk(d_emb, d_lab, k, rows.t, idx=idx.t)
        torch.cuda.synchronize()
        assert torch.equal(idx.cpu(), want)
        assert torch.equal(rows.cpu(), labels[want.long()])
        rows2 = Out(cuda, (5, k, D), torch.float32, -7.0)
        ops.label_topk(d_emb, d_lab, k, rows2.t)              # idx=None
        torch.cuda.synchronize()
        assert torch.equal(rows2.cpu(), labels[want.long()])


@pytest.mark.parametrize("k", [3, 5])
def test_label_choice_float(cuda, k):
    """Random-normal data at D = 1024, L = 527 against the float64 top-k (margin >= 1e-3,
    asserted in test_glue_ref.py); the unaligned fallback agrees."""
    emb, labels = G.label_float_case(k)
    want = G.label_select(emb, labels, k)
    ltok = torch.arange(527 * 2, dtype=I32).view(527, 2)
    llen = torch.full((527,), 2, dtype=I32)
    for lab in (labels.to(cuda), _offset(labels, cuda)):
        _, _, chosen = _run_labels(cuda, emb.to(cuda), lab, k, ltok, llen, 32)
        assert torch.equal(chosen, want)


@pytest.mark.parametrize("with_chosen", [True, False])
@pytest.mark.parametrize("cap", ["roomy", "exact", "small", "tiny"])
@pytest.mark.parametrize("k", [0, 3, 5])
def test_prompt_assembly(cuda, k, cap, with_chosen):
    """Label lengths 0, 1, max_tok and beyond max_tok (clamped); an h_cap that fits exactly and
    ones too small (truncated, hard_len == h_cap, nothing behind the row); zero padding."""
    emb, labels, ltok, llen = G.prompt_case()
    want = G.label_select(emb, labels, k)
    _, full = G.prompt_ids(want, ltok, llen, 64)
    h_cap = {"roomy": int(full.max()) + 5, "exact": int(full.max()), "small": max(int(full.min()) - 2, 3),
             "tiny": 1}[cap]
    ids, lens = G.prompt_ids(want, ltok, llen, h_cap)
    hard, hlen, chosen = _run_labels(cuda, emb.to(cuda), labels.to(cuda), k, ltok, llen, h_cap,
                                     with_chosen)
    assert torch.equal(hard, ids) and torch.equal(hlen, lens)
    if with_chosen:
        assert torch.equal(chosen, want)
    if cap in ("small", "tiny"):
        assert bool((hlen == h_cap).all())
    if cap == "exact":
        assert int(hlen.max()) == h_cap and bool((hlen <= h_cap).all())
    if k == 0:
        assert hard[0, :min(7, h_cap)].tolist() == [1858, 389, 1223, 287, 428, 6597, 13][:h_cap]


# ------------------------------------------------------------------ embeddings
def _tables(V, npos, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, D, generator=g).to(dtype), torch.randn(npos, D, generator=g).to(dtype))


@pytest.mark.parametrize("optional", [True, False])
@pytest.mark.parametrize("D", [768, 200])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_prefill_embed(cuda, dtype, D, optional):
    """hard_len 0 / 1 / h_cap in one launch, Pmax > h_cap + n_soft, soft_ld > n_soft * D,
    embed / last_row present and None: one f32 add per element, so exact."""
    ops = _ops()
    B, h_cap, n_soft, V = 3, 4, 3, 50
    Pmax = h_cap + n_soft + 2
    soft_ld = n_soft * D + 8
    wte, wpe = _tables(V, Pmax, D, dtype, 1)
    g = torch.Generator().manual_seed(2)
    hard_ids = torch.randint(0, V, (B, h_cap), generator=g, dtype=I32)
    hard_len = torch.tensor([0, 1, h_cap], dtype=I32)
    soft = torch.randn(B * soft_ld, generator=g)
    embed = Out(cuda, (B, Pmax, D), torch.float32, -7.0) if optional else None
    last = Out(cuda, (B,), I32, -7) if optional else None
    x = Out(cuda, (B, Pmax, D), torch.float32, -7.0)
    plen = Out(cuda, (B,), I32, -7)
    ops.prefill_embed(hard_ids.to(cuda), hard_len.to(cuda), soft.to(cuda), soft_ld, n_soft,
                      wte.to(cuda), wpe.to(cuda), B, Pmax, embed.t if embed else None, x.t, plen.t,
                      last.t if last else None)
    torch.cuda.synchronize()
    r_embed, r_x, r_plen, r_last = G.prefill_embed(hard_ids, hard_len, soft, soft_ld, n_soft, wte,
                                                   wpe, B, Pmax)
    assert torch.equal(x.cpu(), r_x) and torch.equal(plen.cpu(), r_plen)
    if optional:
        assert torch.equal(embed.cpu(), r_embed) and torch.equal(last.cpu(), r_last)


@pytest.mark.parametrize("D", [768, 200])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_tokens(cuda, dtype, D):
    """Direct and rowmap forms (padding slots, cpos present and None)."""
    ops = _ops()
    V, npos, nphys = 50, 20, 7
    wte, wpe = _tables(V, npos, D, dtype, 3)
    g = torch.Generator().manual_seed(4)
    tok = torch.randint(0, V, (nphys,), generator=g, dtype=I32)
    pos = torch.randint(0, npos, (nphys,), generator=g, dtype=I32)
    d = [t.to(cuda) for t in (tok, pos, wte, wpe)]
    x = Out(cuda, (nphys, D), torch.float32, -7.0)
    ops.embed_tokens(d[0], d[1], d[2], d[3], x.t)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), G.embed_tokens(tok, pos, wte, wpe)[0])
    x5 = Out(cuda, (5, D), torch.float32, -7.0)
    ops.embed_tokens(d[0], d[1], d[2], d[3], x5.t, R=5)
    torch.cuda.synchronize()
    assert torch.equal(x5.cpu(), G.embed_tokens(tok, pos, wte, wpe, R=5)[0])
    rowmap = torch.tensor([0, 2, 5, 7, 6, 7], dtype=I32)       # 7 = nphys: padding slots
    r_x, r_cpos = G.embed_tokens(tok, pos, wte, wpe, rowmap, nphys)
    for with_cpos in (True, False):
        xm = Out(cuda, (6, D), torch.float32, -7.0)
        cpos = Out(cuda, (6,), I32, -7) if with_cpos else None
        ops.embed_tokens_map(d[0], d[1], rowmap.to(cuda), nphys, d[2], d[3], xm.t, 6,
                             cpos=cpos.t if cpos else None)
        torch.cuda.synchronize()
        assert torch.equal(xm.cpu(), r_x)
        if with_cpos:
            assert torch.equal(cpos.cpu(), r_cpos)


@pytest.mark.parametrize("extra", [0, 3])
def test_prefix_ids_assemble(cuda, extra):
    ops = _ops()
    B, h_cap, n_soft = 4, 5, 3
    Pmax = h_cap + n_soft + extra
    g = torch.Generator().manual_seed(6)
    hard_ids = torch.randint(1, 50257, (B, h_cap), generator=g, dtype=I32)
    hard_len = torch.tensor([0, 1, h_cap, 3], dtype=I32)
    soft_idx = torch.randint(1, 50257, (B, n_soft), generator=g, dtype=I32)
    out = Out(cuda, (B, Pmax), I32, -7)
    ops.prefix_ids_assemble(hard_ids.to(cuda), hard_len.to(cuda), soft_idx.to(cuda), n_soft, B,
                            Pmax, out.t)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), G.prefix_ids(hard_ids, hard_len, soft_idx, n_soft, B, Pmax))


# ------------------------------------------------------------------ argmax over partials
@pytest.mark.parametrize("nblk", [1, 63, 64, 65, "lmhead"])
@pytest.mark.parametrize("M", [1, 5, 8])
def test_argmax_finalize(cuda, M, nblk):
    """Integer-valued partials (ties everywhere); row 0 has its maximum twice, in block nblk // 3
    and in the last block, the last block holding the lower index; odd rows have their maximum
    in the last block alone."""
    ops = _ops()
    nblk = ops.lmhead_nblk(50257) if nblk == "lmhead" else nblk
    g = torch.Generator().manual_seed(M * 100 + nblk)
    pv = torch.randint(0, 50, (M, nblk), generator=g).float()
    pi = torch.stack([torch.randperm(nblk * 4, generator=g)[:nblk] + 1 for _ in range(M)]).to(I32)
    pv[0, nblk // 3] = 100.0
    pv[0, -1] = 100.0
    pi[0, -1] = 0
    pv[1::2, -1] = 99.0
    idx = Out(cuda, (M,), I32, -7)
    ops.argmax_finalize(pv.to(cuda), pi.to(cuda), M, nblk, idx.t)
    torch.cuda.synchronize()
    want = G.argmax_partials(pv, pi)
    assert int(want[0]) == 0 and (M < 2 or int(want[1]) == int(pi[1, -1]))
    assert torch.equal(idx.cpu(), want)


# ------------------------------------------------------------------ greedy step
GREEDY_KEYS = ("out_ids", "out_len", "done", "pos", "next_tok", "step_ctr", "all_done")


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("nblk", [1, 70])
@pytest.mark.parametrize("R", [1, 5, 6, 9])
def test_greedy_step(cuda, R, nblk, mapped):
    """greedy_init, then 6 launches with max_steps = 4: rows that hit stop0, stop1, or never stop,
    maxima tied across blocks (nblk = 70); the rowmap form runs on a bucket of R + 3 slots
    re-compacted before every launch."""
    ops = _ops()
    max_steps, stop0, stop1, V = 4, 13, 14, nblk * 16
    scripts = G.greedy_scripts(R, V, stop0, stop1)
    plen = torch.arange(R, dtype=I32) % 4 + 3
    ref = G.greedy_init(plen, R, max_steps)
    dev = {k: Out(cuda, tuple(ref[k].shape), I32, -7) for k in GREEDY_KEYS}
    ops.greedy_init(R, plen.to(cuda), dev["pos"].t, dev["done"].t, dev["out_len"].t,
                    dev["out_ids"].t, max_steps, dev["step_ctr"].t, dev["all_done"].t)
    dev["next_tok"].t.zero_()
    torch.cuda.synchronize()
    for key in GREEDY_KEYS:
        assert torch.equal(dev[key].cpu(), ref[key]), key
    Rb = R + 3
    rowmap_d = torch.full((Rb,), R, dtype=I32, device=cuda)
    n_act = torch.zeros(1, dtype=I32, device=cuda)
    stops_seen = set()
    for n in range(6):
        step = int(ref["step_ctr"][0])
        rows = torch.stack([scripts[r].row(step, int(ref["next_tok"][r]) if n else -1)
                            for r in range(R)])
        _, pv, pi = G.partials_from_logits(rows, nblk, 1)
        if mapped:
            rowmap = torch.full((Rb,), R, dtype=I32)
            rowmap[:R] = G.compact_rows(ref["done"])
            ops.compact_rows(dev["done"].t, R, rowmap_d, n_act)
            torch.cuda.synchronize()
            assert torch.equal(rowmap_d.cpu(), rowmap) and int(n_act) == int((ref["done"] == 0).sum())
            act = rowmap.long().clamp(max=R - 1)
            pv_c, pi_c = pv[act].clone(), pi[act].clone()
            pv_c[rowmap >= R] = 1e9                     # padding slots: junk that would win
            pi_c[rowmap >= R] = 7
            ref, alive_in = G.greedy_step(ref, pv_c, pi_c, max_steps, stop0, stop1, rowmap, R)
            ops.greedy_step_map(pv_c.to(cuda), pi_c.to(cuda), Rb, rowmap_d, R, nblk,
                                dev["step_ctr"].t, max_steps, stop0, stop1, dev["out_ids"].t,
                                dev["out_len"].t, dev["done"].t, dev["pos"].t, dev["next_tok"].t,
                                dev["all_done"].t)
        else:
            ref, alive_in = G.greedy_step(ref, pv, pi, max_steps, stop0, stop1)
            ops.greedy_step(pv.to(cuda), pi.to(cuda), R, nblk, dev["step_ctr"].t, max_steps, stop0,
                            stop1, dev["out_ids"].t, dev["out_len"].t, dev["done"].t,
                            dev["pos"].t, dev["next_tok"].t, dev["all_done"].t)
        torch.cuda.synchronize()
        got = {k: dev[k].cpu() for k in GREEDY_KEYS}
        for key in ("out_ids", "out_len", "done", "next_tok", "step_ctr"):
            assert torch.equal(got[key], ref[key]), (key, n)
        assert torch.equal(got["pos"][alive_in], ref["pos"][alive_in]), n
        assert got["all_done"].tolist() == ref["all_done"].tolist(), n   # [flag, 0 (re-armed), alive]
        if n >= max_steps:
            assert torch.equal(got["out_ids"], prev_got["out_ids"])
            assert torch.equal(got["out_len"], prev_got["out_len"])
        prev_got = got
        for r in range(R):
            if int(ref["done"][r]):
                stops_seen.add(int(ref["out_ids"][r, int(ref["out_len"][r]) - 1]))
    assert int(ref["all_done"][0]) == 1
    if R >= 3:
        assert stops_seen == {stop0, stop1} and not bool(ref["done"].all())


# ------------------------------------------------------------------ beam step
BEAM_KEYS_I = ("seq_len", "stopped", "next_tok", "pos", "kvrow", "step_ctr")


@pytest.mark.parametrize("beam,nblk,topk", G.BEAM_CASES)
def test_beam_step(cuda, beam, nblk, topk):
    """Seven launches (max_steps = 6) of three clips on the scripted logits of
    glue_ref.beam_scripts, state compared with glue_ref.beam_step after every launch: one clip
    finishes early and must stay frozen, one has every kept candidate from source 1 and carries a
    stopped beam beside live ones, one never stops (the run ends by max_steps) and has exact ties
    inside a row across blocks and between two sources (conditions asserted on the CPU in
    test_glue_ref.py::test_gpu_beam_case_conditions).

    Scores: |kernel - float64 reference| <= 4 * yardstick + 1e-6, the yardstick being the same
    reference evaluated in float32 on the CPU against its float64 run, the largest difference
    over all cases of this test (one number for all cases: it measures what float32 costs on
    this kind of input, and a single case's own figure can be small by luck).
    Measured on an MI355X: yardstick 1.41e-06, worst kernel error 2.44e-06 (beam 1, nblk 70), so
    the tolerance is 6.65e-06."""
    ops = _ops()
    C, max_steps, Lmax = 3, G.BEAM_MAX_STEPS, G.BEAM_LMAX
    R = C * beam
    init, trace = G.beam_case_trace(beam, nblk)
    yard = G.beam_yardstick()
    tol = 4.0 * yard + 1e-6
    dev = {}
    for key, t in init.items():
        dt = torch.float32 if t.dtype == torch.float64 else I32
        dev[key] = Out(cuda, tuple(t.shape), dt, -7, init=t.to(dt))
    tok_tmp = Out(cuda, (R, max_steps), I32, -7)
    kv_tmp = Out(cuda, (R, Lmax), I32, -7)
    worst = 0.0
    for n, (rows, first, ref, _) in enumerate(trace):
        pstat, pv, pi = G.partials_from_logits(rows, nblk, topk)
        ops.beam_step(pstat.to(cuda), pv.to(cuda), pi.to(cuda), C, beam, nblk, topk, first,
                      G.STOP, dev["step_ctr"].t, max_steps, dev["scores"].t, dev["seq_len"].t,
                      dev["stopped"].t, dev["tokens"].t, tok_tmp.t, dev["kvrow"].t, kv_tmp.t, Lmax,
                      dev["pos"].t, dev["next_tok"].t, dev["all_done"].t)
        torch.cuda.synchronize()
        tok_tmp.cpu(), kv_tmp.cpu()                       # guards
        got = {k: dev[k].cpu() for k in dev}
        assert torch.equal(got["tokens"], ref["tokens"]), n
        for key in BEAM_KEYS_I:
            assert torch.equal(got[key], ref[key].to(got[key].dtype)), (key, n)
        assert int(got["all_done"][0]) == int(ref["all_done"][0]), n
        err = float((got["scores"].double() - ref["scores"]).abs().max())
        worst = max(worst, err)
        assert err <= tol, (n, err, tol)
    print(f"beam {beam} nblk {nblk} topk {topk}: score error {worst:.3e}, yardstick {yard:.3e}, "
          f"tolerance {tol:.3e}")
