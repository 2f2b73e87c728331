"""CPU tests that pin tests/glue_ref.py, the reference the GPU glue tests compare against:
glue_ref's beam / greedy / prompt functions against oracle/caption.py on scripted logits, and
the input conditions (selection margins, the cases each scenario must contain) of every
float-valued case of tests/test_gpu_glue.py, so a bad seed fails here and not on the GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ref as G  # noqa: E402
from oracle import caption as OC  # noqa: E402

P0 = 3      # prompt rows in front of the generated tokens


def _oracle_script(V, seed, stop_from=1):
    """Rows without ties (torch.topk's tie order is no contract): V distinct multiples of 1/8 from
    [0, 8] per row; from ``stop_from`` on the stop token is raised by 4 (the one column it may then
    equal goes to -1/8), so beams stop at different steps."""
    def distinct(r, step, prev):
        rng = np.random.default_rng([seed, 77, step, prev + 1])
        r = torch.from_numpy(rng.permutation(65)[:V] / 8.0)
        if step >= stop_from:
            r[G.STOP] = r[G.STOP] + 4.0
            for t in (r == r[G.STOP]).nonzero().flatten().tolist():
                if t != G.STOP:
                    r[t] = -0.125
        else:
            r[G.STOP] = -1.0
        return r
    return G.Script(V, seed, hi=8.0, rules=[(None, None, distinct)])


def _stub(script, V):
    """gpt2_logits over a one-hot wte: the last row of ``generated`` names the previous token and
    its length the step."""
    def gpt2_logits(embeds, sd, past=None, pos0=0):
        B, L, _ = embeds.shape
        step = L - P0
        out = torch.zeros(B, L, V)
        for b in range(B):
            prev = int(embeds[b, -1].argmax()) if step > 0 else -1
            out[b, -1] = script.row(step, prev).float()
        return out, None
    return gpt2_logits


# beam, entry_length, seed: (5, 3) ends by length; (3, 8) and (8, 8) stop beam by beam
@pytest.mark.parametrize("beam,entry,seed", [(1, 8, 1), (3, 8, 2), (5, 3, 3), (8, 8, 4), (5, 8, 5)])
def test_beam_ref_matches_oracle(monkeypatch, beam, entry, seed):
    V = 48
    script = _oracle_script(V, seed)
    monkeypatch.setattr(OC, "gpt2_logits", _stub(script, V))
    sd = {"gpt.transformer.wte.weight": torch.eye(V)}
    toks, scores = OC.generate_beam(torch.zeros(1, P0, V), sd, beam_size=beam, entry_length=entry)
    _, tr = G.beam_trace([script], beam, entry, [P0], P0 + entry + 1, entry + 1)
    info = [d for x in tr for d in x[3]]
    gap, _ = G.decisive_gaps(info)
    ties = G.has_ties(info)
    assert gap >= G.MARGIN and not ties, (gap, ties)      # torch.topk's tie order is no contract
    final = tr[-1][2]
    rt, rs = G.beam_result(final, 0, beam)
    assert all(abs(a - b) >= 1e-4 for a, b in zip(rs[:-1], rs[1:])), rs
    assert rt == toks
    assert max(abs(a - b) for a, b in zip(rs, scores)) <= 1e-5, (rs, scores)
    # the launch past the end changed nothing but the step counter
    for key in ("tokens", "scores", "seq_len", "stopped", "kvrow", "pos", "next_tok"):
        assert torch.equal(tr[-1][2][key], tr[-2][2][key]), key
    stopped = [x[2]["stopped"] for x in tr]
    if (beam, entry) == (5, 3):
        assert not bool(final["stopped"].all()) and int(final["all_done"][0]) == 1
    if beam in (3, 8):
        assert any(0 < int(s.sum()) < beam for s in stopped), "beams must stop at different steps"
        assert bool(final["stopped"].all())


@pytest.mark.parametrize("seed,entry", [(4, 12), (2, 12), (3, 4)])
def test_greedy_ref_matches_oracle(monkeypatch, seed, entry):
    V, nblk = 768, 48                       # stop1 = 764 needs 765 columns
    stop0, stop1 = OC.STOP_GREEDY

    def boost(r, step, prev):        # a distinct top four per row, the stops rising with the step
        rng = np.random.default_rng([seed, 78, step, prev + 1])
        r = r.clone()
        r[torch.from_numpy(rng.choice(V, 4, replace=False))] = torch.tensor([8.5, 9.0, 9.5, 10.25]).double()
        a, b = (stop0, stop1) if seed % 2 else (stop1, stop0)
        r[a] = 6.0 + 0.75 * step          # passes the row's 10.25 at step 6, never equals it
        r[b] = r[a] - 0.25
        return r
    script = G.Script(V, seed, hi=8.0, rules=[(None, None, boost)])
    monkeypatch.setattr(OC, "gpt2_logits", _stub(script, V))
    sd = {"gpt.transformer.wte.weight": torch.eye(V)}
    margins = []
    toks = OC.generate2(torch.zeros(1, P0, V), sd, entry_length=entry, margins=margins)
    assert min(margins) >= 0.125                     # argmax ties are no contract of torch.argmax
    state = G.greedy_init(torch.tensor([P0]), 1, entry)
    for n in range(entry + 1):
        step = int(state["step_ctr"][0])
        prev = int(state["next_tok"][0]) if n else -1
        _, pv, pi = G.partials_from_logits(script.row(step, prev)[None], nblk, 1)
        state, _ = G.greedy_step(state, pv, pi, entry, stop0, stop1)
        if int(state["done"][0]):
            break
    assert state["out_ids"][0, :int(state["out_len"][0])].tolist() == toks
    assert int(state["all_done"][0]) == 1
    if entry == 4:
        assert len(toks) == 4 and toks[-1] not in (stop0, stop1)      # ended by length
    else:
        assert toks[-1] in (stop0, stop1)


@pytest.mark.parametrize("k", [0, 1, 3, 5])
def test_label_prompt_ref_matches_oracle(k):
    g = torch.Generator().manual_seed(7 + k)
    emb, labels = torch.randn(4, 64, generator=g), torch.randn(40, 64, generator=g)
    assert G.label_margin(emb, labels, max(k, 1)) >= G.MARGIN
    lens = torch.randint(1, 5, (40,), generator=g, dtype=torch.int32)
    tok = torch.randint(20, 5000, (40, 4), generator=g, dtype=torch.int32)
    chosen = G.label_select(emb, labels, k)
    if k:
        assert torch.equal(chosen.long(), OC.sound_effect_choice(emb.double(), labels.double(), k))
    ids, hl = G.prompt_ids(chosen, tok, lens, 40)
    table = [tok[l, :int(lens[l])].tolist() for l in range(40)]
    for b in range(4):
        want = OC.prompt_ids(chosen[b].tolist(), table)
        assert ids[b, :int(hl[b])].tolist() == want and int(hl[b]) == len(want)
        assert not ids[b, int(hl[b]):].any()


def test_label_select_is_stable():
    """Equal similarities keep the lower label index, at the kept/dropped edge too."""
    emb = torch.tensor([[1.0, 0.0]])
    labels = torch.tensor([[4.0, 0], [5.0, 1], [4.0, 2], [6.0, 3], [4.0, 4]])
    assert G.label_select(emb, labels, 3).tolist() == [[3, 1, 0]]
    assert G.label_select(emb, labels, 4).tolist() == [[3, 1, 0, 2]]


def test_partials_and_argmax_ref():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0, 2.0, 3.0, 1.0, 0.5]])
    pstat, pv, pi = G.partials_from_logits(x, 2, 2)
    assert pv.tolist() == [[[3.0, 3.0], [3.0, 2.0]]] and pi.tolist() == [[[1, 2], [5, 4]]]
    assert pstat[0, :, 0].tolist() == [3.0, 3.0]
    lse = torch.log((pstat[0, :, 1].double() * torch.exp(pstat[0, :, 0].double() - 3.0)).sum()) + 3.0
    assert abs(float(lse - torch.logsumexp(x.double(), -1))) < 1e-6
    assert G.argmax_partials(pv[:, :, :1], pi[:, :, :1]).tolist() == [1]


# ------------------------------------------------------------------ input conditions of the GPU cases
@pytest.mark.parametrize("k", [3, 5])
def test_gpu_label_float_margin(k):
    emb, labels = G.label_float_case(k)
    assert G.label_margin(emb, labels, k) >= G.MARGIN


def _insertion_topk(sim, k, K, fixed):
    """The prompt kernel's running top-k on one similarity row: labels visited in increasing
    index, a new value placed in front of the first entry it strictly beats.  ``fixed`` False is
    the loop before the fix (the displaced entry carried down with a strict compare, so it
    jumped over equal entries below it); True shifts everything below down by one."""
    tv, sel = [-float("inf")] * K, [2 ** 31 - 1] * K
    for l, sv in enumerate(sim):
        if K == 3 and not sv > tv[2]:
            continue
        placed = False
        for i in range(K):
            if i < k and ((fixed and placed) or sv > tv[i]):
                tv[i], sv = sv, tv[i]
                sel[i], l = l, sel[i]
                placed = True
    return sel[:k]


LABEL_INPUTS = sorted({(G.LABEL_D[v], L, k) for v, L, k in G.LABEL_CASES})


@pytest.mark.parametrize("D,L,k", LABEL_INPUTS)
def test_gpu_label_exact_case_conditions(D, L, k):
    """Every exact-tie input of test_gpu_glue.py has an answer that depends on the data: the
    similarities of a clip are not constant, the expected labels are not simply 0 .. k-1, the
    clips differ, and (L >= 3, k >= 3) clip 0 holds the arranged tie that tells the insertion
    loop before the fix from the stable order, while the fixed loop gives the stable order on
    every clip."""
    variant = {1024: "d1024", 64: "d64", 100: "d100"}[D]
    emb, labels = G.label_case(variant, L, k)
    for other in ("d1024_labels_off", "d1024_emb_off"):
        if D == 1024:                                   # the unaligned variants run the same data
            assert all(torch.equal(a, b) for a, b in zip(G.label_case(other, L, k), (emb, labels)))
    want = G.label_select(emb, labels, k).tolist()
    sim = G.similarities(emb, labels).tolist()
    K = 3 if k == 3 else 16
    for b in range(5):
        if L >= 3:
            assert len(set(sim[b])) >= max(2, min(L, k + 1) // 2), (b, sorted(sim[b]))
        if k:
            assert _insertion_topk(sim[b], k, K, True) == want[b]
    if L >= 3 and k >= 1:
        assert len({tuple(w) for w in want}) >= 2, want
        assert any(w != list(range(k)) for w in want), want
    if L >= 3 and k >= 3:
        p, q, r = (0, 1, L - 1) if L < 8 else (1, L // 2, L - 2)
        assert want[0][:3] == [r, p, q] and sim[0][p] == sim[0][q] < sim[0][r]
        assert not torch.equal(labels[p], labels[q])
        assert _insertion_topk(sim[0], k, K, False) != want[0]


def test_gpu_label_cases_reach_the_last_row():
    """For every L > 1 some case (k < L) chooses the last label row: the loader's tail counts."""
    for D in (1024, 64, 100):
        for L in G.LABEL_L[1:]:
            hit = False
            for k in G.LABEL_K:
                if 1 <= k < L:
                    variant = {1024: "d1024", 64: "d64", 100: "d100"}[D]
                    hit |= bool((G.label_select(*G.label_case(variant, L, k), k) == L - 1).any())
            assert hit, (D, L)


def test_gpu_prompt_case_conditions():
    """test_prompt_assembly's chosen labels cover token counts 0, 1, max_tok and more than
    max_tok, and the clips choose different labels."""
    emb, labels, ltok, llen = G.prompt_case()
    assert ltok.shape[1] == G.PROMPT_MAX_TOK
    for k in (3, 5):
        want = G.label_select(emb, labels, k)
        lens = {int(llen[i]) for i in want.flatten().tolist()}
        assert {0, 1, G.PROMPT_MAX_TOK} <= lens and max(lens) > G.PROMPT_MAX_TOK, lens
        assert len({tuple(w) for w in want.tolist()}) == 5
        _, n = G.prompt_ids(want, ltok, llen, 64)
        assert len(set(n.tolist())) >= 2          # rows of different length: "exact" fits only the longest


def _props(beam, nblk):
    init, tr = G.beam_case_trace(beam, nblk)
    props = set()
    for n, (rows, first, st, info) in enumerate(tr):
        prev = tr[n - 1][2] if n else init
        for c, d in enumerate(info):
            if d["skipped"]:
                if n < G.BEAM_MAX_STEPS:
                    props.add("frozen_clip")
                continue
            if not first and beam > 1 and len(set(d["src"])) == 1 and d["src"][0] != 0:
                props.add("one_source")
            if not first:
                was = [int(prev["stopped"][c * beam + i]) for i in d["src"]]
                if any(was) and not all(was):
                    props.add("stopped_carried")
            for a, b in zip(d["cand"][:-1], d["cand"][1:]):
                if b[0] == -float("inf"):
                    continue
                if a[0] == b[0] and a[1] == b[1] and a[2] // G.BEAM_W != b[2] // G.BEAM_W:
                    props.add("row_tie_across_blocks")
                if a[0] == b[0] and a[1] != b[1]:
                    props.add("source_tie")
    final = tr[-1][2]
    if not bool(final["stopped"].all()) and int(tr[G.BEAM_MAX_STEPS - 1][2]["all_done"][0]):
        props.add("ends_by_max_steps")
    return props


@pytest.mark.parametrize("beam,nblk", sorted({(b, n) for b, n, _ in G.BEAM_CASES}))
def test_gpu_beam_case_conditions(beam, nblk):
    """Margins and content of the beam scenario test_gpu_glue.py replays at this (beam, nblk)."""
    _, tr = G.beam_case_trace(beam, nblk)
    gap, structural = G.decisive_gaps([d for x in tr for d in x[3]])
    assert gap >= G.MARGIN and structural, (gap, structural)
    # float32 makes the same choices (the yardstick compares like with like)
    _, tr32 = G.beam_case_trace(beam, nblk, torch.float32)
    for a, b in zip(tr, tr32):
        for key in ("tokens", "stopped", "kvrow", "next_tok", "pos"):
            assert torch.equal(a[2][key], b[2][key]), key
    for x in tr:            # no log-probability underflows: every row's spread stays small
        assert float((x[0].max(-1).values - x[0].min(-1).values).max()) <= 20.0
    props = _props(beam, nblk)
    want = {"frozen_clip", "ends_by_max_steps"}
    if beam >= 2:
        want |= {"source_tie", "stopped_carried"}
    if nblk >= 3:
        want.add("row_tie_across_blocks")
    if 2 <= beam <= 5 or (beam > 5 and nblk >= 3):
        want.add("one_source")
    assert want <= props, want - props


def test_gpu_beam_yardstick_is_small():
    y = G.beam_yardstick()
    print("beam score yardstick (float32 vs float64 reference):", y)
    assert 0 < y < 1e-4
