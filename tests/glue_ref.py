"""Plain CPU references of the GPT-2 decode glue ops (csrc/gpt2.hip), one function per op.

Pure torch / numpy on the CPU, float64 wherever a float is computed; nothing here reads a golden
or the original project.  Each function states the op's contract the way the kernel comments and
oracle/caption.py do; tests/test_glue_ref.py ties these functions to the oracle, and
tests/test_gpu_glue.py compares the kernels with them.

The second half builds the inputs both test files share: scripted logits ``row(step, previous
token)`` (a fixed pseudo-random table, quantised to multiples of 1/8) and the beam / greedy
scenarios made from them.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

VOCAB = 50257            # the stride of generate_beam's flattened candidate index src * V + tok
HEAD = (1858, 389)       # "There", " are"
TAIL = (287, 428, 6597, 13)   # " in", " this", " audio", "."
SOMETHING = 1223
COMMA = 11
I32 = torch.int32


# ------------------------------------------------------------------ prompt
def similarities(emb: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    return emb.double() @ labels.double().t()


def label_select(emb: torch.Tensor, labels: torch.Tensor, k: int) -> torch.Tensor:
    """sound_effect_choice: per clip the indices of the k largest emb . label, ordered by value
    descending, then label index ascending (a stable sort).  [B, k] int32."""
    sim = similarities(emb, labels)
    order = torch.argsort(sim, dim=-1, descending=True, stable=True)
    return order[:, :k].to(I32).contiguous()


def selection_gaps(sorted_vals: torch.Tensor, k: int) -> torch.Tensor:
    """The gaps that decide a top-k selection of descending ``sorted_vals`` [.., n]: between
    neighbours in the kept order and between the last kept and the first dropped."""
    n = min(k + 1, sorted_vals.shape[-1])
    return sorted_vals[..., :n - 1] - sorted_vals[..., 1:n]


def label_margin(emb, labels, k) -> float:
    """Smallest non-tie gap deciding label_select (inf when there is none)."""
    v = torch.sort(similarities(emb, labels), dim=-1, descending=True).values
    g = selection_gaps(v, k)
    g = g[g > 0]
    return float(g.min()) if g.numel() else float("inf")


def prompt_ids(chosen: torch.Tensor, label_tok: torch.Tensor, label_len: torch.Tensor, h_cap: int):
    """compose_discrete_prompts + padding: "There are" + the chosen labels' tokens joined by ","
    + "in this audio."; k = 0 gives "There are something in this audio.".  A label contributes
    min(label_len, max_tok) tokens (max_tok = label_tok.shape[1]).  Rows are truncated to h_cap
    and zero padded; hard_len = min(n, h_cap).  -> (hard_ids [B, h_cap], hard_len [B]) int32."""
    B, k = chosen.shape
    max_tok = label_tok.shape[1]
    ids = torch.zeros(B, h_cap, dtype=I32)
    lens = torch.zeros(B, dtype=I32)
    for b in range(B):
        out = list(HEAD)
        if k == 0:
            out.append(SOMETHING)
        for q in range(k):
            l = int(chosen[b, q])
            out += label_tok[l, :min(int(label_len[l]), max_tok)].tolist()
            if q + 1 < k:
                out.append(COMMA)
        out += list(TAIL)
        n = min(len(out), h_cap)
        ids[b, :n] = torch.tensor(out[:n], dtype=I32)
        lens[b] = n
    return ids, lens


# ------------------------------------------------------------------ embeddings
def prefill_embed(hard_ids, hard_len, soft, soft_ld, n_soft, wte, wpe, B, Pmax):
    """clap_to_gpt's concat + the wte / wpe lookup.  Row (b, p): embed = wte[hard id] for
    p < H_b, the soft row p - H_b (``soft`` is flat, clip b starts at b * soft_ld) for
    H_b <= p < P_b = H_b + n_soft, zero beyond; x = embed + wpe[p] for p < P_b, zero beyond;
    plen = P_b; last_row = b * Pmax + P_b - 1.  -> (embed, x) f32 [B, Pmax, D], (plen, last_row)."""
    D = wte.shape[1]
    w, pe, sf = wte.double(), wpe.double(), soft.double().reshape(-1)
    embed = torch.zeros(B, Pmax, D, dtype=torch.float64)
    x = torch.zeros(B, Pmax, D, dtype=torch.float64)
    plen = torch.zeros(B, dtype=I32)
    last = torch.zeros(B, dtype=I32)
    for b in range(B):
        H = int(hard_len[b])
        P = H + n_soft
        for p in range(min(P, Pmax)):
            if p < H:
                e = w[int(hard_ids[b, p])]
            else:
                o = b * soft_ld + (p - H) * D
                e = sf[o:o + D]
            embed[b, p] = e
            x[b, p] = e + pe[p]
        plen[b] = P
        last[b] = b * Pmax + P - 1
    return embed.float(), x.float(), plen, last


def embed_tokens(tok, pos, wte, wpe, rowmap=None, nphys=None, R=None):
    """Decode-step input: x[r] = wte[tok[ph]] + wpe[pos[ph]] with ph = r (direct) or rowmap[r];
    a slot with rowmap[r] >= nphys is padding: a zero row and cpos 0.  cpos[r] = pos[ph].
    -> (x f32 [R, D], cpos int32 [R])."""
    R = R if R is not None else (tok.numel() if rowmap is None else rowmap.numel())
    D = wte.shape[1]
    w, pe = wte.double(), wpe.double()
    x = torch.zeros(R, D, dtype=torch.float64)
    cpos = torch.zeros(R, dtype=I32)
    for r in range(R):
        ph = r if rowmap is None else int(rowmap[r])
        if rowmap is not None and ph >= nphys:
            continue
        x[r] = w[int(tok[ph])] + pe[int(pos[ph])]
        cpos[r] = pos[ph]
    return x.float(), cpos


def prefix_ids(hard_ids, hard_len, soft_idx, n_soft, B, Pmax):
    """get_prefix_tokens' id row: the hard id (p < H_b), the soft row's argmax
    (H_b <= p < H_b + n_soft), 0 for padding.  [B, Pmax] int32."""
    out = torch.zeros(B, Pmax, dtype=I32)
    for b in range(B):
        H = int(hard_len[b])
        for p in range(Pmax):
            if p < H:
                out[b, p] = hard_ids[b, p]
            elif p < H + n_soft:
                out[b, p] = soft_idx[b, p - H]
    return out


# ------------------------------------------------------------------ LM-head partials
def partials_from_logits(logits: torch.Tensor, nblk: int, topk: int):
    """What the LM head hands over for ``logits`` [M, nblk * W]: per block of W columns
    pstat[.., 0] = the block max, pstat[.., 1] = sum exp(x - block max), and the block's top-`topk`
    (value descending, index ascending) as pv / pi with pi the global column.
    -> pstat f32 [M, nblk, 2], pv f32 [M, nblk, topk], pi int32 [M, nblk, topk]."""
    M, V = logits.shape
    W = V // nblk
    assert W * nblk == V and topk <= W
    x = logits.double().reshape(M, nblk, W)
    mx = x.max(-1).values
    pstat = torch.stack((mx, torch.exp(x - mx[..., None]).sum(-1)), -1)
    order = torch.argsort(x, dim=-1, descending=True, stable=True)[..., :topk]
    pv = torch.gather(x, -1, order)
    pi = order + (torch.arange(nblk) * W)[None, :, None]
    assert torch.equal(pv.float().double(), pv), "logits must be exact in f32"
    return pstat.float().contiguous(), pv.float().contiguous(), pi.to(I32).contiguous()


def argmax_partials(pv: torch.Tensor, pi: torch.Tensor) -> torch.Tensor:
    """Per row the index of the best partial: value descending, index ascending.  [M] int32."""
    M = pv.shape[0]
    v = pv.reshape(M, -1).double().numpy()
    i = pi.reshape(M, -1).numpy().astype(np.int64)
    out = [int(i[m][np.lexsort((i[m], -v[m]))[0]]) for m in range(M)]
    return torch.tensor(out, dtype=I32)


# ------------------------------------------------------------------ greedy (generate2)
def greedy_init(plen: torch.Tensor, R: int, max_steps: int) -> Dict[str, torch.Tensor]:
    return dict(pos=(plen[:R] - 1).to(I32), done=torch.zeros(R, dtype=I32),
                out_len=torch.zeros(R, dtype=I32), out_ids=torch.zeros(R, max_steps, dtype=I32),
                next_tok=torch.zeros(R, dtype=I32), step_ctr=torch.zeros(1, dtype=I32),
                all_done=torch.zeros(3, dtype=I32))


def compact_rows(done: torch.Tensor) -> torch.Tensor:
    """rowmap: the rows with done == 0 in increasing order, then nrows (padding)."""
    n = done.numel()
    act = [r for r in range(n) if not int(done[r])]
    return torch.tensor(act + [n] * (n - len(act)), dtype=I32)


def greedy_step(state, pv, pi, max_steps, stop0, stop1, rowmap=None, nphys=None):
    """One step of generate2's bookkeeping over the partial rows c < R (physical row r = c, or
    rowmap[c]; r >= nphys is a padding slot).  A row that is not done and has step < max_steps
    appends its argmax and is done once that is stop0 or stop1; next_tok takes the argmax of
    every visited row; pos advances while step < max_steps (it is only meaningful for rows alive
    at entry: ``alive_in``).  Then step_ctr += 1, all_done = [no row alive or step + 1 >=
    max_steps, 0, rows still alive].  -> (new state, alive_in bool [nrows])."""
    s = copy.deepcopy(state)
    step = int(s["step_ctr"][0])
    best = argmax_partials(pv, pi)
    alive_in = torch.zeros(s["done"].numel(), dtype=torch.bool)
    total = 0
    for c in range(pv.shape[0]):
        r = c if rowmap is None else int(rowmap[c])
        if rowmap is not None and r >= nphys:
            continue
        t = int(best[c])
        d = int(s["done"][r])
        alive_in[r] = not d
        if not d and step < max_steps:
            s["out_ids"][r, step] = t
            s["out_len"][r] = step + 1
            d = int(t == stop0 or t == stop1)
            s["done"][r] = d
        total += int(not d)
        s["next_tok"][r] = t
        if step < max_steps:
            s["pos"][r] += 1
    s["step_ctr"][0] = step + 1
    s["all_done"] = torch.tensor([int(total == 0 or step + 1 >= max_steps), 0, total], dtype=I32)
    return s, alive_in


# ------------------------------------------------------------------ beam (generate_beam)
def beam_init(C: int, beam: int, plen: Sequence[int], max_steps: int, Lmax: int,
              dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The state before the first step: pos of each clip's row 0 = its prompt length."""
    R = C * beam
    pos = torch.zeros(R, dtype=I32)
    pos[::beam] = torch.tensor(list(plen), dtype=I32)
    return dict(scores=torch.zeros(R, dtype=dtype), seq_len=torch.ones(R, dtype=dtype),
                stopped=torch.zeros(R, dtype=I32), tokens=torch.zeros(R, max_steps, dtype=I32),
                kvrow=torch.zeros(R, Lmax, dtype=I32), pos=pos,
                next_tok=torch.zeros(R, dtype=I32), step_ctr=torch.zeros(1, dtype=I32),
                all_done=torch.zeros(3, dtype=I32))


def beam_step(state, logits_rows: torch.Tensor, first: bool, beam: int, stop: int,
              max_steps: int, info: Optional[list] = None):
    """One step of generate_beam's selection for every clip (C = rows / beam), in the dtype of
    state["scores"] (float64: the reference; float32: the yardstick of the kernel's error).

    logits_rows: [C, V'] on the first step (one prefill row per clip), [C * beam, V'] after.
    log_softmax per row.  First step: the top-`beam` tokens (log-prob descending, token
    ascending) become beams 0.. with score = log-prob, length 1.  Later steps: a stopped row
    offers only token 0 at zero cost and unchanged length, a live row every token at length + 1;
    candidates are ranked by (score + logp) / newlen descending, then src * 50257 + tok ascending;
    the chosen rows take their source's history, score = average * newlen, stopped = the source's
    flag or tok == stop.  A clip whose beams are all stopped (after the first step), or any clip
    at step >= max_steps, is left untouched.  kvrow[dst][s] names the physical row that wrote
    position s of dst's history: first step r0 (the clip's first row) for s < P, later the
    source's map for s < P, the source row itself at s == P, -1 beyond (P = the clip's pos at
    entry); pos becomes P on the first step, P + 1 after.  Then step_ctr += 1 and
    all_done[0] = every row stopped or step_ctr >= max_steps.

    ``info`` (a list) receives per clip a dict: skipped, src, tok, and the candidates' sorted
    (value, src, tok, score, logp, newlen) rows down to the first dropped one."""
    s = copy.deepcopy(state)
    dt = s["scores"].dtype
    step = int(s["step_ctr"][0])
    R = s["scores"].numel()
    C = R // beam
    Lmax = s["kvrow"].shape[1]
    lp_all = torch.log_softmax(logits_rows.to(dt), dim=-1)
    V = lp_all.shape[1]
    for c in range(C):
        r0 = c * beam
        rows = slice(r0, r0 + beam)
        if (not first and bool(state["stopped"][rows].all())) or step >= max_steps:
            if info is not None:
                info.append(dict(skipped=True))
            continue
        P = int(state["pos"][r0])
        if first:
            lp = lp_all[c]
            score = torch.zeros(1, dtype=dt)
            newlen = torch.ones(1, dtype=dt)
            vals = lp[None, :].clone()
            lps = lp[None, :]
        else:
            st = state["stopped"][rows].bool()
            newlen = torch.where(st, state["seq_len"][rows], state["seq_len"][rows] + 1)
            lps = lp_all[rows].clone()
            lps[st] = -float("inf")
            lps[st, 0] = 0.0
            score = state["scores"][rows]
            vals = (score[:, None] + lps) / newlen[:, None]
        nsrc = vals.shape[0]
        flat = (torch.arange(nsrc)[:, None] * VOCAB + torch.arange(V)[None, :]).reshape(-1)
        order = np.lexsort((flat.numpy(), -vals.reshape(-1).double().numpy()))[:beam + 1]
        src = [int(flat[o]) // VOCAB for o in order]
        tok = [int(flat[o]) % VOCAB for o in order]
        if info is not None:
            info.append(dict(skipped=False, src=src[:beam], tok=tok[:beam], cand=[
                (float(vals[i, t]), i, t, float(score[i]), float(lps[i, t]), float(newlen[i]))
                for i, t in zip(src, tok)]))
        for q in range(beam):
            i, t, dst = src[q], tok[q], r0 + q
            sr = r0 + i
            s["tokens"][dst, :step] = state["tokens"][sr, :step]
            s["tokens"][dst, step] = t
            s["seq_len"][dst] = newlen[i]
            s["scores"][dst] = vals[i, t] * newlen[i]
            s["stopped"][dst] = int(t == stop) if first else int(state["stopped"][sr]) | int(t == stop)
            s["next_tok"][dst] = t
            s["pos"][dst] = P if first else P + 1
            kv = torch.full((Lmax,), -1, dtype=I32)
            if first:
                kv[:P] = r0
            else:
                kv[:P] = state["kvrow"][sr, :P]
                if P < Lmax:
                    kv[P] = sr
            s["kvrow"][dst] = kv
    s["step_ctr"][0] = step + 1
    s["all_done"][0] = int(bool(s["stopped"].all()) or step + 1 >= max_steps)
    return s


def beam_result(state, c: int, beam: int):
    """generate_beam's return for clip c: token lists ordered by score / length descending, and
    those final scores."""
    rows = slice(c * beam, (c + 1) * beam)
    fin = (state["scores"][rows] / state["seq_len"][rows]).double()
    order = torch.argsort(fin, descending=True, stable=True).tolist()
    outs = [state["tokens"][c * beam + i, :int(state["seq_len"][c * beam + i])].tolist() for i in order]
    return outs, [float(fin[i]) for i in order]


# ================================================================== shared inputs
class Script:
    """Scripted logits: row(step, prev) is row [step, prev] of a fixed pseudo-random table with V
    columns (prev = -1 before the first token): uniform in [0, hi), quantised to multiples of 1/8
    (exact in f32; equal entries are exactly equal), then the edits of ``rules`` applied in order.
    A rule is (step or None, prev or None, {tok: value} or callable(row, step, prev) -> row)."""

    def __init__(self, V: int, seed: int, hi: float = 6.0, rules: Sequence = ()):
        self.V, self.seed, self.hi, self.rules = V, seed, hi, list(rules)
        self._rows: Dict = {}

    def row(self, step: int, prev: int) -> torch.Tensor:
        key = (step, prev)
        if key not in self._rows:
            rng = np.random.default_rng([self.seed, step, prev + 1])
            r = torch.from_numpy(np.floor(rng.uniform(0.0, self.hi, self.V) * 8.0) / 8.0)
            for st, pv, edit in self.rules:
                if (st is None or st == step) and (pv is None or pv == prev):
                    if callable(edit):
                        r = edit(r, step, prev)
                    else:
                        for t, v in edit.items():
                            r[t] = v
            assert float(r.max() - r.min()) <= 20.0
            self._rows[key] = r.clone()
        return self._rows[key]


def decisive_gaps(info: list):
    """(smallest non-tie gap, all ties structural) over the selections recorded in ``info``:
    a tie (zero gap) is structural when both candidates have the same score, log-prob and
    length, so every precision sees it as a tie."""
    mn, ok = float("inf"), True
    for d in info:
        if d["skipped"]:
            continue
        cand = d["cand"]
        for a, b in zip(cand[:-1], cand[1:]):
            if b[0] == -float("inf"):         # a stopped row's other tokens: never candidates
                continue
            g = a[0] - b[0]
            if g == 0.0:
                ok = ok and a[3:] == b[3:]
            else:
                mn = min(mn, g)
    return mn, ok


def has_ties(info: list) -> bool:
    return any(a[0] == b[0] > -float("inf") for d in info if not d["skipped"]
               for a, b in zip(d["cand"][:-1], d["cand"][1:]))


STOP = 13


def beam_scripts(V: int, beam: int, seed: int = 0) -> List[Script]:
    """Three clips for the beam tests (stop = 13, every designed token < 16 or in a later block):

    clip 0  generic rows (hi = 10); at step 2 every source gets the same row with the stop token at
            20, so every beam stops there (ranked by its score) and the clip is finished while
            the others go on;
    clip 1  step 0 ranks tokens 1, 2, .. by 1/8 apart; at step 1 the row after token 2 (source 1)
            holds `beam` high tokens and every other row is nearly flat, so every kept candidate
            comes from source 1; at step 2 the row after token 1 stops (a stopped beam carried
            alongside live ones); later steps favour the stop token a little, so beams stop at
            different steps;
    clip 2  never stops (the stop token is 0 everywhere); step 0 has tokens 3 and `far` (in
            another block when V >= 48) at the same logit above token 5, and the step-1 rows after
            3 and after `far` are identical and contain the same logit twice (7 and `far2`):
            ties inside a row across blocks and between two sources of equal score."""
    far, far2 = (35, 40) if V >= 48 else (9, 11)
    end_row = Script(V, seed * 10 + 5, hi=10.0, rules=[(None, None, {STOP: 20.0})])
    c0 = Script(V, seed * 10 + 1, hi=10.0, rules=[(2, None, lambda r, s, p: end_row.row(2, 0).clone())])

    def flat(r, step, prev):
        return torch.floor(r) / 8.0                   # values in {0, 1/8, .., 5/8}

    c1 = Script(V, seed * 10 + 2, rules=[
        (0, None, {1 + j: 12.0 - j / 8.0 for j in range(8)}),
        (1, None, flat),
        (1, 2, {1 + j: 12.0 - j / 8.0 for j in range(beam)}),
        (2, 1, {STOP: 12.0}),
        (3, None, {STOP: 6.5}), (4, None, {STOP: 7.0}), (5, None, {STOP: 7.5}),
    ])
    tie_row = Script(V, seed * 10 + 4, rules=[(None, None, {STOP: 0.0, 7: 10.0, far2: 10.0, 2: 9.5})])
    c2 = Script(V, seed * 10 + 3, rules=[
        (None, None, {STOP: 0.0}),
        (0, None, {3: 12.0, far: 12.0, 5: 11.5}),
        (1, 3, lambda r, s, p: tie_row.row(1, 0).clone()),
        (1, far, lambda r, s, p: tie_row.row(1, 0).clone()),
    ])
    return [c0, c1, c2]


def beam_trace(scripts: Sequence[Script], beam: int, max_steps: int, plen: Sequence[int], Lmax: int,
               launches: int, dtype=torch.float64, stop: int = STOP):
    """Drives beam_step for ``launches`` launches on the scripts (one per clip).  -> (state before
    the first launch, [(logits_rows, first, state after, info)] per launch).  The rows of launch n
    are row(step, next_tok) of the state before it."""
    C = len(scripts)
    state = beam_init(C, beam, plen, max_steps, Lmax, dtype)
    init = state
    out = []
    for n in range(launches):
        first = n == 0
        step = int(state["step_ctr"][0])
        if first:
            rows = torch.stack([scripts[c].row(0, -1) for c in range(C)])
        else:
            rows = torch.stack([scripts[r // beam].row(step, int(state["next_tok"][r]))
                                for r in range(C * beam)])
        info: list = []
        state = beam_step(state, rows, first, beam, stop, max_steps, info)
        out.append((rows, first, state, info))
    return init, out


def greedy_scripts(R: int, V: int, stop0: int, stop1: int, seed: int = 0) -> List[Script]:
    """One script per row for the greedy tests: row r never stops (r % 3 == 0; with V >= 48 its
    maximum sits twice in the row, in two different blocks, and in the last block at step 1),
    hits stop0 at step 1 + (r // 3) % 3 (r % 3 == 1) or stop1 at step (r // 3) % 2
    (r % 3 == 2)."""
    out = []
    for r in range(R):
        rules: list = [(None, None, {stop0: 0.0, stop1: 0.0})]
        if r % 3 == 0 and V >= 48:
            rules += [(None, None, {20 + r: 9.0, 4: 9.0}), (1, None, {V - 1: 9.0, 4: 0.0, 20 + r: 9.0})]
        if r % 3 == 1:
            rules.append((1 + (r // 3) % 3, None, {stop0: 9.0}))
        if r % 3 == 2:
            rules.append(((r // 3) % 2, None, {stop1: 9.0}))
        out.append(Script(V, seed * 100 + r, hi=8.0, rules=rules))
    return out


# ------------------------------------------------------------------ the GPU beam / label cases
BEAM_CASES = [(b, n, b) for b in (1, 2, 3, 4, 5, 6, 8) for n in (1, 3, 70)] + \
             [(1, 1, 8), (3, 70, 8), (5, 3, 8), (6, 70, 8)]     # (beam, nblk, topk)
BEAM_W = 16               # columns per LM-head block
BEAM_MAX_STEPS = 6
BEAM_LAUNCHES = 7         # one launch past max_steps
BEAM_PLEN = (3, 5, 4)
BEAM_LMAX = 12
MARGIN = 1e-3             # every deciding non-tie gap of a float-valued case, in float64

_traces: Dict = {}


def beam_case_trace(beam: int, nblk: int, dtype=torch.float64):
    key = (beam, nblk, dtype)
    if key not in _traces:
        _traces[key] = beam_trace(beam_scripts(nblk * BEAM_W, beam), beam, BEAM_MAX_STEPS,
                                  BEAM_PLEN, BEAM_LMAX, BEAM_LAUNCHES, dtype)
    return _traces[key]


def beam_yardstick() -> float:
    """The largest |scores(float32 run) - scores(float64 run)| of beam_step over every launch of
    every (beam, nblk) of BEAM_CASES: what plain float32 arithmetic costs on these inputs."""
    worst = 0.0
    for beam, nblk in sorted({(b, n) for b, n, _ in BEAM_CASES}):
        t64, t32 = beam_case_trace(beam, nblk)[1], beam_case_trace(beam, nblk, torch.float32)[1]
        for a, b in zip(t64, t32):
            worst = max(worst, float((a[2]["scores"] - b[2]["scores"].double()).abs().max()))
    return worst


LABEL_L = (1, 3, 4, 5, 8, 9, 13, 16, 527)
LABEL_K = (0, 1, 3, 5, 16)
LABEL_D = {"d1024": 1024, "d1024_labels_off": 1024, "d1024_emb_off": 1024, "d64": 64, "d100": 100}
LABEL_CASES = [(v, L, k) for v in LABEL_D for L in LABEL_L for k in LABEL_K if k <= L]


def label_case(variant: str, L: int, k: int):
    """The inputs of test_label_choice_exact_ties[variant-L-k] (5 clips)."""
    return label_exact_case(5, LABEL_D[variant], L, seed=L * 31 + k)


def label_exact_case(B: int, D: int, L: int, seed: int):
    """Small-integer embeddings [B, D] and labels [L, D] in [-4, 4]: every similarity is exact in
    f32, so equal values tie exactly.  The rows are random (small integers tie now and then by
    themselves); embedding columns 0 and 1 are equal, and for L >= 3 three rows are arranged for
    clip 0: its best label goes to a late index r, the best of the rest to an early index p, and
    index q (p < q < r) takes a copy of row p with 1 moved from column 1 to column 0 -- a different
    row with the same similarities.  Clip 0 then meets two equal values before a larger one, all in its
    top three: the order a running top-k loses when a displaced entry jumps an equal one.
    (p, q, r) = (0, 1, L - 1) for L < 8 and (1, L // 2, L - 2) from 8 on, where clip 1's best
    label also moves to the last row."""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randint(-4, 5, (B, D), generator=g).float()
    labels = torch.randint(-4, 5, (L, D), generator=g).float()
    emb[:, 1] = emb[:, 0]
    if L < 3:
        return emb, labels
    p, q, r = (0, 1, L - 1) if L < 8 else (1, L // 2, L - 2)

    def swap(a, b):
        t = labels[a].clone()
        labels[a] = labels[b]
        labels[b] = t
    sim = similarities(emb[:1], labels)[0]
    swap(int(sim.argmax()), r)
    sim = similarities(emb[:1], labels)[0]
    rest = torch.where(sim < sim[r], sim, torch.full_like(sim, -float("inf")))
    swap(int(rest.argmax()), p)
    labels[q] = labels[p]
    labels[q, 0] += 1.0                 # the embeddings' columns 0 and 1 are equal
    labels[q, 1] -= 1.0
    if L >= 8:                          # clip 1's best label sits in the last row (the loader's tail)
        best = int(similarities(emb[1:2], labels)[0].argmax())
        if best not in (p, q, r):
            swap(best, L - 1)
    return emb, labels


PROMPT_MAX_TOK = 4


def prompt_case():
    """test_prompt_assembly's inputs: 5 clips, 8 labels of D = 64 whose token counts cover 0, 1,
    max_tok and more than max_tok (clamped).  -> emb, labels, label_tok [8, 4], label_len [8]."""
    emb, labels = label_exact_case(5, 64, 8, seed=6)
    llen = torch.tensor([0, 1, 4, 7, 2, 0, 9, 3], dtype=I32)
    ltok = torch.arange(8 * PROMPT_MAX_TOK, dtype=I32).view(8, PROMPT_MAX_TOK) + 1000
    return emb, labels, ltok, llen


def label_float_case(k: int):
    """Random-normal embeddings [5, 1024] and labels [527, 1024] for the float label cases."""
    g = torch.Generator().manual_seed(100 + k)
    return torch.randn(5, 1024, generator=g), torch.randn(527, 1024, generator=g)
