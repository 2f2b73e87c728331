"""Plain CPU references of the magic-decoding and text-tower kernels (csrc/magic.hip, plus
zs_l2norm_rows of csrc/norm.hip), one function per op.

Pure torch / numpy on the CPU; every float is computed in ``dtype``: float64 is the reference,
float32 the yardstick (the same formula in the kernel's precision; its distance from the float64
run on a case's own data is what plain float32 arithmetic costs there).  Nothing here reads a
golden or the original project.  tests/test_magic_ref.py ties these functions to oracle/magic.py
and asserts the input conditions of the GPU cases; tests/test_gpu_magic_kernels.py compares the
kernels with them.

Layout (the header comment of magic.hip): C clips x b beams x W candidates; candidate
c = (k*b + j)*W + w is row c of every per-candidate buffer and also the physical row of the
context store ``ctx`` [rows][Lmax][768]; ``kvrow[beam][t]`` names the physical row that holds
position t of the beam's history.

The second half builds the inputs both test files share.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

D = 768
VOCAB = 50257
STOP = 13
I32 = torch.int32
F64 = torch.float64
F32 = torch.float32
MARGIN = 1e-3            # every deciding gap of a float-valued selection, in float64
NEG_INF = -float("inf")


# ------------------------------------------------------------------ text tower glue
def _ln(v, g, be, eps, dtype):
    v = v.to(dtype)
    c = v - v.mean(-1, keepdim=True)
    var = (c * c).mean(-1, keepdim=True)
    return c * torch.rsqrt(var + eps) * g.to(dtype) + be.to(dtype)


def bert_embed_ln(ids, L, word, pos, type0, g, be, eps=1e-12, dtype=F64):
    """BertEmbeddings: row r of ids [T*L] -> LN(word[ids[r]] + pos[r % L] + type0), eps inside
    the square root, biased variance.  -> [T*L, 768]."""
    r = torch.arange(ids.numel())
    v = word.to(dtype)[ids.long()] + pos.to(dtype)[r % L] + type0.to(dtype)
    return _ln(v, g, be, eps, dtype)


def rows_view(flat, rows, ld, width=D):
    """Rows r * ld .. r * ld + width of a flat buffer as a [rows, width] view."""
    return flat.as_strided((rows, width), (ld, 1))


def layernorm_dual(y, rows, ldy, g, be, eps, x, ldx, dtype=F64):
    """x[r*ldx : r*ldx + 768] = LN(y[r*ldy : r*ldy + 768]) for r < rows on flat buffers; every
    other element of x is untouched.  The operand copy h holds the same rows (stride ldh) rounded
    from the f32 x to h's type.  -> x afterwards (flat, ``dtype``)."""
    out = x.to(dtype).clone()
    rows_view(out, rows, ldx).copy_(_ln(rows_view(y, rows, ldy), g, be, eps, dtype))
    return out


def l2norm_rows(x, eps=1e-12, dtype=F64):
    """x / max(||x||, eps) per row."""
    x = x.to(dtype)
    return x / x.norm(dim=-1, keepdim=True).clamp(min=eps)


# ------------------------------------------------------------------ row top-k
def row_topk(logits, V, k, mode, dtype=F64):
    """Per row of logits [R, ld] the k largest of its first V columns: value descending, then
    index ascending.  Values: mode 0 log(softmax), mode 1 softmax, both over those V columns.
    -> (values [R, k] ``dtype``, indices [R, k] int32)."""
    x = logits[:, :V].to(dtype)
    order = torch.argsort(x, dim=-1, descending=True, stable=True)[:, :k]
    val = torch.log_softmax(x, -1) if mode == 0 else torch.softmax(x, -1)
    return val.gather(1, order), order.to(I32)


# ------------------------------------------------------------------ candidate rows
def expand(kvrow, pos, W, kvrow_c):
    """enlarge_past_key_values as an index copy: candidate c of beam c // W gets
    kvrow_c[c][t] = kvrow[c // W][t] for t < pos[c // W] (later entries untouched) and
    pos_c[c] = pos[c // W].  -> (kvrow_c afterwards, pos_c)."""
    out = kvrow_c.clone()
    n = out.shape[0]
    pos_c = torch.zeros(n, dtype=I32)
    for c in range(n):
        j = c // W
        p = int(pos[j])
        out[c, :p] = kvrow[j, :p]
        pos_c[c] = p
    return out, pos_c


def maxcos(hid, W, ctx, kvrow, pos, dtype=F64):
    """The degeneration penalty: maxcos[c] = max over t < pos[j] of
    cos(ctx[kvrow[j][t]][t], hid[c]) with j = c // W, read from ctx as it is on entry; then
    ctx[c][pos[j]] becomes a bit copy of hid[c] and nothing else of ctx changes.
    hid [ncand, 768] and ctx [rows, Lmax, 768] share a type (f32 or bf16); the arithmetic is in
    ``dtype`` on those values.  -> (maxcos [ncand] ``dtype``, ctx afterwards)."""
    n = hid.shape[0]
    out = ctx.clone()
    mc = torch.zeros(n, dtype=dtype)
    for c in range(n):
        j = c // W
        p = int(pos[j])
        h = hid[c].to(dtype)
        rows = ctx[kvrow[j, :p].long(), torch.arange(p)].to(dtype)          # [p, 768]
        cos = (rows @ h) / (torch.sqrt((rows * rows).sum(-1)) * torch.sqrt((h * h).sum()))
        mc[c] = cos.max()
        out[c, p] = hid[c]
    return mc, out


def score(pval, maxcos_v, text, audio, b, W, nact, temp, alpha, beta, score_temp, out, dtype=F64):
    """plug_and_play_fast_ranking's score with the CLAP term: per clip k over its n = nact * W
    active candidates c = k*b*W + i (i < n): cl = cos(text[c], audio[k]) / temp,
    score = ((1 - alpha) pval - alpha maxcos + beta (cl - logsumexp(cl))) / score_temp; the
    clip's entries i >= n are untouched.  -> ``out`` afterwards (``dtype``)."""
    res = out.to(dtype).clone()
    C = audio.shape[0]
    n = nact * W
    for k in range(C):
        idx = k * b * W + torch.arange(n)
        t = text[idx].to(dtype)
        a = audio[k].to(dtype)
        cl = (t @ a) / (torch.sqrt((t * t).sum(-1)) * torch.sqrt((a * a).sum())) / temp
        clap = cl - torch.logsumexp(cl, 0)
        s = (1.0 - alpha) * pval[idx].to(dtype) - alpha * maxcos_v[idx].to(dtype) + beta * clap
        res[idx] = s / score_temp
    return res


# ------------------------------------------------------------------ the step
STATE_KEYS = ("scores", "seq_len", "stopped", "tokens", "kvrow", "pos", "cdone", "ntok")
JUNK = -7


def step_init(C, b, W, plen: Sequence[int], Smax, Lmax, dtype=F64) -> Dict[str, torch.Tensor]:
    """The state before the first step as the decoder sets it up: the prompt of clip k lives in
    physical row k*b*W at positions < plen[k].  Only beam 0 of a clip carries a history and a
    position then (the first step reads nothing else); what a step must not read or must
    overwrite before use (later kvrow entries, the other beams' rows, tokens) holds JUNK."""
    nb = C * b
    kvrow = torch.full((nb, Lmax), JUNK, dtype=I32)
    pos = torch.full((nb,), JUNK, dtype=I32)
    for k in range(C):
        kvrow[k * b, :plen[k]] = k * b * W
        pos[k * b] = plen[k]
    return dict(scores=torch.zeros(nb, dtype=dtype), seq_len=torch.ones(nb, dtype=dtype),
                stopped=torch.zeros(nb, dtype=I32), tokens=torch.full((nb, Smax), JUNK, dtype=I32),
                kvrow=kvrow, pos=pos, cdone=torch.zeros(C, dtype=I32), ntok=torch.zeros(C, dtype=I32),
                sel_c=torch.full((nb,), -1, dtype=I32))


def _select(vals: torch.Tensor, n: int) -> List[int]:
    """The flat indices of the n largest (+ the first dropped): value descending, index ascending."""
    v = vals.double().numpy()
    return [int(i) for i in np.lexsort((np.arange(v.size), -v))[:n + 1]]


def step(state, score_v, cand, b, W, first, greedy, stop, step_no, max_steps, hid=None,
         info: Optional[list] = None):
    """zs_magic_step: one selection step for every clip, in the dtype of state["scores"].

    A clip with cdone set or step_no >= max_steps[k] is left untouched.  Otherwise, with
    sc = the clip's b*W scores and P = pos of its beam 0:
      greedy (b = 1)  the best of sc[0 .. W): source 0, score 0, length 1, stopped = token == stop;
      first           the b best of sc[0 .. W) (beam 0's row): source 0, score = sc, length 1;
      beam            len1[j] = seq_len[j] + (0 if stopped[j] else 1); a stopped beam offers only
                      w = 0 at value 0 (its other candidates are -inf); avg = (scores[j] + v) /
                      len1[j] over all b*W; the b best: source j, score = avg * len1[j], length
                      len1[j], stopped = stopped[j] or token == stop.
    "best" is value descending, then flat index i = j*W + w ascending.  Beam q (in selection
    order) then takes its source's history: kvrow[q][t < P] and tokens[q][s < step_no] from the
    source as they were on entry, kvrow[q][P] = the chosen candidate's row c, tokens[q][step_no]
    = cand[c], pos[q] = P + 1, sel_h[q] = a bit copy of hid[c]; later entries of kvrow / tokens
    are untouched.  ntok[k] = step_no + 1; cdone[k] = 1 when every new beam is stopped or
    step_no + 1 >= max_steps[k].

    ``sel_c`` records for each beam the candidate row its sel_h came from (-1: never written);
    with ``hid`` given the state's ``sel_h`` is updated too.  ``info`` receives per clip a dict:
    live, branch, src, w, top (the selection values down to the first dropped one)."""
    s = {k: v.clone() for k, v in state.items()}
    dt = state["scores"].dtype
    C = state["cdone"].numel()
    sc_all = score_v.to(dt)
    for k in range(C):
        bw = k * b
        if int(state["cdone"][k]) or step_no >= int(max_steps[k]):
            if info is not None:
                info.append(dict(live=False))
            continue
        sc = sc_all[bw * W:(bw + b) * W]
        if greedy or first:
            order = _select(sc[:W], 1 if greedy else b)
            top = [float(sc[i]) for i in order]
            chosen = order[:1 if greedy else b]
            sel = [(0, i, torch.zeros((), dtype=dt) if greedy else sc[i], torch.ones((), dtype=dt),
                    int(cand[bw * W + i]) == stop) for i in chosen]
            branch = "greedy" if greedy else "first"
        else:
            st = state["stopped"][bw:bw + b].bool()
            len1 = state["seq_len"][bw:bw + b] + (~st).to(dt)
            v = sc.view(b, W).clone()
            v[st] = NEG_INF
            v[st, 0] = 0.0
            avg = ((state["scores"][bw:bw + b, None] + v) / len1[:, None]).reshape(-1)
            order = _select(avg, b)
            top = [float(avg[i]) for i in order]
            sel = [(i // W, i % W, avg[i] * len1[i // W], len1[i // W],
                    bool(st[i // W]) or int(cand[bw * W + i]) == stop) for i in order[:b]]
            branch = "beam"
        P = int(state["pos"][bw])
        for q, (j, w, val, ln, stp) in enumerate(sel):
            c = (bw + j) * W + w
            s["kvrow"][bw + q, :P] = state["kvrow"][bw + j, :P]
            s["kvrow"][bw + q, P] = c
            s["tokens"][bw + q, :step_no] = state["tokens"][bw + j, :step_no]
            s["tokens"][bw + q, step_no] = cand[c]
            s["scores"][bw + q] = val
            s["seq_len"][bw + q] = ln
            s["stopped"][bw + q] = int(stp)
            s["pos"][bw + q] = P + 1
            s["sel_c"][bw + q] = c
            if hid is not None:
                s["sel_h"][bw + q] = hid[c]
        s["ntok"][k] = step_no + 1
        if all(x[4] for x in sel) or step_no + 1 >= int(max_steps[k]):
            s["cdone"][k] = 1
        if info is not None:
            info.append(dict(live=True, branch=branch, src=[x[0] for x in sel],
                             w=[x[1] for x in sel], top=top,
                             was_stopped=[int(state["stopped"][bw + x[0]]) for x in sel]))
    return s


def beam_result(state, k: int, b: int):
    """generate_beam_magic's return for clip k: token lists ordered by score / length descending
    and those final scores."""
    rows = slice(k * b, (k + 1) * b)
    fin = (state["scores"][rows] / state["seq_len"][rows]).double()
    order = torch.argsort(fin, descending=True, stable=True).tolist()
    outs = [state["tokens"][k * b + i, :int(state["seq_len"][k * b + i])].tolist() for i in order]
    return outs, [float(fin[i]) for i in order]


# ================================================================== shared inputs
def selection_margin(info: list) -> float:
    """Smallest gap between consecutive selection values (the kept ones and the first dropped
    one) over the live clips recorded in ``info``; a -inf value (never a candidate) ends a
    clip's list."""
    mn = float("inf")
    for d in info:
        if not d["live"]:
            continue
        for a, c in zip(d["top"][:-1], d["top"][1:]):
            if c == NEG_INF:
                break
            mn = min(mn, a - c)
    return mn


def _repair(v: np.ndarray, fixed: np.ndarray, base: np.ndarray, len1: np.ndarray, W: int, n_sel: int):
    """Moves scripted scores (f32, in place) until the n_sel best averages
    (base[j] + v[i]) / len1[j] and the first dropped one lie at least 2 * MARGIN apart: the lower
    of a close pair drops by 0.05 or a little more in the average (or the upper rises when the
    lower is ``fixed``: a stopped beam's row, whose value the state decides; the amounts vary so
    that the two moves cannot undo each other for ever)."""
    idx = np.arange(v.size)
    for it in range(10000):
        eff = np.where(fixed, np.where(idx % W == 0, 0.0, -np.inf), v.astype(np.float64))
        avg = (base[idx // W] + eff) / len1[idx // W]
        order = np.lexsort((idx, -avg))[:n_sel + 1]
        moved = False
        for a, c in zip(order[:-1], order[1:]):
            if avg[c] == -np.inf:
                break
            if avg[a] - avg[c] < 2 * MARGIN:
                if not fixed[c]:
                    v[c] = np.float32(v[c] - (0.05 + 0.003 * (it % 17)) * len1[c // W])
                elif not fixed[a]:
                    v[a] = np.float32(v[a] + (0.05 + 0.007 * (it % 13)) * len1[a // W])
                else:
                    return
                moved = True
                break
        if not moved:
            return


class Scenario:
    """A scripted multi-step run of ``step``: per step random scores in [-8, -0.5] (repaired to
    the margin against the float64 reference's own state), random candidate tokens with the stop
    token planted with probability stop_p[k] per candidate of clip k, every candidate of clip k
    the stop token at step all_stop[k] (None: never), and, in greedy runs with W > 1, the stop
    token on the lowest-scored candidate of the clips with stop_p 0 (offered, never taken).
    ``inputs[s]`` = (score f32 [R], cand int32 [R]); ``states[s]`` / ``info[s]`` = the float64
    reference after / during step s."""

    def __init__(self, C, b, W, greedy, seed, plen, max_steps, Smax, Lmax, stop_p, all_stop):
        self.C, self.b, self.W, self.greedy = C, b, W, greedy
        self.Smax, self.Lmax, self.plen = Smax, Lmax, tuple(plen)
        self.max_steps = torch.tensor(list(max_steps), dtype=I32)
        self.seed = seed
        R = C * b * W
        self.init = step_init(C, b, W, plen, Smax, Lmax)
        self.inputs, self.states, self.info = [], [], []
        state = self.init
        for s in range(Smax):
            rng = np.random.default_rng([seed, b, W, s])
            v = (-8.0 + 7.5 * rng.random(R)).astype(np.float32)
            cand = rng.integers(0, VOCAB - 1, R)
            cand[cand >= STOP] += 1
            clip = np.arange(R) // (b * W)
            cand[rng.random(R) < np.asarray(stop_p)[clip]] = STOP
            for k in range(C):
                rows = slice(k * b * W, (k + 1) * b * W)
                if all_stop[k] is not None and s == all_stop[k]:
                    cand[rows] = STOP
                first = s == 0
                if greedy or first:
                    n_sel = 1 if greedy else b
                    _repair(v[rows][:W], np.zeros(W, bool), np.zeros(1), np.ones(1), W, n_sel)
                    # (v[rows][:W] is a view: repaired in place)
                else:
                    st = state["stopped"][k * b:(k + 1) * b].bool().numpy()
                    len1 = state["seq_len"][k * b:(k + 1) * b].numpy() + (~st)
                    _repair(v[rows], np.repeat(st, W), state["scores"][k * b:(k + 1) * b].numpy(),
                            len1, W, b)
                if greedy and W > 1 and stop_p[k] == 0 and all_stop[k] is None:
                    cand[k * W + int(np.argmin(v[rows]))] = STOP
            score_v = torch.from_numpy(v.copy())
            cand_t = torch.from_numpy(cand.astype(np.int32))
            info: list = []
            state = step(state, score_v, cand_t, b, W, s == 0, greedy, STOP, s, self.max_steps,
                         info=info)
            self.inputs.append((score_v, cand_t))
            self.states.append(state)
            self.info.append(info)

    def replay(self, dtype):
        """The same inputs through ``step`` in ``dtype``: the states after each step."""
        state = step_init(self.C, self.b, self.W, self.plen, self.Smax, self.Lmax, dtype)
        out = []
        for s, (score_v, cand) in enumerate(self.inputs):
            state = step(state, score_v, cand, self.b, self.W, s == 0, self.greedy, STOP, s,
                         self.max_steps)
            out.append(state)
        return out

    def yardstick(self) -> float:
        """max |scores(float32 run) - scores(float64 run)| over every step."""
        return max(float((a["scores"] - f["scores"].double()).abs().max())
                   for a, f in zip(self.states, self.replay(F32)))

    def hid(self, s: int, dtype=F32) -> torch.Tensor:
        """The candidates' ln_f rows of step s [R, 768]: random, only ever copied."""
        g = torch.Generator().manual_seed(self.seed * 1000 + self.b * 100 + self.W + 7 * s)
        return torch.randn(self.C * self.b * self.W, D, generator=g).to(dtype)

    def props(self) -> set:
        """The situations this scenario contains."""
        out = set()
        b, C = self.b, self.C
        if len(set(self.plen)) == C:
            out.add("ragged_pos")
        for s, info in enumerate(self.info):
            prev = self.states[s - 1] if s else self.init
            now = self.states[s]
            live = [d["live"] for d in info]
            for k, d in enumerate(info):
                frozen_before = bool(prev["cdone"][k])
                if not d["live"]:
                    if frozen_before and any(live):
                        why = "stop" if bool(prev["stopped"][k * b:(k + 1) * b].all()) else "limit"
                        out.add(f"frozen_by_{why}_beside_live")
                    continue
                if s == self.Smax - 1:
                    out.add("last_legal_step")
                src = d["src"]
                if d["branch"] == "beam":
                    if sorted(src) == list(range(b)) and src != list(range(b)):
                        out.add("source_permutation")
                    if len(set(src)) < b:
                        out.add("duplicated_source")
                    # beam q reads source j < q after j was rewritten from another source
                    if any(j < q and src[j] != j for q, j in enumerate(src)):
                        out.add("overwritten_before_read")
                    if any(d["was_stopped"]) and not all(d["was_stopped"]):
                        out.add("stopped_survives")
                if d["branch"] == "greedy":
                    rows = slice(k * self.W, (k + 1) * self.W)
                    offered = bool((self.inputs[s][1][rows] == STOP).any())
                    if bool(now["stopped"][k]):
                        out.add("greedy_stop")
                    elif offered:
                        out.add("stop_offered_not_taken")
        return out


STEP_C, STEP_SMAX, STEP_LMAX = 3, 8, 16
STEP_PLEN = (5, 7, 6)                 # 7 + 8 steps write kvrow up to position 14 < Lmax
STEP_MAX_STEPS = (8, 5, 8)            # clip 1 is frozen by its own limit
STEP_BEAM = [(1, 1), (2, 2), (3, 25), (5, 8), (8, 8), (8, 64)]
STEP_GREEDY_W = [1, 15, 64]
# seeds whose runs contain every situation tests/test_magic_ref.py asks for
STEP_SEED = {(1, 1): 1, (2, 2): 1, (3, 25): 3, (5, 8): 3, (8, 8): 2, (8, 64): 5}

_scenarios: Dict = {}


def step_scenario(b: int, W: int, greedy: bool) -> Scenario:
    """The three-clip scenario of the GPU step test at (b, W): clip 0 meets the stop token now and
    then and on every candidate at step 3 (all beams stop: frozen beside live clips), clip 1
    (b >= 2: stop tokens now and then) is frozen by max_steps 5, clip 2 never stops and runs the
    last legal step.  Greedy: clip 0 stops at step 2."""
    key = (b, W, greedy)
    if key not in _scenarios:
        if greedy:
            sc = Scenario(STEP_C, 1, W, True, 11, STEP_PLEN, STEP_MAX_STEPS, STEP_SMAX, STEP_LMAX,
                          (0.0, 0.0, 0.0), (2, None, None))
        else:
            sc = Scenario(STEP_C, b, W, False, STEP_SEED[(b, W)], STEP_PLEN, STEP_MAX_STEPS,
                          STEP_SMAX, STEP_LMAX, (0.15, 0.15 if b >= 2 else 0.0, 0.0),
                          (3, None, None))
        _scenarios[key] = sc
    return _scenarios[key]


def tie_cases():
    """Exact-tie single steps (all values exact in float32): name -> dict(b, W, first, greedy,
    step, state, score, cand, max_steps, want = per clip the chosen (source, w) in order), two
    clips each."""
    out = {}
    Smax, Lmax = 8, 16
    g = torch.Generator().manual_seed(5)

    def cands(n):
        c = torch.randint(20, VOCAB, (n,), generator=g, dtype=I32)
        return c

    # first branch: b = 3 of W = 8; clip 0 has 3.0 twice and 2.5 three times (one kept), clip 1
    # is all equal
    b, W = 3, 8
    st = step_init(2, b, W, (6, 9), Smax, Lmax)
    sc = torch.tensor([1.0, 2.5, 2.5, 0.5, 2.5, 3.0, 3.0, 0.0] + [9.0] * 16 +
                      [1.25] * 8 + [9.0] * 16)
    out["first"] = dict(b=b, W=W, first=True, greedy=False, step=0, state=st, score=sc,
                        cand=cands(2 * b * W), want=[[(0, 5), (0, 6), (0, 1)], [(0, 0), (0, 1), (0, 2)]])
    # greedy: the maximum at w = 4 and w = 9; clip 1 all equal
    W = 15
    st = step_init(2, 1, W, (6, 9), Smax, Lmax)
    sc = torch.tensor([0.5 * (i % 4) for i in range(W)] + [-2.0] * W)
    sc[4] = sc[9] = 4.0
    out["greedy"] = dict(b=1, W=W, first=True, greedy=True, step=0, state=st, score=sc,
                         cand=cands(2 * W), want=[[(0, 4)], [(0, 0)]])
    # beam branch, step 2.  Clip 0: beams 0 and 1 have equal scores (-2) and lengths (2) and the
    # candidate value -1 at (0,0), (0,1), (1,0), (1,2); beam 2 (-3.5, 2) reaches the same average
    # -1 with 0.5 at (2,0): five equal averages, the three lowest flat indices win.  Clip 1:
    # beam 0 is stopped (score -2, length 2: average -1 through w = 0), beam 1 (score -2, length 1)
    # offers 0 at w = 1 and w = 3 (average -1 twice), beam 2 (-9, 2) reaches -1 with 6 at w = 2
    # (dropped: the highest flat index).
    b, W = 3, 4
    st = step_init(2, b, W, (6, 9), Smax, Lmax)
    nb = 2 * b
    st["scores"] = torch.tensor([-2.0, -2.0, -3.5, -2.0, -2.0, -9.0], dtype=F64)
    st["seq_len"] = torch.tensor([2.0, 2.0, 2.0, 2.0, 1.0, 2.0], dtype=F64)
    st["stopped"] = torch.tensor([0, 0, 0, 1, 0, 0], dtype=I32)
    st["tokens"][:, :2] = torch.randint(20, VOCAB, (nb, 2), generator=g, dtype=I32)
    for k, P in enumerate((8, 11)):
        rows = torch.randint(k * b * W, (k + 1) * b * W, (b, P), generator=g, dtype=I32)
        st["kvrow"][k * b:(k + 1) * b, :P] = rows
        st["pos"][k * b:(k + 1) * b] = P
    sc = torch.tensor([-1.0, -1.0, -4.0, -5.0, -1.0, -4.0, -1.0, -6.0, 0.5, -7.0, -7.0, -7.0,
                       5.0, 5.0, 5.0, 5.0, -3.0, 0.0, -3.0, 0.0, -1.0, -1.0, 6.0, -1.0])
    out["beam"] = dict(b=b, W=W, first=False, greedy=False, step=2, state=st, score=sc,
                       cand=cands(2 * b * W),
                       want=[[(0, 0), (0, 1), (1, 0)], [(0, 0), (1, 1), (1, 3)]])
    for c in out.values():
        c["max_steps"] = torch.tensor([8, 8], dtype=I32)
        assert torch.equal(c["score"].float().double(), c["score"].double())
    return out


# ------------------------------------------------------------------ maxcos / score / top-k inputs
def maxcos_case(C, b, W, Lmax, pos, seed, dtype=F32):
    """hid [C*b*W, 768], ctx [C*b*W, Lmax, 768], kvrow [C*b, Lmax] for ``pos`` [C*b] (ragged).
    hid = a direction shared by all candidates + noise.  Each beam's history is scattered over
    random physical rows of its clip; the slots (row, t) a history names hold noise plus up to
    0.6 of the shared direction (true cosines up to about 0.4),
    every other slot of ctx holds the shared direction (a decoy: its cosine with any candidate
    beats every true one), and so do the kvrow entries at t >= pos (random rows of the clip).  No
    history slot is a slot this launch writes (row c, position pos[c // W])."""
    g = torch.Generator().manual_seed(seed)
    R = C * b * W
    shared = torch.randn(D, generator=g)
    hid = (shared[None] + 0.8 * torch.randn(R, D, generator=g)).to(dtype)
    ctx = (shared[None, None] * (0.5 + torch.rand(R, Lmax, 1, generator=g))).to(dtype)
    kvrow = torch.zeros(C * b, Lmax, dtype=I32)
    written = {(c, int(pos[c // W])) for c in range(R)}
    used = set()
    for j in range(C * b):
        k = j // b
        for t in range(Lmax):
            while True:
                r = int(torch.randint(k * b * W, (k + 1) * b * W, (1,), generator=g))
                if t >= int(pos[j]) or (r, t) not in written:
                    break
            kvrow[j, t] = r
            if t < int(pos[j]):
                used.add((r, t))
    for (r, t) in sorted(used):
        mix = 0.6 * float(torch.rand((), generator=g))
        ctx[r, t] = (mix * shared + torch.randn(D, generator=g)).to(dtype)
    return hid, ctx.contiguous(), kvrow, used


MAXCOS_LMAX = 12
MAXCOS_CASES = {"20cand": (2, 2, 5, (1, 11, 4, 7)), "5cand": (1, 1, 5, (6,))}   # C, b, W, pos


def score_case(C, b, W, nact, E, seed):
    """pval (log-probabilities -12 .. -0.5), maxcos (0.2 .. 0.95), text [C*b*W, E] with cosines
    to the clip's audio between about 0 and 0.6, audio [C, E].  Candidates past the clip's
    nact * W active ones hold NaN everywhere: reading one spoils the clip's scores."""
    g = torch.Generator().manual_seed(seed)
    R = C * b * W
    audio = torch.randn(C, E, generator=g)
    mix = torch.rand(R, 1, generator=g) * 0.75
    clip = torch.arange(R) // (b * W)
    text = mix * audio[clip] + torch.randn(R, E, generator=g)
    pval = -0.5 - 11.5 * torch.rand(R, generator=g)
    mc = 0.2 + 0.75 * torch.rand(R, generator=g)
    idle = (torch.arange(R) % (b * W)) >= nact * W
    text[idle] = float("nan")
    pval[idle] = float("nan")
    mc[idle] = float("nan")
    return pval, mc, text, audio


SCORE_SHAPES = [(1, 15, 1), (3, 25, 1), (3, 25, 3), (8, 64, 8), (2, 2, 2)]     # (b, W, nact)
SCORE_E = (1024, 70)
SCORE_MIX = [(a, be, st) for a in (0.0, 0.1, 1.0) for be in (0.0, 0.2, 1.0) for st in (1.0, 0.7)]
SCORE_TEMP = 0.07

TOPK_CASES = [(50257, 2 * 50257, 1), (50257, 2 * 50257, 25), (50257, 2 * 50257, 64),
              (1000, 1000, 1), (1000, 1000, 25), (1000, 1000, 64),
              (1025, 1025, 1), (1025, 1032, 25), (1025, 1025, 64), (40, 40, 40)]   # (V, ld, k)


def topk_case(V, ld, k):
    """Three random rows (normal * 3) in a [3, ld] buffer whose columns >= V hold +1e9 (a value
    that would win and would swamp the softmax)."""
    g = torch.Generator().manual_seed(V * 7 + k)
    x = torch.full((3, ld), 1e9)
    x[:, :V] = torch.randn(3, V, generator=g) * 3
    return x


def topk_tie_second(V):
    return 5 + 64 * 3 if V > 256 else V // 2


def topk_tie_rows(V):
    """Rows with exact ties, values multiples of 1/8 in [0, 4) below the planted ones:
    0  the maximum 9 at indices 5 and 5 + 64 * 3 (two waves; V // 2 for a short row) and V - 1;
    1  (V > 3072) the maximum at 7 + 2048, 7 + 1024 and 7: three slots of thread 7;
    2  every entry equal;
    3  -inf on every third entry, the finite ones (32 distinct values) full of ties;
    4  (V > 3072) equal runner-ups 8 at 1030, 6 and 2054 below a single 9 at 3000."""
    g = torch.Generator().manual_seed(V)
    x = torch.randint(0, 32, (5, V), generator=g).float() / 8.0
    x[0, 5] = x[0, topk_tie_second(V)] = x[0, V - 1] = 9.0
    if V > 3072:
        x[1, 7] = x[1, 7 + 1024] = x[1, 7 + 2048] = 9.0
        x[4, 3000] = 9.0
        x[4, 1030] = x[4, 6] = x[4, 2054] = 8.0
    x[2] = 1.5
    x[3, ::3] = NEG_INF
    return x
