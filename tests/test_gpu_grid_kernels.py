"""The grid decode's phases (csrc/decode_grid.hip) against the float64 references of
tests/grid_ref.py, one phase launch at a time.

The phase launches run the same device code as the persistent kernel and hand every phase's
output on through memory; ops.gpt2_decode_phase_window narrows a call to chosen launches of a
step's 62, so each phase runs alone on inputs this file wrote -- KV history, pos, next_tok, done and
the workspace regions, sentinels everywhere else -- and its output is compared with the reference
of the same bytes under the project's one rule (4 x the float32 formula's own deviation + 1e-6, a
bf16 output adds 2^-8 |ref|; row by row, grid_ref.row_tolerance).  No pipeline, no goldens, no
prefill.  tests/test_grid_ref.py shows on the CPU that these inputs tell every mutant of
grid_ref.MUTANTS from the reference by more than twice that tolerance.

Then, with 12 distinct blocks packed by Gpt2Weights itself: the 62 launches issued one window at
a time leave the same bytes as one whole-step call; one step of the persistent launch leaves the
same VALUES (K / V, q, att, xb, hid), not only ids, as the phase launches; and one whole step
agrees with the float64 step of the UNFOLDED f32 master weights within 4 x the deviation that
bf16 tables and hand-offs cost that reference.  The f32 parity kernels run the same harness.

ZSAAC_GRID_ERRORS=<file>: every comparison's yardstick, tolerance and worst error are written
there when the module ends (profiles/grid_phase_errors.txt is such a run).
"""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grid_ref as G  # noqa: E402
from grid_ref import BF16, F32, F64, I32, SENT  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("bf16", "f32")
MODE_GRIDS = [(m, g) for m in MODES for g in G.GRIDS[m]]
_RECORDS = []


def _ops():
    from zsaac import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("ZSAAC_GRID_ERRORS")
    if path and _RECORDS:
        with open(path, "w") as f:
            f.write("# what, mode, grid: yardstick (float32 formula vs float64), largest tolerance, "
                    "kernel's worst error, worst error / tolerance\n")
            for r in _RECORDS:
                f.write("%-44s %-4s G%-3d yard %.3e tol %.3e err %.3e ratio %.3f\n" % r)


def _check(what, mode, grid, got, ref, tol, yard):
    """|got - ref| <= tol elementwise; the figures go to the report and into the message."""
    err = (got.double() - ref).abs()
    ratio = float((err / tol).max()) if err.numel() else 0.0
    assert bool(torch.isfinite(got.double()).all()), what
    _RECORDS.append((what, mode, grid, yard, float(tol.max()), float(err.max()), ratio))
    print("%s %s G%d: yard %.3e tol %.3e err %.3e ratio %.3f" % (what, mode, grid, yard,
                                                                 float(tol.max()), float(err.max()), ratio))
    assert ratio <= 1.0, (what, mode, grid, yard, float(err.max()), ratio)


# ------------------------------------------------------------------ device buffers of one call
@pytest.fixture(scope="module")
def tables(cuda):
    """One block's packed tables per mode on the device (all 12 block slots point at them), and
    stand-in embedding / head tables of the right sizes for the phases that do not read them."""
    out = {}
    for mode in MODES:
        t = G.layer_tables(mode)
        st = G._st(mode)
        bias = (lambda f: torch.stack([f["b"], f["cs"]])) if mode == "bf16" else (lambda f: f["b"])
        dev = [G.frag_pack(t["attn"]["w"]), bias(t["attn"]), G.frag_pack(t["proj_w"]), t["proj_b"],
               G.frag_pack(t["fc"]["w"]), bias(t["fc"]), G.frag_pack(t["mproj_w"]), t["mproj_b"]]
        dev = [x.contiguous().to(cuda) for x in dev]
        Vp = 16 * (-(-G.V_SMALL // 16))
        out[mode] = dict(layer=dev, ptrs=(ctypes.c_void_p * 96)(*[x.data_ptr() for x in dev] * 12),
                         wte=torch.zeros(G.V_SMALL, 768, dtype=st, device=cuda),
                         wpe=torch.zeros(1024, 768, dtype=st, device=cuda),
                         head=torch.zeros(Vp * 768, dtype=st, device=cuda),
                         lmb=torch.zeros(2 * Vp, dtype=F32, device=cuda))
    return out


class Rig:
    """The arguments of one grid-decode call: state, KV caches and a workspace whose hand-off
    regions hold the sentinel, with typed views of the regions (the layout mirrored in
    grid_ref.ws_layout)."""

    def __init__(self, dev, mode, R, Lmax, V, tabs, pos, tok, kc, vc, max_steps=4, step=0,
                 temperature=1.0, stop=(-1, -2), layer_ptrs=None, state=None):
        ops = _ops()
        self.dev, self.mode, self.R, self.Lmax, self.V = dev, mode, R, Lmax, V
        self.st = G._st(mode)
        self.lay = G.ws_layout(mode)
        from zsaac._lib import call
        n = call("zs_decode_persist_workspace_bytes" if mode == "bf16" else "zs_decode_persist_f32_workspace_bytes")
        assert n == self.lay["BYTES"]
        self.buf = (ops.decode_persist_workspace if mode == "bf16" else ops.decode_persist_f32_workspace)(dev)
        off = (-self.buf.data_ptr()) % 256
        self.ws = self.buf[off:off + n]
        for name in ("Q", "ATT", "XB", "HID") + (("X",) if mode == "bf16" else ()):
            self.region(name).fill_(SENT)
        i32 = lambda t: t.to(I32).contiguous().to(dev)
        s = state or {}
        self.pos, self.tok = i32(pos), i32(tok)
        self.done = i32(s.get("done", torch.zeros(R)))
        self.out_ids = i32(s.get("out_ids", torch.full((R, max_steps), -7)))
        self.out_len = i32(s.get("out_len", torch.zeros(R)))
        self.step_ctr = i32(torch.tensor([step]))
        self.all_done = torch.zeros(4, dtype=I32, device=dev)
        self.max_steps, self.temperature, self.stop = max_steps, temperature, stop
        self.wte, self.wpe, self.head, self.lmb = tabs["wte"], tabs["wpe"], tabs["head"], tabs["lmb"]
        self.layer_ptrs = layer_ptrs if layer_ptrs is not None else tabs["ptrs"]
        # isolated phases: every block's cache pointer is the one pair; whole steps: 12 pairs
        self.kc = [t.contiguous().to(dev) for t in (kc if isinstance(kc, list) else [kc])]
        self.vc = [t.contiguous().to(dev) for t in (vc if isinstance(vc, list) else [vc])]
        k12 = self.kc if len(self.kc) == 12 else self.kc * 12
        v12 = self.vc if len(self.vc) == 12 else self.vc * 12
        self.kv_ptrs = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in k12 + v12])

    def region(self, name):
        e = 4 if (self.mode == "f32" or name == "X") else 2
        n = 64 * (3072 if name == "HID" else 768) * e
        return self.ws[self.lay[name]:self.lay[name] + n].view(F32 if e == 4 else BF16)

    def put_rows(self, name, x):          # row-major regions: Q, X
        self.region(name).view(64, 768)[:x.shape[0]] = x.to(self.dev)

    def put_frag(self, name, x):          # fragment-order regions: ATT, XB, HID
        self.region(name).copy_(G.frag_pack(x, nrows=64, fill=SENT).to(self.dev))

    def rows(self, name):
        return self.region(name).cpu().view(64, 768)

    def frag(self, name):
        return G.frag_unpack(self.region(name).cpu(), 64, 3072 if name == "HID" else 768)

    def keys(self):
        return self.ws[G.WS_KEY:G.WS_KEY + 2 * 64 * 8].view(torch.int64).cpu()

    def args(self):
        return (self.R, self.Lmax, self.max_steps, self.stop[0], self.stop[1], self.V, self.wte, self.wpe,
                self.head, self.temperature, self.layer_ptrs, self.lmb, self.kv_ptrs, self.pos, self.tok,
                self.done, self.out_ids, self.out_len, self.step_ctr, self.all_done, self.buf)

    def run(self, first, last, grid):
        _ops().gpt2_decode_phase_window(*self.args(), first=first, last=last, grid=grid,
                                        f32=self.mode == "f32")
        torch.cuda.synchronize()

    def step(self, grid):
        ops = _ops()
        (ops.gpt2_decode_phases_f32 if self.mode == "f32" else ops.gpt2_decode_phases)(
            *self.args(), steps=1, grid=grid)
        torch.cuda.synchronize()

    def state(self):
        return {k: getattr(self, k).cpu() for k in ("pos", "tok", "done", "out_ids", "out_len", "step_ctr",
                                                    "all_done")}

    def snapshot(self):
        """Every byte a launch may write: the workspace past the sync page, caches, state."""
        d = dict(ws=self.ws[G.WS_SYNC_BYTES:].cpu(), **self.state())
        for i, (k, v) in enumerate(zip(self.kc, self.vc)):
            d["kc%d" % i], d["vc%d" % i] = k.cpu(), v.cpu()
        return d


def _same(a, b, but=()):
    for k in a:
        if k not in but:
            x, y = a[k], b[k]
            if x.dtype in (BF16, F32):
                x, y = x.view(torch.int16 if x.dtype == BF16 else torch.int32), y.view(torch.int16 if y.dtype == BF16 else torch.int32)
            assert torch.equal(x, y), k


def _untouched(rig, before, after, wrote):
    """Nothing but the regions / caches named in ``wrote`` changed, and of those only rows < R:
    rows >= R of every output region still hold the sentinel."""
    lay, base = rig.lay, G.WS_SYNC_BYTES
    wa, wb = after["ws"].clone(), before["ws"].clone()
    for name in wrote:
        if name in lay:
            e = 4 if (rig.mode == "f32" or name == "X") else 2
            n = 64 * (3072 if name == "HID" else 768) * e
            wa[lay[name] - base:lay[name] - base + n] = 0
            wb[lay[name] - base:lay[name] - base + n] = 0
            reg = rig.rows(name) if name in ("Q", "X") else rig.frag(name)
            assert bool((reg[rig.R:] == SENT).all()), name + ": rows >= R written"
    assert torch.equal(wa, wb), "workspace written outside " + str(wrote)
    caches = [k for k in before if k[:2] in ("kc", "vc")] if "kv" in wrote else []
    _same(before, after, but=["ws"] + caches)


def _rig(cuda, tables, c, **kw):
    R = c["R"]
    tabs = dict(tables[c["mode"]])
    for k in ("wte", "wpe"):
        if k in c:
            tabs[k] = c[k].to(cuda)
    pos = c.get("pos", torch.ones(R, dtype=I32))
    tok = c.get("tok", torch.arange(R, dtype=I32))
    st = G._st(c["mode"])
    Lmax = c.get("Lmax", 40)
    kc = c["kc"] if "kc" in c else G._cache(R + 1, Lmax, st)
    vc = c["vc"] if "vc" in c else G._cache(R + 1, Lmax, st)
    return Rig(cuda, c["mode"], R, Lmax, c.get("V", G.V_SMALL), tabs, pos, tok, kc, vc, **kw)


# ------------------------------------------------------------------ the launch window itself
def test_window_is_checked_by_the_entry_points(cuda, tables):
    from zsaac._lib import ZsError, call
    ops = _ops()
    c = G.case_d("bf16", 1)
    for mode in MODES:
        rig = _rig(cuda, tables, dict(c, mode=mode))
        run = ops.gpt2_decode_phases_f32 if mode == "f32" else ops.gpt2_decode_phases
        before = rig.snapshot()
        try:
            call("zs_tune_set", b"dg_win_lo", 7)
            call("zs_tune_set", b"dg_win_hi", 7)
            with pytest.raises(ZsError, match=r"window \[7, 7\) is empty"):
                run(*rig.args(), steps=1, grid=192)
            call("zs_tune_set", b"dg_win_hi", 9)
            with pytest.raises(ZsError, match=r"narrowed launch window \[7, 9\) runs one step"):
                run(*rig.args(), steps=2, grid=192)
        finally:
            call("zs_tune_set", b"dg_win_lo", 0)
            call("zs_tune_set", b"dg_win_hi", 62)
        torch.cuda.synchronize()
        _same(before, rig.snapshot())


# ------------------------------------------------------------------ isolated phases
@pytest.mark.parametrize("R", G.RS)
@pytest.mark.parametrize("layer", [0, G.LAYER])
@pytest.mark.parametrize("mode,grid", MODE_GRIDS)
def test_phase_a(cuda, tables, mode, grid, layer, R):
    """ln_1 + c_attn: q and the K / V slot at pos[row] of every head against float64; every other
    slot, the spare cache row and rows >= R keep their sentinels."""
    c = G.case_a(mode, layer, R)
    rig = _rig(cuda, tables, c)
    if layer:
        rig.put_frag("XB", c["x"])
    before = rig.snapshot()
    rig.run(G.launch(layer, "A"), G.launch(layer, "A") + 1, grid)
    after = rig.snapshot()
    _untouched(rig, before, after, ("Q", "kv"))
    (q, kc, vc), (yq, ykc, yvc) = c["ref"], c["yard"]
    ar, p = torch.arange(R), c["pos"].long()
    bf = mode == "bf16"
    what = "A layer %d R %d " % (layer, R)
    yard, tol = G.row_tolerance(q, yq, bf)
    _check(what + "q", mode, grid, rig.rows("Q")[:R], q, tol, yard)
    for name, got, ref, yd in (("k", after["kc0"], kc, ykc), ("v", after["vc0"], vc, yvc)):
        yard, tol = G.row_tolerance(ref[ar, :, p], yd[ar, :, p], bf)
        _check(what + name, mode, grid, got[ar, :, p], ref[ar, :, p], tol, yard)
        left = got.clone()
        left[ar, :, p] = SENT
        assert bool((left == SENT).all()), name + ": a slot other than pos written"


@pytest.mark.parametrize("R", G.RS)
@pytest.mark.parametrize("mode,grid", MODE_GRIDS)
def test_phase_d(cuda, tables, mode, grid, R):
    """ln_2 + c_fc + gelu_new -> hid (fragment order), pre-activations from below -10 to above 10."""
    c = G.case_d(mode, R)
    rig = _rig(cuda, tables, c)
    rig.put_frag("XB", c["x"])
    before = rig.snapshot()
    rig.run(G.launch(G.LAYER, "D"), G.launch(G.LAYER, "D") + 1, grid)
    _untouched(rig, before, rig.snapshot(), ("HID",))
    yard, tol = G.row_tolerance(c["ref"], c["yard"], mode == "bf16")
    _check("D R %d hid" % R, mode, grid, rig.frag("HID")[:R], c["ref"], tol, yard)


@pytest.mark.parametrize("mode,grid", MODE_GRIDS)
def test_phase_b(cuda, tables, mode, grid):
    """Attention of 19 rows x 12 heads at pos 1 .. 99 across the 32-key chunk edges."""
    c = G.case_b(mode)
    rig = _rig(cuda, tables, c)
    rig.put_rows("Q", c["q"])
    before = rig.snapshot()
    rig.run(G.launch(G.LAYER, "B"), G.launch(G.LAYER, "B") + 1, grid)
    _untouched(rig, before, rig.snapshot(), ("ATT",))
    yard, tol = G.row_tolerance(c["ref"], c["yard"], mode == "bf16")
    _check("B att", mode, grid, rig.frag("ATT")[:c["R"]], c["ref"], tol, yard)


@pytest.mark.parametrize("R", G.RS)
@pytest.mark.parametrize("which,layer", [("C", 0), ("C", G.LAYER), ("E", G.LAYER)])
@pytest.mark.parametrize("mode,grid", MODE_GRIDS)
def test_phase_c_e(cuda, tables, mode, grid, which, layer, R):
    """Projection + residual: the f32 stream against float64 (plain tolerance), and its bf16 copy
    xb = bf16(x) bit for bit (round to nearest even).  f32 mode: the stream lives in xb itself."""
    c = G.case_ce(mode, which, layer, R)
    rig = _rig(cuda, tables, c)
    rig.put_frag("ATT" if which == "C" else "HID", c["a"])
    if not (which == "C" and layer == 0):
        if mode == "bf16":
            rig.put_rows("X", c["x_old"])
        else:
            rig.put_frag("XB", c["x_old"])
    before = rig.snapshot()
    rig.run(G.launch(layer, which), G.launch(layer, which) + 1, grid)
    _untouched(rig, before, rig.snapshot(), ("X", "XB") if mode == "bf16" else ("XB",))
    yard, tol = G.row_tolerance(c["ref"], c["yard"])
    x = rig.rows("X")[:R] if mode == "bf16" else rig.frag("XB")[:R]
    _check("%s layer %d R %d x" % (which, layer, R), mode, grid, x, c["ref"], tol, yard)
    if mode == "bf16":
        assert torch.equal(rig.frag("XB")[:R].view(torch.int16), G.xb_of(x).view(torch.int16))


def _put_head(rig, c):
    rig.head = G.frag_pack(c["w"]).to(rig.dev)
    rig.lmb = (torch.stack([c["b"], c["cs"]]) if c["mode"] == "bf16" else c["b"]).contiguous().to(rig.dev)
    rig.put_frag("XB", c["x"])


@pytest.mark.parametrize("variant", list(G.F_VARIANTS))
@pytest.mark.parametrize("mode,grid", MODE_GRIDS)
def test_phase_f(cuda, tables, mode, grid, variant):
    """ln_f + LM head + argmax at V = 9217: the key's id is the lowest id within tolerance of the
    reference maximum (planted exact ties: the lowest of the pair), its value the reference logit
    of that id within tolerance."""
    c = G.case_f(mode, variant)
    rig = _rig(cuda, tables, c, temperature=c["temperature"])
    _put_head(rig, c)
    before = rig.snapshot()
    rig.run(60, 61, grid)
    _untouched(rig, before, rig.snapshot(), ())
    val, ids = G.key_decode(rig.keys()[:c["R"]])
    assert bool((rig.keys()[64:] == 0).all())
    lg = c["ref"][0]
    yard, tol = G.f_tolerance(c)
    for r, (cand, strict) in enumerate(G.f_candidates(c)):
        assert int(ids[r]) == cand[0] if strict else int(ids[r]) in cand, (r, int(ids[r]), cand)
    ar = torch.arange(c["R"])
    _check("F %s key value" % variant, mode, grid, val, lg[ar, ids], torch.full((c["R"],), tol, dtype=F64), yard)


@pytest.mark.parametrize("name", list(G.BOOK_CASES))
@pytest.mark.parametrize("mode,grid", MODE_GRIDS)
def test_bookkeeping(cuda, tables, mode, grid, name):
    """Window [60, 62): F, then the bookkeeping kernel on F's keys -- rows already done, rows
    stopping on stop0 / stop1, the last step -- against glue_ref.greedy_step."""
    c, b = G.case_f(mode, "t1"), G.book_case(name)
    s = b["state"]
    assert all(strict for _, strict in G.f_candidates(c))
    rig = _rig(cuda, tables, dict(c, pos=s["pos"], tok=s["next_tok"]), max_steps=b["max_steps"],
               step=int(s["step_ctr"][0]), stop=(b["stop0"], b["stop1"]), state=s)
    _put_head(rig, c)
    rig.run(60, 62, grid)
    want = G.book(s, c["ref"][1], c["ref"][2], b["max_steps"], b["stop0"], b["stop1"])
    got = rig.state()
    for k, gk in (("pos", "pos"), ("next_tok", "tok"), ("done", "done"), ("out_ids", "out_ids"),
                  ("out_len", "out_len"), ("step_ctr", "step_ctr")):
        assert torch.equal(got[gk], want[k]), k
    assert got["all_done"].tolist() == want["all_done"].tolist() + [0]
    assert bool((rig.keys()[:64] == 0).all())           # zeroed for the next step


# ------------------------------------------------------------------ whole steps, 12 distinct blocks
def _sd():
    from zsaac import synthetic as S
    return S.gpt2_state_dict(seed=0, std=0.1, emb_std=0.1)


@pytest.fixture(scope="module")
def models(cuda):
    """Gpt2Weights of 12 distinct blocks packed by the project itself: bf16 at V = 50257 and
    9217, f32 at 9217, with the state dict they came from."""
    from zsaac.decoder import Gpt2Weights
    sd = _sd()
    small = dict(sd)
    small["gpt.transformer.wte.weight"] = sd["gpt.transformer.wte.weight"][:G.V_SMALL].contiguous()
    out = dict(sd=small)
    for key, s, dt in (("bf16", small, BF16), ("bf16_full", sd, BF16), ("f32", small, F32)):
        w = Gpt2Weights(s, cuda, dt)
        ptrs = w.packed_layer_ptrs()
        out[key] = dict(w=w, ptrs=ptrs, wte=w.wte, wpe=w.wpe, head=w.wte_packed(), lmb=w.lm_bias())
    return out


def _whole(cuda, models, key, R, Lmax=40, seed=0, max_steps=4, step=0):
    mode = "f32" if key == "f32" else "bf16"
    m = models[key]
    g = G._gen("whole", key, R, seed)
    st = G._st(mode)
    pos = G._positions(R, Lmax, g, (1, Lmax - 1, 17))
    tok = torch.randint(0, m["w"].V, (R,), generator=g, dtype=I32)
    kc, vc = [], []
    for _ in range(12):
        k, v = G._cache(R + 1, Lmax, st), G._cache(R + 1, Lmax, st)
        for r in range(R):
            p = int(pos[r])
            k[r, :, :p] = torch.randn(12, p, 64, generator=g).to(st)
            v[r, :, :p] = torch.randn(12, p, 64, generator=g).to(st)
        kc.append(k)
        vc.append(v)
    mk = lambda: Rig(cuda, mode, R, Lmax, m["w"].V, m, pos, tok, kc, vc, max_steps=max_steps, step=step,
                     layer_ptrs=m["ptrs"], stop=(13, 764))
    return mk, dict(pos=pos, tok=tok, kc=kc, vc=vc)


@pytest.mark.parametrize("mode,grid", MODE_GRIDS)
def test_walk_equals_step(cuda, models, mode, grid):
    """60 windows of one launch and the window [60, 62) (F's keys do not survive the next call's
    zeroing of the sync page) leave the caches, the workspace and the state byte-equal to one
    whole-step call from the same start: R = 21, ragged pos, 12 distinct blocks."""
    mk, start = _whole(cuda, models, mode, 21)
    a, b = mk(), mk()
    _same(a.snapshot(), b.snapshot())
    for i in range(60):
        a.run(i, i + 1, grid)
    a.run(60, 62, grid)
    b.step(grid)
    sa, sb = a.snapshot(), b.snapshot()
    _same(sa, sb)
    assert bool((sa["out_len"] == 1).all()) and int(sa["step_ctr"][0]) == 1
    assert torch.equal(sa["pos"], start["pos"] + 1)


@pytest.mark.parametrize("key", ["bf16_full", "bf16"])
@pytest.mark.parametrize("grid", G.GRIDS["bf16"])
def test_persistent_step_equals_phase_step_in_values(cuda, models, key, grid):
    """One step of the persistent launch (max_steps = step_ctr + 1) against the phase launches
    from the same state, R = 64: every block's K / V slot at pos, q / att / xb / hid of block 11
    and the integer state byte-equal.  V = 50257: phase F's claimed chunks run at all three grids
    (G FSL 3 <= nvb - G); V = 9217: every block static.  WS_X belongs to the phase launches."""
    from zsaac._lib import call
    ops = _ops()
    V = models[key]["w"].V
    nvb = -(-V // 16)
    assert (grid * 4 * 3 <= nvb - grid) == (key == "bf16_full")
    mk, _ = _whole(cuda, models, key, 64, max_steps=3, step=2)
    a, b = mk(), mk()
    ops.gpt2_decode_persist(*a.args(), grid=grid)
    torch.cuda.synchronize()
    out = ctypes.c_int(-1)
    call("zs_decode_persist_status", ctypes.c_void_p(a.ws.data_ptr()), ctypes.byref(out))
    assert out.value == 0 and int(a.all_done[1]) == 0, "the persistent launch gave up"
    b.step(grid)
    sa, sb = a.snapshot(), b.snapshot()
    x0 = a.lay["X"] - G.WS_SYNC_BYTES
    assert torch.equal(sa["ws"][:x0], sb["ws"][:x0])
    assert bool((a.rows("X") == SENT).all())
    _same(sa, sb, but=("ws",))
    assert int(sa["step_ctr"][0]) == 3 and int(sa["all_done"][0]) == 1


def _cpu_models(models):
    """(the float64 model of the unfolded f32 masters, the model of the bf16 tables as
    Gpt2Weights packed them -- unpacked by grid_ref -- with no LayerNorm affine left)."""
    sd, w = models["sd"], models["bf16"]["w"]
    p = "gpt.transformer."
    V = w.V
    ln = lambda k: (sd[k + ".weight"].double(), sd[k + ".bias"].double())
    ref = dict(wte=sd[p + "wte.weight"].double(), wpe=sd[p + "wpe.weight"].double(), V=V, layers=[],
               lnf=ln(p + "ln_f"), head_w=sd[p + "wte.weight"].double(), head_b=torch.zeros(V, dtype=F64))
    tab = dict(wte=w.wte.cpu(), wpe=w.wpe.cpu(), V=V, layers=[], lnf=None,
               head_w=G.frag_unpack(w.wte_packed().cpu(), 16 * (-(-V // 16)), 768),
               head_b=w.lm_bias()[0].cpu())
    for i, pk in enumerate(w._packed):
        h = p + "h.%d." % i
        t = lambda k: sd[h + k].t().double()
        ref["layers"].append(dict(
            ln1=ln(h + "ln_1"), attn_w=t("attn.c_attn.weight"), attn_b=sd[h + "attn.c_attn.bias"].double(),
            proj_w=t("attn.c_proj.weight"), proj_b=sd[h + "attn.c_proj.bias"].double(),
            ln2=ln(h + "ln_2"), fc_w=t("mlp.c_fc.weight"), fc_b=sd[h + "mlp.c_fc.bias"].double(),
            mproj_w=t("mlp.c_proj.weight"), mproj_b=sd[h + "mlp.c_proj.bias"].double()))
        u = lambda k, n, kk: G.frag_unpack(pk[k].cpu(), n, kk)
        tab["layers"].append(dict(
            ln1=None, attn_w=u("attn_w", 2304, 768), attn_b=pk["attn_b"][0].cpu(),
            proj_w=u("proj_w", 768, 768), proj_b=pk["proj_b"].cpu(),
            ln2=None, fc_w=u("fc_w", 3072, 768), fc_b=pk["fc_b"][0].cpu(),
            mproj_w=u("mproj_w", 768, 3072), mproj_b=pk["mproj_b"].cpu()))
    return ref, tab


@pytest.fixture(scope="module")
def unfolded(cuda, models):
    mk, s = _whole(cuda, models, "bf16", 21, seed=1)
    ref_m, tab_m = _cpu_models(models)
    ref = G.step(ref_m, s["tok"], s["pos"], s["kc"], s["vc"])
    yard = G.step(tab_m, s["tok"], s["pos"], s["kc"], s["vc"], handoff=BF16)
    return mk, s, ref, yard


@pytest.mark.parametrize("grid", G.GRIDS["bf16"])
def test_whole_step_against_the_unfolded_model(cuda, unfolded, grid):
    """One step of the phase launches on tables folded and packed by Gpt2Weights against the
    float64 step of the UNFOLDED f32 masters (LayerNorm affines g != 1, beta != 0; no bf16
    anywhere).  The bound is measured: 4 x the deviation of the float64 step with bf16 tables and
    bf16 rounding at the kernel's hand-off points from that reference, per tensor.  The chosen id's
    reference logit lies within that bound, carried through the head, of the reference maximum."""
    mk, s, ref, yard = unfolded
    rig = mk()
    rig.step(grid)
    R, ar, p = 21, torch.arange(21), s["pos"].long()
    for name, got, r64, y in (("x", rig.rows("X")[:R], ref["x"], yard["x"]),
                              ("k11", rig.kc[11].cpu()[ar, :, p], ref["k"][11], yard["k"][11]),
                              ("v11", rig.vc[11].cpu()[ar, :, p], ref["v"][11], yard["v"][11])):
        yd = float((y - r64).abs().max())
        assert yd > 0
        _check("step vs unfolded " + name, "bf16", grid, got, r64, torch.full_like(r64, 4 * yd), yd)
    tol = 4 * float((yard["logits"] - ref["logits"]).abs().max())
    ids = rig.out_ids.cpu()[:, 0].long()
    gap = ref["best"] - ref["logits"][ar, ids]
    _RECORDS.append(("step vs unfolded logit gap of the id", "bf16", grid, tol / 4, tol, float(gap.max()),
                     float(gap.max()) / tol))
    assert bool((gap <= tol).all()), (gap.max(), tol)
    assert torch.equal(rig.tok.cpu().long(), ids) and bool((rig.pos.cpu() == s["pos"] + 1).all())
