"""GPU: zs_sample_rows against the float64 sampler of tests/sample_ref.py, on the cases whose
input conditions tests/test_sample_ref.py asserts on the CPU.

Every output is filled with a sentinel and has a guard row behind it (gpu_helpers.Out).  Token
ids and the number of kept tokens must EQUAL the reference on every decisive draw (sample_ref's
definition: each of the draw's comparisons has a gap above 4 x yardstick + 1e-6); the
log-probability and the kept mass are compared on the rows whose token (kept set) is the
reference's, with the rule of test_gpu_magic_kernels.py::_check: |got - float64| <= 4 x
yardstick + 1e-6, yardstick = |the float32 formula - float64| on the case's own data.  Each case
prints error / yardstick / tolerance and its share of indecisive draws."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as S  # noqa: E402
from gpu_helpers import Out, offset  # noqa: E402

pytestmark = pytest.mark.gpu
I32, F32 = torch.int32, torch.float32


def _ops():
    from zsaac import ops
    return ops


class Run:
    """One launch over ``logits`` (a device view [R, V]) with sentinel-filled outputs."""

    def __init__(self, dev, logits, temperature, top_k, top_p, seed=S.SEED, step=S.STEP, row_id=None):
        R = logits.shape[0]
        self.pv, self.pi = Out(dev, (R,), F32, -7.0), Out(dev, (R,), I32, -7)
        self.lp, self.kept = Out(dev, (R,), F32, -7.0), Out(dev, (R, 2), F32, -7.0)
        ctr = torch.tensor([step], dtype=I32, device=dev)
        rid = None if row_id is None else torch.as_tensor(row_id, dtype=I32).to(dev)
        _ops().sample_rows(logits, ctr, seed, self.pv.t, self.pi.t, temperature=temperature,
                           top_k=top_k, top_p=top_p, row_id=rid, logprob=self.lp.t, kept=self.kept.t)
        torch.cuda.synchronize()
        assert int(ctr.item()) == step           # the step word is read, never written
        self.tok, self.val = self.pi.cpu().numpy(), self.pv.cpu().numpy()
        self.logprob, k = self.lp.cpu().numpy(), self.kept.cpu().numpy()
        self.count, self.mass = k[:, 0], k[:, 1]

    def same(self, o):
        return all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in
                   ((self.tok, o.tok), (self.val, o.val), (self.logprob, o.logprob),
                    (self.count, o.count), (self.mass, o.mass)))


def _device_case(dev, name):
    x, V = S.case(name)
    ld = x.shape[1]
    xd = torch.from_numpy(np.array(x)).to(dev)
    if ld % 4:                       # rows that do not all start on 16 bytes
        assert any((xd.data_ptr() + 4 * ld * r) % 16 for r in range(x.shape[0]))
    return xd, x, V


@pytest.mark.parametrize("name", list(S.CASES))
def test_sample_rows_cases(cuda, name):
    """Every (temperature, top_k, top_p) of the case in one test: 36 launches on one upload.
    Measured on an MI355X: every decisive draw equal; indecisive 0 % (v1, v5, v64, v4096, v10000),
    0.08 % (v1000), 1.85 % (v4097), 1.39 % (planted), 5.56 % (v32000), 7.41 % (v50257), 8.33 %
    (v65536); closest to its bound: logprob error
    5.53e-07 at yardstick 5.53e-07 (v32000, tolerance 3.21e-06), kept mass 4.63e-07 at 5.23e-07."""
    xd, x, V = _device_case(cuda, name)
    R = x.shape[0]
    n_draws = n_ind = 0
    worst = dict(lp=(0.0, 0.0), mass=(0.0, 0.0))
    for t, k, p in S.settings(name):
        recs = S.reference(name, t, k, p)
        got = Run(cuda, xd[:, :V], t, k, p)
        assert ((got.tok >= 0) & (got.tok < V)).all()
        assert np.array_equal(got.val, x[np.arange(R), got.tok])
        for r, rec in enumerate(recs):
            n_draws += 1
            if not rec["decisive"]:
                n_ind += 1
                continue
            assert got.tok[r] == rec["tok"], (name, t, k, p, r, got.tok[r], rec["tok"])
            assert got.count[r] == rec["count"], (name, t, k, p, r, got.count[r], rec["count"])
        for key, vals, ref, ref32, okrow in (
                ("lp", got.logprob, "logprob", "logprob32", lambda r, rec: got.tok[r] == rec["tok"]),
                ("mass", got.mass, "mass", "mass32",
                 lambda r, rec: got.count[r] == rec["count"] == rec["count32"])):
            rows = [r for r, rec in enumerate(recs) if okrow(r, rec)]
            if not rows:
                continue
            r64 = np.float64([recs[r][ref] for r in rows])
            yard = float(np.abs(np.float64([recs[r][ref32] for r in rows]) - r64).max())
            err = float(np.abs(vals[rows].astype(np.float64) - r64).max())
            tol = 4 * yard + 1e-6
            assert err <= tol, (name, key, t, k, p, err, yard, tol)
            if err / tol >= worst[key][0] / (4 * worst[key][1] + 1e-6):
                worst[key] = (err, yard)
    for key, (err, yard) in worst.items():
        print(f"sample_rows[{name}] {key}: error {err:.3e}, yardstick {yard:.3e}, "
              f"tolerance {4 * yard + 1e-6:.3e} (closest to its bound)")
    print(f"sample_rows[{name}]: {n_ind} of {n_draws} draws indecisive ({n_ind / n_draws:.2%})")
    assert n_ind * 8 <= n_draws


def test_misaligned_base_reads_the_same(cuda):
    """The planted rows from a buffer one float past a 16-byte boundary (single-float loads)
    give the bits of the aligned float4 path."""
    xd, x, V = _device_case(cuda, "planted")
    xo = offset(torch.from_numpy(np.array(x)), cuda)
    for t, k, p in ((1.0, 0, 0.8), (0.7, 5, 1.0), (2.0, 5, 0.8)):
        assert Run(cuda, xd[:, :V], t, k, p).same(Run(cuda, xo[:, :V], t, k, p))


def test_deterministic_and_slot_independent(cuda):
    """Two runs are bit-identical; a row with the same row_id gives the same outputs in another
    slot of a launch of another size; another step or seed changes the draws."""
    xd, x, V = _device_case(cuda, "v1000")
    R = x.shape[0]
    rid = np.arange(R) + 1000
    a = Run(cuda, xd[:, :V], 1.0, 0, 0.8, row_id=rid)
    assert a.same(Run(cuda, xd[:, :V], 1.0, 0, 0.8, row_id=rid))
    perm = np.random.default_rng(0).permutation(R)[:23]
    sub = xd[torch.from_numpy(perm).to(cuda)].contiguous()
    b = Run(cuda, sub[:, :V], 1.0, 0, 0.8, row_id=rid[perm])
    for name in ("tok", "val", "logprob", "count", "mass"):
        assert np.array_equal(getattr(a, name)[perm].view(np.int32), getattr(b, name).view(np.int32)), name
    # without row_id the id is the slot
    c = Run(cuda, xd[:, :V], 1.0, 0, 0.8)
    assert c.same(Run(cuda, xd[:, :V], 1.0, 0, 0.8, row_id=np.arange(R)))
    ref = [r["tok"] for r in S.reference("v1000", 1.0, 0, 0.8)]
    assert (c.tok == np.int32(ref)).mean() > 0.9        # (the cases test pins every decisive one)
    for other in (Run(cuda, xd[:, :V], 1.0, 0, 0.8, step=S.STEP + 1),
                  Run(cuda, xd[:, :V], 1.0, 0, 0.8, seed=S.SEED + 1),
                  Run(cuda, xd[:, :V], 1.0, 0, 0.8, row_id=rid)):
        assert (other.tok != c.tok).mean() > 0.25
        assert np.array_equal(other.count, c.count)     # the filters do not depend on the draw


def test_feeds_greedy_step(cuda):
    """part_val / part_idx are nblk = 1 argmax partials: zs_greedy_step takes the sampled token,
    stops a row on the stop token and advances the step word, which the next draw then reads."""
    ops = _ops()
    xd, x, V = _device_case(cuda, "v64")
    R, steps = 4, 3
    logits = xd[:1, :V].expand(R, V).contiguous()
    i32 = dict(dtype=I32, device=cuda)
    pos, nxt, done = torch.zeros(R, **i32), torch.zeros(R, **i32), torch.zeros(R, **i32)
    out_ids, out_len = torch.zeros(R, steps, **i32), torch.zeros(R, **i32)
    ctr, all_done = torch.zeros(1, **i32), torch.zeros(3, **i32)
    pv, pi = torch.empty(R, device=cuda), torch.empty(R, **i32)
    want = np.stack([[r["tok"] for r in S.sample_rows(np.tile(x[:1], (R, 1)), V, 1.0, 0, 1.0, 5, s)]
                     for s in range(steps)], 1)
    stop = int(want[0, 0])                       # row 0 stops at once
    for s in range(steps):
        ops.sample_rows(logits, ctr, 5, pv, pi)
        ops.greedy_step(pv, pi, R, 1, ctr, steps, stop, -1, out_ids, out_len, done, pos, nxt, all_done)
    torch.cuda.synchronize()
    assert int(ctr.item()) == steps
    ids, lens = out_ids.cpu().numpy(), out_len.cpu().numpy()
    for r in range(R):
        hits = np.nonzero(want[r] == stop)[0]
        n = int(hits[0]) + 1 if len(hits) else steps
        assert lens[r] == n and ids[r, :n].tolist() == want[r, :n].tolist() and not ids[r, n:].any()
    assert lens[0] == 1


def test_bad_arguments_are_refused(cuda):
    from zsaac._lib import ZsError
    ops = _ops()
    x = torch.zeros(2, 8, device=cuda)
    ctr = torch.zeros(1, dtype=I32, device=cuda)
    pv, pi = Out(cuda, (2,), F32, -7.0), Out(cuda, (2,), I32, -7)

    def call(logits=x, **kw):
        ops.sample_rows(logits, ctr, 0, pv.t, pi.t, **kw)

    for kw, msg in ((dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
                    (dict(top_p=0.0), "top_p"), (dict(top_k=-1), "top_k")):
        with pytest.raises(ZsError, match=msg):
            call(**kw)
    with pytest.raises(ZsError, match="65536"):
        call(torch.zeros(1, 65537, device=cuda))
    with pytest.raises(ZsError):
        call(torch.zeros(2, 8, device=cuda, dtype=torch.bfloat16))
    with pytest.raises(ZsError):
        call(torch.zeros(2, 16, device=cuda)[:, ::2])
    from zsaac import _lib
    # ld < V and a pointer off a 4-byte boundary, straight at the C entry
    args = [x.data_ptr(), 2, 8, 4, None, ctr.data_ptr(), 0, 1.0, 0, 1.0, pv.t.data_ptr(),
            pi.t.data_ptr(), None, None, None]
    assert _lib.lib().zs_sample_rows(*args) == -1 and "ld >= V" in _lib.last_error()
    args[3], args[0] = 8, x.data_ptr() + 2
    assert _lib.lib().zs_sample_rows(*args) == -1 and "aligned" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((pv.cpu() == -7.0).all()) and bool((pi.cpu() == -7).all())   # nothing was launched
