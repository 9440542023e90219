"""oniris_sampler_step / oniris_sampler_mse_finish (csrc/elementwise.hip) against tests/sampler_probe_oracle.py (reviewed by
tests/test_sampler_probe_oracle.py): the sampler's update with the churn of the following step and the MSE probe in the launch.
The C-ABI entry points are called directly on NaN-filled buffers with 64 guard elements behind them.

  x_out, x_hat, d_io, sigma_buf      bit for bit (the reference's float32 tensor expressions)
  the two means                      2^-17 mag against float64 (the project's bound for an fp32 reduction; mag = the mean itself)
  workspace rows of other steps, and the whole workspace without a target: still NaN
  two runs: the same bits

Sizes: n = 1000 (a ragged fourth block, fewer blocks than a wave) and n = 70 001 (274 blocks: more than the finish kernel's 256
threads, the last one holding a single element).  Inputs at the magnitudes of fixture G9b's first step.
Every figure is printed as `PROBE <case> <tensor> <worst error / bound>` (pytest -s); profiles/sampler_churn_target_tests.txt."""
import functools

import pytest
import torch

import oracle_hold as OH
import sampler_probe_oracle as PO
import step_edge_cases as SC
from test_step_edge_gpu import Buf, _api, _g, _ptr

pytestmark = pytest.mark.gpu
F32 = torch.float32
COEF, T_A, DT, S_NEXT = 33.125, 37.25, -16.125, 21.125
STEPS, STEP = 3, 1
hold_f32 = functools.partial(OH.hold_f32, tag="PROBE")
hold_exact = functools.partial(OH.hold_exact, tag="PROBE")

_inputs_cache = {}


def _inputs(n):
    if n not in _inputs_cache:
        g = SC.gen(4300 + n)
        _inputs_cache[n] = dict(x_hat=SC.rn(g, n, scale=40.0), x_pred=SC.rn(g, n), d_in=SC.rn(g, n), x_aux=SC.rn(g, n, scale=30.0),
                                noise=SC.rn(g, n), target=SC.rn(g, n, scale=0.5))
    return _inputs_cache[n]


def _run(n, mode, with_noise, with_target, aliased, nsig):
    """One launch + the finish on fresh buffers.  Returns the buffers."""
    ops, lib, check = _api()
    v = _inputs(n)
    blocks = lib.oniris_sampler_ws_blocks(n)
    xh = Buf(n, dtype=F32, init=v["x_hat"])
    d_io = Buf(n, dtype=F32, init=v["d_in"]) if mode != 2 else None
    xo = xh if aliased else Buf(n, dtype=F32)
    sig = Buf(max(nsig, 1), dtype=F32)
    ws, mse = Buf(STEPS, 2, blocks, dtype=F32), Buf(STEPS, 2, dtype=F32)
    xp = _g(v["x_pred"]) if (mode != 2 or with_target) else None
    xa = _g(v["x_aux"]) if mode == 1 else None
    nz = _g(v["noise"]) if with_noise else None
    tg = _g(v["target"]) if with_target else None
    check(lib.oniris_sampler_step(mode, _ptr(ops, xh), ops._p(xp), _ptr(ops, d_io) if d_io else None, ops._p(xa), _ptr(ops, xo), n,
                                  T_A, DT, _ptr(ops, sig) if nsig else None, nsig, S_NEXT, ops._p(nz), COEF, ops._p(tg),
                                  _ptr(ops, ws), STEP, ops._stream()), "sampler_step")
    if with_target:
        check(lib.oniris_sampler_mse_finish(_ptr(ops, ws), STEPS, n, _ptr(ops, mse), ops._stream()), "sampler_mse_finish")
    torch.cuda.synchronize()
    return dict(xh=xh, d_io=d_io, xo=xo, sig=sig, ws=ws, mse=mse, blocks=blocks)


@pytest.mark.parametrize("nsig", [0, 7])
@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [1000, 70001])
def test_sampler_step(n, mode, with_noise, with_target, aliased, nsig):
    v = _inputs(n)
    want = PO.launch(mode, v["x_hat"], v["x_pred"], v["d_in"], v["x_aux"], T_A, DT, v["noise"] if with_noise else None, COEF,
                     v["target"] if with_target else None)
    name = f"sampler_step(n={n},mode={mode},noise={int(with_noise)},target={int(with_target)},aliased={int(aliased)},nsig={nsig})"
    r = _run(n, mode, with_noise, with_target, aliased, nsig)
    assert r["blocks"] == min(-(-n // 256), 1024)
    hold_exact(name, "x_hat", r["xh"].t, want["x_store"] if aliased else want["x_hat"])
    if not aliased:
        if mode == 2 and not with_noise:
            hold_exact(name, "x_out", r["xo"].t, v["x_hat"])           # the plain copy
        else:
            hold_exact(name, "x_out", r["xo"].t, want["x_store"])
    if mode != 2:
        hold_exact(name, "d_io", r["d_io"].t, want["d_io"])
    if nsig:
        hold_exact(name, "sigma_buf", r["sig"].t, torch.full((nsig,), S_NEXT))
    else:
        assert bool(torch.isnan(r["sig"].t).all())
    ws = r["ws"].t
    if with_target:
        assert bool(torch.isnan(ws[0]).all()) and bool(torch.isnan(ws[2]).all()), f"{name}: a workspace row of another step was written"
        assert bool(torch.isfinite(ws[STEP]).all())
        hold_f32(name, "mse_pred", r["mse"].t[STEP, 0:1], want["mse_pred"])
        hold_f32(name, "mse", r["mse"].t[STEP, 1:2], want["mse"])
        again = _run(n, mode, with_noise, with_target, aliased, nsig)
        assert torch.equal(again["ws"].t[STEP], ws[STEP]) and torch.equal(again["mse"].t[STEP], r["mse"].t[STEP]), f"{name}: two runs differ"
        assert torch.equal(again["xo"].t, r["xo"].t)
    else:
        assert bool(torch.isnan(ws).all()), f"{name}: the workspace was written without a target"
    for b_, n_ in ((r["xh"], "x_hat"), (r["d_io"], "d_io"), (r["xo"], "x_out"), (r["sig"], "sigma_buf"), (r["ws"], "mse_ws"), (r["mse"], "mse")):
        if b_ is not None:
            b_.guards_ok(name, n_)


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("n", [1000, 70001])
def test_whole_step(n, last):
    """A step as the frame loop launches it: oniris_sampler_update (Euler, into the graph input) then oniris_sampler_step (Heun, with
    target and the following step's churn, x_aux = x_out = the graph input); the last step: one Euler launch with x_out = x_hat.
    mse_pred comes from the step's LAST prediction, mse from x_next before the injection."""
    ops, lib, check = _api()
    v = _inputs(n)
    t_hat, t_next = T_A, 21.125
    dt = float(torch.tensor(t_next, dtype=F32) - torch.tensor(t_hat, dtype=F32))
    x_pred2 = SC.rn(SC.gen(4400 + n), n)
    want = PO.step(v["x_hat"], v["x_pred"], None if last else x_pred2, t_hat, t_next, None if last else v["noise"], COEF, v["target"])
    name = f"whole_step(n={n},last={int(last)})"
    blocks = lib.oniris_sampler_ws_blocks(n)
    xh, d_io, gx, gt = Buf(n, dtype=F32, init=v["x_hat"]), Buf(n, dtype=F32), Buf(n, dtype=F32), Buf(5, dtype=F32)
    ws, mse = Buf(1, 2, blocks, dtype=F32), Buf(1, 2, dtype=F32)
    xp, xp2, nz, tg = _g(v["x_pred"]), _g(x_pred2), _g(v["noise"]), _g(v["target"])
    if last:
        check(lib.oniris_sampler_step(0, _ptr(ops, xh), ops._p(xp), _ptr(ops, d_io), None, _ptr(ops, xh), n, t_hat, dt, None, 0, 0.0,
                                      None, 0.0, ops._p(tg), _ptr(ops, ws), 0, ops._stream()), "sampler_step")
    else:
        check(lib.oniris_sampler_update(0, _ptr(ops, xh), ops._p(xp), _ptr(ops, d_io), None, _ptr(ops, gx), n, t_hat, dt, _ptr(ops, gt), 5,
                                        t_next, ops._stream()), "sampler_update")
        torch.cuda.synchronize()
        hold_exact(name, "graph input (Euler)", gx.t, want["x_euler"])
        check(lib.oniris_sampler_step(1, _ptr(ops, xh), ops._p(xp2), _ptr(ops, d_io), _ptr(ops, gx), _ptr(ops, gx), n, t_next, dt,
                                      _ptr(ops, gt), 5, S_NEXT, ops._p(nz), COEF, ops._p(tg), _ptr(ops, ws), 0, ops._stream()),
              "sampler_step")
    check(lib.oniris_sampler_mse_finish(_ptr(ops, ws), 1, n, _ptr(ops, mse), ops._stream()), "sampler_mse_finish")
    torch.cuda.synchronize()
    hold_exact(name, "x_hat", xh.t, want["x_store"])
    if not last:
        hold_exact(name, "graph input", gx.t, want["x_store"])
        hold_exact(name, "sigma_buf", gt.t, torch.full((5,), S_NEXT))
    hold_f32(name, "mse_pred", mse.t[0, 0:1], want["mse_pred"])
    hold_f32(name, "mse", mse.t[0, 1:2], want["mse"])
    for b_, n_ in ((xh, "x_hat"), (d_io, "d_io"), (gx, "graph input"), (gt, "sigma_buf"), (ws, "mse_ws"), (mse, "mse")):
        b_.guards_ok(name, n_)


def test_sampler_step_refuses_bad_arguments():
    """Null pointers, n == 0, t_a == 0, nsig > n, a target without workspace: an error code and nothing launched."""
    ops, lib, check = _api()
    n = 1000
    v = _inputs(n)
    xh, d_io, xo, sig, ws, mse = (Buf(n, dtype=F32, init=v["x_hat"]), Buf(n, dtype=F32), Buf(n, dtype=F32), Buf(7, dtype=F32),
                                  Buf(1, 2, 4, dtype=F32), Buf(1, 2, dtype=F32))
    xp, xa, tg = _g(v["x_pred"]), _g(v["x_aux"]), _g(v["target"])
    P = lambda b: _ptr(ops, b)
    good = dict(mode=1, x_hat=P(xh), x_pred=ops._p(xp), d_io=P(d_io), x_aux=ops._p(xa), x_out=P(xo), n=n, t_a=T_A, dt=DT, sig=P(sig), nsig=7,
                s_next=S_NEXT, noise=None, coef=0.0, target=ops._p(tg), ws=P(ws), step=0)
    bad = [dict(mode=3), dict(mode=-1), dict(x_hat=None), dict(x_pred=None), dict(d_io=None), dict(x_aux=None), dict(x_out=None),
           dict(n=0), dict(t_a=0.0), dict(nsig=n + 1), dict(nsig=-1), dict(ws=None), dict(step=-1), dict(mode=2, x_pred=None)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.oniris_sampler_step(a["mode"], a["x_hat"], a["x_pred"], a["d_io"], a["x_aux"], a["x_out"], a["n"], a["t_a"], a["dt"],
                                     a["sig"], a["nsig"], a["s_next"], a["noise"], a["coef"], a["target"], a["ws"], a["step"], ops._stream())
        assert rc < 0, change
    for a in ((None, 1, n, P(mse)), (P(ws), 0, n, P(mse)), (P(ws), 1, 0, P(mse)), (P(ws), 1, n, None)):
        assert lib.oniris_sampler_mse_finish(*a, ops._stream()) < 0, a
    torch.cuda.synchronize()
    assert bool(torch.isnan(xo.t).all()) and bool(torch.isnan(ws.t).all()) and bool(torch.isnan(mse.t).all()) and bool(torch.isnan(sig.t).all())
    assert torch.equal(xh.t.cpu(), v["x_hat"])
