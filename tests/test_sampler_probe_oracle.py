"""CPU review of tests/sampler_probe_oracle.py, the restatement tests/test_sampler_probe_gpu.py holds oniris_sampler_step to:
  1. pin      -- `step` against the reference's loop body written out literally (edm2/sampler.py:56-83) on 0-dim float32 sigmas:
                 the elementwise side bit for bit, the means against torch.mean in float64;
  2. float32  -- the two means evaluated in float32 in the kernel's summation shape (256-element block partials, then the
                 partials) use a small part of the 2^-17 mag bound;
  3. defects  -- each `_defect=` is caught by the very assertions the GPU test makes (oracle_hold.hold_exact on the elementwise
                 outputs, oracle_hold.hold_f32 on the means), run here on the oracle alone: defective oracle as `got`."""
import functools

import pytest
import torch

import oracle_hold as OH
import sampler_probe_oracle as PO
import step_edge_cases as SC

F32, F64 = torch.float32, torch.float64
COEF, T_A, DT = 33.125, 37.25, -16.125
hold_exact = functools.partial(OH.hold_exact, tag="PROBE")
hold_f32 = functools.partial(OH.hold_f32, tag="PROBE")


def _inputs(n, seed=0):
    """The magnitudes of fixture G9b's first step: x_hat ~ 40, noise and x_pred ~ 1, target ~ 0.5."""
    g = SC.gen(4200 + seed)
    return dict(x_hat=SC.rn(g, n, scale=40.0), x_pred=SC.rn(g, n), x_pred2=SC.rn(g, n), noise=SC.rn(g, n), target=SC.rn(g, n, scale=0.5))


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("churned", [False, True])
def test_pin_step_against_the_loop_body(last, churned):
    v = _inputs(1000)
    t_cur, t_next, S_noise = torch.tensor(26.5, dtype=F32), torch.tensor(9.25, dtype=F32), 1
    gamma = 0.25
    # the step that follows is churned from t_next; this step's own x_hat, t_hat are inputs
    t_hat = t_cur + gamma * t_cur
    x_hat, target = v["x_hat"], v["target"]
    x_pred = v["x_pred"]
    d_cur = (x_hat - x_pred) / t_hat                                        # sampler.py:68
    x_next = x_hat + (t_next - t_hat) * d_cur                               # :69
    if not last:
        x_pred = v["x_pred2"]                                               # :73 (the evaluation at x_next, supplied)
        d_prime = (x_next - x_pred) / t_next                                # :74
        x_next = x_hat + (t_next - t_hat) * (0.5 * d_cur + 0.5 * d_prime)   # :75
    mse_pred = torch.mean((x_pred.to(F64) - target.to(F64)) ** 2)           # :79
    mse = torch.mean((x_next.to(F64) - target.to(F64)) ** 2)                # :80
    coef = 0.0
    x_hat_following = x_next
    if churned:                                                             # :57-60 of the following step
        t_hat2 = t_next + gamma * t_next
        coef_t = (t_hat2 ** 2 - t_next ** 2).sqrt() * S_noise
        x_hat_following = x_next + coef_t * v["noise"]
        coef = float(coef_t)
    got = PO.step(x_hat, v["x_pred"], None if last else v["x_pred2"], float(t_hat), float(t_next), v["noise"] if churned else None,
                  coef, target)
    assert torch.equal(got["x_next"], x_next) and torch.equal(got["x_store"], x_hat_following)
    assert abs(got["mse_pred"][0].item() - mse_pred.item()) <= 1e-14 * mse_pred.item()
    assert abs(got["mse"][0].item() - mse.item()) <= 1e-14 * mse.item()
    assert got["mse"][1].item() == got["mse"][0].item() and got["mse_pred"][1].item() == got["mse_pred"][0].item()   # squares: mag = value


def test_pin_inject_only_and_no_target():
    v = _inputs(1000, 1)
    got = PO.launch(2, v["x_hat"], None, None, None, 1.0, 0.0, v["noise"], COEF)
    assert torch.equal(got["x_store"], v["x_hat"] + torch.tensor(COEF, dtype=F32) * v["noise"]) and torch.equal(got["x_next"], v["x_hat"])
    assert got["mse"] is None and got["mse_pred"] is None and got["d_io"] is None
    plain = PO.launch(2, v["x_hat"], None, None, None, 1.0, 0.0)
    assert torch.equal(plain["x_store"], v["x_hat"])


def _kernel_shaped_mean(a, b, blocks):
    """float32: every thread's elements in order (grid-stride), a workgroup's 256 values, then the block partials, times 1 / n."""
    n = a.numel()
    e = (a - b) * (a - b)
    pad = torch.zeros(-(-n // (256 * blocks)) * 256 * blocks, dtype=F32)
    pad[:n] = e
    per_thread = torch.zeros(blocks * 256, dtype=F32)
    for trip in pad.reshape(-1, blocks * 256):
        per_thread = per_thread + trip
    part = per_thread.reshape(blocks, 256).sum(1, dtype=F32)
    return part.sum(dtype=F32) * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(n), dtype=F32))


@pytest.mark.parametrize("n", [1000, 70001])
def test_float32_means_fit_the_bound(n):
    v = _inputs(n, 2)
    ref = PO.launch(0, v["x_hat"], v["x_pred"], None, None, T_A, DT, None, 0.0, v["target"])
    blocks = min(-(-n // 256), 1024)
    for name, a in (("mse_pred", v["x_pred"]), ("mse", ref["x_next"])):
        got = _kernel_shaped_mean(a, v["target"], blocks)
        hold_f32(f"float32 n={n}", name, got.reshape(1), ref[name])


def _caught(fn):
    with pytest.raises(AssertionError):
        fn()


def test_defects_are_caught_by_the_gpu_tests_assertions():
    v = _inputs(1000, 3)
    args = (v["x_hat"], v["x_pred"], v["x_pred2"], T_A, T_A + DT)
    ref = PO.step(*args, v["noise"], COEF, v["target"])
    # the clean oracle passes its own assertions
    hold_exact("clean", "x_store", ref["x_store"], ref["x_store"])
    hold_f32("clean", "mse", ref["mse"][0], ref["mse"])
    bad = PO.step(*args, v["noise"], COEF, v["target"], _defect="mse_after_churn")
    assert torch.equal(bad["x_store"], ref["x_store"])
    _caught(lambda: hold_f32("mse_after_churn", "mse", bad["mse"][0], ref["mse"]))
    hold_f32("mse_after_churn", "mse_pred", bad["mse_pred"][0], ref["mse_pred"])
    bad = PO.step(*args, v["noise"], COEF, v["target"], _defect="euler_pred")
    _caught(lambda: hold_f32("euler_pred", "mse_pred", bad["mse_pred"][0], ref["mse_pred"]))
    hold_f32("euler_pred", "mse", bad["mse"][0], ref["mse"])
    bad = PO.step(*args, v["noise"], COEF, v["target"], _defect="fma")
    moved = int((bad["x_store"] != ref["x_store"]).sum())
    print(f"defect fma: {moved} of 1000 elements differ in the last bit")
    assert moved > 0
    _caught(lambda: hold_exact("fma", "x_store", bad["x_store"], ref["x_store"]))
    bad = PO.step(*args, v["noise"], COEF, v["target"], _defect="sum_not_mean")
    _caught(lambda: hold_f32("sum_not_mean", "mse", bad["mse"][0], ref["mse"]))
    _caught(lambda: hold_f32("sum_not_mean", "mse_pred", bad["mse_pred"][0], ref["mse_pred"]))
    # the same on the last (Euler) step, where euler_pred is no defect: the Euler prediction IS the step's last one
    last = PO.step(v["x_hat"], v["x_pred"], None, T_A, T_A + DT, None, 0.0, v["target"])
    same = PO.step(v["x_hat"], v["x_pred"], None, T_A, T_A + DT, None, 0.0, v["target"], _defect="euler_pred")
    assert last["mse_pred"][0].item() == same["mse_pred"][0].item()
