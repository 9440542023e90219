"""Restatement of the sampler's step with its two side branches (oniris_sampler_step / oniris_sampler_mse_finish, reference
edm2/sampler.py:56-83)  --  TEST INFRASTRUCTURE, in the manner of tests/step_edge_oracle.py.  CPU tensors in.

Two sides:
  * the elementwise outputs (x_next, what x_hat / x_out / the graph input receive, d_io) are the reference's float32 tensor
    expressions themselves, operation by operation, sigmas and the churn coefficient as 0-dim float32 tensors as the reference has
    them: every product and sum is rounded on its own, so the kernel is held to them bit for bit (hold_exact);
  * the two means, mean((x_pred - target)^2) and mean((x_next - target)^2) with x_next BEFORE the injection, are float64 sums of
    those float32 tensors, returned as (value, mag) pairs with mag = sum |addend| / n.  The addends are squares: mag is the value.
    The kernel subtracts, squares and adds in fp32 (chains: ceil(n / (256 * blocks)) per thread, 6 + 4 in a workgroup, then
    ceil(blocks / 256) + 6 + 4 in the finish), well inside the project's bound for an fp32 reduction, 2^-17 mag (hold_f32).

`launch` is one kernel launch; `step` is a whole step of the loop (the Euler launch, then the Heun launch unless it is the last
step), the unit the reference's MSE lines speak about.  `_defect=` are the deliberate defects of tests/test_sampler_probe_oracle.py:
  mse_after_churn   the MSE taken on x_hat' (after the injection) instead of x_next
  euler_pred        mse_pred of a corrected step from the Euler evaluation's prediction (`step` only)
  fma               coef * noise + x with a single rounding
  sum_not_mean      the sums without the division by n"""
import torch

F32 = torch.float32
F64 = torch.float64


def _s(v):
    return torch.tensor(v, dtype=F32)


def _mean_sq(a, b, n_div):
    e = (a.to(F64) - b.to(F64)) ** 2
    v = e.sum() / n_div
    return v.reshape(1), e.abs().sum().reshape(1) / n_div


def launch(mode, x_hat, x_pred, d_io, x_aux, t_a, dt, noise=None, coef=0.0, target=None, _defect=None, _pred_for_mse=None):
    """One launch.  mode 0: Euler, 1: Heun, 2: inject only (x_next = x_hat).  Returns a dict:
      x_next   the step's x_next before any injection                     (float32)
      x_store  what x_out receives (and x_hat, in mode 1 or with noise)   (float32)
      x_hat    what the x_hat buffer holds afterwards                     (float32)
      d_io     what the d_io buffer holds afterwards                      (float32, None in mode 2)
      mse_pred, mse   (value, mag) float64 pairs, None without target"""
    t_a, dt, coef = _s(t_a), _s(dt), _s(coef)
    if mode == 0:
        d = (x_hat - x_pred) / t_a
        x_next, d_out = x_hat + dt * d, d
    elif mode == 1:
        dp = (x_aux - x_pred) / t_a
        x_next, d_out = x_hat + dt * (0.5 * d_io + 0.5 * dp), d_io
    else:
        x_next, d_out = x_hat.clone(), d_io
    if noise is not None:
        if _defect == "fma":
            x_store = (coef.to(F64) * noise.to(F64) + x_next.to(F64)).to(F32)
        else:
            x_store = x_next + coef * noise
    else:
        x_store = x_next
    keeps = mode == 0 and noise is None                 # the Euler launch leaves x_hat alone (unless x_out is that buffer)
    out = dict(x_next=x_next, x_store=x_store, x_hat=x_hat if keeps else x_store, d_io=d_out, mse_pred=None, mse=None)
    if target is not None:
        n_div = 1 if _defect == "sum_not_mean" else x_hat.numel()
        out["mse_pred"] = _mean_sq(x_pred if _pred_for_mse is None else _pred_for_mse, target, n_div)
        out["mse"] = _mean_sq(x_store if _defect == "mse_after_churn" else x_next, target, n_div)
    return out


def step(x_hat, x_pred_euler, x_pred_corr, t_hat, t_next, noise=None, coef=0.0, target=None, _defect=None):
    """A whole step of the loop (sampler.py:65-83) from the step's x_hat: the Euler update at t_hat; with x_pred_corr (every step but
    the last) the second-order correction at t_next.  x_pred_corr is the prediction at the Euler x_next, which this function does not
    evaluate: the caller supplies both predictions.  The MSE of the step uses the LAST evaluation's prediction (:79) and the final
    x_next (:80); the injection of the following step acts on that x_next.  Returns launch()'s dict of the step's last launch, plus
    x_euler (the input of the correcting evaluation)."""
    dt = float(_s(t_next) - _s(t_hat))
    if x_pred_corr is None:
        out = launch(0, x_hat, x_pred_euler, None, None, t_hat, dt, noise, coef, target, _defect)
        out["x_euler"] = None
        return out
    e = launch(0, x_hat, x_pred_euler, None, None, t_hat, dt)
    out = launch(1, x_hat, x_pred_corr, e["d_io"], e["x_next"], t_next, dt, noise, coef, target, _defect,
                 _pred_for_mse=x_pred_euler if _defect == "euler_pred" else None)
    out["x_euler"] = e["x_next"]
    return out
