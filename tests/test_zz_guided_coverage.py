"""Guard for the guided pair evaluation (the pattern of tests/test_zz_dispatch_coverage.py): one guided frame of the gym net at the
training dashboard's settings (reference plotting.py:165 with gym_train.py:129's guidance 2: 16 Heun steps, rho 2, sigma 0.01 .. 80,
8 context frames) is run under the dispatch census, at B = 1 and at the dashboard's micro-batch B = 8, and every (kernel
instantiation, tag) it launches must have been launched by a PASSING oracle-comparing test of this session (tests/conftest.py
ORACLE_CENSUS).  Marked `selfcheck`: its own launches never count as oracle coverage."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.slow, pytest.mark.selfcheck]


def _guided_frame_census(B):
    from autoregressive_diffusion_amd import ops
    from bench import GYM_CFG
    from edm2.networks_edm2 import UNet, Precond
    from edm2.sampler import edm_sampler_with_mse
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    unet = UNet(**GYM_CFG).to(dev)
    torch.nn.init.constant_(unet.out_gain, 1.0)
    net = Precond(unet, sigma_data=1.0).to(dev).eval()
    with torch.no_grad():
        ctx = torch.randn(B, 8, 8, 64, 64, device=dev)
        lab = torch.randint(0, 4, (B, 8), device=dev)
        _, cache = net(ctx, torch.ones(B, 8, device=dev) * 0.05, lab, update_cache=True)
        torch.cuda.synchronize()
        assert net.pair_served()
        ops.census_start()
        try:
            x, _, _, cache = edm_sampler_with_mse(net, cache, conditioning=lab[:, :1], num_steps=16, sigma_min=0.01, sigma_max=80,
                                                  rho=2, guidance=2)
            torch.cuda.synchronize()
        finally:
            seen = ops.census_stop()
    assert bool(torch.isfinite(x).all())
    del net, cache
    torch.cuda.empty_cache()
    return seen


@pytest.mark.parametrize("B", [1, 8])
def test_guided_frame_launches_only_oracle_covered_kernels(B):
    import conftest
    if not conftest.ORACLE_CENSUS:
        pytest.skip("no oracle census in this session (run the whole `-m gpu` suite: this guard reads what the other tests launched)")
    seen = _guided_frame_census(B)
    # the frame ran on the pair path: the guided output pass and launches of both halves
    assert any("precond_out_guided_kernel" in k for k in seen) and any(k.endswith(" [pair-rows]") for k in seen), sorted(seen)
    missing = sorted(k for k in seen if k not in conftest.ORACLE_CENSUS)
    assert not missing, missing
