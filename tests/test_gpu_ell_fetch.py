"""-m gpu: the windowed, fetch-ahead walk of the lane-ELL products (tz_ell_fetch / tz_ell_apply in tz_ipm.hip.h) and the split
parameter maps, at every depth class of the window (tests/test_host_ell_depths.py pins the depths): short closed loops against the
plain-C oracle, and the one-launch step against the four-kernel step."""
import numpy as np
import pytest

from tests import common
from tests.test_host_ell_depths import DEPTHS

pytestmark = pytest.mark.gpu
REL = 1e-6          # as tests/test_gpu_parity.py: state / input trajectories within 1e-6 relative
BN, T = 8, 8


def _loop(ctl, A, B, zon):
    from tzddpc_amd.dist import vertex_noise
    noise = vertex_noise(zon.W.compute_vertices(), 0, BN, T)
    x0 = np.tile(zon.X0.center, (BN, 1))
    return x0, noise, ctl.simulate_batch(x0, noise, A, B)


@pytest.mark.parametrize("case", sorted(DEPTHS))
def test_short_closed_loops_against_c_oracle(built, case):
    ctl, (A, B, zon) = common.gpu_controller(case)
    x0, noise, dev = _loop(ctl, A, B, zon)
    ref = common.c_oracle_for(ctl).simulate_batch(x0, noise, A, B, threads=8)
    assert (dev["status"] == 0).all() and (ref["status"] == 0).all()
    sx = 1 + np.abs(ref["x"]).max(); su = 1 + np.abs(ref["u"]).max()
    Xi, Ui = zon.X.interval, zon.U.interval
    assert np.all(dev["x"] >= Xi.left_limit - 1e-9) and np.all(dev["x"] <= Xi.right_limit + 1e-9)
    assert np.all(dev["u"] >= Ui.left_limit - 1e-9) and np.all(dev["u"] <= Ui.right_limit + 1e-9)
    np.testing.assert_allclose(dev["x"], ref["x"], rtol=0, atol=REL * sx)
    np.testing.assert_allclose(dev["u"], ref["u"], rtol=0, atol=REL * su)


@pytest.mark.parametrize("case", ["di_n20", "pulley_n10"])
def test_fused_plan_equals_unfused_plan(built, case):
    """The parameter maps run inside tz_ipm_kernel (fused) and in tz_affine_kernel (TZ_PLAN_UNFUSED): the same fetch and apply on
    both sides.  Tolerances of test_fused_step_equals_four_kernel_step."""
    from tzddpc_amd import native
    fused, (A, B, zon) = common.gpu_controller(case)
    split, _ = common.gpu_controller(case, plan_flags=native.TZ_PLAN_UNFUSED)
    assert fused._native.plan_info()["fused"] and not split._native.plan_info()["fused"]
    _, _, a = _loop(fused, A, B, zon)
    _, _, b = _loop(split, A, B, zon)
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    np.testing.assert_allclose(a["x"], b["x"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(a["u"], b["u"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(a["cost"], b["cost"], rtol=1e-9, atol=1e-9)
