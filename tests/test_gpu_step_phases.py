"""-m gpu: closed-loop steps of tz_ipm_kernel around the staging of the Newton weights in front of the loop-top reduction (problems
with at most 64 variables and one row per thread: every iteration but the first of a warm start, where the staging buffer holds
lambda for the test of the starting point; restaged behind a rejected test).  The change touches that staging only; the tests run
the whole step on 8 trajectories: closed loops against the plain-C oracle under every shift policy, the benchmark's own
instantiation through its transient (correctors, rejected tests), jittered starts (cold and seeded starts), determinism, and the
instantiations that keep the old sequence (more rows per thread, more than 64 variables).  Helpers and tolerances as
tests/test_gpu_step_prologue.py."""
import functools

import numpy as np
import pytest

from tests import common
from tests.test_gpu_step_prologue import REL, _close

pytestmark = pytest.mark.gpu
BN = 8


@functools.lru_cache(maxsize=None)
def _controller(case, flags=0):
    return common.gpu_controller(case, plan_flags=flags)


def _inputs(zon, T):
    from tzddpc_amd.dist import vertex_noise
    return np.tile(zon.X0.center, (BN, 1)), vertex_noise(zon.W.compute_vertices(), 0, BN, T)


def _loop(ctl, x0, noise, A, B):
    ctl._native.reset_warm()
    return ctl.simulate_batch(x0, noise, A, B)


def _against_oracle(dev, ref):
    assert (dev["status"] == 0).all() and (ref["status"] == 0).all()
    sx = 1 + np.abs(ref["x"]).max(); su = 1 + np.abs(ref["u"]).max()
    print(f"gap x {np.abs(dev['x'] - ref['x']).max() / sx:.3e} u {np.abs(dev['u'] - ref['u']).max() / su:.3e} (relative)")
    np.testing.assert_allclose(dev["x"], ref["x"], rtol=0, atol=REL * sx)
    np.testing.assert_allclose(dev["u"], ref["u"], rtol=0, atol=REL * su)


@pytest.mark.parametrize("pol", [0, 1, 3])
@pytest.mark.parametrize("case", ["di_n5", "di2in_n10", "di_n2"])
def test_closed_loops_against_c_oracle(built, case, pol):
    """32 steps: the quiet budget of 16 runs out, so resting steps are in.  di_n5: n = 2, m = 1, the tube pass with the dimensions
    known at compile time; di2in_n10: the generic one; di_n2: 3 variables, 10 rows, fewer rows than a wave."""
    ctl, (A, B, zon) = _controller(case)
    x0, noise = _inputs(zon, 32)
    ctl._native.set_warm_shift(pol)
    try:
        dev = _loop(ctl, x0, noise, A, B)
    finally:
        ctl._native.set_warm_shift(ctl.warm_shift_policy)
    ref = common.c_oracle_for(ctl, shift_policy=pol).simulate_batch(x0, noise, A, B, threads=8)
    _against_oracle(dev, ref)


def _run_ptr(ctl, A, B, x0n, noise, way):
    """T steps as one launch (`run`: inner steps with the lean epilogue, the warm start inside the prologue) or as T launches of one
    step (`step`: full epilogue, start point read back from memory)."""
    import torch
    nat = ctl._native; n, m = ctl.qp.n, ctl.qp.m
    T = noise.shape[1]
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    w_tb = torch.from_numpy(np.ascontiguousarray(noise.transpose(1, 0, 2))).to(dev)        # [step, trajectory]
    At = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).to(dev)
    Bt = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float64).reshape(n, m)).to(dev)
    x = torch.from_numpy(x0n).to(dev); xbar = x.clone(); e = torch.zeros_like(x)
    u = torch.zeros((BN, m), **f64); cost = torch.zeros(BN, **f64); st = torch.zeros(BN, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    nat.reset_warm()
    ptrs = (At.data_ptr(), Bt.data_ptr(), u.data_ptr(), cost.data_ptr(), st.data_ptr())
    if way == "step":
        status = np.zeros(BN, dtype=np.int32)
        for t in range(T):
            nat.mpc_step_ptr(BN, x.data_ptr(), xbar.data_ptr(), e.data_ptr(), w_tb[t].data_ptr(), *ptrs)
            nat.sync()
            status = np.where(status != 0, status, st.cpu().numpy())
    else:
        nat.mpc_run_ptr(BN, T, x.data_ptr(), xbar.data_ptr(), e.data_ptr(), w_tb.data_ptr(), *ptrs)
        nat.sync()
        status = st.cpu().numpy()
    assert (status == 0).all(), (way, status)
    return dict(x=x.cpu().numpy(), xbar=xbar.cpu().numpy(), e=e.cpu().numpy(), u=u.cpu().numpy(), cost=cost.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _bench_instantiation_runs():
    """di_n20, 12 steps from the centre of X0 (the transient: violated rows after the shift, correctors): computed once, shared, not
    modified.  `run2` repeats `run` from a fresh start."""
    ctl, (A, B, zon) = _controller("di_n20")
    x0, noise = _inputs(zon, 12)
    return {way: _run_ptr(ctl, A, B, x0, noise, way.rstrip("2")) for way in ("run", "step", "run2")}


def test_bench_instantiation_one_launch_equals_twelve(built):
    _close(_bench_instantiation_runs()["run"], _bench_instantiation_runs()["step"], keys=("x", "xbar", "e", "u"))


def test_bench_instantiation_fused_equals_unfused(built):
    from tzddpc_amd import native
    fused, (A, B, zon) = _controller("di_n20")
    split, _ = _controller("di_n20", native.TZ_PLAN_UNFUSED)
    assert fused._native.plan_info()["fused"] and not split._native.plan_info()["fused"]
    x0, noise = _inputs(zon, 12)
    a = _loop(fused, x0, noise, A, B)
    b = _loop(split, x0, noise, A, B)
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    _close(a, b)                                         # whole x / u / cost trajectories
    # closed-loop state after the twelve steps (x, xbar, e, last u and cost), one launch on either plan
    _close(_bench_instantiation_runs()["run"], _run_ptr(split, A, B, x0, noise, "run"), keys=("x", "xbar", "e", "u"))


def test_bench_instantiation_is_deterministic(built):
    a, b = _bench_instantiation_runs()["run"], _bench_instantiation_runs()["run2"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    fused, (A, B, zon) = _controller("di_n20")
    x0, noise = _inputs(zon, 12)
    c = _loop(fused, x0, noise, A, B)
    d = _loop(fused, x0, noise, A, B)
    for k in ("x", "u", "cost", "status"):
        assert np.array_equal(c[k], d[k]), k


def test_jittered_starts_against_c_oracle(built):
    """X0 +- 0.25 (seed 7): the stored start taken as it is, its fall-back to a cold start, violated rows after the shift, warm starts
    with the push at its floor and above it -- in one loop."""
    ctl, (A, B, zon) = _controller("di_n5")
    x0, noise = _inputs(zon, 16)
    x0 = x0 + np.random.default_rng(7).uniform(-0.25, 0.25, size=x0.shape)
    dev = _loop(ctl, x0, noise, A, B)
    ref = common.c_oracle_for(ctl).simulate_batch(x0, noise, A, B, threads=8)
    _against_oracle(dev, ref)


def test_more_than_64_variables_against_c_oracle(built):
    """dim5_n20: tile-triangle class; the early staging is compiled out there, the weights are staged behind the test as before."""
    ctl, (A, B, zon) = _controller("dim5_n20")
    x0, noise = _inputs(zon, 8)
    dev = _loop(ctl, x0, noise, A, B)
    ref = common.c_oracle_for(ctl).simulate_batch(x0, noise, A, B, threads=8)
    _against_oracle(dev, ref)


def test_pulley_one_launch_equals_eight(built):
    ctl, (A, B, zon) = _controller("pulley_n10")
    x0, noise = _inputs(zon, 8)
    _close(_run_ptr(ctl, A, B, x0, noise, "run"), _run_ptr(ctl, A, B, x0, noise, "step"), keys=("x", "xbar", "e", "u"))
