"""-m gpu: the prologue of a closed-loop step in tz_ipm_kernel -- the rows of the three parameter maps fetched in one round trip
(csr_fetch4 / csr_apply4, tz_kernels.hip.h; tests/test_host_map_widths.py pins which case takes which path) -- and the barriers
around it, on 8 trajectories x 8 steps: the one-launch plan against the four-kernel plan, one launch of 8 steps against eight
launches of one, a trajectory whose parameter rows are violated, and closed loops against the plain-C oracle."""
import functools

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu
REL = 1e-6          # as tests/test_gpu_parity.py: state / input trajectories within 1e-6 relative
BN, T = 8, 8


@functools.lru_cache(maxsize=None)
def _controller(case, flags=0):
    return common.gpu_controller(case, plan_flags=flags)


def _inputs(zon):
    from tzddpc_amd.dist import vertex_noise
    return np.tile(zon.X0.center, (BN, 1)), vertex_noise(zon.W.compute_vertices(), 0, BN, T)


def _loop(ctl, x0, noise, A, B):
    ctl._native.reset_warm()
    return ctl.simulate_batch(x0, noise, A, B)


def _close(a, b, keys=("x", "u")):
    """Tolerances of test_fused_plan_equals_unfused_plan (tests/test_gpu_ell_fetch.py), its assertions verbatim: x and u within 1e-9
    absolute, the cost within 1e-9 relative + 1e-9 absolute.  Every figure is printed before the first assertion.  Measured on an
    MI355X: fused against unfused <= 1.4e-13 (x, u) and 1.3e-12 (cost, relative); one launch against eight: di_n2 and pulley_n10
    <= 4e-15, di_n5 4.5e-10 (x), 5.9e-10 (u), cost 2.2e-10 absolute = 1.2e-9 relative -- the two entry points start a step from
    the same point up to rounding (G x carried in registers against G x formed afresh) and both stop at the solver's tolerance."""
    for k in keys:
        print(f"gap {k}: {np.abs(np.asarray(a[k]) - np.asarray(b[k])).max():.3e}")
    cg = np.abs(np.asarray(a["cost"]) - np.asarray(b["cost"]))
    print(f"gap cost: {cg.max():.3e} absolute, {(cg / np.maximum(np.abs(np.asarray(b['cost'])), 1e-300)).max():.3e} relative")
    for k in keys:
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-9, err_msg=k)
    np.testing.assert_allclose(a["cost"], b["cost"], rtol=1e-9, atol=1e-9, err_msg="cost")


@pytest.mark.parametrize("case", ["di_n2", "di2in_n10", "dim5_n20"])
def test_fused_plan_equals_unfused_plan(built, case):
    """di_n2: 10 rows / 3 variables, fewer rows than a wave; dim5_n20: maps of 7 entries (row by row), more than 256 rows; the
    tile-triangle class shares the map code."""
    from tzddpc_amd import native
    fused, (A, B, zon) = _controller(case)
    split, _ = _controller(case, native.TZ_PLAN_UNFUSED)
    assert fused._native.plan_info()["fused"] and not split._native.plan_info()["fused"]
    x0, noise = _inputs(zon)
    a = _loop(fused, x0, noise, A, B)
    b = _loop(split, x0, noise, A, B)
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    _close(a, b)


@pytest.mark.parametrize("case", ["di_n2", "di_n5", "pulley_n10"])
def test_one_launch_of_eight_steps_equals_eight_launches(built, case):
    """tz_mpc_run (inner steps: lean epilogue, the warm start inside the prologue's barrier intervals) against tz_mpc_step (every step
    a launch of its own: full epilogue, start point read back from memory)."""
    import torch
    ctl, (A, B, zon) = _controller(case)
    nat = ctl._native; n, m = ctl.qp.n, ctl.qp.m
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    x0n, noise = _inputs(zon)
    w_tb = torch.from_numpy(np.ascontiguousarray(noise.transpose(1, 0, 2))).to(dev)        # [step, trajectory]
    At = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).to(dev)
    Bt = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float64).reshape(n, m)).to(dev)
    x0 = torch.from_numpy(x0n).to(dev)
    runs = {}
    for way in ("step", "run"):
        x = x0.clone(); xbar = x0.clone(); e = torch.zeros_like(x0)
        u = torch.zeros((BN, m), **f64); cost = torch.zeros(BN, **f64); st = torch.zeros(BN, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        nat.reset_warm()
        ptrs = (At.data_ptr(), Bt.data_ptr(), u.data_ptr(), cost.data_ptr(), st.data_ptr())
        if way == "step":
            first = np.zeros(BN, dtype=np.int32)
            for t in range(T):
                nat.mpc_step_ptr(BN, x.data_ptr(), xbar.data_ptr(), e.data_ptr(), w_tb[t].data_ptr(), *ptrs)
                nat.sync()
                first = np.where(first != 0, first, st.cpu().numpy())
            status = first
        else:
            nat.mpc_run_ptr(BN, T, x.data_ptr(), xbar.data_ptr(), e.data_ptr(), w_tb.data_ptr(), *ptrs)
            nat.sync()
            status = st.cpu().numpy()
        runs[way] = dict(x=x.cpu().numpy(), xbar=xbar.cpu().numpy(), e=e.cpu().numpy(), u=u.cpu().numpy(), cost=cost.cpu().numpy())
        assert (status == 0).all(), (way, status)
    _close(runs["run"], runs["step"], keys=("x", "xbar", "e", "u"))


@pytest.mark.parametrize("plan", ["fused", "unfused"])
def test_violated_parameter_row(built, plan):
    """One trajectory starts 1.0 outside X: its parameter rows are violated, the step is not solved (status 3), the input is u = K e
    and the nominal state follows Phi; the other seven trajectories do not notice."""
    from tzddpc_amd import TZDDPC, native
    from tzddpc_amd.builder import theta_reference
    ctl, (A, B, zon) = _controller("di_n2", native.TZ_PLAN_UNFUSED if plan == "unfused" else 0)
    assert ctl._native.plan_info()["fused"] == (plan == "fused")
    qp = ctl.qp; n, m = qp.n, qp.m
    x0, noise = _inputs(zon)
    bad = 3
    x0v = x0.copy(); x0v[bad, 0] = zon.X.interval.right_limit[0] + 1.0
    a = _loop(ctl, x0, noise, A, B)
    b = _loop(ctl, x0v, noise, A, B)
    others = np.arange(BN) != bad
    assert (a["status"] == 0).all() and (b["status"][others] == 0).all() and b["status"][bad] == 3
    for k in ("x", "u", "cost"):
        assert np.array_equal(a[k][others], b[k][others]), k
    # the steps of the bad trajectory for as long as its parameter rows stay violated (at least the first)
    args, _ = TZDDPC._native_args(qp, {})
    Part, par0 = np.atleast_2d(np.asarray(args["Part"], float)), np.asarray(args["par0"], float)
    lo, hi = np.asarray(args["par_lo"], float), np.asarray(args["par_hi"], float)
    K = np.asarray(ctl.theta.K, float).reshape(m, n); Phi1 = np.asarray(qp.Phi, float)[n:2 * n]
    Bm = np.asarray(B, float).reshape(n, m)
    xbar = x0v[bad].copy(); checked = 0
    for t in range(T):
        x = b["x"][bad, t]; e = x - xbar
        v = par0 + Part @ theta_reference(qp, xbar, e)
        if not ((v < lo - 1e-6) | (v > hi + 1e-6)).any():       # (clearly violated only: the device's own margin is 1e-9)
            break
        u = K @ e
        np.testing.assert_allclose(b["u"][bad, t], u, rtol=0, atol=1e-12 * (1 + np.abs(u).max()))
        xn = A @ x + Bm @ b["u"][bad, t] + noise[bad, t]
        np.testing.assert_allclose(b["x"][bad, t + 1], xn, rtol=0, atol=1e-12 * (1 + np.abs(xn).max()))
        xbar = Phi1 @ xbar; checked += 1
    assert checked >= 1


@pytest.mark.parametrize("case", ["di_n5", "di2in_n10"])
def test_closed_loops_against_c_oracle(built, case):
    ctl, (A, B, zon) = _controller(case)
    x0, noise = _inputs(zon)
    dev = _loop(ctl, x0, noise, A, B)
    ref = common.c_oracle_for(ctl).simulate_batch(x0, noise, A, B, threads=8)
    assert (dev["status"] == 0).all() and (ref["status"] == 0).all()
    sx = 1 + np.abs(ref["x"]).max(); su = 1 + np.abs(ref["u"]).max()
    print(f"gap x {np.abs(dev['x'] - ref['x']).max() / sx:.3e} u {np.abs(dev['u'] - ref['u']).max() / su:.3e} (relative)")
    np.testing.assert_allclose(dev["x"], ref["x"], rtol=0, atol=REL * sx)
    np.testing.assert_allclose(dev["u"], ref["u"], rtol=0, atol=REL * su)
