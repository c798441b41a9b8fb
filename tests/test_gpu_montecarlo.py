"""Monte Carlo over the model set on the device: the counter-based sampler against its numpy statement, closed loops with one
plant per trajectory against the shared-plant entry points (bit for bit) and against the plain-C oracle (one call per plant)."""
import itertools

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu
REL = 1e-6          # as tests/test_gpu_parity.py: state / input trajectories within 1e-6 relative
EPS = 2.0 ** -52

_CTL = {}


def controller(case, **kw):
    """One controller per (case, options) for the whole module."""
    key = (case, tuple(sorted(kw.items())))
    if key not in _CTL:
        _CTL[key] = common.gpu_controller(case, **kw)
    return _CTL[key]


def _zonotope(n, m, ngen, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, n + m)), 0.1 * rng.standard_normal((ngen, n, n + m)),
            rng.standard_normal(n), 0.1 * rng.standard_normal((ngen, n)))


def _bound(centre, gen):
    """Elementwise bound on a sum of ngen + 1 terms in any association, fused or not: (ngen + 2) eps (|centre| + sum_i |gen_i|)."""
    return (gen.shape[0] + 2) * EPS * (np.abs(centre) + np.abs(gen).sum(axis=0))


# ---- 5. sampler against the host reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["uniform", "vertex"])
@pytest.mark.parametrize("n,m,ngen", [(2, 1, 6), (5, 2, 35), (4, 1, 401), (2, 1, 0), (3, 1, 129)])
def test_sampler_equals_the_host_reference(built, n, m, ngen, mode):
    """Every entry of the plant and noise tables within the summation bound of the numpy statement of the stream (exact without
    generators): 1, 67 and 300 trajectories (a partly filled workgroup, several workgroups), first = 0 and across 2^32, the noise in the
    trajectory-major and the step-major layout.  129 generators: one past a 128-bit vertex block (the issue asks it of the vertex
    mode; the uniform mode runs it too)."""
    from tzddpc_amd import montecarlo as mc, native
    centre, gen, wc, wg = _zonotope(n, m, ngen, seed=ngen)
    tolM, tolW, T = _bound(centre, gen), _bound(wc, wg), 5
    for Bn in (1, 67, 300):
        for first in (0, 2 ** 32 - 3):
            A, B = native.sample_plants(0, 17, first, Bn, centre, gen, n, mode)
            rA, rB = mc.reference_plants(17, first, Bn, centre, gen, n, mode)
            assert A.shape == (Bn, n, n) and B.shape == (Bn, n, m)
            dA, dB = np.abs(A - rA), np.abs(B - rB)
            print(f"plants n={n} m={m} ngen={ngen} {mode} B={Bn} first={first}: max |dA| {dA.max():.2e} |dB| {dB.max():.2e} (bound {tolM.max():.2e})")
            assert (dA <= tolM[:, :n]).all() and (dB <= tolM[:, n:]).all()
            ref = mc.reference_noise(17, first, Bn, T, wc, wg, mode)
            w_bt = native.sample_noise(0, 17, first, Bn, T, wc, wg, mode)
            w_tb = native.sample_noise(0, 17, first, Bn, T, wc, wg, mode, step_major=True)
            assert w_bt.shape == (Bn, T, n) and w_tb.shape == (T, Bn, n)
            print(f"noise  n={n} ngen={ngen} {mode} B={Bn} first={first}: max |dw| {np.abs(w_bt - ref).max():.2e} (bound {tolW.max():.2e})")
            assert (np.abs(w_bt - ref) <= tolW).all()
            assert np.array_equal(w_tb, w_bt.transpose(1, 0, 2))                 # same kernel, same values, other addresses
            if mode == "vertex" and ngen:
                assert not np.array_equal(w_bt[:, 0], w_bt[:, 1]) or Bn == 1      # steps draw their own coefficients


def test_sampler_leaves_the_gaps_of_a_wider_table_alone(built):
    """Rows wider than n (a table with other columns beside the disturbance): only the n entries of every row are written."""
    import ctypes as C
    from tzddpc_amd import montecarlo as mc, native
    _, _, wc, wg = _zonotope(2, 1, 6, seed=1)
    Bn, T, n, wide = 9, 4, 2, 5
    out = np.full((Bn, T, wide), -7.0)
    rc = native.lib().tz_sample_noise(0, 3, 0, Bn, T, n, 6, wc.ctypes.data_as(C.c_void_p), wg.ctypes.data_as(C.c_void_p), native.TZ_SAMPLE_VERTEX,
                                      T * wide, wide, out.ctypes.data_as(C.c_void_p), native.TZ_MEM_HOST)
    assert rc == 0, native.lib().tz_last_error()
    assert (out[:, :, n:] == -7.0).all()
    assert (np.abs(out[:, :, :n] - mc.reference_noise(3, 0, Bn, T, wc, wg, "vertex")) <= _bound(wc, wg)).all()


# ---- 6. shard independence, device against device --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["uniform", "vertex"])
def test_sampled_tables_do_not_depend_on_the_sharding(built, mode):
    from tzddpc_amd import native
    from tzddpc_amd.dist import shard_range
    centre, gen, wc, wg = _zonotope(5, 2, 35, seed=2)
    A, B = native.sample_plants(0, 9, 0, 300, centre, gen, 5, mode)
    W = native.sample_noise(0, 9, 0, 300, 5, wc, wg, mode)
    parts = [shard_range(300, 3, r) for r in range(3)]
    pa = [native.sample_plants(0, 9, lo, hi - lo, centre, gen, 5, mode) for lo, hi in parts]
    assert np.array_equal(np.concatenate([a for a, _ in pa]), A) and np.array_equal(np.concatenate([b for _, b in pa]), B)
    assert np.array_equal(np.concatenate([native.sample_noise(0, 9, lo, hi - lo, 5, wc, wg, mode) for lo, hi in parts]), W)


# ---- 7. B copies of one plant: the shared-plant call, bit for bit ----------------------------------------------------------------
def _three_entry_points(nat, n, m, Bn, T, x0, noise, A, B, plants):
    """simulate, mpc_run and T x mpc_step from the same start; `plants`: through the *_plants entry points (A, B then 3-D)."""
    import torch
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    w_bt = up(noise); w_tb = w_bt.transpose(0, 1).contiguous()
    At, Bt, x0t = up(A), up(B), up(x0)
    step = nat.mpc_step_plants_ptr if plants else nat.mpc_step_ptr
    run = nat.mpc_run_plants_ptr if plants else nat.mpc_run_ptr
    sim = nat.simulate_batch_plants_ptr if plants else nat.simulate_batch_ptr
    out = {}
    for way in ("sim", "run", "step"):
        x = x0t.clone(); xbar = x0t.clone(); e = torch.zeros_like(x0t)
        u = torch.zeros((Bn, m), **f64); cost = torch.zeros(Bn, **f64); st = torch.zeros(Bn, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        nat.reset_warm()
        if way == "sim":
            xt = torch.zeros((Bn, T + 1, n), **f64); ut = torch.zeros((Bn, T, m), **f64); ct = torch.zeros((Bn, T), **f64)
            torch.cuda.synchronize()
            sim(Bn, T, x0t.data_ptr(), w_bt.data_ptr(), At.data_ptr(), Bt.data_ptr(), xt.data_ptr(), ut.data_ptr(), ct.data_ptr(), st.data_ptr())
            nat.sync()
            r = dict(x=xt, u=ut, cost=ct, status=st)
        elif way == "run":
            run(Bn, T, x.data_ptr(), xbar.data_ptr(), e.data_ptr(), w_tb.data_ptr(), At.data_ptr(), Bt.data_ptr(), u.data_ptr(), cost.data_ptr(), st.data_ptr())
            nat.sync()
            r = dict(x=x, xbar=xbar, e=e, u=u, cost=cost, status=st)
        else:
            us, cs, ss = [], [], []
            for t in range(T):
                step(Bn, x.data_ptr(), xbar.data_ptr(), e.data_ptr(), w_tb[t].data_ptr(), At.data_ptr(), Bt.data_ptr(), u.data_ptr(), cost.data_ptr(), st.data_ptr())
                nat.sync()
                us.append(u.cpu().numpy().copy()); cs.append(cost.cpu().numpy().copy()); ss.append(st.cpu().numpy().copy())
            r = dict(x=x, xbar=xbar, e=e, u=np.stack(us, 1), cost=np.stack(cs, 1), status=np.stack(ss, 1))
        out[way] = {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in r.items()}
    return out


@pytest.mark.parametrize("case,flags,Bn,T", [("di_n5", 0, 8, 6), ("di_n5", "unfused", 8, 6), ("di_n80", 0, 8, 2)])
def test_copies_of_one_plant_equal_the_shared_plant_call(built, case, flags, Bn, T):
    """Fused small class, four-kernel step (tz_plant_kernel) and tile-triangle class; tz_simulate_batch, tz_mpc_run and repeated
    tz_mpc_step each against its *_plants form fed B copies of the true plant: x, u, cost, status (and xbar, e where the entry
    point has them) identical."""
    from tzddpc_amd import native
    from tzddpc_amd.dist import vertex_noise
    kw = dict(plan_flags=native.TZ_PLAN_UNFUSED) if flags == "unfused" else {}
    ctl, (A, B, zon) = controller(case, **kw)
    nat = ctl._native; n, m = ctl.qp.n, ctl.qp.m
    info = nat.plan_info()
    assert info["fused"] == (flags != "unfused") and (ctl.qp.nz > 64) == (case == "di_n80")
    noise = vertex_noise(zon.W.compute_vertices(), 0, Bn, T)
    x0 = np.tile(zon.X0.center, (Bn, 1)) + 0.05 * np.random.default_rng(4).standard_normal((Bn, n))
    shared = _three_entry_points(nat, n, m, Bn, T, x0, noise, A, np.asarray(B, float).reshape(n, m), plants=False)
    A3 = np.tile(np.asarray(A, float), (Bn, 1, 1)); B3 = np.tile(np.asarray(B, float).reshape(n, m), (Bn, 1, 1))
    own = _three_entry_points(nat, n, m, Bn, T, x0, noise, A3, B3, plants=True)
    for way in ("sim", "run", "step"):
        assert (shared[way]["status"] == 0).all(), (way, shared[way]["status"])
        assert set(shared[way]) == set(own[way]) and {"x", "u", "cost", "status"} <= set(own[way])
        for q in shared[way]:
            assert np.array_equal(shared[way][q], own[way][q]), (case, flags, way, q, np.abs(shared[way][q] - own[way][q]).max())
    # the host-pointer path of the controller (upload of B plants) as well
    a = ctl.simulate_batch(x0, noise, A, B); b = ctl.simulate_batch(x0, noise, A3, B3); c = ctl.simulate_batch(x0, noise, A3, B)
    for q in ("x", "u", "cost", "status"):
        assert np.array_equal(a[q], b[q]) and np.array_equal(a[q], c[q]), q


# ---- 8. / 9. one plant per trajectory against the C oracle -----------------------------------------------------------------------
def _corner_plants(ctl, signs):
    M = ctl.Mdata.center[None] + np.tensordot(np.asarray(signs, float), ctl.Mdata.generators, axes=(1, 0))
    n = ctl.dim_x
    return np.ascontiguousarray(M[:, :, :n]), np.ascontiguousarray(M[:, :, n:])


def _signs(ctl, case):
    g = ctl.Mdata.num_generators
    if case == "pulley_n10":
        assert g == 20
        return np.random.default_rng(3).choice([-1., 1.], (64, 20))
    return np.array(list(itertools.product((-1., 1.), repeat=g)))


def _device_and_oracle(case, T):
    """Trajectory b on corner plant b of Mdata, noise vertex_noise(vertices, 0, B, T), from the centre of X0: the device in one call,
    the oracle (one plant per call) once per trajectory with batch 1."""
    from tzddpc_amd.dist import vertex_noise
    ctl, (A, B, zon) = controller(case)
    A3, B3 = _corner_plants(ctl, _signs(ctl, case))
    Bn = A3.shape[0]
    noise = vertex_noise(zon.W.compute_vertices(), 0, Bn, T)
    x0 = np.tile(zon.X0.center, (Bn, 1))
    dev = ctl.simulate_batch(x0, noise, A3, B3)
    orc = common.c_oracle_for(ctl)
    rs = [orc.simulate_batch(x0[b:b + 1], noise[b:b + 1], A3[b], B3[b]) for b in range(Bn)]
    ref = {k: np.concatenate([r[k] for r in rs]) for k in ("x", "u", "status")}
    return ctl, zon, dev, ref


@pytest.mark.parametrize("case,T,count", [("di_n5", 12, 64), ("di2in_n10", 10, 256), ("pulley_n10", 10, 64)])
def test_per_trajectory_plants_against_c_oracle(built, case, T, count):
    """Every corner of the boxed Mdata (pulley: 64 random corners of its 2^20) as the plant of one closed loop: every state and
    input against the plain-C oracle, 1e-6 (1 + max |ref|); all solved and inside X and U (1e-9: the double integrators' inputs sit
    on their bound within rounding in the oracle as well)."""
    ctl, zon, dev, ref = _device_and_oracle(case, T)
    assert dev["x"].shape[0] == count
    assert (dev["status"] == 0).all() and (ref["status"] == 0).all(), (np.nonzero(dev["status"])[0], np.nonzero(ref["status"])[0])
    sx = 1 + np.abs(ref["x"]).max(); su = 1 + np.abs(ref["u"]).max()
    print(f"{case}: max |dx| {np.abs(dev['x'] - ref['x']).max():.3e} (bound {REL * sx:.3e}), max |du| {np.abs(dev['u'] - ref['u']).max():.3e} (bound {REL * su:.3e})")
    Xi, Ui = zon.X.interval, zon.U.interval
    assert np.all(dev["x"] >= Xi.left_limit - 1e-9) and np.all(dev["x"] <= Xi.right_limit + 1e-9)
    assert np.all(dev["u"] >= Ui.left_limit - 1e-9) and np.all(dev["u"] <= Ui.right_limit + 1e-9)
    np.testing.assert_allclose(dev["x"], ref["x"], rtol=0, atol=REL * sx)
    np.testing.assert_allclose(dev["u"], ref["u"], rtol=0, atol=REL * su)
    assert np.abs(dev["x"][1:, 1:] - dev["x"][0, 1:]).max() > 1e-3                # the plants did differ: so do the closed loops


def test_the_corner_of_di_n2_that_leaves_X(built):
    """Double integrator of examples/1.double_integrator_sim.py, N = 2, on the 64 corner plants of its Mdata: in the oracle exactly one
    closed loop ends with a non-zero status, its state 4.0 outside X.  The device reports a non-zero status for that trajectory and
    no other; the 63 solved ones agree to 1e-6.  Steps after a failure are not compared."""
    from tzddpc_amd.montecarlo import closed_loop_margins
    ctl, zon, dev, ref = _device_and_oracle("di_n2", 12)
    bad = np.nonzero(ref["status"])[0]
    assert dev["x"].shape[0] == 64 and bad.size == 1, bad
    sm, _, first = closed_loop_margins(ref["x"], ref["u"], zon)
    print(f"di_n2: oracle trajectory {bad[0]} status {ref['status'][bad[0]]}, state margin {sm[bad[0]]:.3f} from step {first[bad[0]]}; device status {dev['status'][bad[0]]}")
    assert abs(sm[bad[0]] + 4.0) < 0.05 and (np.delete(sm, bad[0]) >= -1e-9).all()
    assert np.array_equal(np.nonzero(dev["status"])[0], bad), (np.nonzero(dev["status"])[0], bad)
    ok = ref["status"] == 0
    sx = 1 + np.abs(ref["x"][ok]).max(); su = 1 + np.abs(ref["u"][ok]).max()
    print(f"di_n2: 63 solved, max |dx| {np.abs(dev['x'][ok] - ref['x'][ok]).max():.3e}, max |du| {np.abs(dev['u'][ok] - ref['u'][ok]).max():.3e}")
    np.testing.assert_allclose(dev["x"][ok], ref["x"][ok], rtol=0, atol=REL * sx)
    np.testing.assert_allclose(dev["u"][ok], ref["u"][ok], rtol=0, atol=REL * su)
    dm, _, dfirst = closed_loop_margins(dev["x"], dev["u"], zon)                  # the audit finds it in the device's own record
    assert dfirst[bad[0]] >= 0 and dm[bad[0]] < -1.0 and (np.delete(dm, bad[0]) >= -1e-9).all()      # (inputs sit on their bound within rounding)


# ---- 10. cutting-plane host path ---------------------------------------------------------------------------------------------------
def test_cutting_plane_closed_loop_with_per_trajectory_plants(built):
    """The dense-generator problem of test_dense_generators_by_cutting_planes (Girard order-2 generators, build_problem_simplified(1,
    20), cutting-plane form), 4 trajectories, 3 steps: stacked copies of one plant give the shared-plant result exactly; two
    distinct plants in one batch give, row by row, the results of the two shared-plant runs.  The runs that are compared all solve
    the same device problem: the cuts are found by warm-up runs first and the count is checked not to move."""
    from tests.test_gpu_parity import _oracle_setup
    from tzddpc_amd import TZDDPC, Data, Theta
    from tzddpc_amd.harness import system
    from tzddpc_amd.zonotope import MatrixZonotope
    s, u, x, idn, rng = _oracle_setup("di_cc")
    A, B, zon, T = system("di_cc")
    n, m = B.shape
    dK, dD = idn["MdataK_raw"].reduce(2), idn["Mdelta_raw"].reduce(2)
    ctl = TZDDPC(Data(u, x))
    ctl.build_zonotopes_theta(zon, theta=Theta(idn["K"], np.zeros_like(A), np.zeros_like(B)))
    ctl.MdataK, ctl.Mdelta = MatrixZonotope(dK.center, dK.generators), MatrixZonotope(dD.center, dD.generators)
    ctl.build_problem_simplified(1, 20, common.loss_di, common.nocons)
    assert ctl._cuts is not None
    Bn, T = 4, 3
    Wv = zon.W.compute_vertices()
    noise = Wv[np.random.default_rng(9).integers(0, Wv.shape[0], size=(Bn, T))]
    x0 = np.tile(zon.X0.center, (Bn, 1)) + 0.05 * np.random.default_rng(10).standard_normal((Bn, n))
    A2 = np.asarray(idn["A"], float); B2 = np.asarray(idn["B"], float).reshape(n, m)           # a second model of Mdata: its centre
    assert np.abs(A2 - A).max() + np.abs(B2 - B).max() > 1e-6
    pick = np.array([0, 1, 1, 0])
    Amix = np.where(pick[:, None, None] == 0, np.asarray(A, float)[None], A2[None])
    Bmix = np.where(pick[:, None, None] == 0, np.asarray(B, float).reshape(1, n, m), B2[None])
    for _ in range(3):                                   # warm-up: every cut these closed loops ask for
        before = ctl.num_cuts()
        ctl.simulate_batch(x0, noise, A, B); ctl.simulate_batch(x0, noise, A2, B2); ctl.simulate_batch(x0, noise, Amix, Bmix)
        if ctl.num_cuts() == before:
            break
    ncuts = ctl.num_cuts()
    one = ctl.simulate_batch(x0, noise, A, B)
    two = ctl.simulate_batch(x0, noise, A2, B2)
    stacked = ctl.simulate_batch(x0, noise, np.tile(np.asarray(A, float), (Bn, 1, 1)), np.tile(np.asarray(B, float).reshape(n, m), (Bn, 1, 1)))
    mixed = ctl.simulate_batch(x0, noise, Amix, Bmix)
    assert ctl.num_cuts() == ncuts
    assert (one["status"] == 0).all() and (two["status"] == 0).all()
    assert np.abs(one["x"] - two["x"]).max() > 1e-6
    for q in ("x", "u", "cost", "status"):
        assert np.array_equal(stacked[q], one[q]), q
        assert np.array_equal(mixed[q][pick == 0], one[q][pick == 0]) and np.array_equal(mixed[q][pick == 1], two[q][pick == 1]), q


# ---- 11. montecarlo.run end to end -------------------------------------------------------------------------------------------------
def test_run_samples_simulates_and_audits(built):
    """128 closed loops of di_n5 on corner plants and sign-pattern disturbances drawn on the device (seed 1): all solved, nothing outside
    X or U (every corner plant of this Mdata is checked against the oracle above); trajectories 64 .. 127 on their own are rows
    64 .. 127 bit for bit; the plants handed back are the sampler's."""
    from tzddpc_amd import montecarlo as mc
    ctl, (A, B, zon) = controller("di_n5")
    out = mc.run(ctl, 128, 12, 1, plants="vertex", noise="vertex")
    assert out["x"].shape == (128, 13, 2) and out["u"].shape == (128, 12, 1) and out["A"].shape == (128, 2, 2) and out["B"].shape == (128, 2, 1)
    print(f"run: statuses {np.unique(out['status'])}, smallest state margin {out['state_margin'].min():.3e}, input margin {out['input_margin'].min():.3e}")
    assert (out["status"] == 0).all(), np.nonzero(out["status"])[0]
    assert (out["state_margin"] >= -1e-9).all() and (out["input_margin"] >= -1e-9).all()
    rA, rB = mc.reference_plants(1, 0, 128, ctl.Mdata.center, ctl.Mdata.generators, 2, "vertex")
    tol = (ctl.Mdata.num_generators + 2) * EPS * (np.abs(ctl.Mdata.center) + np.abs(ctl.Mdata.generators).sum(axis=0))
    assert (np.abs(out["A"] - rA) <= tol[:, :2]).all() and (np.abs(out["B"] - rB) <= tol[:, 2:]).all()
    assert len(np.unique(out["A"].reshape(128, -1), axis=0)) > 8                  # corners, and many of them
    half = mc.run(ctl, 64, 12, 1, plants="vertex", noise="vertex", first_trajectory=64)
    for q in ("x", "u", "cost", "status", "A", "B", "noise", "state_margin", "input_margin", "first_violation"):
        assert np.array_equal(half[q], out[q][64:]), q
    given = mc.run(ctl, 64, 12, 1, plants=(out["A"][64:], out["B"][64:]), noise="vertex", first_trajectory=64)
    assert np.array_equal(given["x"], half["x"])
    uni = mc.run(ctl, 32, 6, 2, plants="uniform", noise="uniform")                # the interior of both sets
    assert (uni["status"] == 0).all() and (uni["state_margin"] >= -1e-9).all() and (uni["input_margin"] >= -1e-9).all()
    W = zon.W.interval
    assert (uni["noise"] >= W.left_limit - 1e-12).all() and (uni["noise"] <= W.right_limit + 1e-12).all()
