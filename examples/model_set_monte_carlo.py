"""Does the closed loop keep its constraints on the OTHER models that explain the data?  Every trajectory runs on its own plant of the
identified model set Mdata (the reference samples Mdata only for the gain, tzddpc/utils.py:105-129; the closed loops of its
examples run on the true system, examples/1.double_integrator_sim.py:85).

The double integrator of examples/1.double_integrator_sim.py with its horizon N = 2, data seed 25, at all 64 corners of the boxed
Mdata, 12 steps under vertex disturbances: one corner's closed loop ends with a failed solve and a state outside X; the other 63,
and the true plant, stay inside.  Then the same audit on plants and disturbances drawn on the device."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tzddpc_amd import TZDDPC, cplite as cp, montecarlo
from tzddpc_amd.dist import vertex_noise
from tzddpc_amd.harness import generate_trajectories, system


def loss(u, x):
    cost = 0
    for i in range(u.shape[0]):
        cost += cp.norm(x[i, :], p=2) ** 2 + 1e-2 * cp.norm(u[i], p=1)
    return cost


if __name__ == "__main__":
    T, N = 12, 2
    A, Bm, zon, Tdata = system("di_sim")
    ctl = TZDDPC(generate_trajectories(A, Bm, zon.X0, zon.U, zon.W, 1, Tdata, np.random.default_rng(25)))
    ctl.build_zonotopes_theta(zon)
    ctl.build_problem(N, loss, lambda u, x: [])
    n = ctl.dim_x
    signs = np.array(list(itertools.product((-1.0, 1.0), repeat=ctl.Mdata.num_generators)))
    M = ctl.Mdata.center[None] + np.tensordot(signs, ctl.Mdata.generators, axes=(1, 0))      # the 64 corner plants [A | B]
    count = len(signs)
    noise = vertex_noise(zon.W.compute_vertices(), 0, count, T)
    out = montecarlo.run(ctl, count, T, seed=0, plants=(M[:, :, :n], M[:, :, n:]), x0=np.tile(zon.X0.center, (count, 1)))
    sim = ctl.simulate_batch(np.tile(zon.X0.center, (count, 1)), noise, M[:, :, :n], M[:, :, n:])
    sm, um, first = montecarlo.closed_loop_margins(sim["x"], sim["u"], zon)
    true = ctl.simulate_batch(zon.X0.center[None], noise[:1], A, Bm)
    print(f"true plant: status {true['status'][0]}, state margin {montecarlo.closed_loop_margins(true['x'], true['u'], zon)[0][0]:.3f}")
    print(f"{count} corner plants of Mdata, {T} steps, horizon {N}: {(sim['status'] != 0).sum()} closed loop(s) with a failed solve")
    for b in np.nonzero((sim["status"] != 0) | (sm < -1e-9))[0]:
        print(f"  corner {b} (signs {signs[b].astype(int).tolist()}): status {sim['status'][b]}, state leaves X by {-sm[b]:.3f} at step {first[b]}")
    bad = (out["status"] != 0) | (out["state_margin"] < -1e-9)
    print(f"same corners under sign-pattern disturbances drawn on the device: {bad.sum()} closed loop(s) leave X: {np.nonzero(bad)[0].tolist()}")
    mc = montecarlo.run(ctl, 4096, T, seed=1, plants="uniform", noise="vertex")
    bad = (mc["status"] != 0) | (mc["state_margin"] < -1e-9)
    print(f"4096 plants drawn uniformly from Mdata: {bad.sum()} closed loop(s) leave X; smallest state margin {mc['state_margin'].min():.3f}")
