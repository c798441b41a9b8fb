"""Monte Carlo over the model set: closed loops on plants drawn from ``Mdata``, disturbances drawn from ``W``.

The controller is robust by construction against every ``[A | B]`` in the identified matrix zonotope and every disturbance in
``W``; the reference samples ``Mdata`` only to test the gain (``tzddpc/utils.py:105-129``).  Here every trajectory of a batch runs
on its own sampled plant (``tz_simulate_batch_plants``; the plant update is ``examples/1.double_integrator_sim.py:85``), and both
the plants and the disturbances are drawn on the device by a counter-based generator (``tz_sample_plants`` / ``tz_sample_noise``):
what trajectory ``i`` gets depends on ``(seed, i, step)`` only, never on how the batch is cut into calls or ranks.

``philox4x32_10``, ``reference_plants`` and ``reference_noise`` are the numpy statement of that stream (``include/tzddpc.h``),
independent of the kernel: the tests hold the device against them.
"""
from __future__ import annotations

import numpy as np

from . import native

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
STREAM_PLANTS, STREAM_NOISE = 0, 1


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10.  counter (..., 4), key (..., 2) (broadcast against each other), words below 2^32 -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    for r in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _mode(mode) -> str:
    if mode not in ("uniform", "vertex"):
        raise ValueError("mode must be 'uniform' or 'vertex'")
    return mode


def reference_coefficients(seed: int, first: int, count: int, steps: int, ngen: int, mode: str, stream: int) -> np.ndarray:
    """beta (count, steps, ngen) of global trajectories first .. first + count - 1."""
    _mode(mode)
    seed, first, ngen = int(seed), int(first), int(ngen)
    per = 2 if mode == "uniform" else 128
    nblk = (ngen + per - 1) // per
    i = np.uint64(first) + np.arange(count, dtype=np.uint64)
    ctr = np.zeros((count, steps, nblk, 4), dtype=np.uint64)
    ctr[..., 0] = (i & _MASK)[:, None, None]
    ctr[..., 1] = (i >> _S32)[:, None, None]
    ctr[..., 2] = np.arange(steps, dtype=np.uint64)[None, :, None]
    ctr[..., 3] = np.uint64(stream << 24) + np.arange(nblk, dtype=np.uint64)[None, None, :]
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)).astype(np.uint64)
    if mode == "uniform":
        k = ((w[..., 0::2] >> np.uint64(5)) << np.uint64(26)) + (w[..., 1::2] >> np.uint64(6))      # (..., nblk, 2), 53 bits
        beta = k.astype(np.float64) * 2.0 ** -52 - 1.0
    else:
        bits = (w[..., :, None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)                   # (..., nblk, 4, 32)
        beta = np.where(bits == 1, 1.0, -1.0)
    return beta.reshape(count, steps, nblk * per)[:, :, :ngen]


def _points(beta, centre, gen):
    """centre + sum_i beta[..., i] gen[i], accumulated in increasing i (one pass over the generators, vectorised over the rest)."""
    out = np.broadcast_to(centre, beta.shape[:-1] + centre.shape).copy()
    for i in range(gen.shape[0]):
        out += beta[..., i].reshape(beta.shape[:-1] + (1,) * centre.ndim) * gen[i]
    return out


def reference_plants(seed: int, first: int, count: int, centre, gen, n: int, mode: str = "uniform"):
    """Host statement of ``tz_sample_plants``: centre (n, n + m), gen (ngen, n, n + m) -> (A (count, n, n), B (count, n, m))."""
    centre = np.asarray(centre, float); gen = np.asarray(gen, float).reshape((-1,) + centre.shape)
    beta = reference_coefficients(seed, first, count, 1, gen.shape[0], mode, STREAM_PLANTS)[:, 0]
    M = _points(beta, centre, gen)
    return np.ascontiguousarray(M[:, :, :n]), np.ascontiguousarray(M[:, :, n:])


def reference_noise(seed: int, first: int, count: int, steps: int, centre, gen, mode: str = "vertex") -> np.ndarray:
    """Host statement of ``tz_sample_noise``: centre (n,), gen (ngen, n) -> (count, steps, n)."""
    centre = np.asarray(centre, float).reshape(-1); gen = np.asarray(gen, float).reshape(-1, centre.size)
    return _points(reference_coefficients(seed, first, count, steps, gen.shape[0], mode, STREAM_NOISE), centre, gen)


def sample_plants(model_set, count: int, seed: int, first_trajectory: int = 0, mode: str = "uniform", device: int = 0):
    """`count` plants of the matrix zonotope `model_set` (``ctl.Mdata``: [A | B], n x (n + m)) drawn on the device -> (A (count, n, n),
    B (count, n, m)).  "uniform": coefficients in [-1, 1), the interior; "vertex": +-1, corners of the set."""
    n = model_set.center.shape[0]
    return native.sample_plants(device, seed, first_trajectory, count, model_set.center, model_set.generators, n, _mode(mode))


def sample_noise(W, count: int, steps: int, seed: int, first_trajectory: int = 0, mode: str = "vertex", device: int = 0) -> np.ndarray:
    """Disturbances of the zonotope `W` drawn on the device -> (count, steps, n), the table ``simulate_batch`` takes."""
    return native.sample_noise(device, seed, first_trajectory, count, steps, W.center, np.asarray(W.generators, float).T, _mode(mode))


def closed_loop_margins(x, u, zonotopes):
    """Audit of recorded closed loops (x (B, T + 1, n), u (B, T, m)) against ``X.interval`` and ``U.interval``.
    -> (state_margin (B,), input_margin (B,), first_violation (B,)): the smallest signed distance of any recorded state / input to a
    face of its box (negative: outside by that much) and the first step at which either is negative (-1: none; a state x[t + 1]
    counts for step t + 1, the input u[t] for step t)."""
    x = np.asarray(x, float); u = np.asarray(u, float)
    Xi, Ui = zonotopes.X.interval, zonotopes.U.interval
    dx = np.minimum(x - Xi.left_limit, Xi.right_limit - x).min(axis=2)              # (B, T + 1)
    du = np.minimum(u - Ui.left_limit, Ui.right_limit - u).min(axis=2)              # (B, T)
    worst = dx.copy()
    worst[:, :du.shape[1]] = np.minimum(worst[:, :du.shape[1]], du)
    bad = worst < 0.0
    first = np.where(bad.any(axis=1), bad.argmax(axis=1), -1)
    return dx.min(axis=1), du.min(axis=1), first


def run(ctl, count: int, steps: int, seed: int, plants="uniform", noise="vertex", x0=None, first_trajectory: int = 0):
    """Sample, simulate, audit: `count` closed loops of `steps` steps, trajectory i on its own plant of ``ctl.Mdata`` (`plants`:
    "uniform", "vertex", or the plants themselves as (A, B)) under disturbances of ``W`` (`noise`: "vertex" or "uniform"), from `x0`
    (default: the centre of X0).  Returns what ``simulate_batch`` returns plus ``state_margin``, ``input_margin``,
    ``first_violation`` (``closed_loop_margins``) and the plants ``A``, ``B``.  Rows first_trajectory .. of a larger run are
    reproduced bit for bit."""
    zon = ctl.zonotopes
    if isinstance(plants, str):
        A, B = sample_plants(ctl.Mdata, count, seed, first_trajectory, plants, ctl.device)
    else:
        A, B = plants
    w = sample_noise(zon.W, count, steps, seed, first_trajectory, noise, ctl.device)
    if x0 is None:
        x0 = np.tile(zon.X0.center, (count, 1))
    out = ctl.simulate_batch(x0, w, A, B)
    out["state_margin"], out["input_margin"], out["first_violation"] = closed_loop_margins(out["x"], out["u"], zon)
    out["A"], out["B"], out["noise"] = np.asarray(A, float), np.asarray(B, float), w
    return out
