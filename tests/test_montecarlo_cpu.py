"""Monte Carlo over the model set, host side: the numpy statement of the device's sampling stream (Philox4x32-10 and the counter
layout of include/tzddpc.h), the new entry points in header and binding, the argument checks that need no device, and the audit
of recorded closed loops."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import common

NEW_SYMBOLS = ("tz_simulate_batch_plants", "tz_mpc_step_plants", "tz_mpc_run_plants", "tz_sample_plants", "tz_sample_noise")


def _words(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter,key,out", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, out):
    """The three published known-answer vectors of Philox4x32-10."""
    from tzddpc_amd.montecarlo import philox4x32_10
    got = philox4x32_10(_words(counter), _words(key))
    assert got.dtype == np.uint32 and [int(v) for v in got] == _words(out)


def test_philox_is_vectorised():
    """Stacked counters give the stacked answers (the reference stream has no per-trajectory loop)."""
    from tzddpc_amd.montecarlo import philox4x32_10
    ctr = np.array([_words("00000000 00000000 00000000 00000000"), _words("243f6a88 85a308d3 13198a2e 03707344")])
    key = np.array([_words("00000000 00000000"), _words("a4093822 299f31d0")])
    got = philox4x32_10(ctr, key)
    assert got.shape == (2, 4)
    assert [int(v) for v in got[0]] == _words("6627e8d5 e169c58d bc57ac4c 9b00dbd8")
    assert [int(v) for v in got[1]] == _words("d16cfe09 94fdcceb 5001e420 24126ea1")


def _set(n, m, ngen, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n + m)), 0.1 * rng.standard_normal((ngen, n, n + m))


def test_coefficients_uniform_and_vertex():
    from tzddpc_amd import montecarlo as mc
    bu = mc.reference_coefficients(7, 0, 50, 3, 301, "uniform", mc.STREAM_NOISE)
    assert bu.shape == (50, 3, 301) and (bu >= -1.0).all() and (bu < 1.0).all()
    assert abs(bu.mean()) < 0.02 and abs(bu.var() - 1.0 / 3.0) < 0.02           # 45150 draws: sd of the mean 0.0027, of the variance 0.0014
    k = (bu + 1.0) * 2.0 ** 52
    assert np.array_equal(k, np.round(k))                                        # multiples of 2^-52: 53-bit integers, exactly
    bv = mc.reference_coefficients(7, 0, 50, 3, 301, "vertex", mc.STREAM_NOISE)
    assert bv.shape == (50, 3, 301) and np.array_equal(np.abs(bv), np.ones_like(bv))
    assert abs(bv.mean()) < 0.02
    # the layout itself, from the generator: uniform coefficient 5 of trajectory 3, step 2 is words (2, 3) of block 2; vertex coefficient 133
    # is bit 5 of word 0 of block 1
    w = mc.philox4x32_10([3, 0, 2, (1 << 24) + 2], [7, 0]).astype(np.uint64)
    assert bu[3, 2, 5] == float((int(w[2]) >> 5) * 2 ** 26 + (int(w[3]) >> 6)) * 2.0 ** -52 - 1.0
    w = mc.philox4x32_10([3, 0, 2, (1 << 24) + 1], [7, 0])
    assert bv[3, 2, 133] == (1.0 if (int(w[0]) >> 5) & 1 else -1.0)


@pytest.mark.parametrize("mode", ["uniform", "vertex"])
def test_reference_tables_do_not_depend_on_the_slice(mode):
    """Rows [a, a + c) of the table from first = 0 are the table from first = a; also across first + b = 2^32."""
    from tzddpc_amd import montecarlo as mc
    centre, gen = _set(2, 1, 6)
    A, B = mc.reference_plants(11, 0, 40, centre, gen, 2, mode)
    a, b = mc.reference_plants(11, 13, 9, centre, gen, 2, mode)
    assert np.array_equal(a, A[13:22]) and np.array_equal(b, B[13:22])
    wc, wg = np.array([0.1, -0.2]), 0.05 * np.random.default_rng(1).standard_normal((3, 2))
    W = mc.reference_noise(11, 0, 40, 5, wc, wg, mode)
    assert W.shape == (40, 5, 2) and np.array_equal(mc.reference_noise(11, 13, 9, 5, wc, wg, mode), W[13:22])
    base = 2 ** 32 - 3
    A, B = mc.reference_plants(11, base, 8, centre, gen, 2, mode)
    a, b = mc.reference_plants(11, base + 2, 4, centre, gen, 2, mode)             # rows 2 .. 5: global indices 2^32 - 1 .. 2^32 + 2
    assert np.array_equal(a, A[2:6]) and np.array_equal(b, B[2:6])
    W = mc.reference_noise(11, base, 8, 5, wc, wg, mode)
    assert np.array_equal(mc.reference_noise(11, base + 2, 4, 5, wc, wg, mode), W[2:6])
    assert not np.array_equal(W[2], W[3])                                         # the high counter word counts: 2^32 - 1 and 2^32 differ ...
    low = mc.reference_noise(11, 0, 1, 5, wc, wg, mode)
    assert not np.array_equal(W[3], low[0])                                       # ... and 2^32 is not 0 again


def test_streams_and_seeds_differ():
    from tzddpc_amd import montecarlo as mc
    for mode in ("uniform", "vertex"):
        p = mc.reference_coefficients(5, 0, 16, 1, 64, mode, mc.STREAM_PLANTS)
        q = mc.reference_coefficients(5, 0, 16, 1, 64, mode, mc.STREAM_NOISE)
        r = mc.reference_coefficients(6, 0, 16, 1, 64, mode, mc.STREAM_PLANTS)
        hi = mc.reference_coefficients(5 + (1 << 32), 0, 16, 1, 64, mode, mc.STREAM_PLANTS)      # the high key word
        assert not np.array_equal(p, q) and not np.array_equal(p, r) and not np.array_equal(p, hi)
        assert (p != q).mean() > 0.4 and (p != r).mean() > 0.4


def test_no_generators_give_the_centre():
    from tzddpc_amd import montecarlo as mc
    centre, gen = _set(2, 1, 0)
    for mode in ("uniform", "vertex"):
        A, B = mc.reference_plants(3, 5, 4, centre, gen, 2, mode)
        assert np.array_equal(A, np.tile(centre[:, :2], (4, 1, 1))) and np.array_equal(B, np.tile(centre[:, 2:], (4, 1, 1)))
        W = mc.reference_noise(3, 5, 4, 6, np.array([0.5, -1.0]), np.zeros((0, 2)), mode)
        assert np.array_equal(W, np.tile([0.5, -1.0], (4, 6, 1)))


def test_reference_points_are_the_affine_image():
    """The tables are centre + beta . gen of the coefficients above (summed in increasing i), split [A | B]."""
    from tzddpc_amd import montecarlo as mc
    centre, gen = _set(3, 2, 7)
    beta = mc.reference_coefficients(9, 4, 5, 1, 7, "uniform", mc.STREAM_PLANTS)[:, 0]
    A, B = mc.reference_plants(9, 4, 5, centre, gen, 3, "uniform")
    M = centre + np.tensordot(beta, gen, axes=(1, 0))
    np.testing.assert_allclose(np.concatenate([A, B], axis=2), M, rtol=0, atol=1e-14)
    assert A.shape == (5, 3, 3) and B.shape == (5, 3, 2)


def test_header_and_binding_carry_the_new_entry_points(built):
    from tzddpc_amd import native
    hdr = open(os.path.join(common.__file__.rsplit("/tests/", 1)[0], "include", "tzddpc.h")).read()
    names = set(re.findall(r"^(?:int|const char\*)\s+(tz_\w+)\s*\(", hdr, flags=re.M))
    assert set(NEW_SYMBOLS) <= names and set(NEW_SYMBOLS) <= set(native.EXPORTED_SYMBOLS)
    assert re.search(r"^#define\s+TZ_ABI_VERSION\s+6\s*$", hdr, flags=re.M)
    assert re.search(r"TZ_SAMPLE_UNIFORM\s*=\s*0\s*,\s*TZ_SAMPLE_VERTEX\s*=\s*1", hdr)
    assert (native.TZ_SAMPLE_UNIFORM, native.TZ_SAMPLE_VERTEX) == (0, 1)
    L = native.lib()
    for nm in NEW_SYMBOLS:
        assert hasattr(L, nm)
    assert native.TZ_ABI_VERSION == 6 and L.tz_abi_version() == 6
    for nm in ("mpc_step_plants_ptr", "mpc_run_plants_ptr", "simulate_batch_plants_ptr"):
        assert callable(getattr(native.Problem, nm))


def test_sampler_argument_checks_need_no_device(built):
    """A bad mode, a negative generator count, an empty batch and null pointers are TZ_ERR_INVALID before any device query: the
    same answer on a machine without a GPU."""
    from tzddpc_amd import native
    L = native.lib()
    centre, gen = np.zeros(6), np.zeros((2, 6))
    A, B, W = np.zeros((1, 2, 2)), np.zeros((1, 2, 1)), np.zeros((1, 3, 2))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def plants(B_=1, n=2, m=1, ngen=2, mode=0, c=vp(centre), g=vp(gen), a=vp(A), b=vp(B), first=0):
        return L.tz_sample_plants(0, 1, first, B_, n, m, ngen, c, g, mode, a, b, native.TZ_MEM_HOST)

    def noise(B_=1, T=3, n=2, ngen=2, mode=1, c=vp(centre), g=vp(gen), o=vp(W), ts=6, ss=2, first=0):
        return L.tz_sample_noise(0, 1, first, B_, T, n, ngen, c, g, mode, ts, ss, o, native.TZ_MEM_HOST)
    for call in (plants, noise):
        for bad in (dict(mode=2), dict(mode=-1), dict(ngen=-1), dict(B_=0), dict(B_=-4), dict(c=None), dict(g=None), dict(first=-1),
                    dict(n=0), dict(n=17)):
            assert call(**bad) == native.TZ_ERR_INVALID, (call.__name__, bad, L.tz_last_error())
            assert L.tz_last_error()
    assert plants(a=None) == native.TZ_ERR_INVALID and plants(b=None) == native.TZ_ERR_INVALID and plants(m=9) == native.TZ_ERR_INVALID
    assert noise(o=None) == native.TZ_ERR_INVALID and noise(T=0) == native.TZ_ERR_INVALID
    assert noise(B_=2, ts=2, ss=2) == native.TZ_ERR_INVALID                          # rows of two trajectories on top of each other
    assert b"mode" in (plants(mode=7), L.tz_last_error())[1]
    with pytest.raises(ValueError, match="mode"):
        native.sample_plants(0, 1, 0, 1, centre.reshape(2, 3), gen.reshape(2, 2, 3), 2, mode="corners")


def test_closed_loop_margins_on_a_hand_made_trajectory():
    from types import SimpleNamespace
    from tzddpc_amd.montecarlo import closed_loop_margins
    from tzddpc_amd.zonotope import Zonotope
    zon = SimpleNamespace(X=Zonotope([1.0, 0.0], np.diag([4.0, 2.0])), U=Zonotope([0.0], [[1.5]]))      # X = [-3, 5] x [-2, 2], U = [-1.5, 1.5]
    x = np.zeros((3, 6, 2)); u = np.zeros((3, 5, 1))
    x[0, 3] = [5.25, 0.0]                       # 0.25 outside at step 3
    x[0, 5] = [0.0, -2.125]                     # later and smaller: neither the margin nor the first step
    x[1, 2] = [4.0, 1.5]; u[1, 4] = 1.25        # inside: 0.5 from a state face, 0.25 from an input face
    u[2, 1] = -1.75; x[2, 4] = [-3.5, 0.0]      # the input leaves first (step 1), the state later and further
    sm, um, first = closed_loop_margins(x, u, zon)
    np.testing.assert_allclose(sm, [-0.25, 0.5, -0.5], rtol=0, atol=1e-15)
    np.testing.assert_allclose(um, [1.5, 0.25, -0.25], rtol=0, atol=1e-15)
    assert first.tolist() == [3, -1, 1]


def test_plants_argument_of_simulate_batch_is_2d_or_3d():
    """native.Problem.plants: 2-D stays the shared plant; a 3-D one turns the other into one copy per trajectory."""
    from tzddpc_amd import native
    p = native.Problem.__new__(native.Problem); p.n, p.m = 2, 1
    A, B = np.array([[1.0, 0.1], [0.0, 1.0]]), np.array([[0.0], [0.1]])
    a, b, per = p.plants(A, B, 5)
    assert not per and a.shape == (2, 2) and b.shape == (2, 1)
    A3 = np.stack([A * (1 + k) for k in range(5)])
    a, b, per = p.plants(A3, B, 5)
    assert per and np.array_equal(a, A3) and b.shape == (5, 2, 1) and all(np.array_equal(b[k], B) for k in range(5))
    a, b, per = p.plants(A, np.stack([B] * 5), 5)
    assert per and a.shape == (5, 2, 2) and all(np.array_equal(a[k], A) for k in range(5)) and a.flags.c_contiguous and b.flags.c_contiguous
    with pytest.raises(ValueError):
        p.plants(A3[:3], B, 5)
