"""CPU: the host planner (tzddpc_amd/csrc/tz_plan.h) compiled with UBSan and the libstdc++ assertions, run on the descriptions the
product sends for every case of tests/common.CASES, and every table it makes checked against numpy.  The kernels trust these
tables blindly (an offset out of range is an out-of-bounds read on the device), and nothing else executes this code without a GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import common
from tzddpc_amd import native

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_MAX = 160 * 1024
ENT = np.dtype([("val", "<f8"), ("off", "<u4"), ("pad", "<u4")])
ITEM = np.dtype([(k, "<i4") for k in ("I0", "q0", "nq", "kptr", "klen")])
UNIT = np.dtype([(k, "<i4") for k in ("ib", "jb", "s0")])
CHUNK = np.dtype([(k, "<i4") for k in ("seg", "src", "a", "b")])          # GsChunk (g0, g1) and GsChunkM (q0, nq)
DTYPES = {"ent": ENT, "items": ITEM, "gunits": UNIT, "chunks": CHUNK, "chunks_m": CHUNK, "idx": np.dtype("<u2")}
F64 = {"P", "Gp", "val", "c0", "CKpow", "Ttube", "act_scale", "rec0", "recx", "recy", "shift_xs", "shift_ls", "lit", "srt", "mf", "mfn"}
SCALARS = ("nzp mip Tz Kc nquads nklist nP maxr ncg tt staircase ksplit TS ntile gu hsize nell ntube lds_bytes wgs_per_cu lean_epilogue "
           "fused mfma_gram mfma_chol mfma_issued eg.L eg.VL et.L et.VL q.rows q.W h.rows h.W par.rows par.W").split()
TABLES = ("permc permr vpos P Gp klist item_ptr smask items eg.ent eg.seg eg.val eg.idx et.ent et.seg et.val et.idx q.ent q.c0 h.ent h.c0 "
          "par.ent par.c0 CKpow Ttube act_scale row_of rec0 recx recy shift_var shift_row shift_xs shift_ls gunits gunit_ptr").split()
GS_SCALARS = "rec nchunk G mfma rows_mf have_cZ".split()
GS_TABLES = "lit srt chunks seg_chunk_ptr mf mfn chunks_m".split()


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "libplan_host.so")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-shared", "-fPIC", "-D_GLIBCXX_ASSERTIONS", "-fsanitize=undefined",
                           "-fno-sanitize-recover=undefined", "-static-libubsan", "-o", out, os.path.join(HERE, "native", "plan_host.cpp")])
    lib = C.CDLL(out)
    lib.plan_error.restype = C.c_char_p
    for f in (lib.plan_scalar, lib.genstack_scalar, lib.layout_const):
        f.restype = C.c_longlong; f.argtypes = [C.c_char_p]
    for f in (lib.plan_table, lib.genstack_table):
        f.restype = C.c_void_p; f.argtypes = [C.c_char_p, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lib.lds_doubles.restype = C.c_longlong
    lib.lds_doubles.argtypes = [C.c_longlong] + [C.c_int] * 10
    lib.plan_build.argtypes = [C.POINTER(native.ProblemDesc)]
    lib.genstack_build.argtypes = [C.POINTER(native.GenstackDesc)]
    return lib


def _fetch(scalar, table, scalars, tables):
    out = {k: int(scalar(k.encode())) for k in scalars}
    for k in tables:
        cnt, eb = C.c_longlong(0), C.c_int(0)
        ptr = table(k.encode(), C.byref(cnt), C.byref(eb))
        assert cnt.value >= 0, k
        leaf = k.split(".")[-1]
        dt = DTYPES.get(leaf, np.dtype("<f8") if leaf in F64 else np.dtype("<i4"))
        assert dt.itemsize == eb.value, k
        out[k] = np.frombuffer(C.string_at(ptr, cnt.value * eb.value), dtype=dt).copy() if cnt.value else np.zeros(0, dt)
    return out


def build_plan(shim, args, plan_flags=0):
    """(return code, message, plan as a dict) of the planner for the keyword arguments of native.problem_desc."""
    d, keep = native.problem_desc(**dict(args, plan_flags=plan_flags))
    rc = shim.plan_build(C.byref(d))
    msg = shim.plan_error().decode()
    return rc, msg, (_fetch(shim.plan_scalar, shim.plan_table, SCALARS, TABLES) if rc == 0 else None)


@functools.lru_cache(maxsize=None)
def case_args(case):
    from tzddpc_amd import TZDDPC
    _, qp, _ = common.identified_qp(case)
    args, _ = TZDDPC._native_args(qp, {})
    return args


def ell_expand(pl, key, NL, compact, nout, nin):
    """Dense (nout x nin) sum of the records of a lane-ELL table and how often each position is hit; checks the table's shape."""
    L, VL, seg = pl[key + ".L"], pl[key + ".VL"], pl[key + ".seg"]
    assert VL % NL == 0 and VL > 0 and L >= 1 and len(seg) == max(nout, 1)
    if compact:
        val, idx = pl[key + ".val"], pl[key + ".idx"].astype(np.int64)
        assert len(val) == len(idx) == VL * L and len(pl[key + ".ent"]) == 0
    else:
        ent = pl[key + ".ent"]
        assert len(ent) == VL * L and len(pl[key + ".val"]) == 0 and len(pl[key + ".idx"]) == 0
        assert not ent["pad"].any() and not (ent["off"] % 8).any()
        val, idx = ent["val"], ent["off"].astype(np.int64) // 8
    assert (idx < nin).all()                                   # every record, padding included, addresses an existing input
    M = np.zeros((nout, nin)); hits = np.zeros((nout, nin), dtype=np.int64)
    used = np.zeros(VL * L, dtype=bool)
    lane_end = 0
    for o in range(nout):
        lane0, cnt = int(seg[o]) & 0xFFFF, int(seg[o]) >> 16
        assert lane0 == lane_end and lane0 + cnt <= VL            # consecutive lanes, inside the table
        lane_end = lane0 + cnt
        vl = np.repeat(np.arange(lane0, lane0 + cnt), L); slot = np.tile(np.arange(L), cnt)
        pos = ((vl // NL) * L + slot) * NL + vl % NL
        used[pos] = True
        nzr = val[pos] != 0.0
        np.add.at(M[o], idx[pos][nzr], val[pos][nzr]); np.add.at(hits[o], idx[pos][nzr], 1)
    assert not val[~used].any()                                    # lanes no output owns hold nothing
    return M, hits


def map_expand(pl, key, ncols):
    rows, W, ent = pl[key + ".rows"], pl[key + ".W"], pl[key + ".ent"]
    assert len(ent) == W * max(rows, 1) and len(pl[key + ".c0"]) == rows and not ent["pad"].any() and not (ent["off"] % 8).any()
    col = ent["off"].astype(np.int64) // 8
    assert (col < ncols).all()
    M = np.zeros((rows, ncols))
    if rows:
        e = ent.reshape(W, rows); c = col.reshape(W, rows)
        for w in range(W):
            nzr = e["val"][w] != 0.0
            assert not M[np.nonzero(nzr)[0], c[w][nzr]].any()      # a column appears once per row
            M[np.nonzero(nzr)[0], c[w][nzr]] = e["val"][w][nzr]
    return M


def tube_reference(args):
    """The recursion of tz_plan_tube evaluated directly: R_0 = D_K, R_d = D_K Tx_{d-1}; Tx_d = sum_j X_{d-j} R_j; Tu_d = sum_j U_{d-j} R_j."""
    n, m, pm = int(args["n"]), int(args["m"]), int(args["pmax"])
    CK, DK = np.asarray(args["CK"], float).reshape(n, n), np.asarray(args["DK"], float).reshape(n, n)
    X = np.asarray(args["absCKpow"], float).reshape(-1, n, n); U = np.asarray(args["absKCKpow"], float).reshape(-1, m, n)
    ckp = [np.eye(n)]
    for _ in range(pm):
        ckp.append(CK @ ckp[-1])
    R, T = [], []
    for d in range(pm):
        R.append(DK if d == 0 else DK @ T[d - 1][:n])
        T.append(np.vstack([sum(X[d - j] @ R[j] for j in range(d + 1)), sum(U[d - j] @ R[j] for j in range(d + 1))]))
    return np.array(ckp), (np.array(T) if pm else np.zeros((1, n + m, n)))


def check_plan(shim, args, flags, pl):
    n, m, N = int(args["n"]), int(args["m"]), int(args["N"])
    G = np.ascontiguousarray(args["G"], float); P = np.ascontiguousarray(args["P"], float)
    mi, nz = G.shape
    nv, ntheta = N * m, 2 * n + N * (2 * n + m)
    NW, TH = shim.layout_const(b"TZ_NWAVES"), shim.layout_const(b"TZ_THREADS")
    Tz, Kc, nzp, mip = pl["Tz"], pl["Kc"], pl["nzp"], pl["mip"]
    assert (Tz, nzp, Kc, mip) == ((nz + 3) // 4, 4 * ((nz + 3) // 4), (mi + 3) // 4, 4 * ((mi + 3) // 4))
    assert pl["maxr"] == -(-mi // TH) and pl["ncg"] == -(-nzp // 64) and bool(pl["tt"]) == (pl["ncg"] >= 2 or pl["maxr"] > 4)
    tt = bool(pl["tt"])
    assert bool(pl["staircase"]) == (tt and not flags & native.TZ_PLAN_NO_STAIRCASE)
    assert bool(pl["ksplit"]) == (not tt and Tz <= shim.layout_const(b"TZ_KS_TZ") and not flags & native.TZ_PLAN_ITEM_GRAM)

    # ---- orderings, dense copies -------------------------------------------------------------------------------------------------
    permc, permr = pl["permc"], pl["permr"]
    assert sorted(permc) == list(range(nz)) and sorted(permr) == list(range(mi))
    if not pl["staircase"]:
        assert (permc == np.arange(nz)).all() and (permr == np.arange(mi)).all() and len(pl["vpos"]) == 0
    invc = np.argsort(permc); invr = np.argsort(permr)
    Gd, Pd = G[permr][:, permc], P[permc][:, permc]
    Ppad = np.zeros((nzp, nzp)); Ppad[:nz, :nz] = Pd
    assert np.array_equal(pl["P"].reshape(nzp, nzp), Ppad)
    assert pl["nP"] == (np.nonzero(Pd.any(axis=1))[0].max() + 1 if Pd.any() else 0)
    Gpad = np.zeros((4 * (Kc + 1), 4 * (Tz + 1))); Gpad[:mi, :nz] = Gd
    assert np.array_equal(pl["Gp"].reshape(Kc + 1, Tz + 1, 4, 4), Gpad.reshape(Kc + 1, 4, Tz + 1, 4).transpose(0, 2, 1, 3))
    if pl["staircase"]:
        assert np.array_equal(pl["vpos"], invc[:nv])

    # ---- the two lane-ELL tables of G ----------------------------------------------------------------------------------------------
    for key, NL, A in (("eg", TH, Gd), ("et", TH - 64, Gd.T)):
        M, hits = ell_expand(pl, key, NL, tt, A.shape[0], A.shape[1])
        assert np.array_equal(hits, (A != 0).astype(np.int64)) and np.array_equal(M, A)
    assert pl["nell"] == max(pl["eg.VL"], pl["et.VL"])

    # ---- Gram item plan, super-step masks ------------------------------------------------------------------------------------------
    S = (Kc + 3) // 4
    nzpatch = Gpad.reshape(Kc + 1, 4, Tz + 1, 4).any(axis=(1, 3))             # [patch row, tile column]
    sstep = np.zeros((S, Tz + 1), dtype=bool)
    for s in range(S):
        sstep[s] = nzpatch[4 * s:4 * s + 4].any(axis=0)
    klist, items, item_ptr, smask = pl["klist"], pl["items"], pl["item_ptr"], pl["smask"]
    assert pl["nquads"] == sum(I // 4 + 1 for I in range(Tz))                  # tile row I holds quads 0 .. I // 4
    if tt:                                                                    # the blocked Gram reads none of them: not built
        assert len(klist) == len(items) == len(item_ptr) == len(smask) == 0
    else:
        assert ((klist >= 0) & (klist <= Kc)).all()
        quads = []
        for it in items:
            IB = it["I0"] // 4
            assert it["I0"] % 4 == 0 and it["nq"] >= 1
            lst = klist[it["kptr"]:it["kptr"] + it["klen"]]
            want = np.nonzero(nzpatch[:Kc, 4 * IB:min(4 * IB + 4, Tz)].any(axis=1))[0]
            assert np.array_equal(lst, want)                                       # in the list iff a non-zero in the block, all < Kc
            assert (klist[it["kptr"] + it["klen"]:it["kptr"] + it["klen"] + 8] == Kc).all() and it["kptr"] + it["klen"] + 8 <= len(klist)
            quads += [(IB, q) for q in range(it["q0"], it["q0"] + it["nq"])]
        assert sorted(quads) == [(IB, q) for IB in range((Tz + 3) // 4) for q in range(IB + 1)]      # every quad of every tile row once
        assert sum(min(4, Tz - 4 * IB) for IB, _ in quads) == pl["nquads"]
        assert len(item_ptr) == NW + 1 and item_ptr[0] == 0 and item_ptr[-1] == len(items) and (np.diff(item_ptr) >= 0).all()
        assert len(smask) == S + 1 and smask[S] == 0
        if Tz <= 31:
            assert [int(x) for x in smask[:S]] == [sum(1 << I for I in range(Tz) if sstep[s, I]) for s in range(S)]

    # ---- kernel class, LDS ---------------------------------------------------------------------------------------------------------
    assert pl["lds_bytes"] * pl["wgs_per_cu"] <= LDS_MAX and pl["wgs_per_cu"] >= 1
    if tt:
        assert pl["nklist"] == 2 and pl["TS"] in (16, 17) and pl["ntile"] == Tz * (Tz + 1) // 2 and pl["hsize"] == pl["ntile"] * pl["TS"]
        assert pl["lds_bytes"] == 8 * shim.lds_doubles(pl["hsize"], 1, Tz, nzp, mip, 2, ntheta, 0, pl["ntube"], pl["nell"], 0)
        cmax = np.array([np.nonzero(sstep[s])[0].max() if sstep[s].any() else -1 for s in range(S)])
        if pl["staircase"]:
            assert (np.diff(cmax) >= 0).all()
        U, units, uptr = pl["gu"], pl["gunits"], pl["gunit_ptr"]
        assert 1 <= U <= shim.layout_const(b"TZ_TT_GU1" if pl["wgs_per_cu"] == 1 else b"TZ_TT_GU2")
        nr = -(-Tz // U)
        assert sorted((int(u["ib"]), int(u["jb"])) for u in units) == [(a * U, b * U) for a in range(nr) for b in range(a + 1)]
        assert len(uptr) == NW + 1 and uptr[0] == 0 and uptr[-1] == len(units) and (np.diff(uptr) >= 0).all()
        for u in units:
            touching = np.nonzero(cmax >= u["ib"])[0]
            assert u["s0"] == (touching.min() if len(touching) else S)
            assert not sstep[:u["s0"], u["ib"]:].any()                       # nothing of the row range before s0
    else:
        assert pl["nklist"] == max(len(klist), S + 1) and pl["hsize"] == pl["nquads"] * shim.layout_const(b"TZ_QSTR")
        assert pl["lds_bytes"] == 8 * shim.lds_doubles(pl["hsize"], 0, Tz, nzp, mip, pl["nklist"], ntheta, int(pl["ksplit"]), pl["ntube"], pl["nell"], 1)
        assert len(pl["gunits"]) == 0

    # ---- affine maps, row maps, shift maps, recovery -------------------------------------------------------------------------------
    for key, Mt, c0, perm in (("q", args["Qt"], args["q0"], permc), ("h", args["Ht"], args["h0"], permr), ("par", args["Part"], args["par0"], None)):
        Mt = np.atleast_2d(np.asarray(Mt, float)); c0 = np.asarray(c0, float)
        rows = len(c0)
        perm = np.arange(rows) if perm is None else perm
        assert pl[key + ".rows"] == rows
        assert np.array_equal(map_expand(pl, key, ntheta), Mt[perm] if Mt.size else np.zeros((rows, ntheta)))
        assert np.array_equal(pl[key + ".c0"], c0[perm])
    assert np.array_equal(pl["row_of"], np.asarray(args["row_of"])[permr]) and np.array_equal(pl["act_scale"], np.asarray(args["act_scale"], float)[permr])
    sv, sr = np.asarray(args["shift_var"]), np.asarray(args["shift_row"])
    assert np.array_equal(pl["shift_var"], invc[sv[permc]]) and np.array_equal(pl["shift_row"], invr[sr[permr]])
    assert ((pl["shift_var"] >= 0) & (pl["shift_var"] < nz)).all() and ((pl["shift_row"] >= 0) & (pl["shift_row"] < mi)).all()
    assert np.array_equal(pl["shift_xs"], np.asarray(args["shift_xscale"], float)[permc])
    assert np.array_equal(pl["shift_ls"], np.asarray(args["shift_lscale"], float)[permr])
    if args.get("rec_y") is not None:
        assert np.array_equal(pl["recy"].reshape(nv, nz), np.asarray(args["rec_y"], float).reshape(nv, nz)[:, permc])
        assert np.array_equal(pl["rec0"], np.asarray(args["rec_c0"], float).ravel()) and np.array_equal(pl["recx"], np.asarray(args["rec_x0"], float).ravel())
        assert not pl["lean_epilogue"]
    else:
        assert len(pl["recy"]) == len(pl["rec0"]) == len(pl["recx"]) == 0
        Gam1 = np.asarray(args["Gam"], float).reshape((N + 1) * n, nv)[n:2 * n]
        assert bool(pl["lean_epilogue"]) == (not Gam1[:, m:].any())
    assert bool(pl["fused"]) == (max(int(args["pmax"]), 1) * n <= pl["hsize"])

    # ---- tube tables (floating point: the same sums, possibly in another order) ----------------------------------------------------
    ckp, T = tube_reference(args)
    np.testing.assert_allclose(pl["CKpow"].reshape(ckp.shape), ckp, rtol=1e-13, atol=0)
    np.testing.assert_allclose(pl["Ttube"].reshape(T.shape), T, rtol=1e-13, atol=0)


def _flag_sets(pl):
    if pl["tt"]:
        return [native.TZ_PLAN_NO_STAIRCASE]
    return [native.TZ_PLAN_ITEM_GRAM] if pl["ksplit"] else []


@pytest.mark.parametrize("case", sorted(common.CASES))
def test_plan_tables_of_every_case(shim, case):
    args = case_args(case)
    rc, msg, pl = build_plan(shim, args)
    assert rc == 0, msg
    check_plan(shim, args, 0, pl)
    for flags in _flag_sets(pl):                      # the flag that applies to the case's class
        rc, msg, pf = build_plan(shim, args, flags)
        assert rc == 0, msg
        check_plan(shim, args, flags, pf)
    rc, msg, pu = build_plan(shim, args, native.TZ_PLAN_UNFUSED)
    assert rc == 0 and not pu["fused"]


def test_case_classes_are_the_ones_the_cases_were_chosen_for(shim):
    """The sizes of tests/common.CASES reach every branch of the planner."""
    cls = {}
    for case in ("di_n2", "di_n20", "di_n20_k1", "di2in_n10_k1", "di_n40", "di_n80", "di_n10_eq"):
        rc, msg, pl = build_plan(shim, case_args(case))
        assert rc == 0, msg
        cls[case] = pl
    assert cls["di_n2"]["ksplit"] and cls["di_n20"]["ksplit"] and not cls["di_n20"]["tt"]
    assert not cls["di_n20_k1"]["ksplit"] and not cls["di_n20_k1"]["tt"] and cls["di_n20_k1"]["maxr"] == 2 and cls["di2in_n10_k1"]["maxr"] == 1
    assert cls["di_n40"]["tt"] and cls["di_n40"]["ncg"] == 2 and cls["di_n80"]["tt"] and cls["di_n80"]["ncg"] == 3 and cls["di_n80"]["maxr"] == 5
    assert len(cls["di_n10_eq"]["recy"]) > 0


def synthetic_args(nz, mi, N, seed=3):
    """A dense-ish description of a given size (n = 2, m = 1): what the planner reads, with no controller behind it."""
    rng = np.random.default_rng(seed)
    n, m = 2, 1
    ntheta = 2 * n + N * (2 * n + m)
    G = rng.standard_normal((mi, nz)) * (rng.random((mi, nz)) < 0.2)
    return dict(n=n, m=m, N=N, P=np.eye(nz), G=G, q0=np.zeros(nz), Qt=np.zeros((nz, ntheta)), h0=np.ones(mi), Ht=np.zeros((mi, ntheta)),
                par0=np.zeros(0), Part=np.zeros((0, ntheta)), par_lo=np.zeros(0), par_hi=np.zeros(0), cost_scale=1.0, r0=0.0, r1=np.zeros(n),
                R2=np.zeros((n, n)), Dz=np.ones(nz), Phi=np.zeros(((N + 1) * n, n)), Gam=np.zeros(((N + 1) * n, N * m)), nc_rows=mi,
                row_of=np.arange(mi), act_scale=np.ones(mi), CK=0.5 * np.eye(n), DK=0.1 * np.ones((n, n)), K=np.ones((m, n)), pmax=1,
                absCKpow=np.eye(n)[None], absKCKpow=np.ones((1, m, n)), power=np.zeros(N, dtype=np.int32))


def test_lds_refusal_names_the_bytes(shim):
    """198 variables: the factor alone is 1275 tiles of 16 doubles (163 200 bytes) -- with the vectors, more than the 160 KiB of a CU."""
    args = synthetic_args(198, 400, 100)
    rc, msg, _ = build_plan(shim, args)
    assert rc == -3, (rc, msg)                                            # TZ_ERR_UNSUPPORTED
    import re
    mt = re.fullmatch(r"not supported: the problem needs (\d+) bytes of LDS per workgroup \(nz=198, mi=400\); limit is 160 KiB", msg)
    assert mt and int(mt.group(1)) > LDS_MAX, msg
    rc, msg, pl = build_plan(shim, synthetic_args(150, 400, 100))          # the same description, smaller: placed
    assert rc == 0, msg
    assert pl["tt"] and 0 < pl["lds_bytes"] * pl["wgs_per_cu"] <= LDS_MAX


def test_bad_descriptions_keep_their_messages(shim):
    args = synthetic_args(20, 40, 5)
    assert build_plan(shim, args, 2)[:2] == (-1, "plan_flags 0x2: unknown bits 0x2")
    assert build_plan(shim, dict(args, row_of=np.full(40, 40)))[:2] == (-1, "row_of[0] out of range")
    bad = dict(args, shift_var=np.full(20, 20), shift_row=np.arange(40), shift_xscale=np.ones(20), shift_lscale=np.ones(40))
    assert build_plan(shim, bad)[:2] == (-1, "shift_var[0] out of range")
    assert build_plan(shim, synthetic_args(257, 40, 5))[0] == -3


# ---- generator stack --------------------------------------------------------------------------------------------------------------

def _stack(case, N, k0, repeat=1):
    from tzddpc_amd.genstack import build_stack
    ctl, _, (_, _, zon) = common.identified_qp(case)
    st = build_stack(ctl.MdataK, ctl.Mdelta, ctl.theta.K, zon.W, ctl.dim_x, ctl.dim_u, N, k0, nseg=N)
    if repeat > 1:                                      # the generators of the last tube `repeat` times over: chunks get cut
        a = int(st.seg_ptr[-2])
        st.src = np.concatenate([st.src[:a]] + [st.src[a:]] * repeat)
        st.m0 = np.concatenate([st.m0[:a]] + [st.m0[a:]] * repeat); st.M = np.concatenate([st.M[:a]] + [st.M[a:]] * repeat)
        st.seg_ptr = st.seg_ptr.copy(); st.seg_ptr[-1] = len(st.src)
    return st


@pytest.mark.parametrize("case,N,k0,repeat", [("di_n5", 4, None, 1), ("di2in_n10", 3, 1, 1), ("di_n5", 3, None, 400)])
def test_genstack_plan(shim, case, N, k0, repeat):
    st = _stack(case, N, k0, repeat)
    d, keep = native.GenStack.desc(st)
    rc = shim.genstack_build(C.byref(d))
    assert rc == 0, shim.plan_error()
    g = _fetch(shim.genstack_scalar, shim.genstack_table, GS_SCALARS, GS_TABLES)
    n, m = st.n, st.m
    p, rec, Gn = n + m, n * (1 + n + m), int(st.seg_ptr[-1])
    CH = shim.layout_const(b"TZ_GS_CHUNK")
    assert g["rec"] == rec and g["G"] == Gn and bool(g["have_cZ"]) == bool(np.any(st.cZ))
    lit = np.concatenate([st.m0.reshape(Gn, n), st.M.reshape(Gn, n * p)], axis=1)
    assert np.array_equal(g["lit"].reshape(Gn, rec), lit)
    srt = g["srt"].reshape(Gn, rec)
    assert sorted(r.tobytes() for r in srt) == sorted(r.tobytes() for r in lit)          # a permutation of the literal records
    chunks, scp = g["chunks"][:g["nchunk"]], g["seg_chunk_ptr"]
    assert len(g["chunks"]) == max(g["nchunk"], 1) and len(scp) == st.nseg + 1 and scp[0] == 0 and scp[-1] == g["nchunk"]
    pos = 0
    src_sorted = np.full(Gn, -9)
    for k in range(st.nseg):
        key = sorted(zip(st.src[st.seg_ptr[k]:st.seg_ptr[k + 1]], range(int(st.seg_ptr[k]), int(st.seg_ptr[k + 1]))))
        src_sorted[int(st.seg_ptr[k]):int(st.seg_ptr[k + 1])] = [s for s, _ in key]
        assert np.array_equal(srt[int(st.seg_ptr[k]):int(st.seg_ptr[k + 1])], lit[[i for _, i in key]])     # stable sort by source inside a tube
        for ch in chunks[scp[k]:scp[k + 1]]:
            assert ch["seg"] == k and ch["a"] == pos and 0 < ch["b"] - ch["a"] <= CH          # contiguous, bounded
            assert (src_sorted[ch["a"]:ch["b"]] == ch["src"]).all()                            # constant in (tube, source)
            pos = int(ch["b"])
        assert pos == st.seg_ptr[k + 1]
    if repeat > 1:
        assert (chunks["b"] - chunks["a"] == CH).any() and g["nchunk"] > len(set(zip(chunks["seg"], chunks["src"])))     # a boundary occurred
    assert bool(g["mfma"]) == (3 <= p <= 7) and g["rows_mf"] == (n if m == 1 else p)
    # un-laying-out the matrix-core copies: [M; K M], [m0; K m0] of the sorted stack, zero generators only as padding
    K = np.atleast_2d(np.asarray(st.K, float))
    m0s, Ms = srt[:, :n], srt[:, n:].reshape(Gn, n, p)
    KM = np.zeros((Gn, m, p)); Km0 = np.zeros((Gn, m))
    for i in range(n):                                      # the short sums, in the planner's order
        KM += K[None, :, i, None] * Ms[:, None, i, :]; Km0 += K[None, :, i] * m0s[:, i, None]
    ext = np.concatenate([Ms, KM], axis=1); ext0 = np.concatenate([m0s, Km0], axis=1)
    cm = g["chunks_m"]
    assert len(cm) == g["nchunk"]
    if g["rows_mf"] == p:
        assert len(g["mfn"]) == 0
    for RW, mf in [(p, g["mf"])] + ([(g["rows_mf"], g["mfn"])] if g["rows_mf"] != p else []):      # the narrow copy: the first n rows
        GD = 4 * RW * (p + 1)
        grp = mf.reshape(-1, GD)
        assert len(grp) == int(cm["b"].sum())
        q = 0
        for ch, c4 in zip(chunks, cm):
            ng = ch["b"] - ch["a"]
            assert (c4["seg"], c4["src"], c4["a"], c4["b"]) == (ch["seg"], ch["src"], q, (ng + 3) // 4)
            blk = grp[q:q + c4["b"]]
            Mg = blk[:, :4 * RW * p].reshape(-1, RW, 4, p).transpose(0, 2, 1, 3).reshape(-1, RW, p)      # [generator][c][k]
            m0g = blk[:, 4 * RW * p:].reshape(-1, RW, 4).transpose(0, 2, 1).reshape(-1, RW)
            assert np.array_equal(Mg[:ng, :n], ext[ch["a"]:ch["b"], :n]) and np.array_equal(m0g[:ng, :n], ext0[ch["a"]:ch["b"], :n])
            np.testing.assert_allclose(Mg[:ng, n:], ext[ch["a"]:ch["b"], n:RW], rtol=1e-15, atol=0)
            np.testing.assert_allclose(m0g[:ng, n:], ext0[ch["a"]:ch["b"], n:RW], rtol=1e-15, atol=0)
            assert not Mg[ng:].any() and not m0g[ng:].any()
            q += int(c4["b"])
