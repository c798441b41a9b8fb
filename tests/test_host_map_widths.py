"""CPU: the widths (entries per row) of the three parameter maps q, h and par for the cases tests/test_gpu_step_prologue.py drives.
The fused prologue of tz_ipm_kernel fetches the rows a thread owns in one round trip when every map has at most TZ_MAP_W4 entries
per row (csr_fetch4 / csr_apply4, tz_kernels.hip.h) and evaluates wider maps row by row (csr_row, up to TZ_ELL_REG records in
registers, a tail loop beyond).  The facts that split relies on are pinned here, so that a change of the builder or of the planner
cannot silently move a case to another path or empty the coverage of one."""
import os
import re

import numpy as np
import pytest

from tests.test_host_plan import build_plan, case_args, shim      # noqa: F401  (shim: the planner compiled for the host)

HERE = os.path.dirname(os.path.abspath(__file__))
# case: (non-zeros per row of q, h, par; parameter rows)
WIDTHS = {"di_n2": ((2, 4, 3), 4), "di_n20": ((2, 4, 3), 4), "di2in_n10": ((2, 4, 3), 4), "pulley_n10": ((0, 6, 3), 8),
          "dim5_n20": ((0, 7, 3), 12)}


def _define(name):
    src = open(os.path.join(HERE, "..", "tzddpc_amd", "csrc", "tz_kernels.hip.h")).read()
    return int(re.search(r"^#define %s (\d+)\s*$" % name, src, re.M).group(1))


@pytest.fixture(scope="module")
def plans(shim):                                       # noqa: F811
    out = {}
    for case in WIDTHS:
        rc, msg, pl = build_plan(shim, case_args(case))
        assert rc == 0, msg
        out[case] = pl
    return out


@pytest.mark.parametrize("case", sorted(WIDTHS))
def test_map_widths_of_the_prologue_cases(plans, case):
    pl = plans[case]
    (wq, wh, wp), npar = WIDTHS[case]
    assert pl["par.rows"] == npar
    for key, width in (("q", wq), ("h", wh), ("par", wp)):
        rows, W, ent = pl[key + ".rows"], pl[key + ".W"], pl[key + ".ent"]
        assert rows >= 1 and len(ent) == W * rows
        nnz = (ent["val"].reshape(W, rows) != 0.0).sum(axis=0)
        assert nnz.max() == width, (key, nnz.max())
        assert W == max(width, 1)                      # the planner keeps at least one (padding) record per row
        pad = ent[ent["val"] == 0.0]
        assert not pad["off"].any() and not pad["pad"].any()          # every padded record is (0.0, offset 0)
        assert not np.signbit(pad["val"]).any()
        assert W <= _define("TZ_ELL_REG")              # no case enters the tail loop of csr_row


def test_widths_reach_both_paths(plans):
    W4, REG = _define("TZ_MAP_W4"), _define("TZ_ELL_REG")
    assert 1 <= W4 < REG
    narrow = [c for c, pl in plans.items() if max(pl["q.W"], pl["h.W"], pl["par.W"]) <= W4]
    wide = [c for c, pl in plans.items() if max(pl["q.W"], pl["h.W"], pl["par.W"]) > W4]
    assert {"di_n2", "di_n20", "di2in_n10"} <= set(narrow)             # one round trip for the three maps
    assert {"pulley_n10", "dim5_n20"} <= set(wide)                     # row by row
    assert any(plans[c]["h.W"] == W4 for c in narrow)                  # the widest map the narrow path takes: no slot re-read
    assert any(plans[c]["q.W"] < W4 for c in narrow)                   # ... and one with slots behind W (re-read, left out of the sum)
    assert any(plans[c]["maxr"] > 1 for c in wide)                     # more than one row of h per thread
