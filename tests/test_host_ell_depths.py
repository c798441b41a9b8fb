"""CPU: the depths (records per virtual lane) of the two lane-ELL tables of G for the cases tests/test_gpu_ell_fetch.py drives.  The
windowed walk of tz_ipm.hip.h (tz_ell_fetch / tz_ell_apply) takes another path for a depth below the window, a whole number of
quads, each tail length, and a depth of more than one window: the cases are pinned here so that a change of the planner cannot
silently empty that coverage."""
import os
import re

import pytest

from tests.test_host_plan import build_plan, case_args, shim      # noqa: F401  (shim: the planner compiled for the host)

HERE = os.path.dirname(os.path.abspath(__file__))
DEPTHS = {"di_n2": (1, 1), "di_n10": (4, 5), "pulley_n10": (4, 10), "di2in_n10_k1": (5, 12), "di_n20_k2": (4, 18), "di_n20": (9, 20),
          "di2in_n10": (3, 8)}         # (the only quad-class case of tests/common.CASES with a tail of three entries)


def window():
    src = open(os.path.join(HERE, "..", "tzddpc_amd", "csrc", "tz_ipm.hip.h")).read()
    return int(re.search(r"^#define TZ_ELL_D (\d+)\s*$", src, re.M).group(1))


@pytest.mark.parametrize("case", sorted(DEPTHS))
def test_depths_of_the_walk_cases(shim, case):        # noqa: F811
    rc, msg, pl = build_plan(shim, case_args(case))
    assert rc == 0, msg
    assert not pl["tt"]                                # 16-byte records: the class the windowed walk serves
    assert (pl["eg.L"], pl["et.L"]) == DEPTHS[case]


def test_depths_reach_every_path_of_the_window():
    D = window()
    assert D % 4 == 0 and 4 <= D <= 20                  # quads never straddle a window; beyond 20 the cases above no longer exceed it
    depths = {d for pair in DEPTHS.values() for d in pair}
    assert any(d < D for d in depths)
    assert any(d % 4 == 0 for d in depths)
    assert {1, 2, 3} <= {d % 4 for d in depths}
    assert any(d > D for d in depths)
    assert any(d > 2 * D for d in depths) or D > 8      # more windows than are in flight at once
