"""The host-side planning queries of csrc/conv_mfma.hip answer exactly what tests/golden/conv_plan.npz recorded: which shapes run the
persistent / Winograd kernels, how many statistics tiles a launch writes, which fused forms a shape supports.  No device is needed
(the queries launch nothing), no tolerance, every entry of the grid, under both settings of SMSUT_WINOGRAD (one child process each:
the library reads the variable once)."""
import importlib.util
import os

import numpy as np
import pytest

import __graft_entry__ as ge

GOLDEN = os.path.join(ge.ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_conv_plan_golden", os.path.join(GOLDEN, "make_conv_plan_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    ge.build()
    assert os.path.exists(ge.LIB)
    return np.load(os.path.join(GOLDEN, "conv_plan.npz"), allow_pickle=False)


def test_fixture_describes_the_generators_grid(golden):
    assert [str(c) for c in golden["columns"]] == gen.COLUMNS
    assert golden["shapes"].tolist() == [list(s) for s in gen.shapes()]
    assert len(gen.shapes()) == len(gen.NS) * len(gen.PLANES) * len(gen.CHANNELS) ** 2


@pytest.mark.parametrize("setting", sorted(gen.SETTINGS))
def test_planning_queries_answer_as_recorded(golden, setting):
    want = golden[f"plan_{setting}"]
    got = gen.record(setting, ge.LIB)
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(gen.shapes()[i], gen.COLUMNS[j], int(got[i, j]), int(want[i, j])) for i, j in bad[:10]]
