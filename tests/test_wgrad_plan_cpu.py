"""The weight-gradient planning queries of csrc/conv_mfma.hip answer exactly what tests/golden/wgrad_plan.npz recorded: which shapes
the fused-shortcut, fp16 and paired forms take and how many floats of split slabs each launch needs.  No device is needed (the
queries launch nothing and read no environment), no tolerance, every entry of the grid."""
import importlib.util
import os

import numpy as np
import pytest

import __graft_entry__ as ge

GOLDEN = os.path.join(ge.ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_wgrad_plan_golden", os.path.join(GOLDEN, "make_wgrad_plan_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    ge.build()
    assert os.path.exists(ge.LIB)
    return np.load(os.path.join(GOLDEN, "wgrad_plan.npz"), allow_pickle=False)


def test_fixture_describes_the_generators_grid(golden):
    assert [str(c) for c in golden["columns"]] == gen.COLUMNS
    assert golden["shapes"].tolist() == [list(s) for s in gen.shapes()]
    assert golden["plan"].dtype == np.int64 and golden["plan"].shape == (len(gen.shapes()), len(gen.COLUMNS))


def test_grid_reaches_every_family(golden):
    plan = golden["plan"]
    for name in gen.SUPPORTED:
        assert set(np.unique(plan[:, gen.COLUMNS.index(name)]).tolist()) == {0, 1}, name
    for name in gen.REJECTED:
        assert not plan[:, gen.COLUMNS.index(name)].any(), name


def test_planning_queries_answer_as_recorded(golden):
    want = golden["plan"]
    got = gen.answers(ge.LIB)
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(gen.shapes()[i], gen.COLUMNS[j], int(got[i, j]), int(want[i, j])) for i, j in bad[:10]]
