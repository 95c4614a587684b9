"""tests/golden/metrics.npz (test-phase metrics fixture): it loads, its designed cases say what they were built to say, and --
where scipy is installed -- its generator reproduces every committed array."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def fx(golden):
    return golden("metrics")


def counts(a):
    return np.bincount(a.ravel(), minlength=256)


def test_cleanup_cases_are_what_they_claim(fx):
    assert counts(fx["cc3_corner_chain"])[1] == 90                 # the corner-only chain falls apart under 18-connectivity
    assert counts(fx["cc3_edge_chain"])[1] == 102                  # the edge-connected chain joins the block
    assert counts(fx["ccs_diagonal_chain"])[2] == 204              # 8-connected in plane
    assert counts(fx["cc3_z_column"])[3] == 102 and counts(fx["ccs_z_column"])[3] == 101     # split per slice
    assert counts(fx["p_tenth"])[1] == 100 and counts(fx["cc3_tenth"])[1] == 90               # exactly F/10: dropped
    assert counts(fx["p_tenth"])[2] == 100 and counts(fx["cc3_tenth"])[2] == 100              # F/10 + 1: kept
    assert counts(fx["cc3_touching_classes"])[1] == 90 and counts(fx["cc3_touching_classes"])[2] == 16
    c = counts(fx["cc3_above_n_modal"])
    assert c[4] == 16 and c[5:].sum() == 0
    assert not fx["cc3_empty"].any()
    assert (fx["cc3_all_foreground"] == 1).all()
    for n in fx["names"]:
        assert fx[f"cc3_{n}"].dtype == np.uint8 and fx[f"cc3_{n}"].shape == fx[f"p_{n}"].shape
        assert fx[f"cc3_{n}"].max() <= 4


def test_surface_cases_are_what_they_claim(fx):
    st = fx["st_pair3"]
    assert st[0].tolist() == [0, 1, 1, 1, 3.0, 1, 3.0] and float(fx["pair3_assd"]) == 3.0
    af = fx["st_all_foreground"][0]                                # every voxel on an array face is border: 4x7x9 minus 2x5x7
    assert af[1] == 252 and af[3] == 252 - 2 * 5 * 7
    assert np.isnan(fx["st_empty"][:, 4]).all() and (fx["st_empty"][:, :4] == 0).all()
    for n in fx["names"]:
        st = fx[f"st_{n}"]
        assert st.shape == (4, 7)
        p, g = fx[f"p_{n}"], fx[f"g_{n}"]
        for lab in range(1, 5):
            assert st[lab - 1, 1] == np.count_nonzero(p == lab) and st[lab - 1, 2] == np.count_nonzero(g == lab)


def test_matrix_set_covers_every_modality_and_the_maxassd_rule(fx):
    keys = [str(k) for k in fx["gam_keys"]]
    assert {k.split("_")[0] for k in keys} == {"ct", "t1in", "t1out", "t2"}
    p = fx["gam_p_t1in_005"]
    assert not (p == 1).any() and not (p == 3).any()
    for m in ("gam_dc", "gam_hd", "gam_assd"):
        assert fx[m].shape == (5, 5) and np.isfinite(fx[m]).all()
    assert np.array_equal(fx["gam_dc"], fx["gam_hd"])                 # the reference's placeholder: t = s


def test_fixture_is_small():
    import os
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "metrics.npz")) < 300 * 1024


def test_generator_reproduces_fixture(fx):
    pytest.importorskip("scipy")
    import importlib.util
    import os
    from conftest import GOLDEN
    spec = importlib.util.spec_from_file_location("make_metrics_golden", os.path.join(GOLDEN, "make_metrics_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    data = gen.build()
    assert sorted(data) == sorted(fx.files)
    for k, v in data.items():
        np.testing.assert_array_equal(np.asarray(v), fx[k], err_msg=k)
