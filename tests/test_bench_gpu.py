"""bench.py's roofline leg times a kernel the timed step really launches (r03's leg called
``smsut_conv2d_fwd_mfma_stats_cat``, which the fp32 iteration had not launched since the shortcut fusion)."""
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_roofline_legs_are_calls_of_the_recorded_iteration(monkeypatch):
    """One eager uganConsis iteration at the bench's geometry (8 + 8 slices @256^2 is what the line is quoted on; 2 + 2 here, the
    entry points and every argument but the batch are the same) recorded through ``profiling.record_step``: both roofline legs'
    (entry point, integer / float arguments) are among its C-ABI calls, and the dominant one launches the register-row kernel."""
    import bench
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg, profiling, _hip as H
    from smsut_amd.trainer.uganConsisTrainer import UGANConsisTrainer
    from smsut_amd.misc.synthetic import SyntheticSliceLoader
    monkeypatch.setenv("SMSUT_GRAPH", "0")
    old = (cfg.input_size, cfg.batch_size)
    B = 4
    try:
        cfg.input_size, cfg.batch_size = 256, B // 2
        tr = UGANConsisTrainer("train", types.SimpleNamespace(fold=0, expr_name=None, write_env=False))
        tr.net.train(); tr.D.train()
        tr.iter, tr.epoch = 1000, 100
        (x1, y1, m1, _), (x2, _, m2, _) = (next(iter(SyntheticSliceLoader(B // 2, device="cuda", labeled=True, n_batches=2))),
                                           next(iter(SyntheticSliceLoader(B // 2, device="cuda", labeled=False, n_batches=2))))
        batch = (torch.cat([x1, x2], 0), y1, torch.cat([m1, m2], 0))
        tr.train_iteration(*batch)
        rec = profiling.record_step(lambda: tr.train_iteration(*batch))
    finally:
        cfg.input_size, cfg.batch_size = old
    # the one-launch SGD step ran in the recorded iteration but is NOT in the recording: its arguments are device-side pointer tables that
    # are only valid at the moment of the call (a replay of a stale one faulted in bench.py's byte census, r05) ...
    assert tr.optimizer._smsut_stepper.enabled and "smsut_sgd_momentum_multi" in profiling._NO_REPLAY
    assert not any(name in profiling._NO_REPLAY for name, _ in rec)
    rows = profiling.replay(rec, reps=1)                                              # ... so the recording replays cleanly
    assert len(rows) > 50
    keys = set()
    for name, conv in rec:
        sig = H.SIGNATURES[name].replace(" ", "")
        keys.add((name, tuple(round(a, 6) if isinstance(a, float) else a for c, a in zip(sig, conv) if c in "ilfd")))
    name, args = bench.dominant_wgrad_call(B, 256)
    assert (name, tuple(round(a, 6) if isinstance(a, float) else a for a in args)) in keys, sorted(k for k in keys if k[0] == name)
    # roofline_fwd: decoder level 1, conv1 + shortcut -- since r05 with its InstanceNorm statistics finalised inside the launch
    assert ("smsut_conv2d_fwd_mfma_stats_sc_fin", (1e-05, B, 256, 256, 32, 16)) in keys
    assert not any(k[0] == "smsut_conv2d_fwd_mfma_stats_cat" for k in keys)           # (what r03's leg timed: not a call of the step)
    r = bench.measure_dominant_wgrad(torch.device("cuda"), B, 256)
    assert r["entry_point"] == name and r["avg_launch_ms"] > 0 and r["call_ms_with_reduction"] >= r["avg_launch_ms"]
    f = bench.measure_dominant_conv(torch.device("cuda"), B, 256)
    assert f["entry_point"] == "smsut_conv2d_fwd_mfma_stats_sc_fin" and f["executed_mfma_tflops"] <= f["achieved"]


def _plain_run(out_dir):
    import json
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--per-gpu-batch", "4",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_is_the_headline_and_dumps_its_last_step(tmp_path):
    """A plain ``bench.py`` run times exactly ``--steps`` steps and prints the headline without the side legs of ``--full``;
    ``--dump-outputs`` writes the last timed step's loss scalars and the trained weights, the same ones for the same arguments."""
    import numpy as np
    lines = [_plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")]
    for line in lines:
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
        assert line["metric"].startswith("slices/sec uganConsisTrainer step") and line["unit"] == "slices/s" and line["dtype"] == "f32"
        assert abs(line["value"] - 4 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"] + 0.01
        assert not {"end_to_end", "roofline", "unet_step", "config5", "dist_overhead", "cpu_baseline"} & set(line)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert "loss_scalars.npy" in names and any(n.startswith("net.") for n in names) and any(n.startswith("D.") for n in names)
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 64e6
    scal = np.load(tmp_path / "a" / "loss_scalars.npy")
    assert scal.dtype == np.float32 and scal.shape == (10,) and np.isfinite(scal).all()
    np.testing.assert_allclose(scal, lines[0]["last_step_scalars"], rtol=1e-4, atol=1e-5)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape, n
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=n)
