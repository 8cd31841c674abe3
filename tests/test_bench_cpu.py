"""bench.py's host-side pieces: the command line and --dump-outputs (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_command_line_has_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         check=True).stdout
    for opt in ("--steps", "--warmup", "--gpus", "--full", "--dump-outputs"):
        assert opt in out, opt


def _outs():
    g = torch.Generator().manual_seed(0)
    post = {"class_scores": torch.randn(2, 6, 1, 128, 8, generator=g).bfloat16(), "moods": [["model happy"] * 6] * 2}
    stats = {"labels": torch.tensor(0.25), "cardinality": torch.tensor([3, 4])}
    od = ([torch.rand(7, 4, generator=g, dtype=torch.float64)], [torch.ones(5, dtype=torch.bool)],
          torch.randn((1 << 20) + 3, generator=g), 11)
    return post, torch.tensor(1.5), stats, od


def test_dump_outputs_names_dtypes_and_samples(tmp_path):
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(1100, 1000), torch.nn.Linear(1000, 2))
    model[0].weight.grad = torch.full_like(model[0].weight, 2.0)       # model[0].bias and model[1] without a gradient
    outs = _outs()
    bench.dump_outputs(str(tmp_path / "a"), outs, model)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"post.class_scores", "loss", "stats.labels", "stats.cardinality", "od.0.0", "od.1.0",
                        "od.2.sample", "od.3", "grads_sample"}
    np.testing.assert_array_equal(got["post.class_scores"], outs[0]["class_scores"].float().numpy())
    assert got["post.class_scores"].dtype == np.float32 and got["loss"].dtype == np.float32 and got["loss"] == 1.5
    assert got["stats.cardinality"].dtype == np.float64 and list(got["stats.cardinality"]) == [3.0, 4.0]
    assert got["od.0.0"].dtype == np.float64 and got["od.1.0"].dtype == np.float64 and float(got["od.3"]) == 11.0
    assert got["od.2.sample"].shape == (bench.DUMP_SAMPLE,)
    assert np.isin(got["od.2.sample"], outs[3][2].numpy()).all()
    assert got["grads_sample"].shape == (bench.DUMP_SAMPLE,)
    assert set(np.unique(got["grads_sample"])) == {0.0, 2.0}
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT
    # the same outputs -> the same files (the samples are fixed)
    bench.dump_outputs(str(tmp_path / "b"), outs, model)
    for name, a in got.items():
        np.testing.assert_array_equal(np.load(tmp_path / "b" / (name + ".npy")), a)


def test_restore_state_puts_parameters_and_moments_back():
    import bench
    from types import SimpleNamespace
    p = torch.nn.Parameter(torch.arange(6.0))
    opt = SimpleNamespace(param_groups=[{"params": [p]}], state={}, _step_no=0, _dev_step=torch.zeros(1, dtype=torch.float64))
    snap = bench.snapshot_state(opt)
    with torch.no_grad():                     # what training steps do: new values, moments, step count
        p.add_(1.0)
    opt.state[p] = {"exp_avg": torch.ones(6), "exp_avg_sq": torch.ones(6)}
    opt._step_no = 7
    opt._dev_step.fill_(7.0)
    ptr = p.data_ptr()
    bench.restore_state(opt, snap)
    assert p.data_ptr() == ptr and torch.equal(p.detach(), torch.arange(6.0))
    assert not opt.state[p]["exp_avg"].any() and not opt.state[p]["exp_avg_sq"].any()
    assert opt._step_no == 0 and float(opt._dev_step) == 0.0
