"""CPU: what a plain `bench.py` run measures and what only `--full` adds.  The worker runs with every leg replaced by a
stand-in that records its call, so its control flow is checked without a GPU: a plain run times the main line and
prints the line; the sampling legs, per-kernel rooflines, extras and CPU baselines run under --full only."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("sample", "sample_bf16_split_experiment", "step_profile", "roofline_hbm", "extra")


@pytest.fixture
def bench_run(monkeypatch, capsys):
    """run(*argv) -> (the JSON line as a dict, the legs called in order)."""
    sys.path.insert(0, ROOT)
    import bench
    from sdeflow_light_amd import ops
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MSGM_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda dev: None)
    monkeypatch.setattr(ops, "lib", lambda: None)
    monkeypatch.setattr(bench, "free_gpu", lambda: None)
    calls = []
    ws = {"algorithmic_tflops_per_gpu": 80.0, "frac_of_f32_mfma_peak": 0.5, "flop_per_step": 1.0, "note": ""}

    def train(workload, a, rank, world, dev, main_line=False):
        calls.append(("train", workload, main_line))
        return ({"value": 9.0, "ms_per_step": 111.0, "blocks_s": [1.1], "final_loss": 1.0, "global_batch": 256,
                 "graph": True, "whole_step": ws}, object(), 12288)

    def sample(gen, d, a, rank, world, dev, main_line=False):
        calls.append(("sample", os.environ.get("MSGM_SAMPLER_BF16X3"), main_line))
        return {"sample_steps_per_s": 2.0, "ms_per_sample_step": 500.0, "rows_per_gpu": 8192, "sampler_finite": True,
                "workload": "c5", "algorithmic_tflops_per_gpu": 90.0, "frac_of_f32_mfma_peak": 0.6}

    def mlp(a, rank, world, dev, steps=200, sample_steps=200, main_line=False, full=True):
        calls.append(("mlp", main_line, full))
        r = {"workload": "c2", "train_steps_per_s": 3000.0, "ms_per_step": 0.3, "final_loss": 1.0}
        if full:
            r.update(sample_steps_per_s=25000.0, roofline={"kernel": "k_mlp"})
        return r

    def profile(dev, Bp):
        calls.append(("step_profile",))
        return [{"family": "3x3 conv (k_conv_wino)", "bound": "mfma", "achieved": 140.0, "frac": 0.9, "ms": 21.0,
                 "calls": 72, "flop": 1.0, "share_of_step": 0.2}], 110.0

    monkeypatch.setattr(bench, "build_unet", lambda workload, dev: (object(), 12288))
    monkeypatch.setattr(bench, "leg_train_unet", train)
    monkeypatch.setattr(bench, "leg_sample_unet", sample)
    monkeypatch.setattr(bench, "leg_mlp", mlp)
    monkeypatch.setattr(bench, "leg_step_profile", profile)
    monkeypatch.setattr(bench, "hbm_rooflines", lambda dev: calls.append(("hbm_rooflines",)) or [])
    monkeypatch.setattr(bench, "leg_msgm", lambda dev: calls.append(("msgm",)) or {})
    monkeypatch.setattr(bench, "cpu_baseline_unet", lambda w: calls.append(("cpu_baseline", w)) or {})
    monkeypatch.setattr(bench, "cpu_baseline_mlp", lambda: calls.append(("cpu_baseline", "c2")) or {})

    def run(*argv):
        capsys.readouterr()
        bench.worker(bench.parse_args(list(argv)))
        line = capsys.readouterr().out.strip().splitlines()[-1]
        return json.loads(line), calls
    return run


def test_full_is_off_by_default():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


@pytest.mark.parametrize("workload", ["c2", "c3", "c4", "c5"])
def test_plain_run_times_the_main_line_only(bench_run, workload):
    out, calls = bench_run("--workload", workload, "--steps", "4", "--warmup", "2")
    main = {"c2": ("mlp", True, False), "c3": ("train", "c3", True), "c4": ("train", "c4", True),
            "c5": ("sample", None, True)}[workload]
    assert calls == [main]
    assert all(k in out for k in HEADLINE), out
    assert not any(k in out for k in FULL_ONLY), out
    assert out["cpu_baseline"] is None
    if workload in ("c3", "c4"):
        assert out["value"] == 9.0 and out["ms_per_step"] == 111.0 and out["steps"] == 4 and out["warmup"] == 2
        assert out["roofline"]["kernel"] == "whole step (all kernels)" and out["roofline"]["achieved"] == 80.0


def test_full_run_adds_every_other_leg(bench_run):
    out, calls = bench_run("--full", "--steps", "4", "--warmup", "2")
    assert calls == [("train", "c4", True), ("sample", None, False), ("sample", "1", False), ("step_profile",),
                     ("hbm_rooflines",), ("mlp", False, True), ("train", "c3", False), ("msgm",), ("cpu_baseline", "c4")]
    assert all(k in out for k in HEADLINE + FULL_ONLY), out
    assert out["value"] == 9.0 and out["ms_per_step"] == 111.0
    assert out["roofline"]["kernel"] == "3x3 conv (k_conv_wino)"


def test_full_run_of_c2_keeps_its_sampler_roofline_and_cpu_baseline(bench_run):
    out, calls = bench_run("--workload", "c2", "--full")
    assert calls == [("mlp", True, True), ("cpu_baseline", "c2")]
    assert out["sample_steps_per_s"] == 25000.0 and out["roofline"] == {"kernel": "k_mlp"} and out["cpu_baseline"] == {}
