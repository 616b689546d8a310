"""CPU: what a plain ``bench.py`` run does besides its timed steps (nothing but the headline line) and what ``--full`` adds.  The
benchmark's ``main`` runs in a child process with the GPU work replaced by stubs that record their calls (no GPU here)."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONTRACT = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "elbo_iters_per_sec", "detail"}


def _run(tmp_path, *argv):
    calls = tmp_path / "calls.json"
    driver = tmp_path / "driver.py"
    driver.write_text(textwrap.dedent(f"""
        import atexit, json, sys
        sys.path.insert(0, {ROOT!r})
        import torch
        torch.cuda.device_count = lambda: 1
        torch.cuda.is_available = lambda: True
        torch.cuda.set_device = lambda device: None
        import bench
        calls = []
        atexit.register(lambda: open({str(calls)!r}, "w").write(json.dumps(calls)))

        def measure(workload, batch, args, device, distributed, world, dump_dir=None):
            calls.append(["measure", workload, batch, dump_dir])
            fields = {{"value": 1e4, "unit": "paths/s", "ms_per_step": 50.0, "elbo_iters_per_sec": 20.0,
                       "config": {{"workload": workload, "global_batch": batch, "parallelism": "dp1", "hip_graph": True}}}}
            if args.full:
                fields.update(sampled_paths_per_sec=1e5, roofline={{"frac": 0.2, "backward": {{}}}}, mfma_util={{"frac": 0.1}})
            return fields, ("problem", {{}})

        def recorder(name, result):
            def fn(*a, **k):
                calls.append([name])
                return None if result is None else dict(result)
            return fn
        bench.measure = measure
        bench.measure_pmc_traffic = recorder("pmc", None)
        bench.parity_gate = recorder("parity", {{"pass": True, "batch": 64}})
        bench.cpu_baseline = recorder("cpu_baseline", {{"value": 6.0, "unit": "paths/s", "cores": 16, "kind": "port",
                                                        "lv_seconds_per_micro_batch": 10.0}})
        sys.argv = ["bench.py"] + {list(argv)!r}
        bench.main()
    """))
    r = subprocess.run([sys.executable, str(driver)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), json.loads(calls.read_text())


def test_plain_run_times_the_step_and_prints_the_contract_fields_only(tmp_path):
    line, calls = _run(tmp_path, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", "out")
    assert calls == [["measure", "lv", 512, "out"]]
    assert set(line) == CONTRACT
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] == 50.0 and line["value"] == 1e4
    assert line["unit"] == "paths/s" and line["higher_is_better"] is True
    assert line["metric"] == "sampled-paths/sec + ELBO-iters/sec (value = global_batch * ELBO-iters/s)"
    assert line["dtype"] == "f32 (GRU/ELBO kernels) + bf16-autocast encoder"


def test_full_run_adds_the_pmc_passes_ou_parity_and_cpu_baseline(tmp_path):
    line, calls = _run(tmp_path, "--gpus", "1", "--steps", "3", "--warmup", "1", "--full")
    assert calls[0] == ["pmc"] and calls[1] == ["measure", "lv", 512, None] and calls[2] == ["measure", "ou", 128, None]
    assert [c[0] for c in calls[3:]] == ["parity", "parity", "cpu_baseline"]
    assert CONTRACT < set(line)
    assert line["parity"]["pass"] is True and line["cpu_baseline"]["value"] == 6.0 and line["roofline"]["frac"] == 0.2
    assert "ou" in line and line["ms_per_step"] == 50.0
