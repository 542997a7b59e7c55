"""bench.py's multi-GPU launch contract, on CPU (no GPU is touched):
``python bench.py --gpus N`` with no outer launcher starts N rank processes
itself (torch.distributed.run, rendezvous on 127.0.0.1) and a WORLD_SIZE that
disagrees with --gpus is refused, so a bench line can never report n_gpus
other than the ranks that ran (VERDICT r2 "Next round" item 2)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_launch_plan_single_and_outer_launcher():
    import bench
    assert bench.launch_plan(1, ["--gpus", "1"], {}) is None
    # launched by torch.distributed.run (the driver's N > 1 form): one rank
    assert bench.launch_plan(4, ["--gpus", "4"], {"WORLD_SIZE": "4"}) is None
    with pytest.raises(SystemExit):
        bench.launch_plan(8, ["--gpus", "8"], {"WORLD_SIZE": "1"})
    with pytest.raises(SystemExit):
        bench.launch_plan(1, [], {"WORLD_SIZE": "2"})


def test_self_launch_maps_ranks(tmp_path):
    """The command --gpus N builds starts N processes with RANK / LOCAL_RANK
    0..N-1 and WORLD_SIZE N on 127.0.0.1 (each rank later binds cuda:LOCAL_RANK):
    run here with a stand-in script in place of bench.py."""
    import bench
    cmd = bench.launch_plan(2, ["--gpus", "2", "--steps", "3"], {})
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "2"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "2", "--steps", "3"]
    probe = tmp_path / "probe.py"
    probe.write_text(
        "import json, os, sys\n"
        "r = int(os.environ['RANK'])\n"
        f"open(os.path.join({str(tmp_path)!r}, f'r{{r}}.json'), 'w').write(json.dumps(\n"
        "    {k: os.environ[k] for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR')}\n"
        "    | {'argv': sys.argv[1:]}))\n")
    i = cmd.index(os.path.abspath(bench.__file__))
    cmd = cmd[:i] + [str(probe)] + cmd[i + 1:]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    subprocess.run(cmd, check=True, env=env, timeout=120, capture_output=True)
    got = [json.loads((tmp_path / f"r{r}.json").read_text()) for r in range(2)]
    for r, g in enumerate(got):
        assert g["RANK"] == str(r) and g["LOCAL_RANK"] == str(r)
        assert g["WORLD_SIZE"] == "2" and g["MASTER_ADDR"] == "127.0.0.1"
        assert g["argv"] == ["--gpus", "2", "--steps", "3"]


def test_plain_run_is_lean_and_full_keeps_the_protocol():
    """A plain run times one window of --steps steps and skips the probe and
    the CPU baseline; --full restores the 3-window protocol with both, and
    the explicit switches still hold there."""
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.repeats) == (7, 2, 1)
    assert a.no_probe and a.no_cpu_baseline and a.dump_outputs is None
    f = bench.parse(["--full"])
    assert f.repeats == 3 and not f.no_probe and not f.no_cpu_baseline
    f = bench.parse(["--full", "--no-probe", "--repeats", "2"])
    assert f.repeats == 2 and f.no_probe and not f.no_cpu_baseline
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


def test_dump_outputs_writes_float32_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: small arrays whole, an array over its share cut to a
    fixed sample (the same indices on every run), every file float32, the
    files together within the budget."""
    import numpy as np
    import torch
    import bench
    assert bench.DUMP_BUDGET_BYTES <= 64 * 10 ** 6
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    big = torch.arange(5000, dtype=torch.float64).reshape(50, 100)
    arrays = {"loss": torch.tensor(1.5, dtype=torch.bfloat16), "big": big,
              "small": torch.arange(6, dtype=torch.float32).reshape(2, 3)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss"].shape == () and got["loss"] == 1.5
    assert np.array_equal(got["small"], arrays["small"].numpy())
    s = got["big"]
    assert s.ndim == 1 and 500 < s.size < 5000 and np.all(np.diff(s) > 0)      # distinct elements of big
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 4096


def test_roofline_traffic_reads_the_newest_pmc_summary():
    """roofline.traffic comes from the newest committed PMC summary: run tags
    order by round, then by letters (r4q after r3aq, r3aa after r3z)."""
    import bench
    base = os.path.basename(bench.PMC_TRAFFIC)
    tags = sorted(f.split("_")[0] for f in os.listdir(os.path.join(REPO, "profiles"))
                  if f.endswith("_pmc_traffic.json"))
    rounds = [int("".join(ch for ch in t[1:] if ch.isdigit())) for t in tags]
    assert int("".join(ch for ch in base.split("_")[0][1:] if ch.isdigit())) == max(rounds)
    bytes_, per = bench.pmc_traffic("conv3r_kernel")
    assert bytes_ and per and all(v["hbm_bytes_per_launch"] > 0 for v in per.values())
