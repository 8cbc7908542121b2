"""bench.py's driver options: ``--dump-outputs`` (a fixed, seeded sample of the sorted table as
float32 ``.npy``), ``--full`` (the valsort check, off in a plain run) and the result line."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return np.load(os.path.join(d, "sorted_rows.npy")), np.load(os.path.join(d, "sorted_rows_index.npy"))


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    world = types.SimpleNamespace(size=1, rank=0)
    n = 2 * bench.DUMP_EDGE_ROWS + bench.DUMP_SAMPLE_ROWS + 4097      # past the size dumped whole
    g = torch.Generator().manual_seed(5)
    out = torch.randint(0, 256, (n, 100), dtype=torch.uint8, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), out, world)
    bench.dump_outputs(str(tmp_path / "b"), out, world)
    rows, idx = _load(tmp_path / "a")
    rows_b, idx_b = _load(tmp_path / "b")
    assert rows.dtype == np.float32 and idx.dtype == np.float64
    assert np.array_equal(idx, idx_b) and np.array_equal(rows, rows_b)
    assert rows.shape == (idx.shape[0], 100) and rows.nbytes + idx.nbytes <= 64 << 20
    assert np.all(np.diff(idx) > 0) and idx[0] == 0 and idx[-1] == n - 1
    assert np.array_equal(rows, out[torch.from_numpy(idx.astype(np.int64))].numpy().astype(np.float32))
    # a table that fits is dumped whole
    bench.dump_outputs(str(tmp_path / "c"), out[:777], world)
    rows_c, idx_c = _load(tmp_path / "c")
    assert np.array_equal(idx_c, np.arange(777)) and np.array_equal(rows_c, out[:777].numpy().astype(np.float32))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_run_dumps_the_sorted_table(tmp_path):
    n, steps = 300_001, 3
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", "1", "--records-per-gpu", str(n), "--dump-outputs", str(tmp_path / "d")],
                         capture_output=True, text=True, timeout=280, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "GB/s"
    assert line["config"]["validated"] is None          # the valsort check runs with --full only
    assert abs(line["value"] - n * 100 / 1e9 / (line["ms_per_step"] / 1e3)) <= 0.01 * line["value"] + 1e-3
    rows, idx = _load(tmp_path / "d")
    assert rows.dtype == np.float32 and rows.shape == (idx.shape[0], 100)
    assert idx[0] == 0 and idx[-1] == n - 1 and np.all(np.diff(idx) > 0)
    keys = [bytes(r) for r in rows[:, :10].astype(np.uint8)]
    assert keys == sorted(keys)
    # the same rows as the generator's table sorted by key (keys of this table are distinct)
    from dryad_amd.ops import terasort as TS
    src = torch.empty((n, 100), dtype=torch.uint8, device="cuda")
    from dryad_amd.models.terasort import TeraSortConfig
    TS.generate(src, 0, TeraSortConfig().seed)
    h = src.cpu().numpy()
    order = sorted(range(n), key=lambda i: bytes(h[i, :10]))
    assert np.array_equal(rows.astype(np.uint8), h[np.asarray(order)[idx.astype(np.int64)]])
