"""bench.py's plain run, --full and --dump-outputs: the option parser and the output sampler on the CPU, and
on the GPU a plain run whose dumped coefficients equal rti.fit's on the same (seeded) inputs, twice."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    try:
        import bench as b
    finally:
        sys.path.remove(ROOT)
    return b


def test_full_and_dump_options_default_off(bench):
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7


def test_dump_outputs_samples_to_budget(bench, tmp_path, monkeypatch):
    """Outputs over the budget are cut to one fixed pixel sample shared by every array with a pixel axis;
    floating outputs are written as float32, integer ones as float64, arrays without a pixel axis whole."""
    P, k = 1000, 6
    coef = torch.arange(P * k, dtype=torch.float32).reshape(1, P, k)
    tab = torch.arange(3 * P, dtype=torch.int32).reshape(3, P)
    st = torch.tensor([5], dtype=torch.int32)
    wl = types.SimpleNamespace(P=P, outputs=lambda last: [("coef", coef, 1), ("tables", tab, 1), ("status", st, None)])
    ctx = types.SimpleNamespace(world=1, rank=0, dev=torch.device("cpu"))
    per_px = 4 * k + 8 * 3
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8 + per_px * 100 + per_px // 2)
    for d in ("a", "b"):
        bench.dump_outputs(wl, ctx, 0, str(tmp_path / d))
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("coef", "tables", "status")}
    assert got["coef"].dtype == np.float32 and got["tables"].dtype == np.float64 and got["status"].dtype == np.float64
    assert got["coef"].shape == (1, 100, k) and got["tables"].shape == (3, 100) and got["status"].tolist() == [5.0]
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET
    px = (got["coef"][0, :, 0] / k).astype(np.int64)  # the sampled pixels, from the values themselves
    assert len(set(px)) == 100 and (np.diff(px) > 0).all()
    np.testing.assert_array_equal(got["tables"][1], P + px)
    np.testing.assert_array_equal(got["coef"][0], coef[0].numpy()[px])
    for n, a in got.items():
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / f"{n}.npy"))
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 20)  # under the budget: everything, unsampled
    bench.dump_outputs(wl, ctx, 0, str(tmp_path / "c"))
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "coef.npy"), coef.numpy())


def _run_bench(extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    return subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
                             "--shape", "37x100", "--steps", "3", "--warmup", "1"] + extra,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT)


def _line(p):
    out, err = p.communicate(timeout=240)
    assert p.returncode == 0, err[-3000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_fit_returns(cuda, bench, tmp_path):
    """Two plain runs and one --full run with the same arguments: the plain line has the headline figures and
    none of the --full legs, --steps is the number of timed steps, and every run dumps the same coefficients —
    those rti.fit returns for the bench's seeded stack (the same kernel on the same input: bit for bit)."""
    import rti

    runs = [_run_bench(["--dump-outputs", str(tmp_path / "a")]), _run_bench(["--dump-outputs", str(tmp_path / "b")]),
            _run_bench(["--dump-outputs", str(tmp_path / "f"), "--full", "--no-cpu"])]
    plain, plain_b, full = (_line(p) for p in runs)
    for line in (plain, plain_b, full):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["higher_is_better"] is True
        assert line["unit"] == "Mpix*lights/s" and line["dtype"] == "f32" and line["value"] > 0
        # both figures are rounded in the line: ms_per_step to 1e-4, timed_region_ms to 1e-3 (÷ 3 steps)
        assert line["ms_per_step"] == pytest.approx(line["timed_region_ms"] / 3, abs=0.5e-4 + 0.5e-3 / 3 + 1e-9)
    for key in ("roofline", "kernel_ms_stats", "value_kernel", "parity", "cpu_baseline"):
        assert key not in plain and key in full, key
    assert plain["metric"] == full["metric"] and full["parity"]["ok"]
    H, W, N = 37, 100, 50
    lu, lv = bench.synth_dirs(N, seed=2)
    I = bench.synth_stack(H, W, N, 1, "ptm", lu, lv, seed=1000, device=cuda)
    ref = rti.fit(I[0].reshape(N, H, W), lu, lv).reshape(1, H * W, 6).cpu().numpy()
    for d in ("a", "b", "f"):
        assert sorted(os.listdir(tmp_path / d)) == ["coef.npy"]
        got = np.load(tmp_path / d / "coef.npy")
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, ref)
