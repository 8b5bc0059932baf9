"""The bench line's contract: ONE stdout line the driver can parse -- under 8 KB, the contract's keys plus `roofline`,
`cpu_baseline`, a short parity summary and one compact object per other workload; everything else goes to bench_detail.json / stderr.

  * CPU: `bench.compact_line` on the committed full record of round 5 (`profiles/r05_bench_full.json`, the 24.7 KB line the driver could not
    parse) and on a record padded far beyond it;
  * GPU (-m gpu): `bench.py --full --scale 0.05` at N = 1, every leg on (CPU baseline, parity, other workloads); the plain flagship run
    `bench.py --gpus 1 --steps 20 --warmup 5`, which times the headline alone and spends at most 30 s besides its steps."""
import json
import os
import subprocess
import sys
import time

import pytest

import conftest

sys.path.insert(0, conftest.ROOT)
import bench  # noqa: E402

CONTRACT_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}
ROOFLINE_KEYS = {"bound", "achieved", "peak", "unit", "frac", "traffic"}
CPU_KEYS = {"value", "unit", "cores", "kind", "sample"}


def _check_line(d, text, other_workloads=True):
    assert len(text) < bench.LINE_CAP_BYTES, len(text)
    assert CONTRACT_KEYS <= set(d), CONTRACT_KEYS - set(d)
    assert ROOFLINE_KEYS <= set(d["roofline"]), d["roofline"]
    assert d["roofline"]["bound"] in ("hbm", "valu", "lds") and d["roofline"]["unit"] == "GB/s" and d["roofline"]["peak"] == 8000.0
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-4
    assert CPU_KEYS <= set(d["cpu_baseline"]) and d["cpu_baseline"]["kind"] in ("port", "reference")
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["vs_baseline"] is None and d["dtype"] == "f32"
    assert {"oracle"} <= set(d["parity"]) and "psnr_db" in d["parity"]["oracle"]
    if other_workloads:
        assert set(d["other_workloads"]) == {label for label, *_ in bench.OTHER_WORKLOADS}
        for w in d["other_workloads"].values():
            assert "error" not in w, w
            assert {"value", "ms_per_step", "dominant_kernel", "frac", "traffic"} <= set(w), w

    def strings(o):
        if isinstance(o, dict):
            for v in o.values():
                yield from strings(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                yield from strings(v)
        elif isinstance(o, str):
            yield o
    assert max(len(x) for x in strings(d)) <= 160   # (the driver shortens long strings)


def test_compact_line_of_the_round_5_record_fits_the_cap():
    full = json.load(open(os.path.join(conftest.ROOT, "profiles", "r05_bench_full.json")))
    assert len(json.dumps(full)) > 20000          # the record that could not be parsed
    o = bench.compact_line(full)
    text = json.dumps(o)
    _check_line(o, text)
    assert len(text) < 6000
    # the numbers are the record's own
    assert o["value"] == full["value"] and o["roofline"]["frac"] == full["roofline"]["frac"] and o["cpu_baseline"]["value"] == full["cpu_baseline"]["value"]
    assert o["parity"]["reference_build"]["keys_equal"] is True and o["parity"]["oracle"]["explained"] == "2/2" and o["parity"]["oracle"]["closed"] is True
    assert o["other_workloads"]["C5"]["closed"] is True and o["other_workloads"]["C3"]["list_equal"] is True


def test_emit_sheds_optional_objects_instead_of_losing_the_line(tmp_path, monkeypatch):
    full = json.load(open(os.path.join(conftest.ROOT, "profiles", "r05_bench_full.json")))
    # forty other workloads instead of four: the optional objects go, the contract's stay
    full["other_workloads"] = {f"W{i}": dict(full["other_workloads"]["C5"]) for i in range(40)}
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    r, w = os.pipe()
    bench.emit(w, full)
    os.close(w)
    text = os.read(r, 1 << 20).decode()
    os.close(r)
    assert text.endswith("\n") and text.count("\n") == 1 and len(text) < bench.LINE_CAP_BYTES
    d = json.loads(text)
    assert CONTRACT_KEYS <= set(d) and "roofline" in d and "cpu_baseline" in d and "other_workloads" not in d
    assert json.load(open(tmp_path / "bench_detail.json"))["other_workloads"].keys() == full["other_workloads"].keys()


def test_the_committed_round_6_line_is_what_the_driver_can_parse():
    """profiles/r06_bench_full.json is the stdout line of the default run on the round's final kernels: one bounded JSON object with the contract's
    keys, the roofline of both render kernels WITH measured traffic, the CPU baseline, and a traffic figure for every other workload."""
    text = open(os.path.join(conftest.ROOT, "profiles", "r06_bench_full.json")).read().strip()
    assert text.count("\n") == 0
    d = json.loads(text)
    _check_line(d, text)
    assert d["roofline"]["traffic"] and d["roofline"]["second"]["traffic"]
    assert all(w["traffic"] for w in d["other_workloads"].values())
    assert d["other_workloads"]["C3"]["dominant_kernel"].startswith("render_kbuffer_ring_kernel<16")
    assert d["leg_seconds"]["total"] < 60.0


@pytest.mark.gpu
def test_bench_prints_one_bounded_line_at_n1():
    env = dict(os.environ, TMPDIR=os.environ.get("TMPDIR", "/tmp"))
    p = subprocess.run([sys.executable, os.path.join(conftest.ROOT, "bench.py"), "--full", "--scale", "0.05", "--steps", "3", "--warmup", "1"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    _check_line(d, lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert "[bench detail] {" in p.stderr


@pytest.mark.gpu
def test_plain_bench_run_times_the_headline_alone(tmp_path):
    """Without --full: the flagship's line with the contract's keys and the roofline of the timed steps, the dumped outputs, none of the
    other legs, and at most 30 s of the whole process's wall time outside the warm-up and timed steps."""
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(conftest.ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path / "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert len(lines[0]) < bench.LINE_CAP_BYTES and CONTRACT_KEYS <= set(d) and ROOFLINE_KEYS <= set(d["roofline"])
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["value"] > 0 and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["config"]["P"] == 1_000_000
    assert not {"cpu_baseline", "parity", "hbm_measured", "other_workloads", "fma_depth_build", "with_torch_loss"} & set(d), sorted(d)
    assert set(d["leg_seconds"]) == {"headline", "total"}
    assert {"color.npy", "radii.npy", "dL_dmeans3D.npy"} <= {f.name for f in (tmp_path / "out").iterdir()}
    outside = wall - (steps + warmup) * d["ms_per_step"] / 1000.0
    assert outside < 30.0, (wall, d["ms_per_step"], d["leg_seconds"])


def test_dump_outputs_writes_the_last_step_within_the_cap(tmp_path):
    """--dump-outputs: float32/float64 .npy files only, under 64 MB for a C4-sized frame, the per-Gaussian
    arrays on the same fixed sample from run to run, the image rows of an oversized frame subsampled with their index written."""
    import types

    import numpy as np
    import torch

    P, H, W = 200_000, 2160, 3840
    leaves = [torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 16, 3), torch.zeros(P, 3), torch.zeros(P, 4)]
    for i, x in enumerate(leaves):
        x.grad = torch.full_like(x, float(i + 1))
    color = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(3, H, W).contiguous()
    radii = torch.arange(P, dtype=torch.int32)
    wl = types.SimpleNamespace(state={"color": color, "radii": radii}, means3D=leaves[0], dev=torch.device("cpu"),
                               tensors=lambda: tuple(leaves))
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        bench.dump_outputs(wl, str(d))
        runs.append({f.name: np.load(f) for f in d.iterdir()})
        assert sum(f.stat().st_size for f in d.iterdir()) < 64 << 20
    a, b = runs
    assert a.keys() == b.keys() == {"color.npy", "color_row_index.npy", "gaussian_index.npy", "radii.npy", "dL_dmeans3D.npy", "dL_dmeans2D.npy",
                                    "dL_dopacity.npy", "dL_dshs.npy", "dL_dscales.npy", "dL_drotations.npy"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    idx = a["gaussian_index.npy"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and np.array_equal(a["radii.npy"], idx.astype(np.float32))
    assert a["dL_dshs.npy"].shape == (bench.DUMP_SAMPLE, 16, 3) and np.all(a["dL_dshs.npy"] == 4.0)
    rows = a["color_row_index.npy"].astype(np.int64)
    assert np.array_equal(a["color.npy"][0, :, 0], rows.astype(np.float32)) and a["color.npy"].size <= bench.DUMP_IMAGE_FLOATS
