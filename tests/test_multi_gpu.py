"""GPU tests (-m gpu) of the tile-row sharded path with MORE THAN ONE RANK running the HIP kernels (north_star: frames shard by
screen-tile row with an RCCL gather of the image).

  * two ranks on ONE GPU, gloo backend (the exchange code stages device tensors through the host): runs on the 1-GPU box and
    covers everything but RCCL itself -- partition, windowed binning / render / backward, gather of the three channel segments
    into the root's tensor, all-reduce of the gradient records between the two halves of the backward, work-balanced
    re-partition, the refusal of render_depth;
  * two ranks on two GPUs, nccl (= RCCL) backend: the same worker, skipped unless the box has two devices.
Sharded frame vs the unsharded HIP run: image bit for bit, gradients <= 1e-5 of the largest entry."""
import os
import socket
import subprocess
import sys

import pytest
import torch

import conftest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(conftest.ROOT, "tests", "_shard_gpu_worker.py")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _spawn(backend, world=2):
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, WORKER, backend], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    assert "SHARD_GPU_OK" in outs[0]


def test_two_ranks_on_one_gpu_host_staged_exchange():
    _spawn("gloo")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL between them)")
def test_two_ranks_two_gpus_rccl():
    _spawn("nccl")


def _bench_two_ranks(extra):
    """bench.py as the driver launches it for N = 2 (one process per rank, rendezvous on 127.0.0.1), in its one-GPU self-test mode
    (`--test-one-gpu`: both ranks on cuda:0, gloo process group): exercises the N > 1 code path -- with `--full`, fallback measurement first,
    tile-row headline under the watchdog; the JSON line -- on the 1-GPU box.  The numbers mean nothing; the shape of the line does."""
    import json
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(conftest.ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                                       "--test-one-gpu", "--scale", "0.1", "--probe-timeout", "240"] + extra,
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[1][-2000:] for o in outs)
    lines = [ln for ln in outs[0][0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and not any(ln.startswith("{") for ln in outs[1][0].splitlines())   # ONE line, from rank 0
    return json.loads(lines[0])


def test_bench_n2_plain_run_times_the_tile_row_headline_alone():
    d = _bench_two_ranks([])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["parallelism"] == "tilerows2", d
    assert d["rccl_ranks"]["world_size"] == 2 and d["rccl_ranks"]["all_reduce_of_ones"] == 2 and d["value"] > 0
    assert "frame_shard" not in d and "tile_shard" not in d and "hbm_measured" not in d


def test_bench_n2_tile_row_headline_with_frame_shard_side_object():
    d = _bench_two_ranks(["--full"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["parallelism"] == "tilerows2", d
    assert d["rccl_ranks"]["world_size"] == 2 and d["rccl_ranks"]["all_reduce_of_ones"] == 2
    assert d["value"] > 0 and d["frame_shard"]["scaling"] == "weak" and d["frame_shard"]["value"] > 0
    assert "tile_shard" not in d   # (the error object of a tile-row exchange that hung or failed)


def test_bench_n2_frames_headline_keeps_the_tile_row_side_object():
    d = _bench_two_ranks(["--full", "--shard", "frames"])
    assert d["scaling"] == "weak" and d["config"]["parallelism"] == "frames2" and d["tile_shard"]["scaling"] == "strong" and d["tile_shard"]["value"] > 0


class _InProcessTransport:
    """Stand-in for torch.distributed with DEVICE-side semantics (what RCCL gives the exchange code and gloo does not): point-to-point operations
    are ordered behind the stream that is current when they are posted, `wait()` makes the current stream wait, nothing is staged through the host.
    Two "ranks" are two threads of this process on cuda:0; a send parks (tensor, event) in a queue, the matching receive copies it on its own
    stream behind that event.  It lets the overlapped branch of tile_shard.gather_image -- side stream, start / half-strip events, two batches --
    run on a one-GPU box; it says nothing about RCCL itself."""

    isend, irecv = "isend", "irecv"

    def __init__(self, world):
        import queue
        self.q = {(s, d): queue.Queue() for s in range(world) for d in range(world)}
        self.posted = []          # (rank, kind, stream id): which stream every operation was posted under

    class P2POp:
        def __init__(self, op, tensor, peer):
            self.op, self.tensor, self.peer = op, tensor, peer

    def bind(self, rank):
        outer = self

        class Bound:
            isend, irecv, P2POp = outer.isend, outer.irecv, outer.P2POp

            @staticmethod
            def get_backend():
                return "nccl"

            @staticmethod
            def batch_isend_irecv(ops):
                stream = torch.cuda.current_stream()
                reqs = []
                for o in ops:
                    outer.posted.append((rank, o.op, stream.cuda_stream))
                    if o.op == "isend":
                        ev = torch.cuda.Event(); ev.record(stream)
                        outer.q[(rank, o.peer)].put((o.tensor, ev))
                        reqs.append(type("Req", (), {"wait": staticmethod(lambda: None)}))
                    else:
                        def wait(o=o, stream=stream):
                            src, ev = outer.q[(o.peer, rank)].get(timeout=60)
                            with torch.cuda.stream(stream):
                                stream.wait_event(ev)
                                o.tensor.copy_(src)
                            done = torch.cuda.Event(); done.record(stream)
                            torch.cuda.current_stream().wait_event(done)
                        reqs.append(type("Req", (), {"wait": staticmethod(wait)}))
                return reqs
        return Bound


def test_overlapped_strip_exchange_on_one_gpu_with_an_in_process_transport():
    """The branch of gather_image that only a device-side transport takes: forward in two launches (stp_set_forward_split), the upper half-strip
    posted under the side stream behind the event between them, the root's receives posted beside its own render.  Two threads = two ranks."""
    import threading
    import numpy as np
    sys.path.insert(0, os.path.join(conftest.ROOT, "tests"))
    from helpers import FULL_STP, GpuRun, ext_settings, settings_dict
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import scenes, tile_shard
    dev = torch.device("cuda", 0)
    world = 2
    for skw, sd in ((dict(P=6000, W=256, H=208, sigma_min=1.5, sigma_max=12.0, seed=61, camera="orbit"), settings_dict(**FULL_STP)),
                    (dict(P=4000, W=160, H=144, sigma_min=1.5, sigma_max=10.0, seed=62), settings_dict(2, per_pixel=16))):
        sc = scenes.make_scene(**skw)
        full = GpuRun(sc, sd, backward=False)
        tr = _InProcessTransport(world)
        out, errors = {}, []

        def run(rank):
            try:
                torch.cuda.set_device(dev)
                t = lambda a: torch.tensor(a, device=dev)
                rs = dgr.GaussianRasterizationSettings(
                    image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t(sc.bg), scale_modifier=sc.scale_modifier,
                    viewmatrix=t(sc.viewmatrix), projmatrix=t(sc.projmatrix), inv_viewprojmatrix=t(sc.inv_viewprojmatrix), sh_degree=sc.sh_degree,
                    campos=t(sc.campos), prefiltered=False, settings=ext_settings(sd), render_depth=False, debug=False)
                r = tile_shard.TileRowShardedRasterizer(rs, tr.bind(rank), rank, world)
                color, radii = r(t(sc.means3D), torch.zeros(sc.means3D.shape, device=dev), t(sc.opacities), shs=t(sc.shs), scales=t(sc.scales), rotations=t(sc.rotations))
                torch.cuda.synchronize(dev)
                out[rank] = (color.cpu().numpy(), radii.cpu().numpy(), r.parts)
            except Exception as ex:   # (a thread's exception must fail the test, not vanish)
                import traceback
                errors.append(traceback.format_exc())

        threads = [threading.Thread(target=run, args=(k,)) for k in range(world)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
        assert not errors, errors[0]
        assert np.array_equal(out[0][0], full.color)                       # the root holds the whole frame, bit for bit
        parts = out[0][2]
        assert all(tile_shard.split_row(p) for p in parts)                 # both blocks were rendered in two launches
        y0, y1 = parts[1]
        assert np.array_equal(out[1][0][:, 16 * y0:min(16 * y1, sc.H)], full.color[:, 16 * y0:min(16 * y1, sc.H)])   # the peer keeps its own strip
        # the upper halves (and every receive of the root) were posted under a stream that is not the ranks' compute stream
        compute = torch.cuda.current_stream(dev).cuda_stream
        side = {s for (_, _, s) in tr.posted if s != compute}
        assert side, tr.posted
        assert all(s != compute for (rk, kind, s) in tr.posted if rk == 0 and kind == "irecv")
        assert sum(1 for (rk, kind, s) in tr.posted if rk == 1 and kind == "isend" and s != compute) == 3    # three channel segments of the upper half
        assert sum(1 for (rk, kind, s) in tr.posted if rk == 1 and kind == "isend" and s == compute) == 3    # ... and of the lower half
