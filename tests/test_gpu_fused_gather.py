"""The hierarchical forwards sort and gather their tiles of up to 1024 entries themselves (RenderArgs::fused_gather, stp_render_hier.inc)
instead of leaving that to tile_sort_gather_kernel's launch in front of them.  STP_FUSED_GATHER=0 keeps the separate launch.  It is read once
per process, so the two run in children: keys, list, entry records, image, n_contrib and the blend log are the same bit for bit, gradients to
the summation order of the atomics."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = "mode=3, order=3, rect=True, tight=True, tbc=True, h44=True, lb=True"
CASES = {
    # (scene, settings, how): "train" = forward + backward with the blend log, "infer" = forward only, "split" = forward in two launches
    "clustered_ordered": ("P=30000, W=640, H=480, sigma_min=1.0, sigma_max=8.0, seed=77, clusters=(5, 0.6, 0.03)", FULL, "train"),  # 1200 tiles: longest first
    "window_remap": ("P=6000, W=256, H=192, sigma_min=2.0, sigma_max=14.0, seed=11, camera='orbit'", FULL, "train"),               # 192 tiles
    "lists_over_1024": ("P=30000, W=320, H=240, sigma_min=1.0, sigma_max=8.0, seed=77, clusters=(5, 0.6, 0.03)", FULL, "train"),  # 23 of 300 tiles
    "empty_tiles": ("P=40, W=320, H=240, sigma_min=1.0, sigma_max=3.0, seed=5", FULL, "train"),
    "no_culling": ("P=6000, W=256, H=192, sigma_min=2.0, sigma_max=14.0, seed=12, camera='orbit'", "mode=3, order=3", "train"),
    "inference": ("P=30000, W=640, H=480, sigma_min=1.0, sigma_max=8.0, seed=77, clusters=(5, 0.6, 0.03)", FULL, "infer"),
    "split": ("P=6000, W=256, H=192, sigma_min=2.0, sigma_max=14.0, seed=13, camera='orbit'", FULL, "split"),
    "mid12": ("P=6000, W=256, H=192, sigma_min=2.0, sigma_max=14.0, seed=11, camera='orbit'", FULL + ", tile_2x2=12", "train"),
    "mid20": ("P=6000, W=256, H=192, sigma_min=2.0, sigma_max=14.0, seed=11, camera='orbit'", FULL + ", tile_2x2=20, per_pixel=8", "train"),
}

CHILD = r"""
import ctypes, sys, numpy as np, torch
sys.path[:0] = ['tests', 'stopthepop-rasterization_amd', '.']
import conftest
from helpers import *
from diff_gaussian_rasterization import scenes, _C

def entries(buf, R, name):  # the list-ordered entry records (float4 per entry), like _C.binning_array
    L = _C._load()
    off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
    lay = int(L.stp_binning_layout_count(ctypes.c_void_p(buf.data_ptr()), int(R)))
    assert lay > 0 and L.stp_binning_layout(lay, name.encode(), ctypes.byref(off), ctypes.byref(cnt)) == 0
    return _C._view(buf, off.value, cnt.value // lay * int(R), torch.float32).cpu().numpy().view(np.uint32)

def binning(out, buf, R):
    out['keys'] = _C.binning_array(buf, R, 'keys').cpu().numpy()
    out['list'] = _C.binning_array(buf, R, 'point_list').cpu().numpy()
    for e in ('entA', 'entB', 'entC', 'entD', 'entF'):
        out[e] = entries(buf, R, e)

scene_kw, sd_kw, how, dst = sys.argv[1:5]
sc = eval('scenes.make_scene(' + scene_kw + ')')
sd = eval('settings_dict(' + sd_kw + ')')
out = {'wh': np.array([sc.W, sc.H])}
if how == 'split':
    dev = 'cuda:0'
    t = lambda a: torch.tensor(a, device=dev)
    empty = torch.Tensor([])
    sd = {**sd, '_record_blend_log': True, '_backward_mode': 'replay'}
    ev = torch.cuda.Event(); ev.record()
    _C.set_forward_split(((sc.H + 15) // 16) // 2, ev)
    o = _C.rasterize_gaussians(t(sc.bg), t(sc.means3D), empty, t(sc.opacities), t(sc.scales), t(sc.rotations), sc.scale_modifier, empty,
                               t(sc.viewmatrix), t(sc.projmatrix), t(sc.inv_viewprojmatrix), sc.tanfovx, sc.tanfovy, sc.H, sc.W, t(sc.shs),
                               sc.sh_degree, t(sc.campos), False, sd, False, False)
    ev.synchronize()
    R = int(o[0])
    out['color'] = o[1].cpu().numpy()
    out['n_contrib'] = _C.image_array(o[5], sc.W, sc.H, 'n_contrib').cpu().numpy()
    binning(out, o[4], R)
else:
    g = GpuRun(sc, sd, backward=(how == 'train'))
    R = g.num_rendered
    out['color'] = g.color
    binning(out, g.binning, R)
    lens = np.diff(g.image_array('ranges').view(np.uint32).reshape(-1, 2), axis=1).ravel()
    out['lens'] = lens
    if how == 'train':
        out['n_contrib'] = g.image_array('n_contrib')
        out['log'] = g.image_array('blend_log').view(np.uint16)
        out['log_depth'] = np.array(_C.blend_log_depth(g.img))
        for k in ('dL_dmeans3D', 'dL_dsh', 'dL_dopacity', 'dL_dscales', 'dL_drotations'):
            out['g_' + k] = g.grads[k]
np.savez(dst, **out)
"""


def _rel(a, b):
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-12)


def _log_records(log, n_contrib, depth, W, H):
    """The blend log's valid records ([tile][wave][record][lane] in hierarchical mode; record k of a pixel is valid below min(n_contrib, depth)),
    as one array: the slots behind them hold whatever the memory held."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rows = log.size // (gx * gy * 4 * 64)
    assert rows * gx * gy * 4 * 64 == log.size and rows > depth
    log = log.reshape(gy, gx, 4, rows, 64)
    lane = np.arange(64)
    s, x = lane >> 4, lane & 15
    m, q = x >> 2, x & 3
    w = np.arange(4)[:, None]
    dx, dy = 4 * s + 2 * (m & 1) + (q & 1), 4 * w + 2 * (m >> 1) + (q >> 1)          # (wave, lane) -> pixel offset inside the tile
    px = np.arange(gx)[None, :, None, None] * 16 + dx[None, None, None, :]
    py = np.arange(gy)[:, None, None, None] * 16 + dy[None, None, :, :]
    inside = (px < W) & (py < H)
    nrec = np.where(inside, n_contrib.reshape(H, W)[np.minimum(py, H - 1), np.minimum(px, W - 1)], 0)   # [gy, gx, 4, 64]
    valid = np.arange(rows)[None, None, None, :, None] < np.minimum(nrec, depth)[:, :, :, None, :]
    return log[valid]


@pytest.mark.parametrize("case", list(CASES))
def test_fused_gather_changes_nothing(case):
    scene_kw, sd_kw, how = CASES[case]
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for mode in ("1", "0"):
            f = os.path.join(d, f"o{mode}.npz")
            subprocess.run([sys.executable, "-c", CHILD, scene_kw, sd_kw, how, f], check=True, timeout=600,
                           env=dict(os.environ, STP_FUSED_GATHER=mode), cwd=ROOT)
            res[mode] = dict(np.load(f))
    a, b = res["1"], res["0"]
    assert set(a) == set(b)
    if "lens" in a:  # the scene has what the case is there for
        lens = a["lens"]
        if case == "lists_over_1024":
            assert lens.max() > 1024 and ((lens > 0) & (lens <= 1024)).any(), lens
        if case == "empty_tiles":
            assert (lens == 0).any() and (lens > 0).any(), lens
        if case == "clustered_ordered":
            assert lens.size > 1024
        if case == "window_remap":
            assert lens.size <= 1024
    for k in a:
        if k.startswith("g_"):
            assert _rel(a[k], b[k]) < 2e-5, (k, _rel(a[k], b[k]))
        elif k == "log":
            assert int(a["log_depth"]) == int(b["log_depth"])
            n = a["n_contrib"].astype(np.int64)
            W, H = (int(v) for v in a["wh"])
            la = _log_records(a["log"], n, int(a["log_depth"]), W, H)
            lb = _log_records(b["log"], n, int(a["log_depth"]), W, H)
            assert la.size > 0 and np.array_equal(la, lb), k
        else:
            assert np.array_equal(a[k], b[k]), k
