"""CPU tests of the camera-gradient extension: the C ABI's workspace size and the float64 reference the GPU tests pin it against."""
import ctypes

import numpy as np

from diff_gaussian_rasterization import scenes
import torch_ref
import torch_ref_camera


def test_camera_grad_workspace_bytes():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert hasattr(L, "stp_camera_grad_workspace_bytes") and hasattr(L, "stp_set_backward_camera_grads")
    sizes = [_C.camera_grad_workspace_bytes(P) for P in (0, 1, 256, 257, 1000, 1_000_000, 6_000_000)]
    for P, n in zip((0, 1, 256, 257, 1000, 1_000_000, 6_000_000), sizes):
        assert n >= 32 * 4 * ((P + 255) // 256), (P, n)   # one 32-float row per 256-Gaussian block at least
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] and sizes[3] > sizes[2]
    # a NULL output pointer only clears the (thread-local) request: callable without a GPU
    L.stp_set_backward_camera_grads(None, None, None, None, ctypes.c_size_t(0))


def test_reference_agrees_with_torch_ref_inside_the_band():
    """Inside the 1.3 tan_fov band torch_ref_camera is torch_ref with the camera as leaves: same image, same Gaussian gradients."""
    sc = scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=7, camera="orbit")
    img0, g0 = torch_ref.loss_and_grads(sc, order="exact")
    img1, g1 = torch_ref_camera.loss_and_grads(sc, order="exact")
    assert np.max(np.abs(img0 - img1)) < 1e-12
    for n in ("means3D", "opacities", "scales", "rotations", "shs"):
        assert np.max(np.abs(g0[n] - g1[n])) <= 1e-10 * np.max(np.abs(g0[n])), n


def test_reference_translation_gauge_and_unread_entries():
    """The float64 reference satisfies the identity the GPU gauge test checks (moving world and camera together changes nothing),
    with Gaussians in the clamped band, and leaves the entries the forward never reads at zero."""
    sc = torch_ref_camera.with_clamped_gaussians(scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=3, camera="orbit"))
    V, P = sc.viewmatrix.astype(np.float64), sc.projmatrix.astype(np.float64)
    pv = sc.means3D[-2:].astype(np.float64) @ V[:3, :3] + V[3, :3]
    assert np.all(np.abs(pv[:, 0] / pv[:, 2]) > 1.3 * sc.tanfovx)
    for order in ("global", "exact"):
        _, g = torch_ref_camera.loss_and_grads(sc, order=order)
        res = g["means3D"].sum(0) + g["campos"] - V[:3, :] @ g["viewmatrix"][3, :] - P[:3, :] @ g["projmatrix"][3, :]
        assert np.all(np.abs(res) < 1e-9 * np.abs(g["means3D"]).sum(0)), res
        assert np.all(g["viewmatrix"][:, 3] == 0) and np.all(g["projmatrix"][:, 2] == 0)
