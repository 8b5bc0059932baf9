"""CPU pin of the float64 yardsticks (torch_ref.py and the three modules on top of it): they reproduce recorded values.

The kernels' correctness claims rest on these yardsticks, so an edit of the one dense renderer is checked against
tests/golden/yardstick_pin.npz: float64 and bool arrays written by the four modules as they stood at commit 458fdd4, when
torch_ref_camera.py, torch_ref_absgrad.py and torch_ref_blend_stats.py each still carried a renderer of their own.  Made from that
commit's tests/ directory with

    mk = lambda seed: scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=seed, camera="orbit")
    d = {}
    def put(prefix, img, grads):
        d[f"{prefix}/image"] = img
        d.update({f"{prefix}/grad/{n}": g for n, g in grads.items()})
    for order in ("global", "exact"):
        put(f"torch_ref/{order}", *torch_ref.loss_and_grads(mk(7), order=order))
        for n, a in zip(("image", "absgrad", "signed"), torch_ref_absgrad.absgrad(mk(7), order=order)):
            d[f"absgrad/{order}/{n}"] = a
        put(f"camera/{order}", *torch_ref_camera.loss_and_grads(torch_ref_camera.with_clamped_gaussians(mk(3)), order=order))
        for n, a in zip(("stats", "explained", "T_final"), torch_ref_blend_stats.blend_stats(mk(torch_ref_blend_stats.YARD_SEED), order=order)):
            d[f"blend_stats/{order}/{n}"] = a
    np.savez_compressed("tests/golden/yardstick_pin.npz", **d)

Counts, `explained` and every bool array are compared exactly; every float array to 1e-12 of the recorded array's largest absolute
entry: four orders of magnitude above float64 epsilon (room for another CPU's BLAS or exp), two below the tightest tolerance a test
applies to a yardstick (1e-10, test_absgrad_cpu.py).  The refactoring that followed the recording reproduced every array bit for bit.
"""
import os

import numpy as np
import pytest

from diff_gaussian_rasterization import scenes
import torch_ref
import torch_ref_absgrad
import torch_ref_blend_stats
import torch_ref_camera

PIN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yardstick_pin.npz"))
ORDERS = ("global", "exact")


def _scene(seed):
    return scenes.make_scene(P=150, W=40, H=36, sigma_min=1.0, sigma_max=8.0, seed=seed, camera="orbit")


def _check(prefix, arrays):
    """arrays: {name: array}; exactly the names recorded under prefix/, bool arrays equal, float arrays to 1e-12 of the largest entry."""
    recorded = {k[len(prefix) + 1:] for k in PIN.files if k.startswith(prefix + "/")}
    assert recorded and set(arrays) == recorded, (prefix, sorted(set(arrays) ^ recorded))
    for n, got in arrays.items():
        want = PIN[f"{prefix}/{n}"]
        assert got.shape == want.shape and got.dtype == want.dtype, (prefix, n, got.shape, got.dtype)
        if want.dtype == np.bool_:
            assert np.array_equal(got, want), (prefix, n)
        else:
            assert want.dtype == np.float64
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (prefix, n, float(np.max(np.abs(got - want))))


def _with_grads(img, grads):
    return {"image": img, **{f"grad/{n}": g for n, g in grads.items()}}


@pytest.mark.parametrize("order", ORDERS)
def test_torch_ref_reproduces_the_pin(order):
    _check(f"torch_ref/{order}", _with_grads(*torch_ref.loss_and_grads(_scene(7), order=order)))


@pytest.mark.parametrize("order", ORDERS)
def test_torch_ref_camera_reproduces_the_pin(order):
    sc = torch_ref_camera.with_clamped_gaussians(_scene(3))
    _check(f"camera/{order}", _with_grads(*torch_ref_camera.loss_and_grads(sc, order=order)))


@pytest.mark.parametrize("order", ORDERS)
def test_torch_ref_absgrad_reproduces_the_pin(order):
    _check(f"absgrad/{order}", dict(zip(("image", "absgrad", "signed"), torch_ref_absgrad.absgrad(_scene(7), order=order))))


@pytest.mark.parametrize("order", ORDERS)
def test_torch_ref_blend_stats_reproduces_the_pin(order):
    stats, explained, T_final = torch_ref_blend_stats.blend_stats(_scene(torch_ref_blend_stats.YARD_SEED), order=order)
    _check(f"blend_stats/{order}", {"stats": stats, "explained": explained, "T_final": T_final})
    assert np.array_equal(stats[:, 2], PIN[f"blend_stats/{order}/stats"][:, 2])   # the counts: exact
