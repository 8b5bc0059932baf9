"""The bit pin of the loss kernels: the inputs, the two calls and the entries of tests/golden/loss_bits.npz, shared by the recorder
(tools/record_loss_bits.py) and the test (tests/test_gpu_loss_bits.py).

Inputs come from numpy.random.RandomState(seed), a stream numpy keeps frozen, so none are stored.  The shapes are the smallest of the loss
tests' lists with a partial tile, with more than one tile each way (four workgroups per plane) and with a batch.  Pixel values lie in
[-0.25, 1.25]: about a third of them is cut by the clamp.  Two calls per shape, at the level of _C:
  plain     photometric_forward with maps, photometric_backward with g = (0.8, -0.2)
  training  training_loss_forward with maps and every extra (per-image exposure near identity with a bias, clamp, a 0/1 alpha mask with about
            10 % zeros, invdepth, mono_invdepth, a 0/1 depth mask), training_loss_backward with g = (0.8, -0.2, 0.5) and all three gradients
An entry is the raw float32 tensor for the term vectors, the exposure gradient and everything of the (3, 7, 5) case, else the SHA-256 of
the tensor's bytes (32 uint8)."""
import hashlib

import numpy as np
import torch

import torch_ref_photometric as ref

TW, TH = ref.tile()
SHAPES = [(3, 7, 5), (3, TH + 1, TW + 1), (2, 3, 37, 53)]
RAW_SHAPE = (3, 7, 5)                       # every tensor of this case is stored as it is
ALWAYS_RAW = ("terms", "grad_exposure")     # of every case
OUTPUTS = {"plain": ("terms", "maps", "grad_image"), "training": ("terms", "maps", "grad_image", "grad_exposure", "grad_invdepth")}
G = (0.8, -0.2, 0.5)
shape_id = lambda s: "x".join(map(str, s))


def inputs(shape, seed=11):
    """float32 arrays: image, target, exposure, alpha_mask, invdepth, mono_invdepth, depth_mask"""
    rs = np.random.RandomState(seed)
    H, W = shape[-2:]
    lead = shape[:-3]                       # () or (B,)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    image, target = f32(rs.uniform(-0.25, 1.25, shape)), f32(rs.uniform(0.0, 1.0, shape))
    exposure = np.broadcast_to(np.eye(3, 4), lead + (3, 4)) + 0.05 * rs.standard_normal(lead + (3, 4))
    exposure[..., 3] += 0.02
    plane = lead + (1, H, W)
    alpha_mask = rs.uniform(size=plane) > 0.1
    invdepth, mono = rs.uniform(0.0, 2.0, plane), rs.uniform(0.0, 2.0, plane)
    depth_mask = rs.uniform(size=plane) > 0.2
    return dict(image=image, target=target, exposure=f32(exposure), alpha_mask=f32(alpha_mask), invdepth=f32(invdepth), mono_invdepth=f32(mono),
                depth_mask=f32(depth_mask))


def run(shape):
    """{(call, output): float32 numpy array} of the two calls on the library _C currently uses"""
    from diff_gaussian_rasterization import _C
    t = {k: torch.from_numpy(v).cuda() for k, v in inputs(shape).items()}
    g = torch.tensor(G, dtype=torch.float32).cuda()
    out = {}
    terms, maps = _C.photometric_forward(t["image"], t["target"], True)
    out["plain", "terms"], out["plain", "maps"] = terms, maps
    out["plain", "grad_image"] = _C.photometric_backward(t["image"], t["target"], maps, g[:2].contiguous())
    extras = (t["exposure"], True, t["alpha_mask"], t["invdepth"], t["mono_invdepth"], t["depth_mask"])
    terms, maps = _C.training_loss_forward(t["image"], t["target"], *extras, True)
    out["training", "terms"], out["training", "maps"] = terms, maps
    out["training", "grad_image"], out["training", "grad_exposure"], out["training", "grad_invdepth"] = \
        _C.training_loss_backward(t["image"], t["target"], *extras, maps, g, True, True)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def is_raw(shape, output):
    return tuple(shape) == RAW_SHAPE or output in ALWAYS_RAW


def keys():
    """every key the fixture must hold: <shape>.<call>.<output>"""
    return [f"{shape_id(s)}.{call}.{o}" for s in SHAPES for call, outs in OUTPUTS.items() for o in outs]


def entries(shape, results):
    """{key: float32 array (raw) or uint8[32] (SHA-256 of the bytes)} of run(shape)'s results"""
    assert set(results) == {(call, o) for call, outs in OUTPUTS.items() for o in outs}
    out = {}
    for (call, o), a in results.items():
        assert a.dtype == np.float32
        a = np.ascontiguousarray(a)
        out[f"{shape_id(shape)}.{call}.{o}"] = a if is_raw(shape, o) else np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
    return out
