#!/usr/bin/env python3
"""Record tests/golden/loss_bits.npz, the bits tests/test_gpu_loss_bits.py holds the loss kernels to (GPU box).
usage: tools/record_loss_bits.py --lib PATH/libstp_raster.so --out FILE

The fixture was recorded ONCE, on an MI355X, with the library built from commit f1a6b1f ("Add Mip-Splatting 3D filter"), the last one whose
stp_loss.hip held the plain and the training kernels as two separate copies.  It is what proves that sharing their pieces moved no bit.
NEVER re-record it from the code under test: a change that moves the bits on purpose records from a build of the commit before it, passed
with --lib, and says so in its commit message.

The inputs, the two calls and the entries are those of tests/loss_bits_cases.py, which the test shares."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "stopthepop-rasterization_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

import loss_bits_cases as cases
from diff_gaussian_rasterization import _C

ap = argparse.ArgumentParser()
ap.add_argument("--lib", required=True, help="the library to record from: a build of the commit BEFORE the change under test")
ap.add_argument("--out", required=True)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/record_loss_bits.py records on a GPU; there is none")
_C.use_library(os.path.abspath(args.lib))
fixture = {}
for shape in cases.SHAPES:
    fixture.update(cases.entries(shape, cases.run(shape)))
assert sorted(fixture) == sorted(cases.keys())
for k, v in fixture.items():
    assert v.dtype == np.uint8 or np.isfinite(v).all(), f"{k}: a non-finite value cannot pin anything"
np.savez(args.out, **fixture)
print(f"{args.out}: {len(fixture)} entries, {os.path.getsize(args.out)} bytes, from {_C.library_path()}")
