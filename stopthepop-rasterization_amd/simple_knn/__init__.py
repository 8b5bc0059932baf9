"""simple_knn -- the import name of the nearest-neighbour submodule of every 3DGS code base, so that

    from simple_knn._C import distCUDA2

in a trainer's `GaussianModel.create_from_pcd` works unchanged on an MI355X.  The kernels are those of libstp_raster.so
(include/stp_raster.h: stp_knn_mean_dist2); this package holds no binary of its own and forwards to diff_gaussian_rasterization."""
from ._C import distCUDA2

__all__ = ["distCUDA2"]
