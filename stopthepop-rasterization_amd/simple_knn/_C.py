"""`simple_knn._C` -- upstream's pybind module of this name exports one function, distCUDA2(points) -> (P,) float32: the mean of the three
smallest squared distances from every point to the other points.  Here it is diff_gaussian_rasterization.knn_mean_dist2 (hand-written HIP
behind the C ABI of libstp_raster.so), which see for the exact semantics and the refusals.  There is no CPU path."""
from diff_gaussian_rasterization import knn_mean_dist2 as distCUDA2

__all__ = ["distCUDA2"]
