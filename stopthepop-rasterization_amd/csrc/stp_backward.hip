// stp_backward.hip -- backward of the per-Gaussian stages.
//
// Replaces (reference cuda_rasterizer/backward.cu):
//   computeCov2DCUDA              :146-312  (dL/dconic -> dL/dcov3D, covariance path of dL/dmean3D, optional
//                                            Mip-Splatting opacity-scaling gradient)
//   preprocessCUDA<3> (backward)  :384-434  (projection path of dL/dmean3D)
//   computeColorFromSH (backward) :22-141
//   computeCov3D (backward)       :316-379
// The reference runs two kernels back to back; both are per-Gaussian with no cross-thread dependency,
// so here they are one HBM-streaming kernel: each Gaussian's inputs are read once and its nine gradient
// rows written once.
#include "stp_internal.h"
#include "stp_device.h"
#include "stp_sh_dir.h"
#include "stp_activations.h"

namespace stp {

namespace {

struct BwdPreArgs {
    int P, D, M, proper_ewa_scaling;
    float h_x, h_y, tan_fovx, tan_fovy, scale_modifier;
    const float* means3D;
    const int* radii;
    const float* shs;
    const uint8_t* clamped;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3Ds;
    const float* view;
    const float* proj;
    const float* cam;
    const float* grad_rec; // P x grad_stride: sums of the render half (layout: stp_raster.h, stp_backward)
    int grad_stride;       // 16 (one line per Gaussian, two 16-byte loads) or 9 (compact records of a tile-row shard)
    int clear_rec;         // leave every record read zero-filled again (phases bit 3): the caller's buffer is ready for the next backward
    int block0;            // first 256-Gaussian block of this launch (the grid covers a range of blocks: stp_backward_phases, chunked per-Gaussian half)
    float* dL_dmean2D;     // P x 3  (out)
    float* dL_dopacity;    // P      (out)
    float* dL_dcolor;      // P x 3  (out)
    float* dL_dmean3D;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_dscale;
    float* dL_drot;
    float* cam_rows;       // CAM only: one kCamRow-float row of camera-gradient partial sums per workgroup (camera_grad_* below)
    const float* dc;       // SPLIT only: the (P, 3) first SH coefficient; `shs` is then the (P, M-1, 3) rest (not read for M == 1, never nullptr)
    float* dL_ddc;         // SPLIT only: P x 3; dL_dsh is then P x (M-1) x 3
    const float* sh_stash; // STASH only: the forward's nine planes of P floats (stp_sh_dir.h; stp_set_forward_sh_stash)
    int raw;               // stp_set_backward_raw_params: which of opacities / scales / rotations hold raw parameters (stp_activations.h: RAW_*); wave-uniform
};

// The chain rule of the three activations (stp_activations.h) behind the gradient the kernel has for the activated value: what autograd gives for
// torch.sigmoid / torch.exp / F.normalize in front of the call, every step one correctly rounded operation (no contraction can reach into them).
__device__ __forceinline__ float raw_opacity_grad(float g, float o) { return __fmul_rn(g, __fmul_rn(o, __fsub_rn(1.0f, o))); }
__device__ __forceinline__ float raw_scale_grad(float g, float s) { return __fmul_rn(g, s); }
// qh: the normalised quaternion, norm: |q| before the clamp.  (g - qh (qh . g)) / |q|; where the clamp was active the norm took no part: g / eps
__device__ __forceinline__ float4 raw_rotation_grad(float4 g, float4 qh, float norm)
{
    if (norm < kRawQuatEps) return make_float4(__fdiv_rn(g.x, kRawQuatEps), __fdiv_rn(g.y, kRawQuatEps), __fdiv_rn(g.z, kRawQuatEps), __fdiv_rn(g.w, kRawQuatEps));
    const float d = __fmaf_rn(qh.w, g.w, __fmaf_rn(qh.z, g.z, __fmaf_rn(qh.y, g.y, __fmul_rn(qh.x, g.x))));
    return make_float4(__fdiv_rn(__fmaf_rn(-qh.x, d, g.x), norm), __fdiv_rn(__fmaf_rn(-qh.y, d, g.y), norm), __fdiv_rn(__fmaf_rn(-qh.z, d, g.z), norm),
                       __fdiv_rn(__fmaf_rn(-qh.w, d, g.w), norm));
}

// Camera-gradient contributions of one Gaussian (CAM instantiation), in the order of a workspace row:
//   [0..11]  dL/dviewmatrix[i][j], i = 0..3 (world axis; 3 = translation), j = 0..2 (view axis) at 3*i + j  (column 3 is never read)
//   [12..23] dL/dprojmatrix[i][j], i = 0..3, j = 0, 1, 3 at 12 + 3*i + (0, 1, 2)                           (column 2 is never read)
//   [24..26] dL/dcampos
// Matrices in the row-vector layout of stp_raster.h: element [i][j] is view[4*i + j].
constexpr int kCamTerms = 27;
constexpr int kCamRow = 32;

// An opaque copy: the compiler cannot see that it equals its input, so no expression built on it is merged with one built on the input.
__device__ __forceinline__ float opaque(float v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// Everything for one visible Gaussian.  sh_row / dsh_row: this Gaussian's 3M SH coefficients and their gradient,
// both in the SAME LDS row (the kernel stages them, see below): each channel reads what it needs before it writes.
// TERMS = true: the same chain rule evaluated for this Gaussian's camera terms only (cg[kCamTerms]): nothing is stored, and every input is
// read through opaque(), so none of its arithmetic is shared with -- or changes the instruction selection of -- the TERMS = false pass that
// writes the Gaussian's gradients (bit-identical with and without a camera request).
// INVD: the inverse-depth request (stp_set_backward_invdepth): slot STP_GRAD_RECORD_INVDEPTH of the record holds dL/d(1/z) of the Gaussian,
// z = t.z the view-space depth of its centre; -slot / z^2 joins dL/dt_z in front of dL/dmean and the camera terms.  INVD = false is the
// function as it was.
// STASH: the direction derivatives of the three colour channels come from the forward's stash (a.sh_stash, stp_sh_dir.h); sh_row holds zeros
// in the place of the coefficients.  STASH = false is the function as it was.
// a.dL_dcolor / a.dL_dcov3D may be null (outputs nobody receives): a wave-uniform test skips their stores, dcov[] stays in registers.
template <bool TERMS, bool INVD, bool STASH>
__device__ __forceinline__ void gaussian_backward(const BwdPreArgs& a, int idx, float* sh_row, float* cg)
{
    const float* __restrict__ view = a.view;
    const float* __restrict__ proj = a.proj;
    float view_t[TERMS ? 16 : 1], proj_t[TERMS ? 16 : 1];
    if constexpr (TERMS) {
#pragma unroll
        for (int k = 0; k < 16; k++) { view_t[k] = opaque(a.view[k]); proj_t[k] = opaque(a.proj[k]); }
        view = view_t; proj = proj_t;
    }
    float3 mean = make_float3(a.means3D[3 * (size_t)idx], a.means3D[3 * (size_t)idx + 1], a.means3D[3 * (size_t)idx + 2]);
    if constexpr (TERMS) mean = make_float3(opaque(mean.x), opaque(mean.y), opaque(mean.z));
    float3 dmean;
    // the render half's sums: one 64-byte record, two 16-byte loads and a scalar
    float4 rec0, rec1; // colour r g b, mean2D x | mean2D y, conic xx xy yy
    float rec_op;
    if (a.grad_stride == 16) {
        rec0 = *reinterpret_cast<const float4*>(a.grad_rec + 16 * (size_t)idx);
        rec1 = *reinterpret_cast<const float4*>(a.grad_rec + 16 * (size_t)idx + 4);
        rec_op = a.grad_rec[16 * (size_t)idx + 8];
    } else { // compact records: 36-byte stride, scalar loads
        const float* __restrict__ r = a.grad_rec + (size_t)a.grad_stride * idx;
        rec0 = make_float4(r[0], r[1], r[2], r[3]);
        rec1 = make_float4(r[4], r[5], r[6], r[7]);
        rec_op = r[8];
    }
    if constexpr (TERMS) {
        rec0 = make_float4(opaque(rec0.x), opaque(rec0.y), opaque(rec0.z), opaque(rec0.w));
        rec1 = make_float4(opaque(rec1.x), opaque(rec1.y), opaque(rec1.z), opaque(rec1.w));
        rec_op = opaque(rec_op);
    }
    float rec_invz = 0.0f;
    if constexpr (INVD) { // (padded records only: the caller has refused compact ones with the request)
        rec_invz = a.grad_rec[16 * (size_t)idx + STP_GRAD_RECORD_INVDEPTH];
        if constexpr (TERMS) rec_invz = opaque(rec_invz);
        else if (a.clear_rec) const_cast<float*>(a.grad_rec)[16 * (size_t)idx + STP_GRAD_RECORD_INVDEPTH] = 0.0f;
    }
    if (!TERMS && a.clear_rec) { // only records of visible Gaussians are ever written by the render half, and all of those pass through here
        float* const r = const_cast<float*>(a.grad_rec) + (size_t)a.grad_stride * idx;
        if (a.grad_stride == 16) {
            const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            reinterpret_cast<float4*>(r)[0] = z; reinterpret_cast<float4*>(r)[1] = z; reinterpret_cast<float4*>(r)[2] = z;
        } else {
#pragma unroll
            for (int k = 0; k < 9; k++) r[k] = 0.0f;
        }
    }
    if constexpr (!TERMS) {
        if (a.dL_dcolor != nullptr) { a.dL_dcolor[3 * (size_t)idx] = rec0.x; a.dL_dcolor[3 * (size_t)idx + 1] = rec0.y; a.dL_dcolor[3 * (size_t)idx + 2] = rec0.z; }
        a.dL_dmean2D[3 * (size_t)idx] = rec0.w; a.dL_dmean2D[3 * (size_t)idx + 1] = rec1.x;
    }
    float dcov[6]; // dL/dcov3D: stored where somebody receives it, and handed in registers to the scale / rotation path below

    // ---- dL/dconic -> dL/dcov2D -> dL/dcov3D and dL/dmean (covariance path) ----
    {
        const float* cov3D = a.cov3Ds + 6 * (size_t)idx;
        float cov3D_t[TERMS ? 6 : 1];
        if constexpr (TERMS) {
#pragma unroll
            for (int k = 0; k < 6; k++) cov3D_t[k] = opaque(cov3D[k]);
            cov3D = cov3D_t;
        }
        const float dcx = rec1.y, dcy = rec1.z, dcz = rec1.w;
        float3 t;
        t.x = view[0] * mean.x + view[4] * mean.y + view[8] * mean.z + view[12];
        t.y = view[1] * mean.x + view[5] * mean.y + view[9] * mean.z + view[13];
        t.z = view[2] * mean.x + view[6] * mean.y + view[10] * mean.z + view[14];
        const float limx = 1.3f * a.tan_fovx, limy = 1.3f * a.tan_fovy;
        const float txtz = t.x / t.z, tytz = t.y / t.z;
        t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
        t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
        const float x_grad_mul = (txtz < -limx || txtz > limx) ? 0.0f : 1.0f;
        const float y_grad_mul = (tytz < -limy || tytz > limy) ? 0.0f : 1.0f;
        Mat3 J;
        J.m[0][0] = a.h_x / t.z; J.m[0][1] = 0.0f;        J.m[0][2] = -(a.h_x * t.x) / (t.z * t.z);
        J.m[1][0] = 0.0f;        J.m[1][1] = a.h_y / t.z; J.m[1][2] = -(a.h_y * t.y) / (t.z * t.z);
        J.m[2][0] = 0.0f;        J.m[2][1] = 0.0f;        J.m[2][2] = 0.0f;
        Mat3 Wm;
        Wm.m[0][0] = view[0]; Wm.m[0][1] = view[4]; Wm.m[0][2] = view[8];
        Wm.m[1][0] = view[1]; Wm.m[1][1] = view[5]; Wm.m[1][2] = view[9];
        Wm.m[2][0] = view[2]; Wm.m[2][1] = view[6]; Wm.m[2][2] = view[10];
        Mat3 Vrk;
        Vrk.m[0][0] = cov3D[0]; Vrk.m[0][1] = cov3D[1]; Vrk.m[0][2] = cov3D[2];
        Vrk.m[1][0] = cov3D[1]; Vrk.m[1][1] = cov3D[3]; Vrk.m[1][2] = cov3D[4];
        Vrk.m[2][0] = cov3D[2]; Vrk.m[2][1] = cov3D[4]; Vrk.m[2][2] = cov3D[5];
        const Mat3 T = mat_mul(Wm, J);
        const Mat3 cov2D = mat_mul(mat_mul(mat_transpose(T), mat_transpose(Vrk)), T);
        float c_xx = cov2D.m[0][0], c_xy = cov2D.m[0][1], c_yy = cov2D.m[1][1];
        const float det_cov_orig = c_xx * c_yy - c_xy * c_xy;
        const float h_var = 0.3f;
        c_xx += h_var; c_yy += h_var;
        float dL_dc_xx = 0, dL_dc_xy = 0, dL_dc_yy = 0;
        if (a.proper_ewa_scaling) {
            // Mip-Splatting opacity scaling (reference backward.cu:214-238).  As in the reference the closed
            // form below is evaluated with the dilated c_xx / c_yy.
            const float det_plus = c_xx * c_yy - c_xy * c_xy;
            const float h_scal = sqrtf(fmaxf(0.000025f, det_cov_orig / det_plus));
            const float dL_dop_v = rec_op;
            float op_v = a.opacities[idx];
            if (a.raw & RAW_OPACITY) op_v = activate_opacity(op_v); // (recomputed from the raw value: no activated copy exists)
            const float d_h_scal = dL_dop_v * (TERMS ? opaque(op_v) : op_v);
            if constexpr (!TERMS) {
                float g_op = dL_dop_v * h_scal;
                if (a.raw & RAW_OPACITY) g_op = raw_opacity_grad(g_op, op_v);
                a.dL_dopacity[idx] = g_op;
            }
            const float d_inside_root = (det_cov_orig / det_plus) <= 0.000025f ? 0.f : d_h_scal / (2 * h_scal);
            const float x = c_xx, y = c_yy, z = c_xy, w = h_var;
            const float qd = w * w + w * (x + y) + x * y - z * z;
            const float denom_f = d_inside_root / (qd * qd);
            dL_dc_xx = w * (w * y + y * y + z * z) * denom_f;
            dL_dc_yy = w * (w * x + x * x + z * z) * denom_f;
            dL_dc_xy = -2.f * w * z * (w + x + y) * denom_f;
        } else if constexpr (!TERMS) {
            float g_op = rec_op;
            if (a.raw & RAW_OPACITY) g_op = raw_opacity_grad(g_op, activate_opacity(a.opacities[idx])); // (the one read the mask adds: 4 B per Gaussian)
            a.dL_dopacity[idx] = g_op;
        }
        const float denom = c_xx * c_yy - c_xy * c_xy;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
        if (denom2inv != 0) {
            dL_dc_xx += denom2inv * (-c_yy * c_yy * dcx + 2 * c_xy * c_yy * dcy + (denom - c_xx * c_yy) * dcz);
            dL_dc_yy += denom2inv * (-c_xx * c_xx * dcz + 2 * c_xx * c_xy * dcy + (denom - c_xx * c_yy) * dcx);
            dL_dc_xy += denom2inv * 2 * (c_xy * c_yy * dcx - (denom + 2 * c_xy * c_xy) * dcy + c_xx * c_xy * dcz);
            dcov[0] = (T.m[0][0] * T.m[0][0] * dL_dc_xx + T.m[0][0] * T.m[1][0] * dL_dc_xy + T.m[1][0] * T.m[1][0] * dL_dc_yy);
            dcov[3] = (T.m[0][1] * T.m[0][1] * dL_dc_xx + T.m[0][1] * T.m[1][1] * dL_dc_xy + T.m[1][1] * T.m[1][1] * dL_dc_yy);
            dcov[5] = (T.m[0][2] * T.m[0][2] * dL_dc_xx + T.m[0][2] * T.m[1][2] * dL_dc_xy + T.m[1][2] * T.m[1][2] * dL_dc_yy);
            dcov[1] = 2 * T.m[0][0] * T.m[0][1] * dL_dc_xx + (T.m[0][0] * T.m[1][1] + T.m[0][1] * T.m[1][0]) * dL_dc_xy + 2 * T.m[1][0] * T.m[1][1] * dL_dc_yy;
            dcov[2] = 2 * T.m[0][0] * T.m[0][2] * dL_dc_xx + (T.m[0][0] * T.m[1][2] + T.m[0][2] * T.m[1][0]) * dL_dc_xy + 2 * T.m[1][0] * T.m[1][2] * dL_dc_yy;
            dcov[4] = 2 * T.m[0][2] * T.m[0][1] * dL_dc_xx + (T.m[0][1] * T.m[1][2] + T.m[0][2] * T.m[1][1]) * dL_dc_xy + 2 * T.m[1][1] * T.m[1][2] * dL_dc_yy;
        } else {
#pragma unroll
            for (int i = 0; i < 6; i++) dcov[i] = 0;
        }
        if constexpr (!TERMS) {
            if (a.dL_dcov3D != nullptr) {
#pragma unroll
                for (int i = 0; i < 6; i++) a.dL_dcov3D[6 * (size_t)idx + i] = dcov[i];
            }
        }

        const float dL_dT00 = 2 * (T.m[0][0] * Vrk.m[0][0] + T.m[0][1] * Vrk.m[0][1] + T.m[0][2] * Vrk.m[0][2]) * dL_dc_xx +
                              (T.m[1][0] * Vrk.m[0][0] + T.m[1][1] * Vrk.m[0][1] + T.m[1][2] * Vrk.m[0][2]) * dL_dc_xy;
        const float dL_dT01 = 2 * (T.m[0][0] * Vrk.m[1][0] + T.m[0][1] * Vrk.m[1][1] + T.m[0][2] * Vrk.m[1][2]) * dL_dc_xx +
                              (T.m[1][0] * Vrk.m[1][0] + T.m[1][1] * Vrk.m[1][1] + T.m[1][2] * Vrk.m[1][2]) * dL_dc_xy;
        const float dL_dT02 = 2 * (T.m[0][0] * Vrk.m[2][0] + T.m[0][1] * Vrk.m[2][1] + T.m[0][2] * Vrk.m[2][2]) * dL_dc_xx +
                              (T.m[1][0] * Vrk.m[2][0] + T.m[1][1] * Vrk.m[2][1] + T.m[1][2] * Vrk.m[2][2]) * dL_dc_xy;
        const float dL_dT10 = 2 * (T.m[1][0] * Vrk.m[0][0] + T.m[1][1] * Vrk.m[0][1] + T.m[1][2] * Vrk.m[0][2]) * dL_dc_yy +
                              (T.m[0][0] * Vrk.m[0][0] + T.m[0][1] * Vrk.m[0][1] + T.m[0][2] * Vrk.m[0][2]) * dL_dc_xy;
        const float dL_dT11 = 2 * (T.m[1][0] * Vrk.m[1][0] + T.m[1][1] * Vrk.m[1][1] + T.m[1][2] * Vrk.m[1][2]) * dL_dc_yy +
                              (T.m[0][0] * Vrk.m[1][0] + T.m[0][1] * Vrk.m[1][1] + T.m[0][2] * Vrk.m[1][2]) * dL_dc_xy;
        const float dL_dT12 = 2 * (T.m[1][0] * Vrk.m[2][0] + T.m[1][1] * Vrk.m[2][1] + T.m[1][2] * Vrk.m[2][2]) * dL_dc_yy +
                              (T.m[0][0] * Vrk.m[2][0] + T.m[0][1] * Vrk.m[2][1] + T.m[0][2] * Vrk.m[2][2]) * dL_dc_xy;
        const float dL_dJ00 = Wm.m[0][0] * dL_dT00 + Wm.m[0][1] * dL_dT01 + Wm.m[0][2] * dL_dT02;
        const float dL_dJ02 = Wm.m[2][0] * dL_dT00 + Wm.m[2][1] * dL_dT01 + Wm.m[2][2] * dL_dT02;
        const float dL_dJ11 = Wm.m[1][0] * dL_dT10 + Wm.m[1][1] * dL_dT11 + Wm.m[1][2] * dL_dT12;
        const float dL_dJ12 = Wm.m[2][0] * dL_dT10 + Wm.m[2][1] * dL_dT11 + Wm.m[2][2] * dL_dT12;
        const float tz = 1.f / t.z, tz2 = tz * tz, tz3 = tz2 * tz;
        const float dL_dtx = x_grad_mul * -a.h_x * tz2 * dL_dJ02;
        const float dL_dty = y_grad_mul * -a.h_y * tz2 * dL_dJ12;
        float dL_dtz_ = -a.h_x * tz2 * dL_dJ00 - a.h_y * tz2 * dL_dJ11 + (2 * a.h_x * t.x) * tz3 * dL_dJ02 + (2 * a.h_y * t.y) * tz3 * dL_dJ12;
        if constexpr (INVD) dL_dtz_ -= rec_invz * tz2; // d(1/z)/dz = -1 / z^2 (every visible Gaussian: no clamp mask on this path)
        const float dL_dtz = dL_dtz_;
        dmean.x = view[0] * dL_dtx + view[1] * dL_dty + view[2] * dL_dtz;
        dmean.y = view[4] * dL_dtx + view[5] * dL_dty + view[6] * dL_dtz;
        dmean.z = view[8] * dL_dtx + view[9] * dL_dty + view[10] * dL_dtz;
        if constexpr (TERMS) {
            // t = mean @ view (+ translation row): dL/dview[i][j] = mean_i dL/dt_j.  T = J Wm with Wm.m[k][c] = view[4c + k]:
            // dL/dWm.m[k][c] = sum_r J.m[r][k] dL/dT_rc -- the transpose of the dL/dJ chain above.
            const float dt[3] = {dL_dtx, dL_dty, dL_dtz};
            const float mu[3] = {mean.x, mean.y, mean.z};
            const float dT0[3] = {dL_dT00, dL_dT01, dL_dT02}, dT1[3] = {dL_dT10, dL_dT11, dL_dT12};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                cg[3 * c + 0] = mu[c] * dt[0] + J.m[0][0] * dT0[c];
                cg[3 * c + 1] = mu[c] * dt[1] + J.m[1][1] * dT1[c];
                cg[3 * c + 2] = mu[c] * dt[2] + J.m[0][2] * dT0[c] + J.m[1][2] * dT1[c];
            }
            cg[9] = dt[0]; cg[10] = dt[1]; cg[11] = dt[2];
        }
    }

    // ---- projection path of dL/dmean (reference backward.cu:408-425) ----
    {
        const float mhw = proj[3] * mean.x + proj[7] * mean.y + proj[11] * mean.z + proj[15];
        const float m_w = 1.0f / (mhw + 0.0000001f);
        const float mul1 = (proj[0] * mean.x + proj[4] * mean.y + proj[8] * mean.z + proj[12]) * m_w * m_w;
        const float mul2 = (proj[1] * mean.x + proj[5] * mean.y + proj[9] * mean.z + proj[13]) * m_w * m_w;
        const float gx = rec0.w, gy = rec1.x;
        dmean.x += (proj[0] * m_w - proj[3] * mul1) * gx + (proj[1] * m_w - proj[3] * mul2) * gy;
        dmean.y += (proj[4] * m_w - proj[7] * mul1) * gx + (proj[5] * m_w - proj[7] * mul2) * gy;
        dmean.z += (proj[8] * m_w - proj[11] * mul1) * gx + (proj[9] * m_w - proj[11] * mul2) * gy;
        if constexpr (TERMS) { // p_hom = [mean 1] @ proj: dL/dproj[i][j] = mean_h_i dL/dp_hom_j
            const float dp[3] = {gx * m_w, gy * m_w, -(gx * mul1 + gy * mul2)}; // columns 0, 1, 3
            const float mh[4] = {mean.x, mean.y, mean.z, 1.0f};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) cg[12 + 3 * i + j] = mh[i] * dp[j];
        }
    }

    // ---- SH colour backward, including the view-direction dependence on the mean ----
    if (a.shs != nullptr) {
        float3 cam = make_float3(a.cam[0], a.cam[1], a.cam[2]);
        if constexpr (TERMS) cam = make_float3(opaque(cam.x), opaque(cam.y), opaque(cam.z));
        const float3 v = make_float3(mean.x - cam.x, mean.y - cam.y, mean.z - cam.z);
        float x, y, z;
        sh_unit_dir(v, x, y, z);
        float* const dsh = sh_row; // in place: gradient row over coefficient row
        float dRGB[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) dRGB[ch] = (ch == 0 ? rec0.x : ch == 1 ? rec0.y : rec0.z) * (TERMS ? opaque(a.clamped[3 * (size_t)idx + ch] ? 0.0f : 1.0f) : (a.clamped[3 * (size_t)idx + ch] ? 0.0f : 1.0f));
        float ddir[3] = {0, 0, 0};
        const int D = a.D;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            float dx = 0, dy = 0, dz = 0;
            const float g = dRGB[ch];
            // the coefficients this channel's direction derivative needs, read before their slots are overwritten
            float sh[16];
#pragma unroll
            for (int k = 1; k < 16; k++) sh[k] = (k < a.M && k < (D + 1) * (D + 1)) ? (TERMS ? opaque(sh_row[3 * k + ch]) : sh_row[3 * k + ch]) : 0.0f;
            if constexpr (!TERMS) {
                for (int k = (D + 1) * (D + 1); k < a.M; k++) dsh[3 * k + ch] = 0.0f; // coefficients above the active degree
                dsh[ch] = kSH_C0 * g;
            }
            if (D > 0) {
                if constexpr (!TERMS) { dsh[3 + ch] = (-kSH_C1 * y) * g; dsh[6 + ch] = (kSH_C1 * z) * g; dsh[9 + ch] = (-kSH_C1 * x) * g; }
                sh_dir_deg1(sh, dx, dy, dz);
                if (D > 1) {
                    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                    if constexpr (!TERMS) {
                        dsh[12 + ch] = (kSH_C2[0] * xy) * g; dsh[15 + ch] = (kSH_C2[1] * yz) * g; dsh[18 + ch] = (kSH_C2[2] * (2.f * zz - xx - yy)) * g;
                        dsh[21 + ch] = (kSH_C2[3] * xz) * g; dsh[24 + ch] = (kSH_C2[4] * (xx - yy)) * g;
                    }
                    sh_dir_deg2(x, y, z, sh, dx, dy, dz);
                    if (D > 2) {
                        if constexpr (!TERMS) {
                            dsh[27 + ch] = (kSH_C3[0] * y * (3.f * xx - yy)) * g; dsh[30 + ch] = (kSH_C3[1] * xy * z) * g;
                            dsh[33 + ch] = (kSH_C3[2] * y * (4.f * zz - xx - yy)) * g; dsh[36 + ch] = (kSH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy)) * g;
                            dsh[39 + ch] = (kSH_C3[4] * x * (4.f * zz - xx - yy)) * g; dsh[42 + ch] = (kSH_C3[5] * z * (xx - yy)) * g;
                            dsh[45 + ch] = (kSH_C3[6] * x * (xx - 3.f * yy)) * g;
                        }
                        sh_dir_deg3(xx, yy, zz, xy, yz, xz, sh, dx, dy, dz);
                    }
                }
            }
            if constexpr (STASH) {
                // The row holds ZEROS here (the kernel filled it: no coefficient was read), so dx, dy, dz are zeros so far, and the forward's
                // values join them.  The arithmetic above is kept on purpose: with it the compiler sees the block it sees in the STASH = false
                // kernel and makes the same fusion choices (-ffp-contract=fast) for the dsh[] terms and the normalisation below -- without it
                // dL_dsh and the camera terms came out an ulp apart from the legacy path's (profiles/EXPERIMENTS.md).  The kernel is bound by
                // its memory traffic; the extra multiplications cost it nothing measurable.
                float sx = a.sh_stash[(size_t)(3 * ch + 0) * a.P + idx], sy = a.sh_stash[(size_t)(3 * ch + 1) * a.P + idx], sz = a.sh_stash[(size_t)(3 * ch + 2) * a.P + idx];
                dx += sx; dy += sy; dz += sz;
            }
            ddir[0] += dx * g; ddir[1] += dy * g; ddir[2] += dz * g;
        }
        // derivative of the normalisation (reference auxiliary.h:179-189)
        const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
        const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
        dmean.x += ((+sum2 - v.x * v.x) * ddir[0] - v.y * v.x * ddir[1] - v.z * v.x * ddir[2]) * invsum32;
        dmean.y += (-v.x * v.y * ddir[0] + (sum2 - v.y * v.y) * ddir[1] - v.z * v.y * ddir[2]) * invsum32;
        dmean.z += (-v.x * v.z * ddir[0] - v.y * v.z * ddir[1] + (sum2 - v.z * v.z) * ddir[2]) * invsum32;
        if constexpr (TERMS) { // v = mean - campos: the negated normalisation terms above
            cg[24] = -(((+sum2 - v.x * v.x) * ddir[0] - v.y * v.x * ddir[1] - v.z * v.x * ddir[2]) * invsum32);
            cg[25] = -((-v.x * v.y * ddir[0] + (sum2 - v.y * v.y) * ddir[1] - v.z * v.y * ddir[2]) * invsum32);
            cg[26] = -((-v.x * v.z * ddir[0] - v.y * v.z * ddir[1] + (sum2 - v.z * v.z) * ddir[2]) * invsum32);
        }
    } else if constexpr (TERMS) {
        cg[24] = 0.0f; cg[25] = 0.0f; cg[26] = 0.0f; // precomputed colours: no view direction
    }
    if constexpr (TERMS) return; // (camera terms complete)
    a.dL_dmean3D[3 * (size_t)idx + 0] = dmean.x;
    a.dL_dmean3D[3 * (size_t)idx + 1] = dmean.y;
    a.dL_dmean3D[3 * (size_t)idx + 2] = dmean.z;

    // ---- covariance -> scale / rotation ----
    if (a.scales != nullptr) {
        float4 qv = reinterpret_cast<const float4*>(a.rotations)[idx];
        float s0 = a.scales[3 * (size_t)idx], s1 = a.scales[3 * (size_t)idx + 1], s2 = a.scales[3 * (size_t)idx + 2];
        float q_norm = 0.0f;
        if (a.raw != 0) { // raw parameters: the activations recomputed at the load, their chain rule at the stores below
            if (a.raw & RAW_ROTATION) qv = activate_rotation(qv, &q_norm);
            if (a.raw & RAW_SCALE) { s0 = activate_scale(s0); s1 = activate_scale(s1); s2 = activate_scale(s2); }
        }
        const float r = qv.x, x = qv.y, y = qv.z, z = qv.w;
        const Mat3 R = quat_to_mat(qv);
        const float sx = a.scale_modifier * s0, sy = a.scale_modifier * s1, sz = a.scale_modifier * s2;
        const Mat3 Mm = mat_mul(mat_diag(sx, sy, sz), R);
        const float* d = dcov;
        Mat3 dSig;
        dSig.m[0][0] = d[0];        dSig.m[0][1] = 0.5f * d[1]; dSig.m[0][2] = 0.5f * d[2];
        dSig.m[1][0] = 0.5f * d[1]; dSig.m[1][1] = d[3];        dSig.m[1][2] = 0.5f * d[4];
        dSig.m[2][0] = 0.5f * d[2]; dSig.m[2][1] = 0.5f * d[4]; dSig.m[2][2] = d[5];
        Mat3 M2;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) M2.m[i][j] = 2.0f * Mm.m[i][j];
        const Mat3 dL_dM = mat_mul(M2, dSig);
        const Mat3 Rt = mat_transpose(R);
        Mat3 dMt = mat_transpose(dL_dM);
        float gs0 = Rt.m[0][0] * dMt.m[0][0] + Rt.m[0][1] * dMt.m[0][1] + Rt.m[0][2] * dMt.m[0][2];
        float gs1 = Rt.m[1][0] * dMt.m[1][0] + Rt.m[1][1] * dMt.m[1][1] + Rt.m[1][2] * dMt.m[1][2];
        float gs2 = Rt.m[2][0] * dMt.m[2][0] + Rt.m[2][1] * dMt.m[2][1] + Rt.m[2][2] * dMt.m[2][2];
        if (a.raw & RAW_SCALE) { gs0 = raw_scale_grad(gs0, s0); gs1 = raw_scale_grad(gs1, s1); gs2 = raw_scale_grad(gs2, s2); }
        a.dL_dscale[3 * (size_t)idx + 0] = gs0;
        a.dL_dscale[3 * (size_t)idx + 1] = gs1;
        a.dL_dscale[3 * (size_t)idx + 2] = gs2;
#pragma unroll
        for (int j = 0; j < 3; j++) { dMt.m[0][j] *= sx; dMt.m[1][j] *= sy; dMt.m[2][j] *= sz; }
        float4 dq;
        dq.x = 2 * z * (dMt.m[0][1] - dMt.m[1][0]) + 2 * y * (dMt.m[2][0] - dMt.m[0][2]) + 2 * x * (dMt.m[1][2] - dMt.m[2][1]);
        dq.y = 2 * y * (dMt.m[1][0] + dMt.m[0][1]) + 2 * z * (dMt.m[2][0] + dMt.m[0][2]) + 2 * r * (dMt.m[1][2] - dMt.m[2][1]) - 4 * x * (dMt.m[2][2] + dMt.m[1][1]);
        dq.z = 2 * x * (dMt.m[1][0] + dMt.m[0][1]) + 2 * r * (dMt.m[2][0] - dMt.m[0][2]) + 2 * z * (dMt.m[1][2] + dMt.m[2][1]) - 4 * y * (dMt.m[2][2] + dMt.m[0][0]);
        dq.w = 2 * r * (dMt.m[0][1] - dMt.m[1][0]) + 2 * x * (dMt.m[2][0] + dMt.m[0][2]) + 2 * y * (dMt.m[1][2] + dMt.m[2][1]) - 4 * z * (dMt.m[1][1] + dMt.m[0][0]);
        if (a.raw & RAW_ROTATION) dq = raw_rotation_grad(dq, qv, q_norm);
        reinterpret_cast<float4*>(a.dL_drot)[idx] = dq; // gradient w.r.t. the quaternion as given (not re-normalised; raw: through the normalisation)
    }
}

// One workgroup = 256 consecutive Gaussians.  Their SH coefficients (3M floats each, 192 B at degree 3) and the SH
// gradients are the bulk of this kernel's traffic, and a thread-per-Gaussian access to them is a 192-byte-stride
// gather/scatter (measured: 4x the compulsory HBM traffic).  The block therefore moves both through LDS: coalesced
// 16-byte loads of the whole 256 x 3M block, rows padded to 3M+1 words (conflict-free row access), the gradient
// written over the coefficients in place, coalesced stores back.  Every output row of every Gaussian is written
// (zeros for the invisible ones), so none of the dL_d* outputs needs a zero-fill by the caller.
//
// CAM = true (camera gradients requested, stp_set_backward_camera_grads): each thread also forms its Gaussian's kCamTerms
// camera terms (zeros when invisible); the workgroup sums them -- over each wave with DPP / cross-lane adds, then over its
// four waves in LDS in wave order -- and writes one kCamRow-float row to a.cam_rows[blockIdx.x] with vector stores.  No
// float atomics: camera_grad_partial_kernel / camera_grad_final_kernel sum the rows in a fixed order.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum(float v) // every lane ends with the sum of all 64 (lane 0's value is the one used)
{
    v += dpp_mov<0xB1>(v);  // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);  // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v); // row_half_mirror: the other quad of the 8
    v += dpp_mov<0x140>(v); // row_mirror: the other 8 of the row
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// SPLIT (stp_set_backward_split_sh): the LDS rows come from two global spans (a.dc, a.shs) and leave as two (a.dL_ddc, a.dL_dsh), see stp_device.h:
// split SH rows; everything between the two stagings is the SPLIT = false kernel's.
// STASH (a forward with stp_set_forward_sh_stash wrote a.sh_stash): no SH row is read from global memory; the LDS rows are filled with zeros
// in the place of the stage-in and are otherwise the staging area of the coalesced dL_dsh / dL_ddc stores.  a.shs / a.dc are not read -- except
// with CAM, whose camera-terms pass keeps reading the coefficients (a camera request saves the dcov round trip and the unwanted outputs only).
template <bool CAM, bool INVD, bool SPLIT, bool STASH>
__global__ void __launch_bounds__(256) preprocess_backward_kernel(const BwdPreArgs a)
{
    extern __shared__ float s_rows[]; // [256][3M + 1]
    const int tid = (int)threadIdx.x;
    const int base = ((int)blockIdx.x + a.block0) * 256;
    const int idx = base + tid;
    const int rows = min(256, a.P - base);
    const int row_len = 3 * a.M, row_stride = row_len + 1;
    const bool have_sh = a.shs != nullptr && a.M > 0;
    float cg[CAM ? kCamTerms : 1];
    if constexpr (CAM) {
#pragma unroll
        for (int k = 0; k < kCamTerms; k++) cg[k] = 0.0f;
    }
    // CAM with STASH: the camera terms depend on the nine numbers too (dL/dcampos), and they stay the legacy path's bit for bit: the rows ARE staged
    // in, the camera-terms pass reads them as it always did, and each thread clears its own row in front of its gradient pass (below).
    constexpr bool STAGE_IN = !STASH || CAM;
    if (have_sh && !STAGE_IN) { // zeros in the place of the coefficients (gaussian_backward: STASH)
        for (int f = tid; f < rows * row_stride; f += 256) s_rows[f] = 0.0f;
        __syncthreads();
    }
    if (have_sh && STAGE_IN) {
        const float* __restrict__ src = a.shs + (size_t)base * (SPLIT ? row_len - 3 : row_len);
        const int total = rows * row_len;
        if constexpr (SPLIT) {
            const float* __restrict__ src_dc = a.dc + (size_t)base * 3;
            const bool vec = aligned16(a.dc, row_len > 3 ? a.shs : nullptr); // (views such as rest[1:] are 4-byte aligned only)
            if (row_len == 48 && rows == 256 && vec) {
                float4 v[12];
                split48_load(src_dc, src, tid, v);
                split48_store(s_rows, tid, v);
            } else {
                stage_span_in<256>(src_dc, s_rows, tid, rows, 3, 0, row_stride, vec);
                stage_span_in<256>(src, s_rows, tid, rows, row_len - 3, 3, row_stride, vec);
            }
        } else if (row_len == 48 && rows == 256) { // SH degree 3 (M = 16), full block: every load in flight at once (stp_device.h)
            stage_rows_in<256, 48>(src, s_rows, tid);
        } else if ((row_len & 3) == 0) {
            for (int f = 4 * tid; f < total; f += 4 * 256) {
                const float4 v = *reinterpret_cast<const float4*>(src + f);
                const int r = f / row_len, j = f - r * row_len;
                float* d = s_rows + r * row_stride + j;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        } else {
            for (int f = tid; f < total; f += 256) {
                const int r = f / row_len, j = f - r * row_len;
                s_rows[r * row_stride + j] = src[f];
            }
        }
        __syncthreads();
    }
    if (idx < a.P) {
        if (a.radii[idx] > 0) {
            if constexpr (CAM) {
                // the camera terms first (they read the SH coefficients the gradient pass overwrites), in a block of their own behind an
                // opaque branch: the gradient pass below is the CAM = false kernel's, arithmetic for arithmetic
                int go = 1;
                asm volatile("" : "+s"(go));
                if (go) gaussian_backward<true, INVD, false>(a, idx, s_rows + tid * row_stride, cg);
                if constexpr (STASH) { // (its own row, which no other thread reads before the barrier in front of the stores)
                    if (have_sh) for (int j = 0; j < row_len; j++) s_rows[tid * row_stride + j] = 0.0f;
                    asm volatile("" ::: "memory"); // the gradient pass loads the zeros as it loads coefficients: values the compiler does not know
                }
            }
            gaussian_backward<false, INVD, STASH>(a, idx, s_rows + tid * row_stride, cg);
        } else { // invisible: all gradients are zero
            if (a.dL_dcolor != nullptr) { a.dL_dcolor[3 * (size_t)idx] = 0.0f; a.dL_dcolor[3 * (size_t)idx + 1] = 0.0f; a.dL_dcolor[3 * (size_t)idx + 2] = 0.0f; }
            a.dL_dmean2D[3 * (size_t)idx] = 0.0f; a.dL_dmean2D[3 * (size_t)idx + 1] = 0.0f;
            a.dL_dopacity[idx] = 0.0f;
            if (a.dL_dcov3D != nullptr) {
#pragma unroll
                for (int i = 0; i < 6; i++) a.dL_dcov3D[6 * (size_t)idx + i] = 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 3; i++) a.dL_dmean3D[3 * (size_t)idx + i] = 0.0f;
            if (a.scales != nullptr) {
#pragma unroll
                for (int i = 0; i < 3; i++) a.dL_dscale[3 * (size_t)idx + i] = 0.0f;
                reinterpret_cast<float4*>(a.dL_drot)[idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            if (have_sh) for (int j = 0; j < row_len; j++) s_rows[tid * row_stride + j] = 0.0f;
        }
        a.dL_dmean2D[3 * (size_t)idx + 2] = 0.0f; // z component: never used by the reference either
    }
    if (have_sh) {
        __syncthreads();
        float* __restrict__ dst = a.dL_dsh + (size_t)base * (SPLIT ? row_len - 3 : row_len);
        const int total = rows * row_len;
        if constexpr (SPLIT) {
            float* __restrict__ dst_dc = a.dL_ddc + (size_t)base * 3;
            const bool vec = aligned16(a.dL_ddc, row_len > 3 ? a.dL_dsh : nullptr);
            if (row_len == 48 && rows == 256 && vec) {
                split48_out(dst_dc, dst, s_rows, tid);
            } else {
                stage_span_out<256>(dst_dc, s_rows, tid, rows, 3, 0, row_stride, vec);
                stage_span_out<256>(dst, s_rows, tid, rows, row_len - 3, 3, row_stride, vec);
            }
        } else if (row_len == 48 && rows == 256) {
            stage_rows_out<256, 48>(dst, s_rows, tid);
        } else if ((row_len & 3) == 0) {
            for (int f = 4 * tid; f < total; f += 4 * 256) {
                const int r = f / row_len, j = f - r * row_len;
                const float* d = s_rows + r * row_stride + j;
                *reinterpret_cast<float4*>(dst + f) = make_float4(d[0], d[1], d[2], d[3]);
            }
        } else {
            for (int f = tid; f < total; f += 256) {
                const int r = f / row_len, j = f - r * row_len;
                dst[f] = s_rows[r * row_stride + j];
            }
        }
    }
    if constexpr (CAM) {
        __shared__ float s_cam[4][kCamRow]; // per-wave sums
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int k = 0; k < kCamTerms; k++) {
            const float s = wave_sum(cg[k]);
            if (lane == 0) s_cam[wave][k] = s;
        }
        __syncthreads();
        if (tid < kCamRow / 4) { // 8 threads, 4 columns each: the four waves in order, one 16-byte store
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = 4 * tid + q;
                o[q] = k < kCamTerms ? ((s_cam[0][k] + s_cam[1][k]) + s_cam[2][k]) + s_cam[3][k] : 0.0f;
            }
            reinterpret_cast<float4*>(a.cam_rows + (size_t)blockIdx.x * kCamRow)[tid] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// Sum of the per-workgroup rows, in two fixed-order steps (no atomics: the result depends only on the rows and their count).
// Step 1: block g of `parts` sums rows [g * n / parts, (g + 1) * n / parts) in double -- 32 groups of 32 lanes, lane = column, group r
// takes every 32nd row -- and writes one row of kCamRow doubles.  Step 2: one block sums the `parts` rows and writes the three outputs
// in full, the entries the forward never reads as zeros.
__global__ void __launch_bounds__(1024) camera_grad_partial_kernel(const float* __restrict__ rows, int n_rows, int parts, double* __restrict__ partial)
{
    __shared__ double s[32][kCamRow];
    const int c = (int)threadIdx.x & 31, grp = (int)threadIdx.x >> 5;
    const int r0 = (int)((long long)n_rows * blockIdx.x / parts), r1 = (int)((long long)n_rows * (blockIdx.x + 1) / parts);
    double acc = 0.0;
    for (int r = r0 + grp; r < r1; r += 32) acc += (double)rows[(size_t)r * kCamRow + c];
    s[grp][c] = acc;
    __syncthreads();
    if (grp == 0) {
        double t = 0.0;
        for (int k = 0; k < 32; k++) t += s[k][c];
        partial[(size_t)blockIdx.x * kCamRow + c] = t;
    }
}

__global__ void __launch_bounds__(1024) camera_grad_final_kernel(const double* __restrict__ partial, int parts, float* __restrict__ dview,
                                                                 float* __restrict__ dproj, float* __restrict__ dcam)
{
    __shared__ double s[32][kCamRow];
    const int tid = (int)threadIdx.x, c = tid & 31, grp = tid >> 5;
    double acc = 0.0;
    for (int g = grp; g < parts; g += 32) acc += partial[(size_t)g * kCamRow + c];
    s[grp][c] = acc;
    __syncthreads();
    if (grp == 0) {
        double t = 0.0;
        for (int k = 0; k < 32; k++) t += s[k][c];
        s[0][c] = t; // (each lane reads its own column above and writes it here: no other lane reads s[0][c] before the barrier)
    }
    __syncthreads();
    if (tid < 16) { // view[i][j]: column 3 is never read
        const int i = tid >> 2, j = tid & 3;
        dview[tid] = j == 3 ? 0.0f : (float)s[0][3 * i + j];
    } else if (tid < 32) { // proj[i][j]: column 2 is never read
        const int i = (tid - 16) >> 2, j = (tid - 16) & 3;
        dproj[tid - 16] = j == 2 ? 0.0f : (float)s[0][12 + 3 * i + (j == 3 ? 2 : j)];
    } else if (tid < 35) {
        dcam[tid - 32] = (float)s[0][24 + tid - 32];
    }
}

// absgrad request (stp_set_backward_absgrad): slots STP_GRAD_RECORD_ABS, + 1 of every visible Gaussian's record -> out[3 i], out[3 i + 1];
// column 2 and the invisible Gaussians get zeros (every row is written: the caller does no zero-fill).  A kernel of its own, launched IN
// FRONT of preprocess_backward_kernel -- which clears the records behind its read (clear_rec) and stays the kernel it was.  12 + 4 bytes
// read and 12 written per Gaussian.
__global__ void __launch_bounds__(256) absgrad_extract_kernel(int P, const int* __restrict__ radii, const float* __restrict__ rec, int stride,
                                                              float* __restrict__ out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= P) return;
    float ax = 0.0f, ay = 0.0f;
    if (radii[i] > 0) {
        ax = rec[(size_t)stride * i + STP_GRAD_RECORD_ABS];
        ay = rec[(size_t)stride * i + STP_GRAD_RECORD_ABS + 1];
    }
    out[3 * (size_t)i] = ax; out[3 * (size_t)i + 1] = ay; out[3 * (size_t)i + 2] = 0.0f;
}

// blend-statistics request (stp_set_backward_blend_stats): slots STP_GRAD_RECORD_STATS .. + 2 of every visible Gaussian's record (sum and count
// as floats, the maximum as a non-negative float's bits, which are the float) -> out[3 i .. 3 i + 2]; the invisible Gaussians get zeros
// (every row is written).  Like the kernel above in front of preprocess_backward_kernel, whose clear_rec covers the first 48 bytes of a
// record only -- slots 12, 13 lie behind them --: with `clear` this kernel zeroes the three slots behind its read.
__global__ void __launch_bounds__(256) blend_stats_extract_kernel(int P, const int* __restrict__ radii, float* __restrict__ rec, int stride, int clear,
                                                                  float* __restrict__ out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= P) return;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (radii[i] > 0) {
        float* const r = rec + (size_t)stride * i + STP_GRAD_RECORD_STATS;
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = r[k];
        if (clear) {
#pragma unroll
            for (int k = 0; k < 3; k++) r[k] = 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = v[k];
}

constexpr int kCamMaxParts = 256;
int camera_grad_parts(int n_rows) { return max(1, min(kCamMaxParts, (n_rows + 191) / 192)); }

} // namespace

size_t camera_grad_workspace_bytes(int P)
{
    const size_t n_rows = (size_t)(P > 0 ? (P + 255) / 256 : 0);
    return n_rows * kCamRow * sizeof(float) + (size_t)kCamMaxParts * kCamRow * sizeof(double);
}

hipError_t launch_camera_grad_finalize(int P, const CameraGradRequest& cam, hipStream_t st)
{
    const int n_rows = P > 0 ? (P + 255) / 256 : 0;
    const int parts = camera_grad_parts(n_rows);
    const float* rows = reinterpret_cast<const float*>(cam.workspace);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(cam.workspace) + (size_t)n_rows * kCamRow * sizeof(float));
    hipLaunchKernelGGL(camera_grad_partial_kernel, dim3(parts), dim3(1024), 0, st, rows, n_rows, parts, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(camera_grad_final_kernel, dim3(1), dim3(1024), 0, st, (const double*)partial, parts, cam.dL_dview, cam.dL_dproj, cam.dL_dcam);
    return hipGetLastError();
}

hipError_t launch_preprocess_backward(const FrameParams& f, const GeometryState& g, const int* radii, const BackwardParams& bw, hipStream_t st)
{
    const bool cam = bw.cam.dL_dview != nullptr; // (the caller has refused a chunked half with a request)
    BwdPreArgs a;
    a.P = f.P; a.D = f.D; a.M = f.M; a.proper_ewa_scaling = f.s.proper_ewa_scaling;
    a.h_x = f.focal_x; a.h_y = f.focal_y; a.tan_fovx = f.tan_fovx; a.tan_fovy = f.tan_fovy; a.scale_modifier = f.scale_modifier;
    a.means3D = f.means3D; a.radii = radii; a.shs = f.shs; a.clamped = g.clamped; a.opacities = f.opacities; a.scales = f.scales;
    a.rotations = f.rotations; a.cov3Ds = f.cov3D_precomp ? f.cov3D_precomp : g.cov3D; // reference rasterizer_impl.cu:500
    a.view = f.viewmatrix; a.proj = f.projmatrix; a.cam = f.cam_pos;
    a.dL_dmean2D = bw.dL_dmean2D; a.grad_rec = bw.grad_rec; a.grad_stride = bw.grad_stride; a.clear_rec = bw.clear_rec; a.dL_dopacity = bw.dL_dopacity; a.dL_dcolor = bw.dL_dcolor;
    a.dL_dmean3D = bw.dL_dmean3D; a.dL_dcov3D = bw.dL_dcov3D; a.dL_dsh = bw.dL_dsh; a.dL_dscale = bw.dL_dscale; a.dL_drot = bw.dL_drot;
    a.cam_rows = cam ? reinterpret_cast<float*>(bw.cam.workspace) : nullptr;
    const bool split = f.sh_dc != nullptr && bw.dL_ddc != nullptr; // stp_set_backward_split_sh
    a.dc = f.sh_dc; a.dL_ddc = bw.dL_ddc;
    if (split && a.shs == nullptr) a.shs = a.dc; // M == 1: no rest; the kernel's "have SH" test wants a pointer and reads nothing through this one
    const bool invd = bw.dL_dinvdepth != nullptr; // (stp_set_backward_invdepth; the caller has refused a chunked half and compact records with it: slot 14 exists)
    // the forward's stash (carve_geometry; stp_api.hip has asked the buffer whether one was written): only where there are SH rows to spare
    const bool stash = bw.sh_stash != nullptr && a.shs != nullptr && a.M > 0;
    a.sh_stash = stash ? bw.sh_stash : nullptr;
    a.raw = f.raw_params; // stp_set_backward_raw_params (every chunk of a chunked half: the request is the call's)
    using Kernel = void (*)(const BwdPreArgs);
    static const Kernel kernels[16] = {
        preprocess_backward_kernel<false, false, false, false>, preprocess_backward_kernel<false, false, true, false>,
        preprocess_backward_kernel<false, true, false, false>,  preprocess_backward_kernel<false, true, true, false>,
        preprocess_backward_kernel<true, false, false, false>,  preprocess_backward_kernel<true, false, true, false>,
        preprocess_backward_kernel<true, true, false, false>,   preprocess_backward_kernel<true, true, true, false>,
        preprocess_backward_kernel<false, false, false, true>,  preprocess_backward_kernel<false, false, true, true>,
        preprocess_backward_kernel<false, true, false, true>,   preprocess_backward_kernel<false, true, true, true>,
        preprocess_backward_kernel<true, false, false, true>,   preprocess_backward_kernel<true, false, true, true>,
        preprocess_backward_kernel<true, true, false, true>,    preprocess_backward_kernel<true, true, true, true>};
    const Kernel kernel = kernels[(stash ? 8 : 0) + (cam ? 4 : 0) + (invd ? 2 : 0) + (split ? 1 : 0)];
    const size_t lds = (a.shs != nullptr && a.M > 0) ? (size_t)256 * (3 * a.M + 1) * sizeof(float) : 0;
    if (lds > 64 * 1024) { // above the default dynamic-LDS limit (M > 21: no SH degree the reference knows)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int n_blocks = (f.P + 255) / 256;
    int b0 = 0, b1 = n_blocks;
    if (bw.chunks > 1) { // Gaussians are independent in this half: a tile-row shard runs it on the id range whose records have been all-reduced already
        b0 = (int)((long long)n_blocks * bw.chunk / bw.chunks);
        b1 = (int)((long long)n_blocks * (bw.chunk + 1) / bw.chunks);
    }
    a.block0 = b0;
    if (b1 <= b0) return hipSuccess;
    if (bw.absgrad != nullptr) { // (the caller has refused a chunked half and compact records with the request: all Gaussians, slots 9, 10 exist)
        hipLaunchKernelGGL(absgrad_extract_kernel, dim3(n_blocks), dim3(256), 0, st, f.P, radii, (const float*)bw.grad_rec, bw.grad_stride, bw.absgrad);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (bw.blend_stats != nullptr) { // (refused like the one above: all Gaussians, slots 11..13 exist)
        hipLaunchKernelGGL(blend_stats_extract_kernel, dim3(n_blocks), dim3(256), 0, st, f.P, radii, bw.grad_rec, bw.grad_stride, bw.clear_rec, bw.blend_stats);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (cam) {
        hipLaunchKernelGGL(kernel, dim3(b1 - b0), dim3(256), lds, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        return launch_camera_grad_finalize(f.P, bw.cam, st);
    }
    hipLaunchKernelGGL(kernel, dim3(b1 - b0), dim3(256), lds, st, a);
    return hipGetLastError();
}

} // namespace stp
