// stp_loss.hip -- the fused photometric loss of stp_photometric_forward / stp_photometric_backward (no counterpart in the reference; the
// semantics are those of a 3DGS trainer's l1_loss and ssim() with window_size = 11 and size_average = True, the pair the `fused-ssim`
// extension replaces):
//     out[0] = mean |x - y|        out[1] = mean m,   m = A B / (Cc D)
//     A = 2 mu1 mu2 + C1,  B = 2 s12 + C2,  Cc = mu1^2 + mu2^2 + C1,  D = s1 + s2 + C2
//     mu1 = blur(x), mu2 = blur(y), s1 = blur(x^2) - mu1^2, s2 = blur(y^2) - mu2^2, s12 = blur(x y) - mu1 mu2
// over every (H, W) plane independently, blur = the 11 x 11 Gaussian window (sigma 1.5) with ZERO padding of 5.
//
// Tiling.  A workgroup of 256 threads (four wave64s) owns one LOSS_TW x LOSS_TH = 64 x 16 output tile of one plane; the grid is the flat
// list of (plane, tile row, tile column).  The tile of x and of y is staged with a 5-pixel halo (74 x 26, zeros outside the image) into
// LDS; the window runs separably: a horizontal pass writes the five quantities x, y, x^2, y^2, x y of the 26 rows x 64 columns to LDS
// (lane = column: consecutive lanes on consecutive words in every read and write), a vertical pass gives every thread the FOUR
// consecutive rows 4 * wave .. 4 * wave + 3 of its column from 14 values per quantity.  22 taps per quantity and pixel, not 121.
// LDS: 15.4 KB of inputs + 33.3 KB of horizontal results (forward), 23.1 + 20.0 KB (backward): three workgroups per CU.
//
// Arithmetic.  The window is symmetric, so a pass is  w5 v5 + sum_j w_j (v_j + v_{10-j}):  five additions and a chain of one product and
// five fused multiply-adds, in which a value meets at most 6 roundings -- 12 for the two passes, 13 with the product in front of them
// (tests/torch_ref_photometric.py counts the same).  s1, s2 and s12 are formed with one fused multiply-add each (mu^2 is not rounded on
// its own).  Division is the correctly rounded one.
//
// Forward with maps stores the three derivative maps the backward needs (3 * planes * H * W floats: map k of element e at k * n + e)
//     d1 = dm/dmu1 = 2 [mu2 (B - A) + mu1 m (Cc - D)] / (Cc D)      d2 = dm/ds1 = -m / D      d3 = dm/ds12 = 2 A / (Cc D)
// (d1 is the four-term expression of the header with its terms paired).  The backward stages s * d1, s * d2, s * d3 (s = g1 / n) with
// halo, blurs them the same way (the window is symmetric: the adjoint of blur is blur) and writes
//     dL/dx = blur(s d1) + 2 x blur(s d2) + y blur(s d3) + (g0 / n) sign(x - y).
// g0 and g1 are read from device memory.
//
// Sums in a FIXED order, no atomics: a thread adds its four pixels, a butterfly adds inside each wave, the four waves are added in order
// -> two floats per workgroup; ONE workgroup (photometric_sum_kernel) adds those rows, thread t the rows t, t + 256, ... in order, the
// same tree after that, and divides by n.  Equal inputs give equal bits.
#include "stp_internal.h"

namespace stp {

namespace {

constexpr int LOSS_BLOCK = 256;
constexpr int LOSS_TW = 64, LOSS_TH = 16;   // output tile (== STP_PHOTOMETRIC_TILE_W / _H of the header)
constexpr int LOSS_R = 5;                   // window radius
constexpr int LOSS_HW = LOSS_TW + 2 * LOSS_R, LOSS_HH = LOSS_TH + 2 * LOSS_R; // 74 x 26 with halo
constexpr int LOSS_ROWS = LOSS_TH / (LOSS_BLOCK / 64);                        // rows of a column one thread owns (4)
static_assert(LOSS_TW == 64 && LOSS_TW == STP_PHOTOMETRIC_TILE_W && LOSS_TH == STP_PHOTOMETRIC_TILE_H, "a wave is one tile row");

// exp(-(k - 5)^2 / 4.5) / sum, k = 0 .. 5 (w[10 - k] = w[k]): the float32 roundings
constexpr float LOSS_WIN[6] = {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f};
constexpr float LOSS_C1 = 0.01f * 0.01f, LOSS_C2 = 0.03f * 0.03f;

// one pass of the window over v[0 .. 10]
__device__ __forceinline__ float window11(const float v0, const float v1, const float v2, const float v3, const float v4, const float v5,
                                          const float v6, const float v7, const float v8, const float v9, const float v10)
{
    float a = LOSS_WIN[5] * v5;
    a = __fmaf_rn(LOSS_WIN[4], v4 + v6, a);
    a = __fmaf_rn(LOSS_WIN[3], v3 + v7, a);
    a = __fmaf_rn(LOSS_WIN[2], v2 + v8, a);
    a = __fmaf_rn(LOSS_WIN[1], v1 + v9, a);
    a = __fmaf_rn(LOSS_WIN[0], v0 + v10, a);
    return a;
}
__device__ __forceinline__ float window11(const float* v) { return window11(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]); }

// the workgroup's sum of v in every thread: butterfly inside every wave (the same tree in every lane), then the four waves in order
__device__ __forceinline__ float block_sum(float v, float* s_wave)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads(); // (s_wave is used once per quantity)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

struct LossTile { int plane, x0, y0; };
// blockIdx.x -> (plane, tile): wave-uniform, scalar code
__device__ __forceinline__ LossTile loss_tile(const int tiles_x, const int tiles_y)
{
    const uint32_t per_plane = (uint32_t)tiles_x * (uint32_t)tiles_y;
    const uint32_t plane = blockIdx.x / per_plane, t = blockIdx.x - plane * per_plane;
    const uint32_t ty = t / (uint32_t)tiles_x, tx = t - ty * (uint32_t)tiles_x;
    return LossTile{(int)plane, (int)tx * LOSS_TW, (int)ty * LOSS_TH};
}

// the 74 x 26 halo tile of one plane into LDS, scaled; zeros outside the image
__device__ __forceinline__ void stage_halo(float (*dst)[LOSS_HW], const float* __restrict__ src, const int x0, const int y0, const int H, const int W,
                                           const float scale)
{
    for (int i = (int)threadIdx.x; i < LOSS_HH * LOSS_HW; i += LOSS_BLOCK) {
        const int r = i / LOSS_HW, c = i - r * LOSS_HW;
        const int gy = y0 - LOSS_R + r, gx = x0 - LOSS_R + c;
        float v = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = src[(size_t)gy * W + gx] * scale; // (plane offset is in src; gy * W + gx < n < 2^31)
        dst[r][c] = v;
    }
}

template <bool MAPS>
__global__ void __launch_bounds__(LOSS_BLOCK) photometric_forward_kernel(const float* __restrict__ image, const float* __restrict__ target, const int H, const int W,
                                                                         const int tiles_x, const int tiles_y, const size_t n, float* __restrict__ maps,
                                                                         float* __restrict__ partials)
{
    __shared__ float s_x[LOSS_HH][LOSS_HW], s_y[LOSS_HH][LOSS_HW];
    __shared__ float s_h[5][LOSS_HH][LOSS_TW];
    __shared__ float s_wave[LOSS_BLOCK / 64];
    const LossTile t = loss_tile(tiles_x, tiles_y);
    const size_t plane_off = (size_t)t.plane * H * W;
    stage_halo(s_x, image + plane_off, t.x0, t.y0, H, W, 1.0f);
    stage_halo(s_y, target + plane_off, t.x0, t.y0, H, W, 1.0f);
    __syncthreads();

    const int col = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // horizontal pass: rows wave, wave + 4, ... of the 26
    for (int r = wave; r < LOSS_HH; r += LOSS_BLOCK / 64) {
        float x[11], y[11], xx[11], yy[11], xy[11];
#pragma unroll
        for (int j = 0; j < 11; j++) {
            x[j] = s_x[r][col + j];
            y[j] = s_y[r][col + j];
            xx[j] = x[j] * x[j];
            yy[j] = y[j] * y[j];
            xy[j] = x[j] * y[j];
        }
        s_h[0][r][col] = window11(x);
        s_h[1][r][col] = window11(y);
        s_h[2][r][col] = window11(xx);
        s_h[3][r][col] = window11(yy);
        s_h[4][r][col] = window11(xy);
    }
    __syncthreads();

    // vertical pass: the thread's four rows of its column, 14 values per quantity
    float st[5][LOSS_ROWS];
    const int r0 = wave * LOSS_ROWS;
#pragma unroll
    for (int q = 0; q < 5; q++) {
        float v[LOSS_ROWS + 10];
#pragma unroll
        for (int j = 0; j < LOSS_ROWS + 10; j++) v[j] = s_h[q][r0 + j][col];
#pragma unroll
        for (int o = 0; o < LOSS_ROWS; o++) st[q][o] = window11(v + o);
    }

    float sum_l1 = 0.0f, sum_m = 0.0f;
    const int gx = t.x0 + col;
#pragma unroll
    for (int o = 0; o < LOSS_ROWS; o++) {
        const int gy = t.y0 + r0 + o;
        if (gx < W && gy < H) {
            const float mu1 = st[0][o], mu2 = st[1][o];
            const float s1 = __fmaf_rn(-mu1, mu1, st[2][o]), s2 = __fmaf_rn(-mu2, mu2, st[3][o]), s12 = __fmaf_rn(-mu1, mu2, st[4][o]);
            const float A = __fmaf_rn(2.0f * mu1, mu2, LOSS_C1), B = __fmaf_rn(2.0f, s12, LOSS_C2);
            const float Cc = __fmaf_rn(mu1, mu1, __fmaf_rn(mu2, mu2, LOSS_C1)), D = (s1 + s2) + LOSS_C2;
            const float rcd = 1.0f / (Cc * D);
            const float m = (A * B) * rcd;
            sum_m += m;
            sum_l1 += fabsf(s_x[r0 + o + LOSS_R][col + LOSS_R] - s_y[r0 + o + LOSS_R][col + LOSS_R]);
            if constexpr (MAPS) {
                const size_t e = plane_off + (size_t)gy * W + gx;
                maps[e] = 2.0f * __fmaf_rn(mu2, B - A, (mu1 * m) * (Cc - D)) * rcd;
                maps[n + e] = -m / D;
                maps[2 * n + e] = (2.0f * A) * rcd;
            }
        }
    }
    const float bl1 = block_sum(sum_l1, s_wave);
    const float bm = block_sum(sum_m, s_wave);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = bl1;
        partials[2 * (size_t)blockIdx.x + 1] = bm;
    }
}

// one workgroup: the `groups` partial rows, thread t rows t, t + 256, ... in order, then the workgroup's sum, divided by n
__global__ void __launch_bounds__(LOSS_BLOCK) photometric_sum_kernel(const float* __restrict__ partials, const uint32_t groups, const float n, float* __restrict__ out2)
{
    __shared__ float s_wave[LOSS_BLOCK / 64];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        float acc = 0.0f;
        for (uint32_t r = threadIdx.x; r < groups; r += LOSS_BLOCK) acc += partials[2 * (size_t)r + k];
        const float s = block_sum(acc, s_wave);
        if (threadIdx.x == 0) out2[k] = s / n;
    }
}

__global__ void __launch_bounds__(LOSS_BLOCK) photometric_backward_kernel(const float* __restrict__ image, const float* __restrict__ target, const float* __restrict__ maps,
                                                                          const float* __restrict__ dL_dout2, const int H, const int W, const int tiles_x,
                                                                          const int tiles_y, const size_t n, const float nf, float* __restrict__ dL_dimage)
{
    __shared__ float s_d[3][LOSS_HH][LOSS_HW];
    __shared__ float s_h[3][LOSS_HH][LOSS_TW];
    const LossTile t = loss_tile(tiles_x, tiles_y);
    const size_t plane_off = (size_t)t.plane * H * W;
    const float l1w = dL_dout2[0] / nf, s = dL_dout2[1] / nf;
#pragma unroll
    for (int k = 0; k < 3; k++) stage_halo(s_d[k], maps + (size_t)k * n + plane_off, t.x0, t.y0, H, W, s);
    __syncthreads();

    const int col = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < LOSS_HH; r += LOSS_BLOCK / 64) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float v[11];
#pragma unroll
            for (int j = 0; j < 11; j++) v[j] = s_d[k][r][col + j];
            s_h[k][r][col] = window11(v);
        }
    }
    __syncthreads();

    float b[3][LOSS_ROWS];
    const int r0 = wave * LOSS_ROWS;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float v[LOSS_ROWS + 10];
#pragma unroll
        for (int j = 0; j < LOSS_ROWS + 10; j++) v[j] = s_h[k][r0 + j][col];
#pragma unroll
        for (int o = 0; o < LOSS_ROWS; o++) b[k][o] = window11(v + o);
    }
    const int gx = t.x0 + col;
#pragma unroll
    for (int o = 0; o < LOSS_ROWS; o++) {
        const int gy = t.y0 + r0 + o;
        if (gx < W && gy < H) {
            const size_t e = plane_off + (size_t)gy * W + gx;
            const float x = image[e], y = target[e];
            const float sgn = x > y ? l1w : (x < y ? -l1w : 0.0f); // (a NaN pixel: 0)
            dL_dimage[e] = __fmaf_rn(y, b[2][o], __fmaf_rn(2.0f * x, b[1][o], b[0][o])) + sgn;
        }
    }
}

} // namespace

uint32_t photometric_groups(int planes, int H, int W)
{
    const uint64_t g = (uint64_t)planes * ((H + LOSS_TH - 1) / LOSS_TH) * ((W + LOSS_TW - 1) / LOSS_TW); // <= planes * H * W < 2^31
    return (uint32_t)g;
}

int launch_photometric_forward(int planes, int H, int W, const float* image, const float* target, float* out2, float* maps, float* workspace,
                               hipStream_t st, hipError_t* err)
{
    const int tiles_x = (W + LOSS_TW - 1) / LOSS_TW, tiles_y = (H + LOSS_TH - 1) / LOSS_TH;
    const uint32_t groups = photometric_groups(planes, H, W);
    const size_t n = (size_t)planes * H * W;
    *err = hipSuccess;
    if (maps) hipLaunchKernelGGL(photometric_forward_kernel<true>, dim3(groups), dim3(LOSS_BLOCK), 0, st, image, target, H, W, tiles_x, tiles_y, n, maps, workspace);
    else hipLaunchKernelGGL(photometric_forward_kernel<false>, dim3(groups), dim3(LOSS_BLOCK), 0, st, image, target, H, W, tiles_x, tiles_y, n, maps, workspace);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 0; }
    hipLaunchKernelGGL(photometric_sum_kernel, dim3(1), dim3(LOSS_BLOCK), 0, st, workspace, groups, (float)n, out2);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 1; }
    return 2;
}

int launch_photometric_backward(int planes, int H, int W, const float* image, const float* target, const float* maps, const float* dL_dout2,
                                float* dL_dimage, hipStream_t st, hipError_t* err)
{
    const int tiles_x = (W + LOSS_TW - 1) / LOSS_TW, tiles_y = (H + LOSS_TH - 1) / LOSS_TH;
    const size_t n = (size_t)planes * H * W;
    *err = hipSuccess;
    hipLaunchKernelGGL(photometric_backward_kernel, dim3(photometric_groups(planes, H, W)), dim3(LOSS_BLOCK), 0, st, image, target, maps, dL_dout2, H, W,
                       tiles_x, tiles_y, n, (float)n, dL_dimage);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 0; }
    return 1;
}

} // namespace stp
