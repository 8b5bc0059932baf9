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
//
// The training loss (stp_training_loss_forward / _backward) is the same pair with the trainer's exposure, clamp, alpha mask and depth term:
// kernels of its own further down, under a comment that states the colour transform's fixed chain
//     v_j = fma(E[2][j], x_2, fma(E[1][j], x_1, fma(E[0][j], x_0, E[j][3])))
// Both pairs are their own staging around ONE copy of the numerics, the __device__ __forceinline__ pieces ssim_tile, blur_maps,
// photometric_gradient, rows_sum / photometric_means and loss_tile_at.  Every fused operation of a piece is an explicit __fmaf_rn,
// so it is the same arithmetic in a caller under `fp contract(off)` and in one without.  What holds the bits of both pairs in place is
// tests/test_gpu_loss_bits.py: outputs recorded from the kernels as they were before the pieces were shared.
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
// entry idx of the flat (plane, tile row, tile column) list: wave-uniform, scalar code
__device__ __forceinline__ LossTile loss_tile_at(const uint32_t idx, const int tiles_x, const int tiles_y)
{
    const uint32_t per_plane = (uint32_t)tiles_x * (uint32_t)tiles_y;
    const uint32_t plane = idx / per_plane, t = idx - plane * per_plane;
    const uint32_t ty = t / (uint32_t)tiles_x, tx = t - ty * (uint32_t)tiles_x;
    return LossTile{(int)plane, (int)tx * LOSS_TW, (int)ty * LOSS_TH};
}
__device__ __forceinline__ LossTile loss_tile(const int tiles_x, const int tiles_y) { return loss_tile_at(blockIdx.x, tiles_x, tiles_y); }

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

// The forward of one tile from its staged halo tiles s_x, s_y (the staging's barrier included): the two passes of the window, the SSIM of the
// thread's four pixels, with MAPS the three derivative maps at plane_off, and the tile's sums of |x - y| and of m into row[0], row[1]
template <bool MAPS>
__device__ __forceinline__ void ssim_tile(const float (&s_x)[LOSS_HH][LOSS_HW], const float (&s_y)[LOSS_HH][LOSS_HW], float (&s_h)[5][LOSS_HH][LOSS_TW],
                                          float (&s_wave)[LOSS_BLOCK / 64], const LossTile t, const size_t plane_off, const int H, const int W, const size_t n,
                                          float* __restrict__ maps, float* __restrict__ row)
{
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
        row[0] = bl1;
        row[1] = bm;
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
    ssim_tile<MAPS>(s_x, s_y, s_h, s_wave, t, plane_off, H, W, n, maps, partials + 2 * (size_t)blockIdx.x);
}

// the workgroup's sum of column k of `rows` rows of `stride` floats, in every thread: thread t adds the rows t, t + 256, ... in order, then block_sum
__device__ __forceinline__ float rows_sum(const float* __restrict__ partials, const size_t first, const uint32_t rows, const int stride, const int k, float* s_wave)
{
    float acc = 0.0f;
    for (uint32_t r = threadIdx.x; r < rows; r += LOSS_BLOCK) acc += partials[stride * (first + r) + k];
    return block_sum(acc, s_wave);
}

// out2[0 .. 1] = the two columns of the `groups` partial rows, each summed and then divided by n once
__device__ __forceinline__ void photometric_means(const float* __restrict__ partials, const uint32_t groups, const float n, float* __restrict__ out2, float* s_wave)
{
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float s = rows_sum(partials, 0, groups, 2, k, s_wave);
        if (threadIdx.x == 0) out2[k] = s / n;
    }
}

// one workgroup: the means of the `groups` partial rows
__global__ void __launch_bounds__(LOSS_BLOCK) photometric_sum_kernel(const float* __restrict__ partials, const uint32_t groups, const float n, float* __restrict__ out2)
{
    __shared__ float s_wave[LOSS_BLOCK / 64];
    photometric_means(partials, groups, n, out2, s_wave);
}

// The backward's blur of the three staged maps s_d (the staging's barrier included): b[k][o] = blur(s_d[k]) at the thread's pixel o.  Behind
// the second barrier nobody reads s_d, and s_h is read only before the caller's next barrier
__device__ __forceinline__ void blur_maps(const float (&s_d)[3][LOSS_HH][LOSS_HW], float (&s_h)[3][LOSS_HH][LOSS_TW], float (&b)[3][LOSS_ROWS])
{
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

    const int r0 = wave * LOSS_ROWS;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float v[LOSS_ROWS + 10];
#pragma unroll
        for (int j = 0; j < LOSS_ROWS + 10; j++) v[j] = s_h[k][r0 + j][col];
#pragma unroll
        for (int o = 0; o < LOSS_ROWS; o++) b[k][o] = window11(v + o);
    }
}

// dL/dx of a pixel from its three blurred maps b0, b1, b2 and l1w = g0 / n:  b0 + 2 x b1 + y b2 + l1w sign(x - y)
__device__ __forceinline__ float photometric_gradient(const float x, const float y, const float b0, const float b1, const float b2, const float l1w)
{
    const float sgn = x > y ? l1w : (x < y ? -l1w : 0.0f); // (a NaN pixel: 0)
    return __fmaf_rn(y, b2, __fmaf_rn(2.0f * x, b1, b0)) + sgn;
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
    float b[3][LOSS_ROWS];
    blur_maps(s_d, s_h, b);
    const int col = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * LOSS_ROWS, gx = t.x0 + col;
#pragma unroll
    for (int o = 0; o < LOSS_ROWS; o++) {
        const int gy = t.y0 + r0 + o;
        if (gx < W && gy < H) {
            const size_t e = plane_off + (size_t)gy * W + gx;
            dL_dimage[e] = photometric_gradient(image[e], target[e], b[0][o], b[1][o], b[2][o], l1w);
        }
    }
}

// ---- the training loss: the same tiles with the colour transform, the clamp and the alpha mask in the staging, the depth term in the same
// launch.  Everything these kernels add to the arithmetic of the pieces above is written with explicit fused multiply-adds and is never contracted.
//     v_j = fma(E[2][j], x_2, fma(E[1][j], x_1, fma(E[0][j], x_0, E[j][3])))       (E row-major 3 x 4; the row index is the INPUT channel)
//     clamp: v < 0 ? 0 : v > 1 ? 1 : v (a NaN stays)        x''_j = v_j * alpha_mask       a halo pixel outside the image: 0
// Backward: a workgroup owns an (image, tile) and loops over the image's channels j with the same LDS; g''_j is the expression of
// photometric_backward_kernel on (x''_j, y_j), g'_j = g''_j * alpha_mask where the clamp passes (0 <= v_j <= 1), else 0;
//     dL/dx_i = fma(E[i][2], g'_2, fma(E[i][1], g'_1, fma(E[i][0], g'_0, 0)))
// and, for dL/dE, four workgroup sums per channel (a thread: fma(x_i, g'_j, .) over its four pixels from 0, then block_sum) into 12 floats per
// workgroup, which ONE workgroup (exposure_sum_kernel) adds in order per image.  The depth planes' tiles are extra workgroups behind the
// colour ones: forward sum |(d - m) mask|, backward (g2 / n_d) sign((d - m) mask) mask.
struct LossColour {
    const float* exposure;   // 3 x 4 per image (stride exposure_stride floats: 0 or 12), or null
    const float* alpha_mask; // H x W per image (stride mask_stride floats: 0 or H * W), or null
    int exposure_stride, clamp, channels;
    size_t mask_stride;
};
struct LossDepth { const float *invdepth, *mono, *mask; };

__device__ __forceinline__ float clamp01(const float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// x''_j at pixel `pix` of the image whose first channel plane starts at `img` (E: that image's exposure or null, mk: its mask plane or null)
__device__ __forceinline__ float exposed(const float* __restrict__ img, const size_t hw, const size_t pix, const int j, const float* __restrict__ E,
                                         const int clamp, float* v_out)
{
    float v;
    if (E) v = __fmaf_rn(E[8 + j], img[2 * hw + pix], __fmaf_rn(E[4 + j], img[hw + pix], __fmaf_rn(E[j], img[pix], E[4 * j + 3])));
    else v = img[(size_t)j * hw + pix];
    *v_out = v;
    return clamp ? clamp01(v) : v;
}

// the depth term's part of a tile: sum |(d - m) mask| of the thread's four pixels
__device__ __forceinline__ float depth_tile_sum(const LossDepth d, const LossTile t, const int H, const int W)
{
#pragma clang fp contract(off)
    const int col = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * LOSS_ROWS;
    const size_t plane_off = (size_t)t.plane * H * W;
    const int gx = t.x0 + col;
    float sum = 0.0f;
#pragma unroll
    for (int o = 0; o < LOSS_ROWS; o++) {
        const int gy = t.y0 + r0 + o;
        if (gx < W && gy < H) {
            const size_t e = plane_off + (size_t)gy * W + gx;
            float v = d.invdepth[e] - d.mono[e];
            if (d.mask) v = v * d.mask[e];
            sum += fabsf(v);
        }
    }
    return sum;
}

// grid: the colour_groups (plane, tile) workgroups of photometric_forward_kernel, then the depth planes' tiles.  partials: two per colour
// workgroup, then one per depth workgroup
template <bool MAPS>
__global__ void __launch_bounds__(LOSS_BLOCK) training_forward_kernel(const float* __restrict__ image, const float* __restrict__ target, const LossColour c, const LossDepth d,
                                                                      const int H, const int W, const int tiles_x, const int tiles_y, const uint32_t colour_groups,
                                                                      const size_t n, float* __restrict__ maps, float* __restrict__ partials)
{
    __shared__ float s_x[LOSS_HH][LOSS_HW], s_y[LOSS_HH][LOSS_HW];
    __shared__ float s_h[5][LOSS_HH][LOSS_TW];
    __shared__ float s_wave[LOSS_BLOCK / 64];
    if (blockIdx.x >= colour_groups) { // (workgroup-uniform)
        const float bd = block_sum(depth_tile_sum(d, loss_tile_at(blockIdx.x - colour_groups, tiles_x, tiles_y), H, W), s_wave);
        if (threadIdx.x == 0) partials[2 * (size_t)colour_groups + (blockIdx.x - colour_groups)] = bd;
        return;
    }
    const LossTile t = loss_tile(tiles_x, tiles_y);
    const size_t hw = (size_t)H * W, plane_off = (size_t)t.plane * hw;
    {
        const int b = t.plane / c.channels, j = t.plane - b * c.channels;
        const float* img = image + (size_t)b * c.channels * hw;
        const float* E = c.exposure ? c.exposure + (size_t)b * c.exposure_stride : nullptr;
        const float* mk = c.alpha_mask ? c.alpha_mask + (size_t)b * c.mask_stride : nullptr;
        for (int i = (int)threadIdx.x; i < LOSS_HH * LOSS_HW; i += LOSS_BLOCK) {
            const int r = i / LOSS_HW, cc = i - r * LOSS_HW;
            const int gy = t.y0 - LOSS_R + r, gx = t.x0 - LOSS_R + cc;
            float v = 0.0f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const size_t pix = (size_t)gy * W + gx;
                float raw;
                v = exposed(img, hw, pix, j, E, c.clamp, &raw);
                if (mk) v = v * mk[pix];
            }
            s_x[r][cc] = v;
        }
    }
    stage_halo(s_y, target + plane_off, t.x0, t.y0, H, W, 1.0f);
    ssim_tile<MAPS>(s_x, s_y, s_h, s_wave, t, plane_off, H, W, n, maps, partials + 2 * (size_t)blockIdx.x); // the plain forward on s_x = x''
}

// photometric_sum_kernel with the depth term's column: out3[0 .. 1] by the same additions, out3[2] = the depth rows' sum / n_d (0 without rows)
__global__ void __launch_bounds__(LOSS_BLOCK) training_sum_kernel(const float* __restrict__ partials, const uint32_t groups, const float n, const uint32_t depth_groups,
                                                                  const float n_d, float* __restrict__ out3)
{
    __shared__ float s_wave[LOSS_BLOCK / 64];
    photometric_means(partials, groups, n, out3, s_wave);
    const float s = rows_sum(partials, 2 * (size_t)groups, depth_groups, 1, 0, s_wave);
    if (threadIdx.x == 0) out3[2] = depth_groups ? s / n_d : 0.0f;
}

// grid: image_groups (image, tile) workgroups, then (with dL_dinvdepth) the depth planes' tiles
__global__ void __launch_bounds__(LOSS_BLOCK) training_backward_kernel(const float* __restrict__ image, const float* __restrict__ target, const float* __restrict__ maps,
                                                                       const float* __restrict__ dL_dout3, const LossColour c, const LossDepth d, const int H, const int W,
                                                                       const int tiles_x, const int tiles_y, const uint32_t image_groups, const size_t n, const float nf,
                                                                       const float ndf, float* __restrict__ dL_dimage, float* __restrict__ dL_dinvdepth,
                                                                       float* __restrict__ exposure_partials)
{
#pragma clang fp contract(off)
    __shared__ float s_d[3][LOSS_HH][LOSS_HW];
    __shared__ float s_h[3][LOSS_HH][LOSS_TW];
    __shared__ float s_wave[LOSS_BLOCK / 64];
    const int col = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * LOSS_ROWS;
    const size_t hw = (size_t)H * W;
    if (blockIdx.x >= image_groups) { // (workgroup-uniform) a depth tile
        const LossTile t = loss_tile_at(blockIdx.x - image_groups, tiles_x, tiles_y);
        const float w = dL_dout3[2] / ndf;
        const int gx = t.x0 + col;
#pragma unroll
        for (int o = 0; o < LOSS_ROWS; o++) {
            const int gy = t.y0 + r0 + o;
            if (gx < W && gy < H) {
                const size_t e = (size_t)t.plane * hw + (size_t)gy * W + gx;
                float v = d.invdepth[e] - d.mono[e], mk = 1.0f;
                if (d.mask) {
                    mk = d.mask[e];
                    v = v * mk;
                }
                const float sg = v > 0.0f ? mk : (v < 0.0f ? -mk : 0.0f); // sign((d - m) mask) mask: exact
                dL_dinvdepth[e] = sg * w;
            }
        }
        return;
    }
    const LossTile t = loss_tile(tiles_x, tiles_y); // .plane: the image
    const float* img = image + (size_t)t.plane * c.channels * hw;
    const float* E = c.exposure ? c.exposure + (size_t)t.plane * c.exposure_stride : nullptr;
    const float* mk_plane = c.alpha_mask ? c.alpha_mask + (size_t)t.plane * c.mask_stride : nullptr;
    const float l1w = dL_dout3[0] / nf, s = dL_dout3[1] / nf;
    const int gx = t.x0 + col;
    float acc[3][LOSS_ROWS]; // dL/dx_i of the thread's four pixels (with exposure)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int o = 0; o < LOSS_ROWS; o++) acc[i][o] = 0.0f;

    for (int j = 0; j < c.channels; j++) {
        const size_t plane_off = ((size_t)t.plane * c.channels + j) * hw;
#pragma unroll
        for (int k = 0; k < 3; k++) stage_halo(s_d[k], maps + (size_t)k * n + plane_off, t.x0, t.y0, H, W, s);
        float b[3][LOSS_ROWS];
        blur_maps(s_d, s_h, b);
        float pe[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // the thread's sums of x_0 g', x_1 g', x_2 g', g' of channel j
#pragma unroll
        for (int o = 0; o < LOSS_ROWS; o++) {
            const int gy = t.y0 + r0 + o;
            if (gx < W && gy < H) {
                const size_t pix = (size_t)gy * W + gx;
                float v;
                float x = exposed(img, hw, pix, j, E, c.clamp, &v);
                const bool pass = !c.clamp || (v >= 0.0f && v <= 1.0f);
                float mk = 1.0f;
                if (mk_plane) {
                    mk = mk_plane[pix];
                    x = x * mk;
                }
                float g = photometric_gradient(x, target[plane_off + pix], b[0][o], b[1][o], b[2][o], l1w); // g''
                if (mk_plane) g = g * mk;
                if (!pass) g = 0.0f;
                if (E) {
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        acc[i][o] = __fmaf_rn(E[4 * i + j], g, acc[i][o]);
                        pe[i] = __fmaf_rn(img[(size_t)i * hw + pix], g, pe[i]);
                    }
                    pe[3] += g;
                } else {
                    dL_dimage[plane_off + pix] = g;
                }
            }
        }
        if (exposure_partials) { // (uniform; only with E)
            float* row = exposure_partials + 12 * (size_t)blockIdx.x;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float bs = block_sum(pe[i], s_wave);
                if (threadIdx.x == 0) row[i < 3 ? 4 * i + j : 4 * j + 3] = bs;
            }
        }
        // (the next channel's staging overwrites s_d, which nobody reads after the horizontal pass's barrier; s_h is written again only behind the next barrier)
    }
    if (E) {
#pragma unroll
        for (int o = 0; o < LOSS_ROWS; o++) {
            const int gy = t.y0 + r0 + o;
            if (gx < W && gy < H) {
                const size_t pix = (size_t)gy * W + gx;
#pragma unroll
                for (int i = 0; i < 3; i++) dL_dimage[((size_t)t.plane * 3 + i) * hw + pix] = acc[i][o];
            }
        }
    }
}

// one workgroup: out[e][k] = the sum of the rows e * rows_per .. (e + 1) * rows_per - 1 of 12 partials, thread t the rows t, t + 256, ... in order
__global__ void __launch_bounds__(LOSS_BLOCK) exposure_sum_kernel(const float* __restrict__ partials, const uint32_t rows_per, const uint32_t n_out, float* __restrict__ out)
{
    __shared__ float s_wave[LOSS_BLOCK / 64];
    for (uint32_t e = 0; e < n_out; e++) {
        for (int k = 0; k < 12; k++) {
            const float s = rows_sum(partials, (size_t)e * rows_per, rows_per, 12, k, s_wave);
            if (threadIdx.x == 0) out[12 * (size_t)e + k] = s;
        }
    }
}

// the tiling of `planes` (H, W) planes: tiles per plane, workgroups of a tile kernel (one per (plane, tile)), elements
struct LossGrid {
    int tiles_x, tiles_y;
    uint32_t groups; // <= planes * H * W < 2^31
    size_t n;
    LossGrid(int planes, int H, int W)
        : tiles_x((W + LOSS_TW - 1) / LOSS_TW), tiles_y((H + LOSS_TH - 1) / LOSS_TH), groups((uint32_t)((uint64_t)planes * tiles_y * tiles_x)), n((size_t)planes * H * W) {}
};

// the plain forward's tile kernel over grid g
void launch_photometric_tiles(const LossGrid& g, int H, int W, const float* image, const float* target, float* maps, float* workspace, hipStream_t st)
{
    if (maps) hipLaunchKernelGGL(photometric_forward_kernel<true>, dim3(g.groups), dim3(LOSS_BLOCK), 0, st, image, target, H, W, g.tiles_x, g.tiles_y, g.n, maps, workspace);
    else hipLaunchKernelGGL(photometric_forward_kernel<false>, dim3(g.groups), dim3(LOSS_BLOCK), 0, st, image, target, H, W, g.tiles_x, g.tiles_y, g.n, maps, workspace);
}

bool has_colour_extras(const StpTrainingLoss& x) { return x.exposure || x.alpha_mask || x.clamp; }

LossColour loss_colour(const StpTrainingLoss& x, int H, int W)
{
    return LossColour{x.exposure, x.alpha_mask, x.exposure_batched ? 12 : 0, x.clamp, x.channels, x.alpha_mask_batched ? (size_t)H * W : 0};
}

} // namespace

uint32_t photometric_groups(int planes, int H, int W) { return LossGrid(planes, H, W).groups; }

int launch_photometric_forward(int planes, int H, int W, const float* image, const float* target, float* out2, float* maps, float* workspace,
                               hipStream_t st, hipError_t* err)
{
    const LossGrid g(planes, H, W);
    *err = hipSuccess;
    launch_photometric_tiles(g, H, W, image, target, maps, workspace, st);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 0; }
    hipLaunchKernelGGL(photometric_sum_kernel, dim3(1), dim3(LOSS_BLOCK), 0, st, workspace, g.groups, (float)g.n, out2);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 1; }
    return 2;
}

int launch_photometric_backward(int planes, int H, int W, const float* image, const float* target, const float* maps, const float* dL_dout2,
                                float* dL_dimage, hipStream_t st, hipError_t* err)
{
    const LossGrid g(planes, H, W);
    *err = hipSuccess;
    hipLaunchKernelGGL(photometric_backward_kernel, dim3(g.groups), dim3(LOSS_BLOCK), 0, st, image, target, maps, dL_dout2, H, W, g.tiles_x, g.tiles_y, g.n,
                       (float)g.n, dL_dimage);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 0; }
    return 1;
}

size_t training_loss_workspace_floats(int planes, int H, int W, int depth_planes)
{
    const size_t forward = 2 * (size_t)photometric_groups(planes, H, W) + (depth_planes > 0 ? photometric_groups(depth_planes, H, W) : 0);
    const size_t backward = 12 * (size_t)photometric_groups(planes, H, W); // (>= 12 per (image, tile) workgroup whatever the channel count)
    return forward > backward ? forward : backward;
}

int launch_training_loss_forward(int planes, int H, int W, const float* image, const float* target, const StpTrainingLoss& x, float* out3, float* maps,
                                 float* workspace, hipStream_t st, hipError_t* err)
{
    const LossGrid g(planes, H, W), gd(x.invdepth ? x.depth_planes : 0, H, W); // colour planes, depth planes
    *err = hipSuccess;
    if (!has_colour_extras(x) && !gd.groups) { // the plain call's tile kernel, instantiation for instantiation
        launch_photometric_tiles(g, H, W, image, target, maps, workspace, st);
    } else {
        const LossColour c = loss_colour(x, H, W);
        const LossDepth d{x.invdepth, x.mono_invdepth, x.depth_mask};
        if (maps) hipLaunchKernelGGL(training_forward_kernel<true>, dim3(g.groups + gd.groups), dim3(LOSS_BLOCK), 0, st, image, target, c, d, H, W, g.tiles_x, g.tiles_y, g.groups, g.n, maps, workspace);
        else hipLaunchKernelGGL(training_forward_kernel<false>, dim3(g.groups + gd.groups), dim3(LOSS_BLOCK), 0, st, image, target, c, d, H, W, g.tiles_x, g.tiles_y, g.groups, g.n, maps, workspace);
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 0; }
    hipLaunchKernelGGL(training_sum_kernel, dim3(1), dim3(LOSS_BLOCK), 0, st, workspace, g.groups, (float)g.n, gd.groups, (float)gd.n, out3);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 1; }
    return 2;
}

int launch_training_loss_backward(int planes, int H, int W, const float* image, const float* target, const StpTrainingLoss& x, const float* maps,
                                  const float* dL_dout3, float* dL_dimage, float* dL_dexposure, float* dL_dinvdepth, float* workspace, hipStream_t st,
                                  hipError_t* err)
{
    *err = hipSuccess;
    if (!has_colour_extras(x) && !dL_dinvdepth) // (dL_dout3[0 .. 1] are the plain call's two)
        return launch_photometric_backward(planes, H, W, image, target, maps, dL_dout3, dL_dimage, st, err);
    const LossGrid gi(planes / x.channels, H, W), gd(dL_dinvdepth ? x.depth_planes : 0, H, W); // a workgroup per (image, tile), then the depth planes' tiles
    const size_t n = (size_t)planes * H * W;
    const uint32_t tiles = (uint32_t)gi.tiles_x * (uint32_t)gi.tiles_y;
    hipLaunchKernelGGL(training_backward_kernel, dim3(gi.groups + gd.groups), dim3(LOSS_BLOCK), 0, st, image, target, maps, dL_dout3, loss_colour(x, H, W),
                       LossDepth{x.invdepth, x.mono_invdepth, x.depth_mask}, H, W, gi.tiles_x, gi.tiles_y, gi.groups, n, (float)n, (float)gd.n, dL_dimage, dL_dinvdepth,
                       dL_dexposure ? workspace : nullptr);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 0; }
    if (!dL_dexposure) return 1;
    if (x.exposure_batched) hipLaunchKernelGGL(exposure_sum_kernel, dim3(1), dim3(LOSS_BLOCK), 0, st, workspace, tiles, gi.groups / tiles, dL_dexposure);
    else hipLaunchKernelGGL(exposure_sum_kernel, dim3(1), dim3(LOSS_BLOCK), 0, st, workspace, gi.groups, 1u, dL_dexposure);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { *err = e; return 1; }
    return 2;
}

} // namespace stp

