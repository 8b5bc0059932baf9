// stp_render_tile.hip -- "one thread per pixel, tile list streamed through LDS" render kernels.
//
// Replaces (reference file:line under cuda_rasterizer/):
//   renderCUDA<3,false>            forward.cu:234-366            -> render_global_fwd_kernel
//   renderCUDA<3>  (backward)      backward.cu:437-595           -> render_global_bwd_kernel
//   renderkBufferCUDA<3,W,false>   stopthepop/resorted_render.cuh:17-221  -> render_kbuffer_kernel<W,false>
//   renderkBufferBackwardCUDA<3,W> stopthepop/resorted_render.cuh:223-471 -> render_kbuffer_kernel<W,true>
//   renderSortedFullCUDA<3,false>  stopthepop/resorted_render.cuh:474-675 -> render_full_fwd_kernel
//
// Layout: one 256-thread workgroup (4 wave64) per 16x16 tile; the tile's (tile,depth)-sorted list is
// staged 256 entries at a time into LDS with one coalesced id load + one gather per thread, then
// every lane walks the staged batch with broadcast LDS reads (all lanes look at entry j together).
// In GLOBAL backward all 64 lanes of a wave hold the SAME Gaussian at every step, so the nine
// gradient terms are reduced across the wave with DPP and leave as nine atomics per wave instead
// of 9 x 64.
#include <cstdlib>
#include <cstring>
#include "stp_internal.h"
#include "stp_render_wave.h"

namespace stp {

namespace {

constexpr int BLOCK = 256;

// Sum over the 64 lanes of a wave; result valid in every lane (uniform).
__device__ __forceinline__ float wave_sum(float v)
{
    int t;
    t = __builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true); v += __int_as_float(t);  // quad_perm [1,0,3,2]
    t = __builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true); v += __int_as_float(t);  // quad_perm [2,3,0,1]
    t = __builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true); v += __int_as_float(t); // row_half_mirror
    t = __builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true); v += __int_as_float(t); // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}
// Maximum over the 64 lanes of a wave (finite values); result valid in every lane.
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

struct TileCtx {
    int tile, tx, ty, px, py;
    bool inside;
    uint2 range;
};

__device__ __forceinline__ TileCtx tile_ctx(const RenderArgs& a)
{
    TileCtx c;
    const int t = workgroup_tile(a); // (stp_render_wave.h)
    c.tx = t % a.gx;
    c.ty = a.ty0 + t / a.gx;
    c.tile = c.ty * a.gx + c.tx;
    c.px = c.tx * TILE + (threadIdx.x & 15);
    c.py = c.ty * TILE + (threadIdx.x >> 4);
    c.inside = c.px < a.W && c.py < a.H;
    c.range = a.ranges[c.tile];
    return c;
}

// ------------------------------------------------------------------------------------------------
// GLOBAL forward
// ------------------------------------------------------------------------------------------------
// INVD: the inverse-depth request (stp_set_forward_invdepth) -- a fourth accumulator D += alpha T / z, written to out_invdepth; INVD = false
// is the kernel as it was
template <bool INVD>
__global__ void __launch_bounds__(BLOCK) render_global_fwd_kernel(const RenderArgs a)
{
    __shared__ float s_invz[INVD ? BLOCK : 1];
    __shared__ float2 s_xy[BLOCK];
    __shared__ float4 s_co[BLOCK];
    __shared__ float s_col[3][BLOCK];
    __shared__ float s_dist[BLOCK]; // debug depth visualisation only: |cam - mean| of the staged entries

    const TileCtx c = tile_ctx(a);
    const float pxf = (float)c.px, pyf = (float)c.py;
    bool done = !c.inside;
    const int total = (int)(c.range.y - c.range.x);
    const int rounds = (total + BLOCK - 1) / BLOCK;
    int todo = total;

    float T = 1.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, depth_acc = 0.0f;
    float Dz = 0.0f; // (INVD)
    uint32_t contributor = 0, last_contributor = 0;

    for (int i = 0; i < rounds; i++, todo -= BLOCK) {
        if (__syncthreads_and(done)) break;
        const int progress = i * BLOCK + (int)threadIdx.x;
        if ((int)c.range.x + progress < (int)c.range.y) {
            const int id = (int)a.point_list[c.range.x + progress];
            s_xy[threadIdx.x] = a.means2D[id];
            s_co[threadIdx.x] = a.conic_opacity[id];
            s_col[0][threadIdx.x] = a.features[3 * (size_t)id + 0];
            s_col[1][threadIdx.x] = a.features[3 * (size_t)id + 1];
            s_col[2][threadIdx.x] = a.features[3 * (size_t)id + 2];
            if constexpr (INVD) s_invz[threadIdx.x] = a.invz[id];
            if (a.debug_depth) { // reference forward.cu:337-341
                const float ddx = a.cam[0] - a.means3D[3 * (size_t)id], ddy = a.cam[1] - a.means3D[3 * (size_t)id + 1], ddz = a.cam[2] - a.means3D[3 * (size_t)id + 2];
                s_dist[threadIdx.x] = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz);
            }
        }
        __syncthreads();
        const int n = min(BLOCK, todo);
        for (int j = 0; !done && j < n; j++) {
            contributor++;
            const float2 xy = s_xy[j];
            const float4 co = s_co[j];
            const float dx = xy.x - pxf, dy = xy.y - pyf;
            const float power = blend_power(dx, dy, co);
            if (power > 0.0f) continue;
            const float alpha = fminf(0.99f, co.w * exp_blend(power));
            if (alpha < ALPHA_THRESHOLD) continue;
            const float test_T = T * (1 - alpha);
            if (test_T < T_THRESHOLD) { done = true; continue; }
            C0 += s_col[0][j] * alpha * T;
            C1 += s_col[1][j] * alpha * T;
            C2 += s_col[2][j] * alpha * T;
            if (a.debug_depth) depth_acc += s_dist[j] * alpha * T;
            if constexpr (INVD) Dz += s_invz[j] * alpha * T;
            T = test_T;
            last_contributor = contributor;
        }
    }
    if (c.inside) {
        const size_t N = (size_t)a.W * a.H, pid = (size_t)a.W * c.py + c.px;
        a.final_T[pid] = T;
        a.n_contrib[pid] = last_contributor;
        if constexpr (INVD) a.out_invdepth[pid] = Dz;
        if (a.debug_depth) { // reference outputDebugVis, stopthepop_common.cuh:297-301
            a.out_color[pid] = depth_acc;
            a.out_color[N + pid] = T;
        } else {
            if (a.out_alpha != nullptr) a.out_alpha[pid] = 1.0f - T; // (stp_set_forward_background; see write_forward_pixel)
            if (a.bg_image != nullptr) {
                a.out_color[pid] = C0 + T * a.bg_image[pid];
                a.out_color[N + pid] = C1 + T * a.bg_image[N + pid];
                a.out_color[2 * N + pid] = C2 + T * a.bg_image[2 * N + pid];
            } else {
                a.out_color[pid] = C0 + T * a.bg[0];
                a.out_color[N + pid] = C1 + T * a.bg[1];
                a.out_color[2 * N + pid] = C2 + T * a.bg[2];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// GLOBAL backward: back-to-front with the stored n_contrib / final_T
// ------------------------------------------------------------------------------------------------
// INVD: the inverse-depth request (stp_set_backward_invdepth); INVD = false is the kernel as it was
template <bool INVD>
__global__ void __launch_bounds__(BLOCK) render_global_bwd_kernel(const RenderArgs a)
{
    __shared__ int s_id[BLOCK];
    __shared__ float2 s_xy[BLOCK];
    __shared__ float4 s_co[BLOCK];
    __shared__ float s_col[3][BLOCK];

    const TileCtx c = tile_ctx(a);
    const float pxf = (float)c.px, pyf = (float)c.py;
    const size_t N = (size_t)a.W * a.H, pid = (size_t)a.W * c.py + c.px;
    // inverse-depth request: (1 / z, D, dL/dD) is a fourth channel of the back-to-front recurrence, without a background share
    constexpr bool invd = INVD;
    float dL_dD = 0.0f, accum_rec_z = 0.0f, last_z = 0.0f;
    if constexpr (INVD) dL_dD = c.inside ? a.dL_dinvdepth[pid] : 0.0f;
    const int total = (int)(c.range.y - c.range.x);
    const int rounds = (total + BLOCK - 1) / BLOCK;
    int todo = total;

    const float T_final = c.inside ? a.final_T[pid] : 0.0f;
    float T = T_final;
    uint32_t contributor = (uint32_t)total;
    const uint32_t last_contributor = c.inside ? a.n_contrib[pid] : 0u;
    float accum_rec[3] = {0, 0, 0}, last_color[3] = {0, 0, 0}, dL_dpixel[3] = {0, 0, 0};
    float last_alpha = 0.0f;
    if (c.inside)
        for (int ch = 0; ch < 3; ch++) dL_dpixel[ch] = a.dL_dpix[ch * N + pid];
    // dL/dT_final: the background's share (per pixel with stp_set_backward_background's bg_image) minus the alpha gradient (alpha = 1 - T_final)
    float bg_dot;
    if (a.bg_image != nullptr) bg_dot = c.inside ? a.bg_image[pid] * dL_dpixel[0] + a.bg_image[N + pid] * dL_dpixel[1] + a.bg_image[2 * N + pid] * dL_dpixel[2] : 0.0f;
    else bg_dot = a.bg[0] * dL_dpixel[0] + a.bg[1] * dL_dpixel[1] + a.bg[2] * dL_dpixel[2];
    if (a.dL_dalpha != nullptr) bg_dot -= c.inside ? a.dL_dalpha[pid] : 0.0f;
    const float ddelx_dx = 0.5f * (float)a.W, ddely_dy = 0.5f * (float)a.H;
    const int lane = lane_id();

    for (int i = 0; i < rounds; i++, todo -= BLOCK) {
        __syncthreads();
        const int progress = i * BLOCK + (int)threadIdx.x;
        if ((int)c.range.x + progress < (int)c.range.y) {
            const int id = (int)a.point_list[c.range.y - progress - 1];
            s_id[threadIdx.x] = id;
            s_xy[threadIdx.x] = a.means2D[id];
            s_co[threadIdx.x] = a.conic_opacity[id];
            s_col[0][threadIdx.x] = a.features[3 * (size_t)id + 0];
            s_col[1][threadIdx.x] = a.features[3 * (size_t)id + 1];
            s_col[2][threadIdx.x] = a.features[3 * (size_t)id + 2];
        }
        __syncthreads();
        const int n = min(BLOCK, todo);
        for (int j = 0; j < n; j++) {
            // every lane steps through the same entry; lanes that skip contribute zeros to the reduction
            contributor--;
            bool use = c.inside && contributor < last_contributor;
            const float2 xy = s_xy[j];
            const float4 co = s_co[j];
            const float dx = xy.x - pxf, dy = xy.y - pyf;
            const float power = blend_power(dx, dy, co);
            use = use && !(power > 0.0f);
            const float G = exp_blend(power);
            const float alpha = fminf(0.99f, co.w * G);
            use = use && !(alpha < ALPHA_THRESHOLD);
            if (!__any(use)) continue;

            float g_col[3] = {0, 0, 0}, g_mx = 0, g_my = 0, g_cxx = 0, g_cxy = 0, g_cyy = 0, g_op = 0;
            float g_w = 0; // the pair's blend weight (blend-statistics request)
            if (use) {
                T = T / (1.f - alpha);
                const float dchannel_dcolor = alpha * T;
                g_w = dchannel_dcolor;
                float dL_dalpha = 0.0f;
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const float col = s_col[ch][j];
                    accum_rec[ch] = last_alpha * last_color[ch] + (1.f - last_alpha) * accum_rec[ch];
                    last_color[ch] = col;
                    dL_dalpha += (col - accum_rec[ch]) * dL_dpixel[ch];
                    g_col[ch] = dchannel_dcolor * dL_dpixel[ch];
                }
                if constexpr (INVD) {
                    const float zc = a.invz[s_id[j]]; // (one address for the wave)
                    accum_rec_z = last_alpha * last_z + (1.f - last_alpha) * accum_rec_z;
                    last_z = zc;
                    dL_dalpha += (zc - accum_rec_z) * dL_dD;
                }
                dL_dalpha *= T;
                last_alpha = alpha;
                dL_dalpha += (-T_final / (1.f - alpha)) * bg_dot;
                const float dL_dG = co.w * dL_dalpha;
                const float gdx = G * dx, gdy = G * dy;
                const float dG_ddelx = -gdx * co.x - gdy * co.y;
                const float dG_ddely = -gdy * co.z - gdx * co.y;
                g_mx = dL_dG * dG_ddelx * ddelx_dx;
                g_my = dL_dG * dG_ddely * ddely_dy;
                g_cxx = -0.5f * gdx * dx * dL_dG;
                g_cxy = -0.5f * gdx * dy * dL_dG;
                g_cyy = -0.5f * gdy * dy * dL_dG;
                g_op = G * dL_dalpha;
            }
            const float r0 = wave_sum(g_col[0]), r1 = wave_sum(g_col[1]), r2 = wave_sum(g_col[2]);
            const float r3 = wave_sum(g_mx), r4 = wave_sum(g_my), r5 = wave_sum(g_cxx), r6 = wave_sum(g_cxy), r7 = wave_sum(g_cyy);
            const float r8 = wave_sum(g_op);
            // absgrad request (wave-uniform): the wave's sums of |g_mx|, |g_my| -- absolute values per pixel, then the sum -- ride in lanes 9, 10
            float r9 = 0.0f, r10 = 0.0f;
            if (a.requests & REQ_ABSGRAD) { r9 = wave_sum(fabsf(g_mx)); r10 = wave_sum(fabsf(g_my)); }
            // blend-statistics request (wave-uniform): the wave's sum and maximum of the blend weights and its number of blending pixels ride
            // in lanes 11 .. 13; lane 12 hands its term over with an integer maximum on the float's bits (stp_blend.h)
            const bool stats = (a.requests & REQ_BLEND_STATS) != 0;
            float r11 = 0.0f, r12 = 0.0f, r13 = 0.0f;
            if (stats) { r11 = wave_sum(g_w); r12 = wave_max(g_w); r13 = wave_sum(use ? 1.0f : 0.0f); }
            // inverse-depth request: the wave's sum of alpha T dL/dD rides in lane 14
            float r14 = 0.0f;
            if constexpr (INVD) r14 = wave_sum(g_w * dL_dD);
            // lane k hands over term k: nine (eleven, twelve, fourteen, ...) lanes, one 64-byte record
            if (lane < 9 || ((a.requests & REQ_ABSGRAD) && lane < 11) || (stats && lane >= GRAD_STATS && lane < GRAD_STATS + 3) || (invd && lane == GRAD_INVDEPTH)) {
                float v = r0;
                switch (lane) {
                case 1: v = r1; break;
                case 2: v = r2; break;
                case 3: v = r3; break;
                case 4: v = r4; break;
                case 5: v = r5; break;
                case 6: v = r6; break;
                case 7: v = r7; break;
                case 8: v = r8; break;
                case 9: v = r9; break;
                case 10: v = r10; break;
                case 11: v = r11; break;
                case 12: v = r12; break;
                case 13: v = r13; break;
                case 14: v = r14; break;
                default: break;
                }
                if (lane == GRAD_STATS + 1) max_blend_weight(a, s_id[j], v);
                else atomicAdd(grad_slot(a, s_id[j], lane), v);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// PPX_KBUFFER forward / backward: per-pixel sorted window keyed by depth along the pixel's own ray
// ------------------------------------------------------------------------------------------------
// (min_power_rect: stp_device.h)

// MODE: a render pass of stp_render_pass.h.  The backward re-runs the window sort (the reference's scheme; nine atomics per blended pair); the
// recording forward writes the same log format with the same thread -> pixel mapping as the hierarchical mode, so that its backward is the
// replay kernel of stp_render_replay.hip.
template <int WIN, int MODE>
__global__ void __launch_bounds__(BLOCK) render_kbuffer_kernel(const RenderArgs a)
{
    constexpr bool BACKWARD = pass_backward(MODE);
    constexpr bool RECORD = pass_records(MODE);
    constexpr bool DEPTHVIZ = pass_depthviz(MODE);
    constexpr bool INVD = pass_invdepth(MODE); // forward: D += alpha T / z beside the colour; backward: the fourth channel
    // one staging round = BLOCK entry records (A, B, C, D of BinningState), read with unit stride from the list-ordered
    // entry arrays; the forward passes carry the list position through the window, the backward pass the Gaussian id
    __shared__ float4 s_A[BLOCK];
    __shared__ float4 s_B[BLOCK];
    __shared__ float4 s_C[BLOCK];
    __shared__ float4 s_D[BLOCK];
    // Strip pre-test (ours; results unchanged): a wave's pixels are four rows of the tile, and most entries of a tile's
    // list cannot reach alpha >= 1/255 anywhere in a given 16x4 strip.  The thread that stages an entry computes the
    // EXACT minimum of the exponent's quadratic form over each of the four strips (min_power_rect below -- not the
    // reference's max-contribution estimate, stopthepop_common.cuh:130-174, which in the corner case returns an interior
    // point and is therefore not a bound) and leaves four bits; a wave skips the per-pixel evaluation of an entry whose
    // bit is clear (with a margin of 1e-3 on the threshold against rounding: a skipped entry fails the exact per-pixel
    // test for every pixel of the strip).  The pop-before-look step and the contributor count still run.
    __shared__ uint32_t s_hit[BLOCK];

    TileCtx c = tile_ctx(a);
    if constexpr (BACKWARD) {
        // fallback duty only when the forward recorded blend logs: just the tiles whose log overflowed
        if (a.flag_mode == 1 && a.tile_flags[c.tile] == 0u) return;
    }
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    if constexpr (RECORD) { // the replay kernel's pixel of (wave, lane): wave = row of four 4x4 sub-tiles, 2x2 quads inside
        const WavePixel wp = wave_pixel_map(a);
        c.px = wp.px; c.py = wp.py; c.inside = wp.inside;
    }
    const float pxf = (float)c.px, pyf = (float)c.py;
    bool done = !c.inside;
    const int total = (int)(c.range.y - c.range.x);
    const int rounds = (total + BLOCK - 1) / BLOCK;
    int todo = total;

    const float3 cam = make_float3(a.cam[0], a.cam[1], a.cam[2]);
    const float3 dir = view_ray(a.inv_vp, cam, pxf, pyf, a.W, a.H);

    Window<WIN> win; // payload: Gaussian id, or (recording forward) the entry's position in the tile list
    win.init();
    FwdPixel fp;
    BwdPixel bp;
    if constexpr (BACKWARD) init_bwd_pixel<INVD>(bp, a, c.inside, c.px, c.py);
    else init_fwd_pixel(fp);
    uint32_t contributor = 0;
    float depth_acc = 0.0f;
    FwdDepth fz;
    char* const log_base = RECORD ? log_wave_slice(a.blend_log, c.tile, w, a.log_depth) : nullptr; // [record / 8][lane][record % 8], stp_blend.h
    int nrec = 0;
    const float4* const eF = a.entF + c.range.x;
    const float4* const eCl = a.entC + c.range.x;
    const float4* const eDl = a.entD + c.range.x;

    auto blend_one = [&]() {
        if (win.num == 0) return;
        bool ok;
        if constexpr (BACKWARD) ok = blend_backward<INVD>(bp, a, c.px, c.py, win.id[0], win.store[0]);
        else {
            // The forward windows do not carry alpha (two selects per slot and insertion less): it is evaluated again here,
            // from the same entry record with the same instructions, hence to the same bits as when the entry passed the
            // candidate test.
            const int pos = win.id[0];
            const float4 colr = eF[pos], eCp = eCl[pos], eDp = eDl[pos];
            const float col[3] = {colr.x, colr.y, colr.z};
            const float alpha0 = fminf(0.99f, eDp.w * exp_blend(blend_power(eCp.y - pxf, eCp.z - pyf, eDp)));
            const float T_before = fp.T;
            ok = blend_forward_c(fp, col, alpha0);
            if constexpr (DEPTHVIZ) { if (ok) depth_acc += win.depth[0] * alpha0 * T_before; } // reference resorted_render.cuh:107
            if constexpr (INVD) { if (ok) fz.D = fmaf(alpha0 * T_before, a.invz[__float_as_int(eCp.w)], fz.D); } // (the wave64 kernels' expression, stp_render_kbuf.hip: the same bits)
            if constexpr (RECORD) {
                if (ok) {
                    if (nrec < a.log_depth) *reinterpret_cast<log_t*>(log_base + log_record_offset<true>(2u * (uint32_t)nrec, (uint32_t)lane << LOG_PIECE_SHIFT)) = (log_t)pos;
                    nrec++;
                }
            }
        }
        if (!ok) { win.num--; done = true; return; }
        win.pop();
    };

    for (int i = 0; i < rounds; i++, todo -= BLOCK) {
        if (__syncthreads_and(done)) break;
        const int progress = i * BLOCK + (int)threadIdx.x;
        if ((int)c.range.x + progress < (int)c.range.y) {
            const size_t gi = (size_t)c.range.x + progress;
            s_A[threadIdx.x] = a.entA[gi];
            s_B[threadIdx.x] = a.entB[gi];
            const float4 sc = a.entC[gi], sd = a.entD[gi];
            s_C[threadIdx.x] = sc;
            s_D[threadIdx.x] = sd;
            uint32_t hit = 0;
#pragma unroll
            for (int ww = 0; ww < 4; ww++) {
                const float x0 = (float)(c.tx * TILE), y0 = (float)(c.ty * TILE + 4 * ww);
                const float p = min_power_rect(sd, x0 - sc.y, x0 + 15.0f - sc.y, y0 - sc.z, y0 + 3.0f - sc.z);
                hit |= (sd.w * exp_blend(-p) < ALPHA_THRESHOLD * 0.999f) ? 0u : (1u << ww);
            }
            s_hit[threadIdx.x] = hit;
        }
        __syncthreads();
        const int n = min(BLOCK, todo);
        for (int j = 0; !done && j < n; j++) {
            if (win.num == WIN) blend_one(); // before the next candidate is looked at
            if (done) break;
            contributor++;
            if (((s_hit[j] >> w) & 1u) == 0u) continue; // (the same for every lane of the wave)
            const float4 eCj = s_C[j];
            const float4 co = s_D[j];
            const float dx = eCj.y - pxf, dy = eCj.z - pyf;
            const float power = blend_power(dx, dy, co);
            if (power > 0.0f) continue;
            const float G = exp_blend(power);
            const float alpha = fminf(0.99f, co.w * G);
            if (alpha < ALPHA_THRESHOLD) continue;
            const float depth = depth_along_ray_ent(s_A[j], s_B[j], eCj, dir);
            if (depth < 0.0f) continue;
            win.insert(depth, BACKWARD ? __float_as_int(eCj.w) : i * BLOCK + j, BACKWARD ? G : 0.0f);
        }
    }
    if (!done)
        while (win.num > 0 && !done) blend_one();

    if constexpr (!BACKWARD) {
        if (c.inside) write_forward_pixel<DEPTHVIZ, true>(a, c.px, c.py, fp, depth_acc, RECORD ? (uint32_t)nrec : contributor); // (recording forward: the pixel's number of log records)
        if constexpr (INVD) { if (c.inside) a.out_invdepth[(size_t)a.W * c.py + c.px] = fz.D; }
        if constexpr (RECORD) finish_blend_log(a, c.tile, nrec, total);
    }
}

} // namespace

static RenderArgs make_args(const FrameParams& f, const GeometryState& g, const BinningState& b, const ImageState& img)
{
    RenderArgs a{};
    a.W = f.W; a.H = f.H; a.gx = f.gx; a.ty0 = f.ty0; a.ty1 = f.ty1;
    a.ranges = img.ranges; a.point_list = b.point_list; a.means2D = g.means2D; a.conic_opacity = g.conic_opacity;
    a.cov3D_inv = g.cov3D_inv; a.features = f.colors_precomp ? f.colors_precomp : g.rgb; // reference rasterizer_impl.cu:367,473
    a.inv_vp = f.inv_viewprojmatrix; a.cam = f.cam_pos; a.bg = f.background;
    a.entA = b.entA; a.entB = b.entB; a.entC = b.entC; a.entD = b.entD; a.entF = b.entF;
    a.final_T = img.final_T; a.n_contrib = img.n_contrib;
    a.blend_log = img.blend_log; a.tile_flags = img.tile_flags; a.flag_mode = 0;
    const bool counters = switches().atomic_bin; // (STP_SORT=counters: that path uses tile_cursor itself)
    a.tile_order = (tile_order_used(f) && !counters && !f.split_launch) ? img.tile_cursor + f.gx * f.ty0 : nullptr;
    a.log_depth = img.log_depth; a.log_need = f.log_need; a.log_tag = f.log_tag;
    a.debug_depth = f.s.debug_visualization == STP_DEBUG_DEPTH ? 1 : 0; a.means3D = f.means3D;
    a.fused_gather = 0; // (launch_render_forward: the hierarchical forwards)
    a.gather.keys = b.keys; a.gather.point_list = b.point_list; a.gather.gpack = g.gpack; a.gather.features = a.features;
    a.gather.gx = f.gx; a.gather.cull_mask = subtile_mask_kind(f.s);
    a.gather.entA = b.entA; a.gather.entB = b.entB; a.gather.entC = b.entC; a.gather.entD = b.entD; a.gather.entF = b.entF;
    a.bg_image = f.bg_image; a.out_alpha = f.out_alpha; a.dL_dalpha = nullptr; // (forward: stp_set_forward_background; the backward sets its own)
    a.invz = g.invz; a.out_invdepth = f.out_invdepth; a.invdepth = nullptr; a.dL_dinvdepth = nullptr; // (stp_set_forward_invdepth; the backward sets its own)
    return a;
}

// implemented in the other render files
hipError_t launch_hier(int pass, const FrameParams& f, const RenderArgs& a, hipStream_t st, std::string* err); // stp_render_hier.hip
hipError_t launch_hier_replay(const FrameParams& f, const RenderArgs& a, hipStream_t st);                      // stp_render_replay.hip
hipError_t launch_full_fwd(const FrameParams& f, const RenderArgs& a, hipStream_t st);                         // stp_render_full.hip
hipError_t launch_kbuffer_wave(int pass, const FrameParams& f, const RenderArgs& a, hipStream_t st);           // stp_render_kbuf.hip
hipError_t launch_depth_colormap(float* out_color, int N, uint32_t* minmax, hipStream_t st);                   // stp_debug_viz.hip

template <int MODE> static hipError_t launch_kbuffer_one(const FrameParams& f, const RenderArgs& a, hipStream_t st)
{
    const dim3 grid(f.gx * (f.ty1 - f.ty0)), block(BLOCK);
    const int w = f.s.queue_per_pixel; // reference forward.cu:409-425 / backward.cu:712-731
#define STP_KB(WIN) hipLaunchKernelGGL((render_kbuffer_kernel<WIN, MODE>), grid, block, 0, st, a)
    if (w <= 1) STP_KB(1);
    else if (w <= 2) STP_KB(2);
    else if (w <= 4) STP_KB(4);
    else if (w <= 8) STP_KB(8);
    else if (w <= 12) STP_KB(12);
    else if (w <= 16) STP_KB(16);
    else if (w <= 20) STP_KB(20);
    else STP_KB(24);
#undef STP_KB
    return hipGetLastError();
}

// the k-buffer kernel of this file: the re-sorting backward, and every forward pass under STP_KBUFFER=tile
static hipError_t launch_kbuffer(int pass, const FrameParams& f, const RenderArgs& a, hipStream_t st)
{
    switch (pass) {
    case PASS_FWD: return launch_kbuffer_one<PASS_FWD>(f, a, st);
    case PASS_BWD: return launch_kbuffer_one<PASS_BWD>(f, a, st);
    case PASS_FWD_RECORD: return launch_kbuffer_one<PASS_FWD_RECORD>(f, a, st);
    case PASS_FWD_DEPTH: return launch_kbuffer_one<PASS_FWD_DEPTH>(f, a, st);
    case PASS_FWD_INVD: return launch_kbuffer_one<PASS_FWD_INVD>(f, a, st);
    case PASS_FWD_RECORD_INVD: return launch_kbuffer_one<PASS_FWD_RECORD_INVD>(f, a, st);
    case PASS_BWD_INVD: return launch_kbuffer_one<PASS_BWD_INVD>(f, a, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_render_forward(const FrameParams& f, const GeometryState& g, const BinningState& b, const ImageState& img,
                                 float* out_color, hipStream_t st, std::string* err)
{
    RenderArgs a = make_args(f, g, b, img);
    a.out_color = out_color;
    // (inverse depth: stp_set_forward_invdepth, the kernels' INVD variants; refused with the debug depth visualisation before this point)
    const int pass = render_pass(false, uses_blend_log(f.s), a.debug_depth != 0, a.out_invdepth != nullptr);
    if (pass < 0) { if (err) *err = "invalid render pass"; return hipErrorInvalidValue; }
    const dim3 grid(f.gx * (f.ty1 - f.ty0)), block(BLOCK);
    if (grid.x == 0) return hipSuccess;
    switch (f.s.sort_mode) {
    case MODE_GLOBAL: // (one kernel for the plain forward and the depth visualisation: RenderArgs::debug_depth)
        if (pass_invdepth(pass)) hipLaunchKernelGGL(render_global_fwd_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(render_global_fwd_kernel<false>, grid, block, 0, st, a);
        return hipGetLastError();
    case MODE_KBUFFER:
        // the wave64 kernel of stp_render_kbuf.hip (STP_KBUFFER=tile keeps the one-entry-per-wave kernel of this file for
        // comparison; the results are the same)
        if (switches().kbuffer == Switches::KBUFFER_TILE) return launch_kbuffer(pass, f, a, st);
        return launch_kbuffer_wave(pass, f, a, st);
    case MODE_FULL: return launch_full_fwd(f, a, st);
    case MODE_HIER:
        a.fused_gather = f.fused_gather; // (the forward and recording forward sort + gather their tiles of up to TS_SMALL entries themselves; 0 under the depth visualisation)
        return launch_hier(pass, f, a, st, err);
    default: if (err) *err = "invalid sort mode"; return hipErrorInvalidValue;
    }
}

// The forward of the debug depth visualisation: the render kernels above leave sum(depth * alpha * T) in channel 0 and T
// in channel 1; the frame's extrema and the colormap finish the image (reference applyDebugVisualization,
// rasterizer_impl.cu:54-109).
hipError_t launch_render_debug_finish(const FrameParams& f, const ImageState& img, float* out_color, hipStream_t st)
{
    if (f.s.debug_visualization != STP_DEBUG_DEPTH) return hipSuccess;
    return launch_depth_colormap(out_color, f.W * f.H, img.dbg_minmax, st);
}

hipError_t launch_render_backward(const FrameParams& f, const GeometryState& g, const BinningState& b, const ImageState& img,
                                  const BackwardParams& bw, hipStream_t st, std::string* err)
{
    RenderArgs a = make_args(f, g, b, img);
    a.pixel_colors = bw.pixel_colors; a.dL_dpix = bw.dL_dpix; a.grad_rec = bw.grad_rec; a.grad_stride = bw.grad_stride;
    // (the caller has refused compact records with either request: slots 9 .. 13 exist)
    a.requests = (bw.absgrad != nullptr ? REQ_ABSGRAD : 0) | (bw.blend_stats != nullptr ? REQ_BLEND_STATS : 0) | (bw.dL_dinvdepth != nullptr ? REQ_INVDEPTH : 0);
    a.out_invdepth = nullptr; a.invdepth = bw.invdepth; a.dL_dinvdepth = bw.dL_dinvdepth; // stp_set_backward_invdepth
    // (a backward has no pass of the depth visualisation: that setting does not reach its kernels)
    const int pass = render_pass(true, uses_blend_log(f.s), false, (a.requests & REQ_INVDEPTH) != 0);
    a.bg_image = bw.bg_image; a.out_alpha = nullptr; a.dL_dalpha = bw.dL_dalpha; // stp_set_backward_background
    const dim3 grid(f.gx * (f.ty1 - f.ty0)), block(BLOCK);
    if (grid.x == 0) return hipSuccess;
    switch (f.s.sort_mode) {
    case MODE_GLOBAL:
        if (pass_invdepth(pass)) hipLaunchKernelGGL(render_global_bwd_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(render_global_bwd_kernel<false>, grid, block, 0, st, a);
        return hipGetLastError();
    case MODE_KBUFFER:
    case MODE_HIER:
        if (uses_blend_log(f.s)) { // replay the forward's blend log; the re-sorting kernel only takes overflowed tiles
            hipError_t e = launch_hier_replay(f, a, st);
            if (e != hipSuccess) return e;
            a.flag_mode = 1;
        }
        return f.s.sort_mode == MODE_HIER ? launch_hier(pass, f, a, st, err) : launch_kbuffer(pass, f, a, st);
    default: if (err) *err = "Backward not supported for full per-pixel sort"; return hipErrorInvalidValue;
    }
}

} // namespace stp
