// stp_render_wave.h -- the scaffold of the wave64 render kernels, once: tile order, thread -> pixel map, entry-record load, the quad-level
// pre-test, the head step's candidate evaluation, the quad FIFO in front of the head steps, and the pixel writes of a forward pass.
// Used by stp_render_hier.inc, stp_render_kbuf.hip, stp_render_replay.hip and stp_render_tile.hip.  One exception: stp_render_hier.inc
// writes wave_pixel_map() out (it says why where it does).
// Everything here is __forceinline__ and works on values.
#pragma once

#include "stp_blend.h"

namespace stp {

// XCD-aware tile order: consecutive workgroup ids land on different XCDs (id % 8), so give every XCD
// a contiguous run of tiles -- neighbouring tiles share Gaussians, which then hit in that XCD's L2.
__device__ __forceinline__ int xcd_remap_tile(int wg, int n_wg)
{
    const int q = n_wg >> 3, r = n_wg & 7;
    const int xcd = wg & 7, k = wg >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// the tile of workgroup blockIdx.x inside the frame's window of tile rows: RenderArgs::tile_order (longest list first) or the XCD remap
__device__ __forceinline__ int workgroup_tile(const RenderArgs& a)
{
    const int rows = a.ty1 - a.ty0;
    return a.tile_order ? (int)a.tile_order[blockIdx.x] : xcd_remap_tile((int)blockIdx.x, a.gx * rows);
}

// thread -> pixel: one 256-thread workgroup per 16x16 tile, one WAVE per row of four 4x4 sub-tiles; a sub-tile is a 16-lane DPP row,
// a 2x2 quad is a DPP quad.  The recording forwards and the replay backward share it: record k of (wave, lane) is the same pixel's.
struct WavePixel {
    int lane, w;        // lane of the wave; wave = sub-tile row inside the tile (wave-uniform: an SGPR)
    int s, x, m, q;     // sub-tile (DPP row) inside the wave, lane inside the sub-tile, quad inside the sub-tile, lane inside the quad
    int tile_x, tile_y, tile;
    uint2 range;        // the tile's slice of the list
    int cx, cy;         // my sub-tile's corner pixel
    int px, py;
    bool inside;
};
__device__ __forceinline__ WavePixel wave_pixel_map(const RenderArgs& a)
{
    WavePixel p;
    p.lane = (int)(threadIdx.x & 63);
    p.w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    p.s = p.lane >> 4; p.x = p.lane & 15; p.m = p.x >> 2; p.q = p.x & 3;
    const int t = workgroup_tile(a);
    p.tile_x = t % a.gx; p.tile_y = a.ty0 + t / a.gx; p.tile = p.tile_y * a.gx + p.tile_x;
    p.range = a.ranges[p.tile];
    p.cx = p.tile_x * TILE + 4 * p.s; p.cy = p.tile_y * TILE + 4 * p.w;
    p.px = p.cx + 2 * (p.m & 1) + (p.q & 1); p.py = p.cy + 2 * (p.m >> 1) + (p.q >> 1);
    p.inside = p.px < a.W && p.py < a.H;
    return p;
}

// entry record row `pos` of a list-ordered array: wave-uniform base (an SGPR pair) + one 32-bit byte offset, i.e.
// `global_load_dwordx4 v, v_off, s[base]` with no 64-bit address arithmetic (v_lshl_add_u64 issues at half rate)
__device__ __forceinline__ float4 ent_row(const float4* base, int pos)
{
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + ((uint32_t)pos << 4));
}

// does any pixel of my 2x2 quad still blend?  act = __ballot(active), taken by the caller with every lane of the wave present.  (The ballot as
// an argument, not the predicate: with the ballot inside this function the hierarchical kernels of the larger queue sizes, which live at
// their register limit, spill up to 22 VGPRs more -- profiles/EXPERIMENTS.md, "shared scaffold".)
__device__ __forceinline__ bool quad_live(const unsigned long long act, int lane)
{
    return ((act >> (lane & ~3)) & 0xFull) != 0ull;
}

// The quad-level pre-test in front of the head steps.  Lane-local: can the entry with record rows C (mean in .yz) and D (conic, opacity)
// reach 1/255 at any of the four pixels of the 2x2 quad?  false = certainly not: an upper bound of opacity * exp(power) over the four
// pixels, wide enough to cover every rounding of the per-pixel evaluation.
// (qxc, qyc): the quad's CENTRE.  With d = mean - centre, g = conic * d and e in {+-1/2}^2 the offsets of the four pixels,
// the negated exponent at a pixel is  Q(d) + g.e + Q(e)  with  Q(e) = (a + c) / 8 + b ex ey  -- exactly, for any conic --
// so its minimum over the four pixels is  Q(d) + (a + c) / 8 + min(b/4 - |gx + gy| / 2, -b/4 - |gx - gy| / 2):  sixteen
// instructions instead of the four evaluations' thirty.
__device__ __forceinline__ bool quad_can_blend(const float4 C, const float4 D, const float qxc, const float qyc)
{
    const float dx = C.y - qxc, dy = C.z - qyc;
    const float gx = fmaf(D.y, dy, D.x * dx), gy = fmaf(D.z, dy, D.y * dx);
    const float q2 = fmaf(gy, dy, gx * dx);                                  // 2 Q(d)
    const float m2 = fminf(fmaf(D.y, 0.5f, -fabsf(gx + gy)), fmaf(D.y, -0.5f, -fabsf(gx - gy))); // 2 min(...)
    const float qmin2 = fmaf(D.x + D.z, 0.25f, q2) + m2;                      // 2 x the smallest negated exponent, to a few ulp of its terms
    // |this evaluation - blend_power_quad()| <= 10 * 2^-24 * (|a| + |b| + |c|) * far^2 = 6e-7 * S,  far = the largest |offset| of a pixel
    const float far = fmaxf(fabsf(dx), fabsf(dy)) + 0.5f;
    const float S = (fabsf(D.x) + fabsf(D.z) + fabsf(D.y)) * far * far;
    const float pup = fmaf(qmin2, -0.5f, S * 2.0e-6f);
    const float v = D.w * __builtin_amdgcn_exp2f(pup * 1.44269502162933349609375f); // (relative error < 2e-6 where it matters)
    return !(v < ALPHA_THRESHOLD * 0.9999f);                                          // NaN: kept, the exact test decides
}

// One candidate of a head step.  Lane q of the quad has fetched the record rows A..D of candidate q (list position fid, -1 = none;
// loaded from the clamped position); candidate I is evaluated for my pixel with those rows as DPP quad_perm OPERANDS of the
// arithmetic.  I == 0 first zeroes the opacity of a missing candidate (alpha 0 fails the tests), a VALU result that DPP operands read.
struct HeadCandidate { float depth, alpha; bool pass; };
template <int I, bool FRCP>
__device__ __forceinline__ HeadCandidate head_candidate(const int fid, const float4 eAq, const float4 eBq, const float4 eCq, float4& eDq,
                                                        const float3 pix_dir, const int px, const int py, const bool active)
{
    if constexpr (I == 0) { // (after the caller's pop: the wait for the four loads stays behind it)
        eDq.w = fid < 0 ? 0.0f : eDq.w;
        dpp_hazard_guard_on(eDq.w);
    } else dpp_hazard_guard();
    HeadCandidate c;
    c.depth = depth_along_ray_quad_ent<I, FRCP>(eAq, eBq, eCq, pix_dir);
    const float dx = quad_sub<I>(eCq.y, (float)px), dy = quad_sub<I>(eCq.z, (float)py);
    const float power = blend_power_quad<I>(dx, dy, eDq);
    c.alpha = min_099(quad_mul<I>(eDq.w, exp_blend(power)));
    c.pass = active && !(c.depth < 0.0f) && !(power > 0.0f) && !(c.alpha < ALPHA_THRESHOLD);
    return c;
}

// A quad's FIFO of list positions that passed the pre-test and wait for their head steps: CAP slots in LDS (the caller's `slots`),
// head and count quad-uniform registers.  A power-of-two capacity wraps with a mask, any other by subtraction.
template <int CAP> struct QuadFifo {
    static_assert(CAP >= 20, "one round of survivors adds up to 16 entries on top of a group of four");
    int head = 0, cnt = 0;
    static __device__ __forceinline__ int wrap(int v) // v in [0, 3 CAP) -> [0, CAP)
    {
        if constexpr ((CAP & (CAP - 1)) == 0) return v & (CAP - 1);
        else {
            v -= v >= 2 * CAP ? 2 * CAP : 0;
            return v - (v >= CAP ? CAP : 0);
        }
    }
    // lane q of the quad brings one entry and its verdict: the quad's survivors are parked in lane order
    __device__ __forceinline__ void push(int* const slots, const int q, const bool keep, const int fid)
    {
        int bits = keep ? (1 << q) : 0;
        bits += __builtin_amdgcn_mov_dpp(bits, 0xB1, 0xF, 0xF, true); // quad_perm [1,0,3,2]
        bits += __builtin_amdgcn_mov_dpp(bits, 0x4E, 0xF, 0xF, true); // quad_perm [2,3,0,1]: the quad's four verdicts in every lane
        if (keep) slots[wrap(head + cnt + __popc(bits & ((1 << q) - 1)))] = fid;
        cnt += __popc(bits);
    }
    // Is a head step due?  qlive: some pixel of my quad still blends (otherwise nobody is left to show the parked entries to: dropped).
    // force: until every FIFO is empty (end of the list); otherwise while some quad could not take another round's 16 entries, or
    // every quad with live pixels has a full group of four.
    __device__ __forceinline__ bool round_due(const bool force, const bool qlive)
    {
        if (!qlive) { head = wrap(head + cnt); cnt = 0; }
        if (force) return __any(cnt > 0);
        return __any(cnt > CAP - 16) || (__all(cnt >= 4 || !qlive) && __any(cnt >= 4));
    }
    // the next group of up to four: lane q takes entry q (-1 = none)
    __device__ __forceinline__ int take4(const int* const slots, const int q)
    {
        const int n = min(cnt, 4);
        const int fid = q < n ? slots[wrap(head + q)] : -1;
        head = wrap(head + n);
        cnt -= n;
        return fid;
    }
};

// ---- what a forward pass writes for its pixel --------------------------------------------------------------------------------------
// DEPTHVIZ: sum(depth * alpha * T) in channel 0 and T in channel 1 instead of the colour (reference outputDebugVis, stopthepop_common.cuh:297-301).
// NCONTRIB: the pass writes n_contrib with the pixel (the hierarchical plain forward deliberately does not, reference hierarchical_render.cuh:1019).
template <bool DEPTHVIZ, bool NCONTRIB>
__device__ __forceinline__ void write_background_pixel(const RenderArgs& a, const int px, const int py)
{
    const size_t N = (size_t)a.W * a.H, pid = (size_t)a.W * py + px;
    a.final_T[pid] = 1.0f;
    if constexpr (NCONTRIB) a.n_contrib[pid] = 0u;
    if constexpr (DEPTHVIZ) { a.out_color[pid] = 0.0f; a.out_color[N + pid] = 1.0f; }
    else {
        if (a.out_alpha != nullptr) a.out_alpha[pid] = 0.0f;
        if (a.bg_image != nullptr) { a.out_color[pid] = a.bg_image[pid]; a.out_color[N + pid] = a.bg_image[N + pid]; a.out_color[2 * N + pid] = a.bg_image[2 * N + pid]; }
        else { a.out_color[pid] = a.bg[0]; a.out_color[N + pid] = a.bg[1]; a.out_color[2 * N + pid] = a.bg[2]; }
    }
}
template <bool DEPTHVIZ, bool NCONTRIB>
__device__ __forceinline__ void write_forward_pixel(const RenderArgs& a, const int px, const int py, const FwdPixel& fp, const float depth_acc, const uint32_t n_contrib)
{
    const size_t N = (size_t)a.W * a.H, pid = (size_t)a.W * py + px;
    a.final_T[pid] = fp.T;
    if constexpr (NCONTRIB) a.n_contrib[pid] = n_contrib;
    if constexpr (DEPTHVIZ) {
        a.out_color[pid] = depth_acc;
        a.out_color[N + pid] = fp.T;
    } else {
        // alpha output and per-pixel background (stp_set_forward_background): wave-uniform branches on the request's pointers; the
        // per-pixel form is the uniform one's expression with B[ch, p] in the place of bg[ch]
        if (a.bg_image != nullptr) {
            a.out_color[pid] = fp.C[0] + fp.T * a.bg_image[pid];
            a.out_color[N + pid] = fp.C[1] + fp.T * a.bg_image[N + pid];
            a.out_color[2 * N + pid] = fp.C[2] + fp.T * a.bg_image[2 * N + pid];
        } else {
            a.out_color[pid] = fp.C[0] + fp.T * a.bg[0];
            a.out_color[N + pid] = fp.C[1] + fp.T * a.bg[1];
            a.out_color[2 * N + pid] = fp.C[2] + fp.T * a.bg[2];
        }
        if (a.out_alpha != nullptr) a.out_alpha[pid] = 1.0f - fp.T;
    }
}
// recording forwards, once per wave: a log that overflowed (a pixel with more records than the log's depth, a list too long for a
// 16-bit position) sends the tile's backward to the re-sorting kernel; the frame's need is reported for the next frame's depth
__device__ __forceinline__ void finish_blend_log(const RenderArgs& a, const int tile, const int nrec, const int total)
{
    if (nrec > a.log_depth || total > LOG_MAX_LIST) a.tile_flags[tile] = 1u;
    report_log_need(a.log_need, nrec, a.log_tag);
}

} // namespace stp
