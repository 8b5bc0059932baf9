// stp_render_replay.hip -- backward of the per-pixel-sort modes by REPLAYING the forward's blend log.
//
// No counterpart in the reference: its backward (hierarchical_render.cuh:1038-1175) re-runs the complete
// three-level resort to rediscover the order in which every pixel blended its Gaussians.  MI355X has 288 GB of
// HBM, so the training forward (render_hier_kernel<..., PASS_FWD_RECORD>, render_kbuffer_kernel<WIN, PASS_FWD_RECORD>)
// simply writes that order down -- 2 bytes (the tile-list position) per blended (pixel, Gaussian) pair,
// as many records per pixel as the frames before it needed (RenderArgs::log_depth; 192 + eight spare rows = 400 B per pixel for a frame nothing
// is known about, 304 B per pixel = 0.63 GB at 1080p once C2's 114 blends per pixel are known) -- and this kernel walks each pixel's log
// front to back.  The gradient maths per pair is the reference's (blend_backward_terms); the result is the same sum
// in a different order.  Tiles whose log overflowed (a pixel with more than BLEND_LOG_DEPTH blended entries, a list longer than
// 65535) are flagged by the forward and left to the re-sorting backward kernels, which then run only on those tiles.
//
// Layout: one 256-thread workgroup per tile, thread -> pixel mapping identical to the forward (wave = row of four
// 4x4 sub-tiles), log laid out as the forward's mode wrote it (stp_blend.h): [tile][wave][k][lane] in hierarchical mode (the 64 lanes of a wave
// read record k with one 128-byte load as long as they walk in step), [tile][wave][k / 4][lane][k % 4] in k-buffer mode (a wave's load of "record
// k of every lane" touches the four lines of one 512-byte block, which the next three steps find in the L1).  The nine gradient terms of a blend are summed on chip as 64-bit fixed point (see
// stp_render_hier.inc for why not fp32 LDS atomics) in ONE set of sums per LIST POSITION, shared by the workgroup:
// acc[term][position - window start], 512 positions = 36 KB.  A tile whose list fits (all of C2-full) is one window:
// a blend is nine ds_add_u64 and nothing else, the sums leave the chip once at the end (16-lane group = one position,
// nine lanes = nine sums, one atomic instruction into the Gaussian's 64-byte gradient record).  Longer lists are
// walked with a window that slides in half steps (position p lives in slot p mod 512): a lane pauses at its first
// record beyond the window, and when every lane has left the window's lower half the workgroup meets at a barrier,
// writes that half out and moves on -- every pixel visits the list in (nearly) increasing position, so only the
// few records that the re-sort moved behind the window fall back to global atomics.  Before the LDS adds,
// lanes that hold the same position merge their terms pairwise with DPP (the adds serialise on equal addresses).
#include "stp_internal.h"
#include "stp_render_wave.h"

#include <type_traits>

namespace stp {

#ifdef STP_REPLAY_STATS
__device__ unsigned long long g_replay_stats[16];
#endif

namespace {

// On-chip sums as 64-bit fixed point, not doubles through ds_add_f64: on addresses that 4 / 16 lanes share ds_add_f64 costs 42 / 181 cycles
// against 27 / 119 for ds_add_u64 (tools/lds_atomic_bench.hip), C2-full replay 0.98 -> 1.36 ms (profiles/EXPERIMENTS.md, round 2).  One set
// of nine sums per workgroup, all nine 64-bit: two copies and 32-bit colour sums measured slower (EXPERIMENTS.md, round 3), as did the raw
// conversion bits and red + green packed into one add (round 4).
#ifndef STP_REPLAY_OCC
#define STP_REPLAY_OCC 4
#endif
#ifndef STP_REPLAY_WINDOW
#define STP_REPLAY_WINDOW 512
#endif
constexpr int WINDOW = STP_REPLAY_WINDOW; // list positions per window (9 x 512 x 8 B = 36 KB of LDS: four workgroups per CU)
// The ABS instantiations (absgrad request: eleven sums per position) keep the 512 positions -- 11 x 512 x 8 B = 44 KB, THREE workgroups per
// CU -- rather than a 256-position window at four (22 KB): see DESIGN section 3.2.  -DSTP_REPLAY_ABS_OCC=4 with a 256-position window
// (-DSTP_REPLAY_WINDOW=256, which then also holds for the plain kernel) builds the other choice for a measurement.
#ifndef STP_REPLAY_ABS_OCC
#define STP_REPLAY_ABS_OCC 3
#endif
// The STATS instantiations (blend-statistics request: three more terms per position) keep the 512 positions too: twelve terms are 48 KB and
// three workgroups per CU, fourteen (both requests) 56 KB and two.  -DSTP_REPLAY_STATS_OCC / -DSTP_REPLAY_BOTH_OCC with a smaller
// -DSTP_REPLAY_WINDOW build the other choices for a measurement.
#ifndef STP_REPLAY_STATS_OCC
#define STP_REPLAY_STATS_OCC 3
#endif
#ifndef STP_REPLAY_BOTH_OCC
#define STP_REPLAY_BOTH_OCC 2
#endif
constexpr int EXHAUSTED = 0x7fffffff; // "position" of a lane that has no record left

// (One kernel for both kinds of tile: as two launches the mixed case -- C2-min -- loses more to the half-empty grids
// than the lean loop gains.)
// LOG_BLOCKED: the forward's log layout (stp_blend.h: rows in hierarchical mode, blocked in k-buffer mode)
// ABS: the absgrad request (stp_set_backward_absgrad).  Two more terms per blend, g[9] = |g[3]| and g[10] = |g[4]|, taken per lane BEFORE
// the merge levels (those sum lanes on one list position: the absolute value of a merged sum is another quantity) and carried through the
// merge, the fixed-point sums and the flush like the nine: eleven lanes of a 16-lane group hand a position over with the one atomic
// instruction, into slots 9, 10 of the same 64-byte record.  ABS = false is the kernel as it was, instruction for instruction.
// STATS: the blend-statistics request (stp_set_backward_blend_stats).  Three more terms per blend behind the nine (eleven): the pair's blend
// weight w = alpha T twice -- once to be summed, once to be maximised -- and a one to be counted.  They pass through the merge levels (the
// maximum merges with a max), the window (a scale of their own: they do not depend on dL/dpixel; the maximum as the float's bits under a
// 64-bit LDS max) and the flush into slots 11 .. 13 of the record (the maximum with an integer atomic max on the float's bits).  w comes
// from the FORWARD's expressions (blend_power, exp_blend, a transmittance chain of its own), not from the lean G of the gradient terms: a
// maximum has no summation order, so it is the re-sorting kernels' value bit for bit.  The pair SET is the forward's too -- every record of
// the log --, not the gradient terms': their lean transmittance may call a pixel saturated one record earlier than the forward did, and a
// count has no tolerance.  STATS = false is the kernel as it was.
// INVD: the inverse-depth request (stp_set_backward_invdepth).  (1 / z, D_final, dL/dD) joins the channel sums as a fourth channel -- one more
// product in cd and in FD, CD follows -- and one more term per blend, alpha T dL/dD, passes through the merge levels, the window (the
// gradient terms' fixed point: it is linear in dL/dD, which the tile's scale covers) and the flush into slot 14 of the record.  1 / z comes by
// Gaussian id from the geometry buffer: requested at the END of the step that requested the entry's record (which has arrived by then), a
// whole step ahead of its use.  The window grows by one row: ten .. fifteen terms are 40 .. 60 KB, three workgroups per CU up to thirteen
// terms (52 KB), two beyond.  INVD = false is the kernel as it was.
template <bool ABS, bool STATS, bool INVD> constexpr int replay_occupancy()
{
    if (!INVD) return STATS ? (ABS ? STP_REPLAY_BOTH_OCC : STP_REPLAY_STATS_OCC) : ABS ? STP_REPLAY_ABS_OCC : STP_REPLAY_OCC;
    return ((ABS ? 11 : 9) + (STATS ? 3 : 0) + 1) * WINDOW * 8 <= 52 * 1024 ? 3 : 2; // (160 KB of LDS per CU)
}
template <bool LOG_BLOCKED, bool ABS, bool STATS, bool INVD>
__global__ void __launch_bounds__(256, (replay_occupancy<ABS, STATS, INVD>()))
render_replay_kernel(const RenderArgs a)
{
    constexpr int SI = ABS ? 11 : 9;          // the gradient terms; with STATS also the first statistics term in g[] and s_acc (record slots GRAD_STATS .. + 2)
    constexpr int ZI = SI + (STATS ? 3 : 0);  // INVD: the inverse-depth term in g[] and s_acc (record slot GRAD_INVDEPTH)
    constexpr int NT = ZI + (INVD ? 1 : 0);   // terms per list position
    __shared__ unsigned long long s_acc[NT * WINDOW]; // [term][position - window start]
    __shared__ float s_md[4];

    const WavePixel wp = wave_pixel_map(a); // (the forward's thread -> pixel map, stp_render_wave.h)
    const int lane = wp.lane, w = wp.w, x = wp.x, q = wp.q, tile = wp.tile, px = wp.px, py = wp.py;
    if (a.tile_flags[tile] != 0u) return; // log overflow: the re-sorting backward takes this tile
    const uint2 range = wp.range;
    const bool inside = wp.inside;
    const int list_len = (int)(range.y - range.x);
    if (list_len <= 0) return;

    for (int i = (int)threadIdx.x; i < NT * WINDOW; i += 256) s_acc[i] = 0ull;

    BwdPixel bp;
    init_bwd_pixel<INVD>(bp, a, inside, px, py);
    // channel sums of the pixel (see blend_terms): final . dL, C . dL (running), -T_final (bg . dL)
    float FD_ = fmaf(bp.final_color[2], bp.dL_dpix[2], fmaf(bp.final_color[1], bp.dL_dpix[1], bp.final_color[0] * bp.dL_dpix[0]));
    if constexpr (INVD) FD_ = fmaf(bp.D_final, bp.dL_dD, FD_);
    const float FD = FD_;
    float CD = 0.0f;
    const float tfbg = -bp.T_final * bp.bg_dot;
    int n = inside ? (int)a.n_contrib[(size_t)a.W * py + px] : 0;
    float md = bwd_pixel_scale<INVD>(bp, a, inside, px, py);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) md = fmaxf(md, __shfl_xor(md, off));
    // fixed-point scale of the sums (stp_render_hier.inc: "on-chip gradient window"): one for the workgroup
    if (lane == 0) s_md[w] = md;
    __syncthreads(); // (also: the accumulators are zeroed)
    md = fmaxf(fmaxf(s_md[0], s_md[1]), fmaxf(s_md[2], s_md[3]));
    int md_exp = 0;
    const bool md_ok = md > 0.0f && md < 3.0e38f;
    if (md_ok) (void)frexpf(md, &md_exp);
    constexpr int FX_BITS = 31, FX_CAP_BITS = 20;
    const double fx_scale = ldexp(1.0, FX_BITS - md_exp), fx_inv = ldexp(1.0, md_exp - FX_BITS);
    // factor of term k that the blend step leaves out: applied once per sum
    // (terms 9, 10 are sums of magnitudes: the magnitude of the factors of terms 3, 4)
    auto term_scale = [&](int k) __attribute__((always_inline)) -> float {
        if constexpr (ABS) { if (k == 9) return 0.5f * (float)a.W; if (k == 10) return 0.5f * (float)a.H; }
        return k == 3 ? -0.5f * (float)a.W : k == 4 ? -0.5f * (float)a.H : (k >= 5 && k <= 7) ? -0.5f : 1.0f;
    };
    double fx_inv_term_ = fx_inv * (double)term_scale(lane & 15); // (flush: lane & 15 is the term a lane writes back)
    // the statistics' fixed point does not depend on dL/dpixel.  2^45: a blended pair has alpha >= 1/255 and T >= 1e-4, so w >= 2^-22 and every
    // float w is a whole number of 2^-45 -- the on-chip sum is EXACT (a Gaussian blended once has sum == max, bit for bit); w <= 0.99, 16 lanes
    // merge at most (2^49: inside the rounding trick's 2^51) and at most 256 pixels of a tile share a position (2^53).  The count is an integer.
    constexpr double ST_SCALE = 35184372088832.0;
    if constexpr (STATS) {
        if ((lane & 15) == GRAD_STATS) fx_inv_term_ = 1.0 / ST_SCALE;
        if ((lane & 15) == GRAD_STATS + 2) fx_inv_term_ = 1.0;
    }
    const double fx_inv_term = fx_inv_term_;
    const float fx_cap = (md_ok || md == 0.0f) ? ldexpf(1.0f, min(md_exp + FX_CAP_BITS, 126)) : 0.0f; // (a tile whose M is not finite: nothing fits, every term goes to memory)

    // Addressing: wave-uniform bases (SGPR pairs) + one 32-bit byte offset per load, so that the loop's loads are
    // `global_load ... v_off, s[base]` without 64-bit address arithmetic (v_lshl_add_u64 issues at half the rate of a
    // 32-bit add on gfx950, tools/valu_rate_bench.hip).
    const char* const log_wave = log_wave_slice(a.blend_log, tile, __builtin_amdgcn_readfirstlane(w), a.log_depth);
    // (record indices are clamped to the slice: log_last_row = the last record index that has storage -- the spare block's --,
    // log_last_rec = the last one that can hold a record; a clamped read is readable garbage that is never used)
    const uint32_t log_last_row = (uint32_t)(a.log_depth + BLEND_LOG_SPARE - 1), log_last_rec = (uint32_t)(a.log_depth - 1);
    const uint32_t lane16 = (uint32_t)lane << LOG_PIECE_SHIFT;
    auto log_at = [&](uint32_t k) __attribute__((always_inline)) -> int { // record k of this lane
        return (int)*reinterpret_cast<const log_t*>(log_wave + log_record_offset<LOG_BLOCKED>(2u * k, lane16));
    };
    const float pxf = (float)px, pyf = (float)py;
    const float4* const eC = a.entC + range.x; // list-ordered entry records: mean + Gaussian id, conic + opacity, colour
    const float4* const eD = a.entD + range.x;
    const float4* const eF = a.entF + range.x;
    struct EntryRows { float4 c, d, f; };
    struct EntryZ : EntryRows { float z; }; // INVD: + 1 / z of the entry's Gaussian (fetch_z)
    using Entry = std::conditional_t<INVD, EntryZ, EntryRows>;
    auto make_entry = [&](const float4 c, const float4 d, const float4 f) __attribute__((always_inline)) {
        Entry e; e.c = c; e.d = d; e.f = f;
        if constexpr (INVD) e.z = 0.0f;
        return e;
    };
    // INVD: 1 / z of an entry whose rows were requested a step ago (every row read is an entry of the list: a visible Gaussian's id)
    auto fetch_z = [&](Entry& e) __attribute__((always_inline)) { if constexpr (INVD) e.z = a.invz[__float_as_int(e.c.w)]; };
    auto entry_at = [&](int p) __attribute__((always_inline)) { // (a harmless read of entry 0 where there is no record: no branch)
        const uint32_t off = (uint32_t)(p < list_len ? p : 0) << 4;
        auto at = [&](const float4* base) __attribute__((always_inline)) { return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + off); };
        return make_entry(at(eC), at(eD), at(eF));
    };

    const uint32_t list_last = (uint32_t)(list_len - 1);
    auto entry_at_clamped = [&](uint32_t p) __attribute__((always_inline)) { // (p beyond the list -- a corrupt log word -- reads the last entry)
        const uint32_t off = min(p, list_last) << 4;
        auto at = [&](const float4* base) __attribute__((always_inline)) { return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + off); };
        return make_entry(at(eC), at(eD), at(eF));
    };

    float Tx = 1.0f; // STATS: the pixel's transmittance as the forward chains it (bp.T follows the lean alpha)
    bool g_done = false; // STATS: the lean transmittance has called the pixel saturated: no gradient terms from here on (without STATS the lane stops)
    // the gradient terms of one record (reference maths); false = no gradient terms to add (no record, or the pixel saturates here).
    // With STATS a record (`act`) always has its statistics to add, whatever this returns: see the callers.
    auto blend_terms = [&](bool act, const Entry& cur, float (&g)[NT]) __attribute__((always_inline)) -> bool {
        // Straight-line form: every lane evaluates its (possibly stand-in) entry; a lane without a record, or whose pixel saturates
        // here, is switched off through its FACTORS -- all nine terms are linear in (T, T_final), so T := 0 and T_final := 0 make them
        // exact zeros (every other factor is finite: alpha <= 0.99, test_T >= 1e-6 where it is used, the stand-in is entry 0 of the
        // list) -- three selects instead of two branches and eighteen zeroing moves per step (profiles/EXPERIMENTS.md, round 4).
        const float4 co = cur.d;
        const float dx = cur.c.y - pxf, dy = cur.c.z - pyf;
        // the exponent with contracted products (7 instructions for the forward's 9) and 2^(x log2 e) without the forward's first-order
        // correction of the product's rounding (2 for 6): |relative error of G| < 3e-7 for exponents above -5.6, where a blend can be.
        // The blend SET is the log's; G only weighs gradient terms here, which are compared with a tolerance anyway.
        const float e2 = fmaf(co.y * dx, dy, 0.5f * fmaf(co.z * dy, dy, co.x * dx * dx));
        const float G = __builtin_amdgcn_exp2f(fmaxf(e2, 0.0f) * -1.44269502162933349609375f);
        const float alpha = fminf(0.99f, co.w * G);
        const float test_T = bp.T * (1.0f - alpha);
        bool ok_ = act && !(test_T < T_THRESHOLD);
        if constexpr (STATS) { ok_ = ok_ && !g_done; g_done = g_done || (act && !ok_); }
        const bool ok = ok_;
        // dL/dalpha = sum_ch (c_ch - (final_ch - C_ch) / test_T) dL_ch  with the channel sums taken first: cd = c . dL, FD = final . dL (a
        // constant of the pixel), CD = C . dL (a running scalar, CD += alpha T cd) -- six instructions instead of fifteen, and one
        // accumulated scalar instead of three colours; 1 / (1 - alpha) = T / test_T costs a multiply instead of a second reciprocal
        const float Tm = ok ? bp.T : 0.0f, tfbgm = ok ? tfbg : 0.0f;
        const float dchannel_dcolor = alpha * Tm;
        const float rcp_test_T = __builtin_amdgcn_rcpf(test_T);
        const float rcp_1ma = rcp_test_T * bp.T;
        float cd_ = fmaf(cur.f.z, bp.dL_dpix[2], fmaf(cur.f.y, bp.dL_dpix[1], cur.f.x * bp.dL_dpix[0]));
        if constexpr (INVD) cd_ = fmaf(cur.z, bp.dL_dD, cd_);
        const float cd = cd_;
        CD = fmaf(dchannel_dcolor, cd, CD);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) g[ch] = dchannel_dcolor * bp.dL_dpix[ch];
        float dL_dalpha = fmaf(-rcp_test_T, FD - CD, cd) * Tm;
        dL_dalpha = fmaf(tfbgm, rcp_1ma, dL_dalpha);
        const float dL_dG = co.w * dL_dalpha;
        const float gdx = G * dx, gdy = G * dy;
        // the frame's constant factors of the five geometric terms (-W/2, -H/2, -1/2 three times) are applied to the SUMS when they
        // leave the chip (term_scale), not to every pair: with u = G dx dL/dG, v = G dy dL/dG the five terms are eleven instructions
        const float u = gdx * dL_dG, v = gdy * dL_dG;
        g[3] = fmaf(v, co.y, u * co.x);
        g[4] = fmaf(u, co.y, v * co.z);
        g[5] = u * dx;
        g[6] = u * dy;
        g[7] = v * dy;
        g[8] = G * dL_dalpha;
        if constexpr (ABS) { g[9] = fabsf(g[3]); g[10] = fabsf(g[4]); } // (this lane's pair alone; exact zeros where the lane is switched off)
        if constexpr (INVD) g[ZI] = dchannel_dcolor * bp.dL_dD;         // (alpha T dL/dD: like the colour terms, zero where the lane is switched off)
        if constexpr (STATS) {
            // The pair set is the FORWARD's: every record of the log (`act`), which is what the re-sorting kernels blend.  `ok` may end a
            // pixel one record early -- its lean transmittance is an ulp off the forward's, and the last record of a saturating pixel can
            // sit on the threshold --: that pair's gradient terms are the exact zeros of a switched-off lane, its statistics are counted.
            const float ax = fminf(0.99f, co.w * exp_blend(blend_power(dx, dy, co)));
            const float wx = act ? ax * Tx : 0.0f;
            g[SI] = wx; g[SI + 1] = wx; g[SI + 2] = act ? 1.0f : 0.0f;
            Tx = act ? Tx * (1.0f - ax) : Tx;
        }
        bp.T = ok ? test_T : bp.T;
        return ok;
    };
    // merge lanes on the same position, then add to the window's sums (lo = first position of the window)
    // deep (wave-uniform): also the two mirror levels inside the 16-lane row
    // one_window (a literal at both call sites): the list fits the window -- no position lies in front of it, a position IS its slot
    auto merge_and_add = [&](bool ok, int cur_pos, int cur_id, float (&g)[NT], int lo, const bool deep, const bool one_window) __attribute__((always_inline)) {
        // Pairwise merge (DPP): a lane and its partner -- lane^1, lane^2, then the mirror lanes of its 8-lane half and
        // row -- that hold the same list position sum their terms in registers and only one of them goes to LDS.  Per
        // step 55 lanes blend on 17.5 distinct positions (C2); the LDS atomics serialise on equal addresses and were the
        // limiter (1.38 ms), the VALU had headroom: 0.94 ms.  The partner's value enters as the DPP operand of one
        // v_fmac per term.  (A pre-reduction that needs a whole quad on one position fires for one quad in ten.)
        {
            int key = ok ? cur_pos : -2 - lane; // unique when not blending
#define STP_MERGE_LEVEL(CTRL, LOWER)                                                                                    \
            {                                                                                                       \
                const int pk = __builtin_amdgcn_mov_dpp(key, CTRL, 0xF, 0xF, true);                                 \
                const bool match = pk == key;                                                                       \
                const float mf = (match && (LOWER)) ? 1.0f : 0.0f;                                                  \
                dpp_hazard_guard(); /* g[] was written by ordinary VALU instructions a moment ago */                \
                _Pragma("unroll") for (int kk = 0; kk < NT; kk++) {                                                 \
                    if (STATS && kk == SI + 1) g[kk] = fmaxf(g[kk], partner_fma<CTRL>(g[kk], mf, 0.0f)); /* w >= 0, mf is 0 or 1 */ \
                    else g[kk] = partner_fma<CTRL>(g[kk], mf, g[kk]);                                               \
                }                                                                                                   \
                if (match && !(LOWER)) key = -2 - lane; /* the upper lane of a matching pair has handed its terms over */ \
            }
            STP_MERGE_LEVEL(0xB1, (q & 1) == 0) // partner lane ^ 1 (quad_perm [1,0,3,2])
            STP_MERGE_LEVEL(0x4E, (q & 2) == 0) // partner lane ^ 2 (quad_perm [2,3,0,1])
            if (deep) {
                STP_MERGE_LEVEL(0x141, (x & 7) < 4)  // partner 7 - i inside each 8-lane half (row_half_mirror)
                STP_MERGE_LEVEL(0x140, x < 8)        // partner 15 - i inside the 16-lane row (row_mirror)
            }
#undef STP_MERGE_LEVEL
            ok = key >= 0; // (a lane that blends holds a list position, every other one its negative stand-in: no separate flag to carry through the levels)
        }
#ifdef STP_REPLAY_STATS
        {
            const int nw = __popcll(__ballot(ok)), ns = __popcll(__ballot(ok && cur_pos < lo));
            // lanes whose position a LOWER adding lane also holds (same row / another row): what the LDS serialises
            bool dup_row = false, dup_any = false;
            int mult = 1;
            for (int l = 0; l < 64; l++) {
                const int pl = __shfl(ok ? cur_pos : -1 - lane, l);
                if (ok && pl == cur_pos && l != lane) { mult++; if (l < lane) { dup_any = true; if ((l >> 4) == (lane >> 4)) dup_row = true; } }
            }
            const int n_dup = __popcll(__ballot(ok && dup_any)), n_dup_row = __popcll(__ballot(ok && dup_row));
            int mmax = ok ? mult : 0;
            for (int off = 32; off > 0; off >>= 1) mmax = max(mmax, __shfl_xor(mmax, off));
            if (lane == 0) { atomicAdd(&g_replay_stats[0], 1ull); atomicAdd(&g_replay_stats[2], (unsigned long long)nw); atomicAdd(&g_replay_stats[3], (unsigned long long)ns);
                             atomicAdd(&g_replay_stats[4], (unsigned long long)n_dup); atomicAdd(&g_replay_stats[5], (unsigned long long)n_dup_row); atomicAdd(&g_replay_stats[6], (unsigned long long)mmax); }
        }
#endif
        if (ok) {
            // (the three colour terms are alpha T dL/dpixel: below M each, below 16 M after the merge levels -- they cannot reach the
            // fixed point's cap of 2^20 M and stay out of the range check; the two absolute sums are IN it: after the merge levels a sum of
            // magnitudes can exceed the magnitude of the merged signed term)
            float gmax = fabsf(g[3]);
#pragma unroll
            for (int kk = 4; kk < SI; kk++) gmax = fmaxf(gmax, fabsf(g[kk])); // (the statistics have a scale of their own: not in the check)
            const int slot = one_window ? cur_pos : (cur_pos & (WINDOW - 1));
            if ((one_window || cur_pos >= lo) && gmax < fx_cap) { // nine (eleven) adds, nothing else
#pragma unroll
                for (int kk = 0; kk < SI; kk++) {
                    // round-to-nearest integer of g*scale through the 1.5*2^52 trick (|g*scale| < 2^51 + margin)
                    const double tq = fma((double)g[kk], fx_scale, 6755399441055744.0);
                    const long long qv = __double_as_longlong(tq) - 0x4338000000000000ll;
                    atomicAdd(&s_acc[kk * WINDOW + slot], (unsigned long long)qv);
                }
                if constexpr (INVD) { // (alpha T dL/dD: below M like the colour terms, out of the range check)
                    const double tq = fma((double)g[ZI], fx_scale, 6755399441055744.0);
                    atomicAdd(&s_acc[ZI * WINDOW + slot], (unsigned long long)(__double_as_longlong(tq) - 0x4338000000000000ll));
                }
                if constexpr (STATS) {
                    const double tq = fma((double)g[SI], ST_SCALE, 6755399441055744.0);
                    atomicAdd(&s_acc[SI * WINDOW + slot], (unsigned long long)(__double_as_longlong(tq) - 0x4338000000000000ll));
                    atomicMax(&s_acc[(SI + 1) * WINDOW + slot], (unsigned long long)__float_as_uint(g[SI + 1]));
                    atomicAdd(&s_acc[(SI + 2) * WINDOW + slot], (unsigned long long)(unsigned int)(int)g[SI + 2]); // (1 .. 16 after the merge levels)
                }
            } else { // a record the re-sort moved across a window boundary, or a term too large for the fixed point
#pragma unroll
                for (int kk = 0; kk < SI; kk++) atomicAdd(grad_slot(a, cur_id, kk), g[kk] * term_scale(kk));
                if constexpr (INVD) add_invdepth(a, cur_id, g[ZI]);
                if constexpr (STATS) {
                    atomicAdd(grad_slot(a, cur_id, GRAD_STATS), g[SI]);
                    max_blend_weight(a, cur_id, g[SI + 1]);
                    atomicAdd(grad_slot(a, cur_id, GRAD_STATS + 2), g[SI + 2]);
                }
            }
        }
    };
    // the window's sums leave the chip: 16-lane group = one position, nine lanes = its nine sums, one atomic
    // instruction (one request) into the Gaussian's 64-byte gradient record
    // (positions f0 .. f1 - 1, at most WINDOW of them; position p lives in slot p mod WINDOW)
    auto flush_range = [&](int f0, int f1) __attribute__((always_inline)) {
        __syncthreads();
        const int term = lane & 15;
        for (int pp = f0 + (int)(threadIdx.x >> 4); pp < f1; pp += 16) {
            const int p = pp & (WINDOW - 1);
            // (term = the record slot a lane writes; row = where its sum lives in s_acc: the statistics follow the gradient terms directly)
            const int row = (INVD && term == GRAD_INVDEPTH) ? ZI : (STATS && term >= GRAD_STATS) ? term - GRAD_STATS + SI : term;
            if (term < SI || (STATS && term >= GRAD_STATS && term < GRAD_STATS + 3) || (INVD && term == GRAD_INVDEPTH)) {
                const long long v = (long long)s_acc[row * WINDOW + p];
                if (v != 0) {
                    s_acc[row * WINDOW + p] = 0ull;
                    if (STATS && term == GRAD_STATS + 1) max_blend_weight(a, __float_as_int(eC[pp].w), __uint_as_float((unsigned int)v));
                    else atomicAdd(grad_slot(a, __float_as_int(eC[pp].w), term), (float)((double)v * fx_inv_term));
                }
            }
        }
    };

    // Where the splats are larger than the wave's 16x4 pixels every lane blends the same entries whatever its phase: de-phasing
    // buys nothing there and the two mirror levels of the merge are what keeps the LDS adds apart (workload L1: 2.8 ms with
    // them, 3.1 ms without).  Decided once per wave: do most of its pixels START on the same entry?
    bool same_start;
    {
        const int p0 = n > 0 ? log_at(0) : 0x7fffffff;
        int pmin = p0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pmin = min(pmin, __shfl_xor(pmin, o));
        same_start = __popcll(__ballot(p0 == pmin && n > 0)) >= 40;
    }
    float g[NT] = {};
    // Two dependent loads lead to a blend: log record (list position) -> the entry's record.  They are software
    // pipelined one step apart: `pos` / `en` hold the lane's next record and its entry, `pos1` the position of the one
    // after, each loaded an iteration before it is needed.
    if (list_len <= WINDOW) {
        // ---- the list fits one window (all of C2-full): the lanes walk their logs in step, record k in iteration k ----
        // De-phasing.  The kernel is bound by the LDS adds, and those by lanes that hit one address in one instruction:
        // neighbouring pixels blend the same entries in the same order, so lanes that walk their logs in step sit on the
        // same list position all the time (measured, C2-full, after the four merge levels: 41 adding lanes on 17.5 distinct
        // positions, the largest group 6 lanes; tools/replay_stats.py).  Lane x of every 16-lane row therefore starts x
        // iterations late: 15 % more iterations, but 42 adding lanes on 24 positions with the quad merge alone (half the
        // merge's VALU work), and 0.98 -> 0.92 ms.  (Other patterns measured: by quad 0.96-1.01, by row and lane 1.07, all
        // 64 lanes apart 1.64 ms.)
        const bool dense = same_start; // (wave-uniform)
        const int off = dense ? 0 : x;
        int nmax = n + off;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o));
        // Pipeline: `pos` = list position of my record of this step (-1: none), `raw1` = the log word of the record after it, read a step
        // ago and checked against the record count only now (a count can still shrink, see below); the entry of the NEXT step is
        // requested at the top of a step, the log word of the one after next right behind it -- unconditionally (a row of the log that
        // holds no record of mine is readable garbage): nothing in a step waits for a load issued in the same step.
        int pos = (0 < n && off == 0) ? log_at(0) : -1;
        int raw1 = log_at(min((uint32_t)max(1 - off, 0), log_last_rec));
        Entry en = entry_at(max(pos, 0));
        fetch_z(en);
        // one step: blends `cur` (loaded an iteration ago), loads the entry of the next step into `nxt`
        auto one_step = [&](const int k, const Entry& cur, Entry& nxt) __attribute__((always_inline)) {
            const int kr = k - off; // my record index
            // (index checks as one unsigned compare each -- n >= 0; the entry offset clamped with one unsigned minimum; the log row of a
            // record index outside the log is clamped to the last row of my slice -- the spare row --, whose word is read and never used)
            const bool have = (uint32_t)kr < (uint32_t)n;
            const bool have1 = (uint32_t)(kr + 1) < (uint32_t)n;
            const int cur_pos = pos, cur_id = __float_as_int(cur.c.w);
            const int pos1 = have1 ? raw1 : -1;
            nxt = entry_at_clamped(have1 ? (uint32_t)raw1 : 0u);
            raw1 = log_at(min((uint32_t)(kr + 2), log_last_row));
            pos = pos1;
            const bool ok = blend_terms(have, cur, g);
            if constexpr (STATS) { // every record goes to the merge and the adds with its statistics; the log is not cut short (g_done)
                merge_and_add(have, cur_pos, cur_id, g, 0, dense, true);
            } else {
                if (have && !ok) n = kr; // (an ulp of difference against the forward's transmittance: stop where it says so)
                merge_and_add(ok, cur_pos, cur_id, g, 0, dense, true);
            }
            fetch_z(nxt); // (INVD: the next step's 1 / z, behind this step's work: nxt's rows have arrived)
        };
        // two copies of the step, the entry registers alternating between them (no copy of the ten entry words at the back edge)
        Entry en2 = en;
#pragma unroll 1
        for (int k = 0; k < nmax; k += 2) {
            one_step(k, en, en2);
            if (k + 1 >= nmax) break;
            one_step(k + 1, en2, en);
        }
        flush_range(0, list_len);
    } else {
    // ---- longer lists, window by window: every lane pauses at its first record beyond the window ----
    int k = 0; // records consumed by this lane
    int pos = (0 < n) ? log_at(0) : EXHAUSTED;
    int pos1 = (1 < n) ? log_at(1) : EXHAUSTED;
    Entry en = entry_at(pos);
    fetch_z(en);
    // (Lanes are not de-phased here: measured slower with hard and with sliding windows, profiles/EXPERIMENTS.md, round 3.)
    // The window slides in HALF steps: a phase covers positions [lo, lo + WINDOW), position p lives in slot p mod WINDOW,
    // and the phase ends when every lane has left its LOWER half -- lanes that are ahead keep blending in the upper half meanwhile and
    // stop only at lo + WINDOW.  Then the lower half's sums leave the chip and its slots become the next phase's upper half.  With hard
    // windows (round 2) every lane idled from its last record of a window until the slowest lane of the slowest wave had finished it
    // (C3 replay 1.734 -> 1.645 ms, C5 1.714 -> 1.636; profiles/EXPERIMENTS.md, round 3).
#ifndef STP_REPLAY_RING_DIV
#define STP_REPLAY_RING_DIV 2 // steps of WINDOW / 2.  Quarter / eighth steps (more, smaller flushes and barriers): C3 replay 1.655 -> 1.669 / 1.708 ms,
                              // C5 1.637 -> 1.694 / 1.752
#endif
    constexpr int STEP = WINDOW / STP_REPLAY_RING_DIV;
    static_assert((WINDOW & (WINDOW - 1)) == 0, "slots are addressed by position mod WINDOW");
    for (int lo = 0;; lo += STEP) {
        const int hi = lo + WINDOW;
        const bool last = hi >= list_len;                  // (workgroup-uniform)
        const int leave = last ? EXHAUSTED : lo + STEP;    // the phase is over when every lane's next record is at or beyond this position
        for (;;) {
            if (!__any(pos < leave)) break;
            const bool act = pos < hi; // my next record belongs to this phase (or to an earlier one: a straggler)
            const Entry cur = en;
            const int cur_pos = pos, cur_id = __float_as_int(cur.c.w);
            // issue the next round of loads before touching this step's data
            k += (int)act;
            const int rec = log_at(min((uint32_t)(k + 1), log_last_rec));
            pos = act ? pos1 : pos;
            pos1 = act ? (k + 1 < n ? rec : EXHAUSTED) : pos1;
            en = entry_at(pos);
            const bool ok = blend_terms(act, cur, g);
            if constexpr (STATS) { // (as in the one-window loop)
                merge_and_add(act, cur_pos, cur_id, g, lo, same_start, false);
            } else {
                if (act && !ok) { n = k; pos = EXHAUSTED; pos1 = EXHAUSTED; } // (saturated one record earlier than the forward said)
                merge_and_add(ok, cur_pos, cur_id, g, lo, same_start, false);
            }
            fetch_z(en);
        }
        flush_range(lo, last ? list_len : lo + STEP);
        if (last) break;
        __syncthreads();
    }
    }
}

} // namespace

#ifdef STP_REPLAY_STATS
extern "C" int stp_debug_replay_stats(unsigned long long* out16)
{
    hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_replay_stats), sizeof(unsigned long long) * 16);
    unsigned long long z[16] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_replay_stats), z, sizeof(z));
    return (int)e;
}
#endif

int blend_log_rows(int depth) { return depth + BLEND_LOG_SPARE; }
int blend_log_default_depth() { return BLEND_LOG_DEPTH; }
int blend_log_clamp_depth(int d) // (a multiple of the block: a lane's records come in pieces)
{
    constexpr int Q = 8;
    static_assert(BLEND_LOG_DEPTH_MIN % Q == 0 && BLEND_LOG_DEPTH_MAX % Q == 0 && BLEND_LOG_DEPTH % Q == 0, "log depths are multiples of the block");
    d = d > BLEND_LOG_DEPTH_MAX ? BLEND_LOG_DEPTH_MAX : (d + Q - 1) / Q * Q;
    return d < BLEND_LOG_DEPTH_MIN ? BLEND_LOG_DEPTH_MIN : d;
}

// one instantiation per log layout and set of requests, REQ = RenderArgs::requests (absgrad: two more terms per list position than the nine,
// blend statistics: three, inverse depth: one -- fifteen with all of them)
template <int REQ> static void launch_replay_one(const RenderArgs& a, bool blocked, dim3 grid, hipStream_t st)
{
    constexpr bool ABS = (REQ & REQ_ABSGRAD) != 0, STATS = (REQ & REQ_BLEND_STATS) != 0, INVD = (REQ & REQ_INVDEPTH) != 0;
    if (blocked) hipLaunchKernelGGL((render_replay_kernel<true, ABS, STATS, INVD>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((render_replay_kernel<false, ABS, STATS, INVD>), grid, dim3(256), 0, st, a);
}

hipError_t launch_hier_replay(const FrameParams& f, const RenderArgs& a, hipStream_t st)
{
    static_assert((REQ_ABSGRAD | REQ_BLEND_STATS | REQ_INVDEPTH) == 7, "the table below is indexed by the three request bits");
    static constexpr decltype(&launch_replay_one<0>) BY_REQUESTS[8] = {launch_replay_one<0>, launch_replay_one<1>, launch_replay_one<2>, launch_replay_one<3>,
                                                                       launch_replay_one<4>, launch_replay_one<5>, launch_replay_one<6>, launch_replay_one<7>};
    BY_REQUESTS[a.requests & 7](a, log_blocked(f.s), dim3(f.gx * (f.ty1 - f.ty0)), st);
    return hipGetLastError();
}

} // namespace stp
