// stp_render_hier.inc -- the hierarchical (4x4 tail / 2x2 mid / per-pixel head) resorting blend kernel.
// Included by stp_render_hier_inst.hip, which instantiates it in slices (queue sizes x mode).
//
// Replaces sortGaussiansRayHierarchicaEvaluation + sortGaussiansRayHierarchicalCUDA_forward/_backward
// (reference stopthepop/hierarchical_render.cuh:207-935, 939-1035, 1038-1175) and its sorting
// primitives (:14-192).  The per-pixel blend order it produces is the one specified in SURVEY.md
// Appendix A (32-entry batches, keep 32 / emit 16, mid merges of 4+4, head insertion with
// pop-before-look); the machinery that produces it is redesigned for a 64-lane wavefront:
//
//   * one 256-thread workgroup per 16x16 tile, one WAVE per row of four 4x4 sub-tiles; a sub-tile is a
//     16-lane DPP row, a 2x2 quad is a DPP quad.  The forward's waves never synchronise with each other: every
//     hand-off is intra-wave (LDS in issue order + a compiler fence), there is no s_barrier at all.
//     (The reference's 32-lane warp holds two sub-tiles and relies on implicit lock-step in places.)
//   * all queue payloads are list positions; an entry's data comes from the list-ordered entry records
//     (BinningState::entA..entF): unit-stride loads at batch staging, L1-resident afterwards.
//   * the 32 incoming depths of a batch are produced by the wave's 64 lanes together (lane = entry x
//     sub-tile pair), then each 16-lane row ranks its own 32 candidates and merges them into its
//     sorted tail by counting (rank = #smaller), not by a compare-exchange network: one LDS pass, no
//     serial dependency chain.  Ties between candidates resolve by list position (stable).
//   * the mid queues live in LDS as (key, position) records; the merge of 4 new + old is again by counting,
//     with the 4 new keys exchanged through DPP quad broadcasts (no LDS, no ds_bpermute).
//   * a head feed fetches the four entries' records once per quad (lane q fetches entry q); the candidate
//     evaluation takes them as DPP quad_perm OPERANDS of its multiplies (quad_mul / quad_fma), the head level
//     is straight-line predicated code (head_candidate of stp_render_wave.h, Window::replace_front, pop_forward).
//   * the head queue and the blend state are registers (compile-time indexed); the tail and mid rays sit in LDS.
//
// Template: HEAD = per-pixel queue, MID = 2x2 queue (8,12,20), CULL = hierarchical_4x4_culling, MODE = forward /
// re-sorting backward (the reference's scheme: same traversal, stores G instead of alpha, gradient sums in a
// workgroup-shared LDS window; since the blend log only the fallback for tiles whose log overflowed) / recording
// forward (writes the blend log that stp_render_replay.hip walks) / forward of the debug depth visualisation.
#include "stp_internal.h"
#include "stp_render_wave.h"

namespace stp {

#ifdef STP_HIER_STATS
static __device__ unsigned long long g_hier_stats[16]; // (one copy per translation unit: only the slice below exports its reader)
#if defined(STP_INST_MODE) && STP_INST_MODE == 2 && STP_INST_MID == 8 // (PASS_FWD_RECORD)
extern "C" int stp_debug_hier_stats(unsigned long long* out16)
{
    hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_hier_stats), sizeof(unsigned long long) * 16);
    unsigned long long z[16] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_hier_stats), z, sizeof(z));
    return (int)e;
}
#endif
#endif

namespace {

#ifndef STP_BWD_WIN
#define STP_BWD_WIN 256
#endif
#ifndef STP_BWD_RING
#define STP_BWD_RING 512
#endif
#ifndef STP_BWD_WAVES
#define STP_BWD_WAVES 3 // waves per SIMD the backward kernel is compiled for (LDS allows 3 workgroups per CU at the default window)
#endif
#ifndef STP_FWD_WAVES
#define STP_FWD_WAVES 5 // waves per SIMD the default queue sizes' forward passes (HEAD 4, MID 8) are compiled for.  Five need <= 96 VGPRs and <= 32 KB of LDS
                        // (STP_FIFO_GROUPS = 4: measured neutral on its own).  Round 5, logs bit-identical, one box, alternating
                        // (profiles/r05_experiments/five_waves_ab.txt): C2-full recording forward 0.913 -> 0.866 ms with the mid level's lane views re-derived
                        // from a fresh lane id (STP_QUAD_VIEW: as VGPRs they were what the compiler spilled at 96 registers, reloaded in every push
                        // behind a vmcnt(0): 1.035 ms); C2-min (no culling: fits without that) 1.713 -> 1.576.  At FOUR waves the re-derivation alone
                        // costs 4 % (0.950): it pays only together with the fifth wave.
#endif
constexpr int BWD_WIN = STP_BWD_WIN;   // slots of the workgroup's on-chip gradient window (power of two, >= 256)
constexpr int BWD_RING = STP_BWD_RING; // list positions whose Gaussian id / slot the workgroup keeps in LDS (power of two)

#ifndef STP_FIFO_GROUPS
#define STP_FIFO_GROUPS 4
#endif
constexpr int FIFO_GROUPS = STP_FIFO_GROUPS; // emitted-but-not-yet-consumed groups of 16 a sub-tile may hold (power of two, >= 4)
#ifndef STP_HF_CAP
#define STP_HF_CAP 32
#endif
constexpr int HF_CAP = STP_HF_CAP; // head-level FIFO: list positions a quad may hold (power of two, >= 32: one consumption round adds up to 16)

struct HierLds { // dynamic-LDS carve, per workgroup (16 sub-tiles)
    static __host__ __device__ constexpr size_t tail_key() { return 0; }                         // float [16][64]
    static __host__ __device__ constexpr size_t tail_id() { return 16 * 64 * 4; }                // int   [16][64]
    static __host__ __device__ constexpr size_t new_key() { return 2 * 16 * 64 * 4; }            // float [16][32]
    static __host__ __device__ constexpr size_t new_id() { return 2 * 16 * 64 * 4 + 16 * 32 * 4; } // int [16][32]
    static __host__ __device__ constexpr size_t mid_key() { return 2 * 16 * 64 * 4 + 2 * 16 * 32 * 4; } // float [64][MID]
    static __host__ __device__ constexpr size_t mid_id(int MID) { return mid_key() + 64 * (size_t)MID * 4; }
    static __host__ __device__ constexpr size_t fifo(int MID) { return mid_key() + 2 * 64 * (size_t)MID * 4; }       // int [16][FIFO_GROUPS][16]
    static __host__ __device__ constexpr size_t rays(int MID) { return fifo(MID) + 16 * (size_t)FIFO_GROUPS * 16 * 4; } // float [4 waves][2 halves][8]: the tail rays
    static __host__ __device__ constexpr size_t mid_rays(int MID) { return rays(MID) + 4 * 2 * 8 * 4; }             // float [64 quads][4]: the mid rays
    static __host__ __device__ constexpr size_t fwd_total(int MID) { return mid_rays(MID) + 64 * 4 * 4; }
    // forward passes only (the region overlaps the backward's window, which starts at the same offset): the head-level
    // FIFOs, int [64 quads][HF_CAP] -- list positions that passed the quad-level pre-test and wait for their head steps
    static __host__ __device__ constexpr size_t hfifo(int MID) { return fwd_total(MID); }
    // backward only, shared by the workgroup: acc int64[9][BWD_WIN] (fixed-point gradient sums), tag int[BWD_WIN]
    // (list position that owns a slot, -1 = free), dirty int[BWD_WIN], ring_id / ring_cs int[BWD_RING] (position ->
    // Gaussian id / slot), wave_mask uint[4] (per-wave survivor masks of the batch being staged)
    static __host__ __device__ constexpr size_t acc(int MID) { return fwd_total(MID); }
    static __host__ __device__ constexpr size_t tag(int MID) { return acc(MID) + 9 * (size_t)BWD_WIN * 8; }
    static __host__ __device__ constexpr size_t dirty(int MID) { return tag(MID) + (size_t)BWD_WIN * 4; }
    static __host__ __device__ constexpr size_t ring(int MID) { return dirty(MID) + (size_t)BWD_WIN * 4; }
    static __host__ __device__ constexpr size_t ring_cs(int MID) { return ring(MID) + (size_t)BWD_RING * 4; }
    static __host__ __device__ constexpr size_t wave_mask(int MID) { return ring_cs(MID) + (size_t)BWD_RING * 4; }
    static __host__ __device__ constexpr size_t total(int MID, int mode) { return pass_backward(mode) ? wave_mask(MID) + 16 : hfifo(MID) + 64 * (size_t)HF_CAP * 4; }
};

// MODE: a render pass of stp_render_pass.h (PASS_*; the predicates pass_backward / pass_records / pass_depthviz / pass_invdepth).
// launch bounds: 4 waves per SIMD (<= 128 VGPRs) for the forward passes, 3 (<= 168) for the backward pass.  The passes with the inverse-depth
// output are instantiations of their own, the default queue sizes' at four waves per SIMD (128 VGPRs): their five-wave build has no register to spare.
// waves per SIMD of the forwards with the inverse-depth output: sized so that none of them spills (the four extra registers do not fit
// the budgets the plain forwards of the larger queues already overrun)
constexpr int invd_fwd_waves(int head, bool frcp) { return (head == 4 && frcp) ? 4 : head <= 8 ? 3 : 2; }
// waves per SIMD an instantiation is compiled for.  Backward: STP_BWD_WAVES; with the fourth channel two at heads 12 and 16, whose plain kernels
// spill at three already (the variants do not).  Forward: five for the default queue sizes (STP_FWD_WAVES), otherwise four.
constexpr int hier_waves(int head, int mid, int mode, bool frcp)
{
    if (mode == PASS_BWD_INVD) return head >= 12 ? 2 : STP_BWD_WAVES;
    if (mode == PASS_BWD) return STP_BWD_WAVES;
    if (pass_invdepth(mode)) return invd_fwd_waves(head, frcp);
    return (head == 4 && mid == 8 && frcp) ? STP_FWD_WAVES : 4;
}

// FRCP: the frame's Sigma^-1 entries are all tame (stp_forward knows from preprocess_kernel's status word), the depth
// keys' reciprocal needs no domain check (rcp_ieee<true>)
template <int HEAD, int MID, bool CULL, int MODE, bool FRCP>
__global__ void __launch_bounds__(256, hier_waves(HEAD, MID, MODE, FRCP)) render_hier_kernel(const RenderArgs a)
{
    constexpr bool INVD = pass_invdepth(MODE);
    // (the mid level's lane views from a fresh lane id: only where the register budget needs it -- five waves per SIMD WITH 4x4 culling, see STP_FWD_WAVES)
    constexpr bool FRESH_QUAD = !pass_backward(MODE) && !INVD && HEAD == 4 && MID == 8 && FRCP && STP_FWD_WAVES >= 5 && CULL;
    constexpr bool BACKWARD = pass_backward(MODE);
    constexpr bool RECORD = pass_records(MODE);
    constexpr bool DEPTHVIZ = pass_depthviz(MODE); // accumulate depth * alpha * T instead of colour (reference :1005-1008, stopthepop_common.cuh:264-282)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int OLDN = (MID - 4) / 4; // old mid entries owned per lane

    // thread -> pixel: wave_pixel_map() of stp_render_wave.h, written out.  The one piece of the scaffold this kernel keeps local: taken from
    // the function (same statements, same order) the default recording forwards -- 96 VGPRs for five waves per SIMD -- spill one more
    // register (<4, 8, true, PASS_FWD_RECORD, true>: 0 -> 1, without culling 4 -> 5; profiles/EXPERIMENTS.md, "shared scaffold").
    const int lane = (int)(threadIdx.x & 63);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // wave = sub-tile row inside the tile (wave-uniform: an SGPR)
    const int s = lane >> 4;               // sub-tile (DPP row) inside the wave
    const int x = lane & 15;               // lane inside the sub-tile
    const int m = x >> 2;                  // quad inside the sub-tile
    const int q = x & 3;                   // lane inside the quad
    const int t = workgroup_tile(a);
    const int tile_x = t % a.gx, tile_y = a.ty0 + t / a.gx, tile = tile_y * a.gx + tile_x;
    const uint2 range = a.ranges[tile];
    const int cx = tile_x * TILE + 4 * s, cy = tile_y * TILE + 4 * w; // my sub-tile's corner pixel
    const int px = cx + 2 * (m & 1) + (q & 1), py = cy + 2 * (m >> 1) + (q >> 1);
    const bool inside = px < a.W && py < a.H;
    if constexpr (BACKWARD) {
        // fallback duty only: when the forward recorded blend logs, this kernel handles just the tiles whose log overflowed
        if (a.flag_mode == 1 && a.tile_flags[tile] == 0u) return;
    }
    bool active = inside;
    if constexpr (!BACKWARD) {
        // An empty tile is background.  Not only a shortcut: the forward's pads and stand-ins read "entry 0 of the tile's list" and multiply it
        // by a zero weight, which is harmless only while that entry exists -- in a frame WITHOUT ANY entry (num_rendered == 0 behind a
        // run-ahead launch) the record arrays are uninitialised memory, and 0 x NaN is NaN (found by tools/fuzz_parity.py, round 5).
        if (range.y <= range.x) {
            if (inside) write_background_pixel<DEPTHVIZ, RECORD>(a, px, py);
            if constexpr (INVD) { if (inside) a.out_invdepth[(size_t)a.W * py + px] = 0.0f; }
            return;
        }
    }
    if constexpr (!BACKWARD && !DEPTHVIZ) {
        // Fused entry gather (RenderArgs::fused_gather): the workgroup sorts its tile's list and writes keys, list and entry records itself --
        // what tile_sort_gather_kernel<TS_SMALL> did in a launch of its own in front of this one, whose memory latency lay on the critical
        // path.  Here the other workgroups on the CU, busy blending, hide it.  The keys take the first 8 KB of the LDS carve, which nothing
        // holds yet; the hand-off to the render body below is the gather kernel's own between its passes.  Longer lists stay that kernel's.
        const int n = (int)(range.y - range.x); // (>= 1 here)
        if (a.fused_gather && n <= TS_SMALL) {
            tile_sort_gather_lds(a.gather, reinterpret_cast<uint64_t*>(smem), tile, range, n, (int)threadIdx.x);
            __threadfence_block();
            __syncthreads();
        }
    }

    const int st = w * 4 + s;
    // Register budget.  What the TAIL level needs of the lane's identity -- its sub-tile's tail / staging / FIFO areas, its
    // slot in a batch, the staging rectangle -- is used once per batch of 32 entries but would stay in VGPRs across the whole
    // head level, the kernel's register peak (and the compiler spills exactly these to scratch: every reload then waits on
    // vmcnt(0), i.e. on all the blend-log stores in flight).  The tail-level code therefore re-derives them from a fresh
    // read of the lane id (fresh_lane(): two v_mbcnt the compiler cannot hoist) where it needs them.
    auto fresh_lane = [&]() __attribute__((always_inline)) -> int {
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };
#define STP_ROW_VIEW(L)                                                                                                  \
    const int lrow_ = (L); /* (evaluated once: fresh_lane() is volatile) */                                              \
    const int x = lrow_ & 15;                                                                                            \
    const int st_r = w * 4 + (lrow_ >> 4);                                                                               \
    float* const tk = reinterpret_cast<float*>(smem + HierLds::tail_key()) + st_r * 64;                                  \
    int* const ti = reinterpret_cast<int*>(smem + HierLds::tail_id()) + st_r * 64;                                       \
    float* const nk = reinterpret_cast<float*>(smem + HierLds::new_key()) + st_r * 32;                                   \
    int* const ni = reinterpret_cast<int*>(smem + HierLds::new_id()) + st_r * 32;                                        \
    int* const fifo = reinterpret_cast<int*>(smem + HierLds::fifo(MID)) + st_r * FIFO_GROUPS * 16;
    // The same for the MID level's view of the lane (round 5): its quad's queue / ray / FIFO areas and its position in the quad are needed once per
    // push of four entries, but as VGPRs they are alive through the head level too -- and at five waves per SIMD (96 VGPRs) these were what the
    // compiler spilled, reloaded in every push behind a vmcnt(0).  Re-derived from a fresh lane id where they are used.
    struct QuadView { int q; float* mk; int* mi; int* hfifo; };
#define STP_QUAD_VIEW(L)                                                                                                 \
    const int lquad_ = (L); /* (evaluated once: fresh_lane() is volatile) */                                             \
    const int q = lquad_ & 3;                                                                                            \
    const uint32_t qi_ = (uint32_t)(w * 16) + ((uint32_t)lquad_ >> 2);                                                   \
    const uint32_t qmid_ = (MID & (MID - 1)) == 0 ? qi_ << __builtin_ctz(MID) : qi_ * (uint32_t)MID; /* (shifts: the compiler's choice was a 64-bit mad) */ \
    float* const mk = reinterpret_cast<float*>(smem + HierLds::mid_key()) + qmid_;                                       \
    int* const mi = reinterpret_cast<int*>(smem + HierLds::mid_id(MID)) + qmid_;                                         \
    float* const mray = reinterpret_cast<float*>(smem + HierLds::mid_rays(MID)) + (qi_ << 2);                            \
    int* const hfifo = reinterpret_cast<int*>(smem + HierLds::hfifo(MID)) + (qi_ << __builtin_ctz(HF_CAP));             \
    const QuadView qv{q, mk, mi, hfifo}; (void)qv; (void)mray;

    // rays (reference hierarchical_render.cuh:316-355): pixel ray through the integer pixel position,
    // mid ray through quad corner + 0.5, tail ray through sub-tile corner + 1.5
    const float3 cam = make_float3(a.cam[0], a.cam[1], a.cam[2]);
    const float3 pix_dir = view_ray(a.inv_vp, cam, (float)px, (float)py, a.W, a.H);
    // (the quad's mid ray is needed four times per group of 16 entries: it lives in LDS, not in three registers)
    if (q == 0) {
        float* const mray = reinterpret_cast<float*>(smem + HierLds::mid_rays(MID)) + (st * 4 + m) * 4;
        const float3 md = view_ray(a.inv_vp, cam, (float)cx + 0.5f + 2.0f * (float)(m & 1), (float)cy + 0.5f + 2.0f * (float)(m >> 1), a.W, a.H);
        mray[0] = md.x; mray[1] = md.y; mray[2] = md.z; mray[3] = 0.0f;
    }
    // batch staging: lane handles list entry (lane & 31) for sub-tiles 2*(lane>>5) and 2*(lane>>5)+1
#define STP_STAGE_VIEW(L)                                                                                                \
    const int lstage_ = (L); /* (evaluated once: fresh_lane() is volatile) */                                            \
    const int half = lstage_ >> 5, e = lstage_ & 31;                                                                           \
    const int sxA = tile_x * TILE + 4 * (2 * half), sxB = sxA + 4;                                                       \
    float* const tray = reinterpret_cast<float*>(smem + HierLds::rays(MID)) + (w * 2 + half) * 8;                        \
    float* const nkA = reinterpret_cast<float*>(smem + HierLds::new_key()) + (w * 4 + 2 * half) * 32;                    \
    int* const niA = reinterpret_cast<int*>(smem + HierLds::new_id()) + (w * 4 + 2 * half) * 32;
    // the two tail rays of my half-wave are needed once per batch only: they live in LDS, not in six registers
    {
    STP_STAGE_VIEW(lane)
    if (e == 0) {
        const float3 tA = view_ray(a.inv_vp, cam, (float)sxA + 1.5f, (float)cy + 1.5f, a.W, a.H);
        const float3 tB = view_ray(a.inv_vp, cam, (float)sxB + 1.5f, (float)cy + 1.5f, a.W, a.H);
        tray[0] = tA.x; tray[1] = tA.y; tray[2] = tA.z; tray[3] = 0.0f;
        tray[4] = tB.x; tray[5] = tB.y; tray[6] = tB.z; tray[7] = 0.0f;
    }
    }
    wave_sync();

    // Queue payload.  Forward: the Gaussian id.  Backward: the entry's POSITION in the tile list (relative
    // to range.x), so that gradient terms can be summed on chip per list position; the id is recovered from
    // the wave's ring of recently staged positions (or, for stragglers, from point_list).  -1 = pad.
    unsigned long long* const acc = reinterpret_cast<unsigned long long*>(smem + HierLds::acc(MID)); // [9][BWD_WIN]
    int* const tag = reinterpret_cast<int*>(smem + HierLds::tag(MID));
    int* const dirty = reinterpret_cast<int*>(smem + HierLds::dirty(MID));
    int* const ring = reinterpret_cast<int*>(smem + HierLds::ring(MID)); // (resorting backward only)
    int* const ring_cs = reinterpret_cast<int*>(smem + HierLds::ring_cs(MID));
    unsigned int* const wave_mask = reinterpret_cast<unsigned int*>(smem + HierLds::wave_mask(MID));
    // forward passes: every piece of an entry's data comes from the list-ordered entry arrays, indexed by position
    const float4* const eA = a.entA + range.x;
    const float4* const eB = a.entB + range.x;
    const float4* const eC = a.entC + range.x;
    const float4* const eD = a.entD + range.x;
    const float4* const eF = a.entF + range.x;
    const int list_last = max((int)(range.y - range.x) - 1, 0);
    int staged = 0; // list positions staged so far (workgroup-uniform); the ring covers [staged - BWD_RING, staged)
    int ccount = 0; // entries so far that survived culling for at least one of the tile's 16 sub-tiles (workgroup-uniform)
    auto to_id = [&](int v) __attribute__((always_inline)) -> int {
        // the ring first (a plain LDS read: v = -1 reads slot BWD_RING-1, harmlessly); the few positions that have
        // left the ring take the memory path together, in a wave-uniform branch that is almost never entered
        int r = ring[v & (BWD_RING - 1)];
        const bool old = v >= 0 && v < staged - BWD_RING;
        if (__builtin_expect(__any(old), 0)) {
            if (old) r = (int)a.point_list[range.x + min(v, list_last)];
        }
        return v < 0 ? -1 : r;
    };
    if constexpr (BACKWARD) {
        for (int i = (int)threadIdx.x; i < BWD_WIN; i += 256) {
            tag[i] = -1;
            dirty[i] = 0;
#pragma unroll
            for (int k = 0; k < 9; k++) acc[k * BWD_WIN + i] = 0ull;
        }
        __syncthreads();
    }

    // recording forward: this lane's slice of the blend log and its record count
    // Blend log, [tile][wave][record][lane] in this mode (stp_blend.h).  (Tried and rejected: per-lane contiguous records collected in LDS
    // and written as 32-byte pieces -- every sector written once, but the extra LDS round trips and the replay's
    // strided reads cost more than the partial-line writes: forward 1.85 -> 2.02 ms, replay 1.50 -> 1.80 ms; a ring of 32
    // rows in LDS flushed as whole 128-byte lines -- the kernel is VALU-bound and the bookkeeping costs more than the
    // stores: 1.49 -> 1.79 ms.)
    // Addressing: the wave's slice is a wave-uniform base (SGPR pair) and the lane keeps ONE 32-bit cursor, so a store is
    // `global_store_short v_off, v_pos, s[base]` with no 64-bit address arithmetic in the blend step.
    char* const log_wave = RECORD ? log_wave_slice(a.blend_log, tile, __builtin_amdgcn_readfirstlane(w), a.log_depth) : nullptr;
    // (rows [record][lane], stp_blend.h: the cursor is 2 * records so far -- also beyond the log's depth --, the address (cursor << 6) | 2 * lane)
    const uint32_t log_cap2 = 2u * (uint32_t)a.log_depth; // (wave-uniform) cursor of the first record that does not fit: it maps to the spare block
    const uint32_t log_lane16 = (uint32_t)lane << LOG_PIECE_SHIFT;
    uint32_t log_j2 = 0u;
    auto log_append = [&](bool upd, int pay) __attribute__((always_inline)) {
        // no branch: the record goes to the lane's current slot whether or not the step blends (a later blend overwrites it; behind
        // the log's depth everything lands in the first spare row), only the cursor's advance depends on `upd`.  (A conditional store
        // brings an s_cbranch_execz and a split loop body: C2-full forward 0.88 -> 1.41 ms; non-temporal stores 1.9 -> 3.1 ms, the
        // partial lines then go to HBM one by one.)
        *reinterpret_cast<log_t*>(log_wave + log_record_offset<false>(min(log_j2, log_cap2), log_lane16)) = (log_t)pay;
        log_j2 += upd ? 2u : 0u;
    };
    auto log_records = [&]() __attribute__((always_inline)) -> int { return (int)(log_j2 >> 1); };

    Window<HEAD> head;
    if constexpr (BACKWARD) head.init(); else head.init_padded(); // (forward passes: always-full queue, see Window::replace_front)
    FwdPixel fp;
    BwdPixel bp;
    if constexpr (BACKWARD) init_bwd_pixel<INVD>(bp, a, inside, px, py);
    else init_fwd_pixel(fp);

    int n_tail = 0; // valid entries in my sub-tile's tail (uniform per 16-lane row)
    int n_mid = 0;  // entries in my quad's mid queue (uniform per quad), a multiple of 4
    int mid_pending = 0; // of those, entries that still have to reach the heads (pads of the final flush excluded)

    // ---- backward: on-chip gradient window ------------------------------------------------------
    // The reference issues nine global fp32 atomics per blended (pixel, Gaussian) pair (68-71 ms per C2 frame on
    // MI355X).  Here the workgroup owns a window of BWD_WIN slots x 9 sums in LDS.  The four waves stage every
    // batch of 32 list entries together (two s_barriers per batch -- the only ones in this kernel); slots are
    // handed out round-robin to the entries that survive culling for at least one of the tile's 16 sub-tiles; a
    // slot's sums leave the chip exactly once, when the slot is handed to a newer entry (or at the end), with
    // the waves sharing that work: one set of nine global atomics per (tile, Gaussian) instead of per blended
    // pair.  A blend that arrives after its slot was recycled (a straggler deep in a queue) falls back to
    // global atomics.
    //
    // LDS fp32 atomics are unusable for this on gfx950: ds_add_f32 sustains ~190 cycles per wave instruction,
    // ds_add_u64 ~7 (tools/lds_atomic_bench.hip).  The sums are therefore 64-bit FIXED POINT: every term of a
    // tile is linear in dL/dpixel of one of its 256 pixels, so with M = max |dL/dpixel| over the tile (rounded
    // up to a power of two) a term t is stored as round(t * 2^31 / M); |t| < 2^20 M fits 51 bits (anything
    // larger -- never seen -- goes to memory directly), and integer addition makes the on-chip part of the sum
    // order-independent.  Resolution is M * 4.7e-10 per add, whatever the pixel: below fp32 round-off of the sums
    // only where the Gaussian's pixels have |dL/dpixel| near M.  Dynamic range of dL/dpixel INSIDE a tile costs
    // resolution: against u * sum |term| (u = 2^-24) the half-quantum per add sums to 0.6 (median) .. 8.5 under a
    // dense N(0,1) image, and to 6e5 for a faint Gaussian of a tile with one pixel 2^20 above the others
    // (tests/torch_ref_colour_bound.py: Q; DESIGN.md section 4).
    float wave_md = 0.0f;
    if constexpr (BACKWARD) {
        wave_md = bwd_pixel_scale<INVD>(bp, a, inside, px, py);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) wave_md = fmaxf(wave_md, __shfl_xor(wave_md, off));
        // the window is shared by the four waves: one scale for the whole tile
        if (lane == 0) wave_mask[w] = __float_as_uint(wave_md);
        __syncthreads();
        wave_md = fmaxf(fmaxf(__uint_as_float(wave_mask[0]), __uint_as_float(wave_mask[1])),
                        fmaxf(__uint_as_float(wave_mask[2]), __uint_as_float(wave_mask[3])));
        __syncthreads(); // wave_mask is reused by the staging below
    }
    int md_exp = 0;
    if (wave_md > 0.0f && wave_md < 3.0e38f) (void)frexpf(wave_md, &md_exp); // wave_md <= 2^md_exp
    const double fx_scale = ldexp(1.0, 31 - md_exp), fx_inv = ldexp(1.0, md_exp - 31);
    const float fx_cap = ldexpf(1.0f, min(md_exp + 20, 126)); // a quad-reduced term is compared after the reduction
    auto accumulate = [&](int pos, int id, const float (&g_in)[9]) __attribute__((always_inline)) {
        // Quad pre-reduction: the four pixels of a 2x2 quad see the same candidates and very often blend the same
        // entry at the same instruction.  When all four lanes of my quad are here with the same list position,
        // their terms are summed with two DPP steps and lane 0 alone goes to LDS (4x fewer LDS atomics, no
        // same-address serialisation).
        float g[9];
#pragma unroll
        for (int k = 0; k < 9; k++) g[k] = g_in[k];
        // absgrad request (wave-uniform flag): this pixel's |dL/dmean2D| goes to memory as it is, in front of the quad pre-reduction -- the
        // absolute value of a quad's sum is another quantity.  Two atomics per blend on the tiles this kernel takes; nothing in LDS.
        if (a.requests & REQ_ABSGRAD) add_absgrad(a, id, g_in);
        const unsigned long long here = __ballot(1);
        bool mine = true; // do I write to LDS / memory?
        if (((here >> (lane & ~3)) & 0xFull) == 0xFull) {
            const int p0 = quad_bcast_i<0>(pos), p1 = quad_bcast_i<1>(pos), p2 = quad_bcast_i<2>(pos), p3 = quad_bcast_i<3>(pos);
            if (p0 == p1 && p0 == p2 && p0 == p3) {
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    g[k] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(g[k]), 0xB1, 0xF, 0xF, true)); // quad_perm [1,0,3,2]
                    g[k] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(g[k]), 0x4E, 0xF, 0xF, true)); // quad_perm [2,3,0,1]
                }
                mine = q == 0;
            }
        }
        if (!mine) return;
        int cs = -1;
        if (pos >= staged - BWD_RING) cs = ring_cs[pos & (BWD_RING - 1)];
        // The range check takes the SUM of the magnitudes, not their maximum: fmaxf drops a NaN operand, so with dL/dpixel non-finite in
        // one channel only -- that channel's colour term and the six geometric terms NaN, the other two colour terms finite -- a maximum
        // came out finite, and the NaN terms went through the integer conversion below as large finite garbage.  A sum keeps a NaN or an
        // inf of any term, the comparison is then false and the terms go to memory as they are.  (sum < cap implies every term < cap.)
        float gsum = fabsf(g[0]);
#pragma unroll
        for (int k = 1; k < 9; k++) gsum += fabsf(g[k]);
        if (cs >= 0 && tag[cs] == pos && gsum < fx_cap) {
#pragma unroll
            for (int k = 0; k < 9; k++) {
                // round-to-nearest integer of g*scale through the 1.5*2^52 trick (|g*scale| < 2^51 + margin)
                const double t = fma((double)g[k], fx_scale, 6755399441055744.0);
                const long long qv = __double_as_longlong(t) - 0x4338000000000000ll;
                atomicAdd(&acc[k * BWD_WIN + cs], (unsigned long long)qv);
            }
            dirty[cs] = 1;
        } else {
#pragma unroll
            for (int k = 0; k < 9; k++) atomicAdd(grad_slot(a, id, k), g[k]);
        }
    };
    // write back slot `cs` if it is dirty; `first`/`last` split the nine terms between cooperating lanes
    auto flush_slot = [&](int cs, int first, int last) __attribute__((always_inline)) {
        if (dirty[cs]) {
            const int old_id = to_id(tag[cs]);
            for (int k = first; k < last; k++) {
                const long long v = (long long)acc[k * BWD_WIN + cs];
                acc[k * BWD_WIN + cs] = 0ull;
                if (v != 0) atomicAdd(grad_slot(a, old_id, k), (float)((double)v * fx_inv));
            }
        }
    };
    auto flush_all = [&]() __attribute__((always_inline)) {
        __syncthreads(); // every wave has finished blending
        for (int cs = (int)threadIdx.x; cs < BWD_WIN; cs += 256) flush_slot(cs, 0, 9);
    };

    // Re-sorting backward: the data a blend needs of its Gaussian (conic, mean, colour) is fetched when
    // an entry BECOMES the front of the head queue -- one feed step (>100 instructions) before it is blended --
    // so the gather's latency is off the blend's critical path.
    int front_key = -1; // head.id[0] the registers below belong to
    FrontData front_fd{};
    int front_gid = -1;
    auto refresh_front = [&]() __attribute__((always_inline)) {
        if (active && head.num > 0 && head.id[0] != front_key) {
            front_key = head.id[0];
            front_gid = to_id(front_key);
            front_fd = load_front<INVD>(a, front_gid);
        }
    };
    auto blend_front = [&]() __attribute__((always_inline)) { // reference :386-417
        if (!active) { head.num--; return; }
        float g[9];
        if (head.id[0] != front_key) refresh_front(); // not prefetched (cannot happen after a refresh; kept for safety)
        const float T_before = bp.T;
        const bool ok = blend_backward_terms<INVD>(bp, a, px, py, front_fd, head.store[0], g);
        if (ok) accumulate(head.id[0], front_gid, g);
        // blend-statistics request (wave-uniform flag): this pair's blend weight goes to memory as it is, three atomics per blend
        if (ok && (a.requests & REQ_BLEND_STATS)) add_blend_stats(a, front_gid, blend_weight(T_before, front_fd.co.w, head.store[0]));
        // inverse-depth request (PASS_BWD_INVD): alpha T dL/dD of this pair goes to memory as it is, one atomic per blend
        if constexpr (INVD) if (ok) add_invdepth(a, front_gid, blend_weight(T_before, front_fd.co.w, head.store[0]) * bp.dL_dD);
        if (!ok) { active = false; head.num--; return; }
        head.pop();
    };

    // Forward passes: the branch-free blend of the always-full queue's front (reference :386-417).
    // The colour of the popped entry is only needed to accumulate C, which nothing else depends on: its gather is
    // issued here and consumed at the NEXT pop (one whole feed step later), when the previous pending product
    // pend_w * pend_c is added.  Lanes that do not blend issue a harmless load of Gaussian 0.
    float pend_w = 0.0f;
    float pend_c[3] = {0.0f, 0.0f, 0.0f};
    float depth_acc = 0.0f;
    // INVD: 1 / z of the popped entry rides the same one-step-late product.  It comes by Gaussian id from the geometry buffer, and the id from
    // the entry's record row C: two dependent loads, so the id is requested at the pop, 1 / z at the NEXT pop (the id has arrived by then)
    // and its product is added at the pop after that -- two weights in flight (pend_w2: the entry pend_z belongs to).
    float inv_D = 0.0f, pend_w2 = 0.0f, pend_z = 0.0f, pend_idf = 0.0f;
    auto pop_forward = [&]() __attribute__((always_inline)) { // consumes slot 0 of the always-full queue; replace_front() follows
        if constexpr (INVD) {
            inv_D = fmaf(pend_w2, pend_z, inv_D);
            const float zl = a.invz[__float_as_int(pend_idf)]; // (a lane that did not blend holds a stand-in's id: a harmless load, weight and value zeroed)
            pend_z = pend_w != 0.0f ? zl : 0.0f;
            pend_w2 = pend_w;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ch++) fp.C[ch] = fmaf(pend_w, pend_c[ch], fp.C[ch]);
        const float alpha0 = head.store[0];
        const float test_T = fp.T * (1.0f - alpha0);
        const bool doing = active && !(head.depth[0] < 0.0f); // a pad (depth -FLT_MAX; real depths are >= 0) in front = the reference's queue is not full: nothing to blend
        const bool upd = doing && !(test_T < T_THRESHOLD);
        const int pay = head.id[0]; // (never negative: pads carry position 0)
        const float4 colr = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(eF) + ((uint32_t)pay << 4)); // (uniform base + 32-bit offset; a pad reads entry 0: harmless, see pend_w)
        pend_c[0] = colr.x; pend_c[1] = colr.y; pend_c[2] = colr.z;
        if constexpr (INVD) pend_idf = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(eC) + ((uint32_t)pay << 4) + 12); // (the entry's Gaussian id: the last word of row C)
        pend_w = upd ? alpha0 * fp.T : 0.0f;
        if constexpr (DEPTHVIZ) depth_acc += upd ? head.depth[0] * alpha0 * fp.T : 0.0f;
        fp.T = upd ? test_T : fp.T;
        if constexpr (RECORD) {
            log_append(upd, pay);
        }
        active = active && (upd || !doing); // saturated pixels retire
    };

    // (re-sorting backward only)
    auto feed_one = [&](int cid, float3 p0, float3 p1, float3 p2, float4 co, float2 xy) __attribute__((always_inline)) { // reference :479-522
        const float depth = depth_along_ray<FRCP>(p0, p1, p2, pix_dir);
        const float dx = xy.x - (float)px, dy = xy.y - (float)py;
        const float power = blend_power(dx, dy, co);
        if (!active || depth < 0.0f) return;
        if (power > 0.0f) return;
        const float G = exp_blend(power);
        const float alpha = fminf(0.99f, co.w * G);
        if (alpha < ALPHA_THRESHOLD) return;
        head.insert(depth, cid, G);
    };

    // feed the four front mid entries mk/mi[0..3] to the quad's four head queues (reference :421-536).
    // Pad entries (id -1, only present while draining) are skipped AFTER the pop-before-look step,
    // exactly like the reference's checkvalid path; outside draining no pad can be among the four.
    // feed4_from(fid): lane q of the quad brings candidate q (list position, -1 = none)
    auto feed4_from = [&](const int fid) __attribute__((always_inline)) {
        int pf = 0;
        float4 c0 = make_float4(0, 0, 0, 0), c1 = c0, c2 = c0, co = c0;
        float2 xy = make_float2(0, 0);
        float4 eAq = c0, eBq = c0, eCq = c0, eDq = c0;
        if constexpr (BACKWARD) {
            const int gid_f = to_id(fid); // Gaussian id
            if (fid != -1) { // pads are never dereferenced
                c0 = a.cov3D_inv[3 * (size_t)gid_f + 0];
                c1 = a.cov3D_inv[3 * (size_t)gid_f + 1];
                c2 = a.cov3D_inv[3 * (size_t)gid_f + 2];
                co = a.conic_opacity[gid_f];
                xy = a.means2D[gid_f];
            }
        } else { // entry record by position; a pad (-1, only while draining) reads entry 0; its opacity is zeroed below (head_candidate<0>): alpha 0 fails the candidate tests
            pf = min(max(fid, 0), list_last); // (clamped from above too: depth keys that are NaN -- an overflowing Sigma^-1 -- break the counting ranks, and a stale slot must not become a wild address)
            eAq = ent_row(eA, pf); eBq = ent_row(eB, pf); eCq = ent_row(eC, pf); eDq = ent_row(eD, pf);
        }
// (candidate I's rows as DPP quad_perm operands: staging them through a per-wave LDS slab for plain operands cuts issue cycles but puts
// an LDS round trip into every group step's chain -- measured slower, profiles/EXPERIMENTS.md, round 5)
#define STP_FEED(I)                                                                                                     \
    {                                                                                                                   \
        /* pop before the candidate is looked at */                                                                    \
        if constexpr (BACKWARD) { if (head.num >= HEAD) blend_front(); }                                                \
        else pop_forward();                                                                                             \
        const int cid = quad_bcast_i<I>(BACKWARD ? fid : pf);                                                           \
        if constexpr (!BACKWARD) { /* straight-line evaluation, broadcast operands folded into the arithmetic */         \
            const HeadCandidate c = head_candidate<I, FRCP>(fid, eAq, eBq, eCq, eDq, pix_dir, px, py, active);          \
            head.replace_front(c.pass, c.pass ? c.depth : -FLT_MAX, cid, c.alpha);                                      \
        } else if (cid != -1) {                                                                                         \
            const float3 b0 = make_float3(quad_bcast<I>(c0.x), quad_bcast<I>(c0.y), quad_bcast<I>(c0.z));               \
            const float3 b1 = make_float3(quad_bcast<I>(c1.x), quad_bcast<I>(c1.y), quad_bcast<I>(c1.z));               \
            const float3 b2 = make_float3(quad_bcast<I>(c2.x), quad_bcast<I>(c2.y), quad_bcast<I>(c2.z));               \
            const float4 bco = make_float4(quad_bcast<I>(co.x), quad_bcast<I>(co.y), quad_bcast<I>(co.z), quad_bcast<I>(co.w)); \
            const float2 bxy = make_float2(quad_bcast<I>(xy.x), quad_bcast<I>(xy.y));                                   \
            feed_one(cid, b0, b1, b2, bco, bxy);                                                                        \
        }                                                                                                               \
        if constexpr (BACKWARD) refresh_front();                                                                        \
    }
        STP_FEED(0) STP_FEED(1) STP_FEED(2) STP_FEED(3)
#undef STP_FEED
    };

    // ---- forward passes: quad-level pre-test and FIFO in front of the head level ------------------------------------
    // A candidate that fails the head level's tests is, for the pixel's blend order, a no-op: the reference pops the
    // queue's front when the queue is full BEFORE it looks at a candidate (:455-458), so a failing candidate can cost a
    // pop -- but the next candidate that passes would have popped the very same front entry before being inserted, and a
    // second failing candidate finds the queue no longer full.  By induction the reference's queue is at every moment
    // either the queue of "pop only in front of a passing candidate" or that queue minus its front, and the SEQUENCE of
    // popped (= blended) entries is the same whichever of the failing candidates are shown to the pixel.  (Nothing of the
    // kind holds one level up: a candidate occupies its place in the mid queue whether or not any pixel wants it.)
    // So every entry is tested against the quad as a whole when it ENTERS the quad's mid queue (the lane that computes its
    // mid depth has its record in registers anyway; plain operands): an upper bound of opacity * exp(power) over the
    // quad's four pixels, wide enough to cover every rounding of the per-pixel evaluation.  The verdict travels through
    // the mid queue as a payload bit, and of the four entries a mid queue hands down only the survivors are parked, in
    // order, in the quad's FIFO.
    // Head steps then run on groups of four parked candidates with all 64 lanes of the wave taking part, as often as
    // the fullest quad of the wave needs; the exact per-pixel tests are unchanged.
    QuadFifo<HF_CAP> hf; // (head and count quad-uniform; the slots: HierLds::hfifo)
    constexpr int HF_REJECT = 0x40000000; // payload flag in the mid queue: no pixel of this quad can blend the entry (quad_can_blend, stp_render_wave.h; a pad, -1, carries it too)
    // the four front entries of the quad's mid queue: those that can blend are parked, in order
    auto filter_push = [&](const QuadView& qv) __attribute__((always_inline)) {
        if (!quad_live(__ballot(active), lane)) return; // whole quad saturated / outside
        const int fid = qv.mi[qv.q];
        const bool keep = (fid & HF_REJECT) == 0;
        hf.push(qv.hfifo, qv.q, keep, fid);
#ifdef STP_HIER_STATS
        {   // candidates handed down / kept, one per quad and candidate
            const int shown = __popcll(__ballot(1)), kept = __popcll(__ballot(keep));
            if (lane == __builtin_ctzll(__ballot(1))) { atomicAdd(&g_hier_stats[10], (unsigned long long)shown); atomicAdd(&g_hier_stats[11], (unsigned long long)kept); }
        }
#endif
    };
    // head steps on parked candidates (when one is due: QuadFifo::round_due)
    auto head_round = [&](const bool force) __attribute__((always_inline)) -> bool { // false: nothing (more) to do now
        if (!hf.round_due(force, quad_live(__ballot(active), lane))) return false;
#ifdef STP_HIER_STATS
        {   // head group steps, candidates in them (quad x candidate), forced ones
            const int n = min(hf.cnt, 4);
            const int c = __popcll(__ballot(q < n));
            if (lane == 0) { atomicAdd(&g_hier_stats[12], 1ull); atomicAdd(&g_hier_stats[13], (unsigned long long)c); atomicAdd(&g_hier_stats[14], force ? 1ull : 0ull); }
        }
#endif
        wave_sync();
        STP_QUAD_VIEW(FRESH_QUAD ? fresh_lane() : lane)
        feed4_from(hf.take4(hfifo, q));
        return true;
    };
    auto head_rounds = [&](const bool force) __attribute__((always_inline)) {
#pragma unroll 1
        for (;;) {
            if (!head_round(force)) break;
            if (!head_round(force)) break; // (a second copy of the group step: half as many register shuffles at the loop's back edge)
        }
    };
    // feed the four front mid entries mk/mi[0..3] to the quad's four head queues (reference :421-536).
    auto feed4 = [&](const QuadView& qv) __attribute__((always_inline)) {
        if constexpr (!BACKWARD) filter_push(qv);
        else {
            if (!quad_live(__ballot(active), lane)) return; // whole quad saturated / outside
            feed4_from(qv.mi[qv.q]); // payload: list position; lane q fetches entry q for the whole quad
        }
    };

    // ---- mid level: merge 4 new (one per lane) into the quad's queue (reference :558-681) --------
    // all_pad: the group consists of pads only (final mid drain) -- it flushes real entries to the
    // heads without adding anything that still has to be fed.
    // MID == 8 (the default): the queue never holds more than four entries between two pushes, one per lane of the quad --
    // lane q keeps old entry q (key, payload) in REGISTERS, and a push is straight-line code: eight quad broadcasts, the
    // ranks by compare + add-with-carry, one LDS round trip that doubles as the permutation (the four front slots go to
    // the head level, the four back slots are read back as the new old entries).  An empty queue is four keys of NaN.
    float mq_key = __builtin_nanf(""); // my old entry (MID == 8 only); NaN = none: it compares false with everything and is never written
    int mq_id = -1;
    auto mid_push8 = [&](const float d, const int gid, const bool all_pad, const QuadView& qv) __attribute__((always_inline)) {
        const bool has_old = n_mid != 0; // (quad-uniform)
        const int q = qv.q; float* const mk = qv.mk; int* const mi = qv.mi;
        const float k0 = quad_bcast<0>(d), k1 = quad_bcast<1>(d), k2 = quad_bcast<2>(d), k3 = quad_bcast<3>(d);
        const float o0 = quad_bcast<0>(mq_key), o1 = quad_bcast<1>(mq_key), o2 = quad_bcast<2>(mq_key), o3 = quad_bcast<3>(mq_key);
        // my new entry: rank among the four new keys (ties by lane, reference :129-155) + old entries that stay in front of it
        // (old before new on equal keys)
        const int pn = (int)(k0 < d) + (int)(k1 < d) + (int)(k2 < d) + (int)(k3 < d)
                     + ((int)(k0 == d) & (int)(0 < q)) + ((int)(k1 == d) & (int)(1 < q)) + ((int)(k2 == d) & (int)(2 < q))
                     + (int)(o0 <= d) + (int)(o1 <= d) + (int)(o2 <= d) + (int)(o3 <= d);
        // my old entry: its rank among the old ones + new entries in front of it
        const int po = q + (int)(k0 < mq_key) + (int)(k1 < mq_key) + (int)(k2 < mq_key) + (int)(k3 < mq_key);
        const int base = has_old ? 0 : 4;
        wave_sync(); // (the previous push's reads are done)
        mk[base + pn] = d;
        mi[base + pn] = gid;
        if (has_old) { mk[po] = mq_key; mi[po] = mq_id; }
        if (!all_pad) mid_pending += 4;
        wave_sync();
        mq_key = mk[4 + q];
        mq_id = mi[4 + q];
        n_mid = 4;
        if (has_old) {
            feed4(qv); // slots 0..3
            mid_pending -= 4;
        }
    };
    auto mid_push = [&](float d, int gid, bool all_pad, const QuadView& qv) __attribute__((always_inline)) {
        if constexpr (MID == 8) { mid_push8(d, gid, all_pad, qv); return; }
        const int q = qv.q; float* const mk = qv.mk; int* const mi = qv.mi;
        const float k0 = quad_bcast<0>(d), k1 = quad_bcast<1>(d), k2 = quad_bcast<2>(d), k3 = quad_bcast<3>(d);
        // rank among the four new keys, ties by lane (reference :129-155)
        const int r = (int)(k0 < d || (k0 == d && 0 < q)) + (int)(k1 < d || (k1 == d && 1 < q)) +
                      (int)(k2 < d || (k2 == d && 2 < q)) + (int)(k3 < d || (k3 == d && 3 < q));
        int c = 0; // old entries that stay in front of me (old before new on equal keys)
        for (int i = 0; i < n_mid; i++) c += (int)(mk[4 + i] <= d);
        float okey[OLDN];
        int oid[OLDN], opos[OLDN];
#pragma unroll
        for (int u = 0; u < OLDN; u++) {
            const int p = q + 4 * u;
            okey[u] = 0.0f; oid[u] = -1; opos[u] = -1;
            if (p < n_mid) {
                okey[u] = mk[4 + p];
                oid[u] = mi[4 + p];
                opos[u] = p + (int)(k0 < okey[u]) + (int)(k1 < okey[u]) + (int)(k2 < okey[u]) + (int)(k3 < okey[u]);
            }
        }
        const bool feed = n_mid + 4 > MID - 4;
        const int base = feed ? 0 : 4;
        wave_sync(); // every read above happens before the writes below
        mk[base + r + c] = d;
        mi[base + r + c] = gid;
#pragma unroll
        for (int u = 0; u < OLDN; u++)
            if (opos[u] >= 0) { mk[base + opos[u]] = okey[u]; mi[base + opos[u]] = oid[u]; }
        n_mid += 4;
        if (!all_pad) mid_pending += 4;
        wave_sync();
        if (feed) {
            feed4(qv);
            n_mid -= 4; // the survivors already sit at [4 .. 4+n_mid)
            mid_pending -= 4;
        }
    };

    // ---- tail level ------------------------------------------------------------------------------
    // emit up to 16 front entries of the tail as groups of 4 (padded with (FLT_MAX,-1) only while draining),
    // then close the gap (reference :538-687 + :827-846 / :857-879)
    // Push up to 16 entries (payloads src[0..cnt)) through the mid level as groups of 4; a short last group is
    // padded with (FLT_MAX,-1) (only while draining), cnt == 0 emits one all-pad group that flushes the mid queue.
    auto process16 = [&](const int* src, int cnt) __attribute__((always_inline)) {
        for (int k = 0; k < 4; k++) {
            if (4 * k >= cnt && !(k == 0 && cnt == 0)) break;
            STP_QUAD_VIEW(FRESH_QUAD ? fresh_lane() : lane)
            const float qxc = (float)(px - (q & 1)) + 0.5f, qyc = (float)(py - (q >> 1)) + 0.5f; // centre of my 2x2 quad
            const int pos = 4 * k + q;
            int gid = -1;
            float d = FLT_MAX;
            if (pos < cnt) {
                gid = src[pos];
                if constexpr (BACKWARD) {
                    const int gg = to_id(gid);
                    const float3 p0 = f4_xyz(a.cov3D_inv[3 * (size_t)gg + 0]);
                    const float3 p1 = f4_xyz(a.cov3D_inv[3 * (size_t)gg + 1]);
                    const float3 p2 = f4_xyz(a.cov3D_inv[3 * (size_t)gg + 2]);
                    const float4 mr = *reinterpret_cast<const float4*>(mray);
                    d = depth_along_ray<FRCP>(p0, p1, p2, make_float3(mr.x, mr.y, mr.z));
                } else {
                    const float4 mr = *reinterpret_cast<const float4*>(mray);
                    gid = min(max(gid, 0), list_last); // (see feed4_from)
                    const float4 enA = ent_row(eA, gid), enB = ent_row(eB, gid), enC = ent_row(eC, gid);
                    d = depth_along_ray_ent<FRCP>(enA, enB, enC, make_float3(mr.x, mr.y, mr.z));
                    if constexpr (!BACKWARD) {
                        if (!quad_can_blend(enC, ent_row(eD, gid), qxc, qyc)) gid |= HF_REJECT;
                    }
                }
            }
            mid_push(d, gid, cnt == 0, qv);
        }
    };
    // drop the 16 front entries of the tail (after they were consumed or copied to the FIFO) and close the gap
    auto tail_drop16 = [&]() __attribute__((always_inline)) {
        n_tail = max(n_tail - 16, 0);
        if (n_tail > 0) {
            STP_ROW_VIEW(fresh_lane())
            const float a0 = tk[x + 16], a1 = tk[x + 32], a2 = tk[x + 48];
            const int b0 = ti[x + 16], b1 = ti[x + 32], b2 = ti[x + 48];
            wave_sync();
            tk[x] = a0; tk[x + 16] = a1; tk[x + 32] = a2;
            ti[x] = b0; ti[x + 16] = b1; ti[x + 32] = b2;
            wave_sync();
        }
    };

    // stage one batch of 32 list entries: depth along each sub-tile's tail ray (+ optional 4x4 culling)
    unsigned long long balA = 0, balB = 0; // survivors of the last staged batch: sub-tiles (0,2) in balA, (1,3) in balB
    auto stage_batch = [&](int base_idx) __attribute__((always_inline)) { // reference :700-772
        STP_STAGE_VIEW(fresh_lane())
        const int gi = base_idx + e;
        int id = -1;
        if constexpr (BACKWARD) { if (gi < (int)range.y) id = (int)a.point_list[gi]; }
        else id = gi < (int)range.y ? 0 : -1; // (forward passes never need the Gaussian id: entry data comes by position)
        const int ep = gi - (int)range.x;     // position of my entry in the tile list
        float dA = FLT_MAX, dB = FLT_MAX;
        const bool wave_live = BACKWARD ? (bool)__any(active) : true; // (backward) a finished wave only helps with the staging protocol
        if (id != -1 && wave_live) {
            bool cullA = false, cullB = false;
            float4 enC = make_float4(0, 0, 0, 0);
            if constexpr (!BACKWARD) enC = ent_row(eC, ep); // unit-stride loads: the 32 lanes of a half read 32 consecutive records
            if constexpr (CULL) { // reference :722-743
                if constexpr (!BACKWARD) {
                    // the sixteen sub-tile decisions of this entry were made by the entry gather (stp_tilesort.hip: subtile_cull_mask,
                    // the same functions on the same operands) and sit in the spare word of its colour record
                    const uint32_t mask = __float_as_uint(*reinterpret_cast<const float*>(reinterpret_cast<const char*>(eF) + ((uint32_t)ep << 4) + 12));
                    const uint32_t mine = mask >> (4 * w + 2 * half);
                    cullA = (mine & 1u) == 0u;
                    cullB = (mine & 2u) == 0u;
                } else {
                const float4 co = BACKWARD ? a.conic_opacity[id] : ent_row(eD, ep);
                const float2 xy = BACKWARD ? a.means2D[id] : make_float2(enC.y, enC.z);
                float2 mp;
                // (the two reciprocals of the test depend on the entry only: once for both sub-tiles)
                const float rcp_x = rcp_ieee(3.0f * 3.0f * co.x), rcp_y = rcp_ieee(3.0f * 3.0f * co.z);
                const float pA = max_contrib_power_rect_r(co, xy, make_float2((float)sxA, (float)cy), make_float2((float)sxA + 3.0f, (float)cy + 3.0f), 3.0f, 3.0f, rcp_x, rcp_y, mp);
                const float pB = max_contrib_power_rect_r(co, xy, make_float2((float)sxB, (float)cy), make_float2((float)sxB + 3.0f, (float)cy + 3.0f), 3.0f, 3.0f, rcp_x, rcp_y, mp);
                cullA = fminf(0.99f, co.w * exp_blend(-pA)) < ALPHA_THRESHOLD;
                cullB = fminf(0.99f, co.w * exp_blend(-pB)) < ALPHA_THRESHOLD;
                }
            }
            if (!(cullA && cullB)) {
                float3 p0, p1, p2;
                if constexpr (BACKWARD) {
                    p0 = f4_xyz(a.cov3D_inv[3 * (size_t)id + 0]);
                    p1 = f4_xyz(a.cov3D_inv[3 * (size_t)id + 1]);
                    p2 = f4_xyz(a.cov3D_inv[3 * (size_t)id + 2]);
                } else {
                    const float4 enA = ent_row(eA, ep), enB = ent_row(eB, ep);
                    p0 = make_float3(enA.x, enA.y, enA.z); p1 = make_float3(enA.w, enB.x, enB.y); p2 = make_float3(enB.z, enB.w, enC.x);
                }
                const float4 rA = *reinterpret_cast<const float4*>(tray), rB = *reinterpret_cast<const float4*>(tray + 4);
                if (!cullA) dA = depth_along_ray<FRCP>(p0, p1, p2, make_float3(rA.x, rA.y, rA.z));
                if (!cullB) dB = depth_along_ray<FRCP>(p0, p1, p2, make_float3(rB.x, rB.y, rB.z));
            }
        }
        const int payload = gi - (int)range.x; // queue payload: the entry's position in the tile list in every mode
        // compact the survivors of each sub-tile to the front of its staging area, in list order
        // (ballots are wave-uniform: every row can read its own sub-tile's count from them)
        balA = __ballot(dA != FLT_MAX);
        balB = __ballot(dB != FLT_MAX);
        const unsigned int mA = (unsigned int)(balA >> (32 * half)), mB = (unsigned int)(balB >> (32 * half));
        const unsigned int below = (1u << e) - 1u;
        if (dA != FLT_MAX) { const int i = __popc(mA & below); nkA[i] = dA; niA[i] = payload; }
        if (dB != FLT_MAX) { const int i = __popc(mB & below); nkA[32 + i] = dB; niA[32 + i] = payload; }
        if constexpr (BACKWARD) {
            // hand a window slot to every entry that is alive for the TILE (lanes e and e+32 hold the same entry)
            const unsigned long long bal = __ballot(dA != FLT_MAX || dB != FLT_MAX);
            if (lane == 0) wave_mask[w] = (unsigned int)(bal | (bal >> 32));
            __syncthreads(); // barrier A: all four survivor masks are in LDS
            const unsigned int m32 = wave_mask[0] | wave_mask[1] | wave_mask[2] | wave_mask[3];
            const bool alive = (m32 >> e) & 1u;
            const int cs = (ccount + __popc(m32 & ((1u << e) - 1u))) & (BWD_WIN - 1);
            ccount += __popc(m32);
            // the previous owner's sums leave the chip here; entry e is written back by wave (e & 3)
            if (alive && (e & 3) == w) flush_slot(cs, half ? 5 : 0, half ? 9 : 5);
            wave_sync(); // both halves have read the dirty flag
            if (alive && (e & 3) == w && half == 0) dirty[cs] = 0;
            __syncthreads(); // barrier B: write-back done before anybody can add to a recycled slot
            if (half == 0) { // every wave writes the same values: no further barrier needed before its own reads
                const int pos = gi - (int)range.x;
                ring[pos & (BWD_RING - 1)] = id;
                ring_cs[pos & (BWD_RING - 1)] = alive ? cs : -1;
                if (alive) tag[cs] = pos;
            }
        }
        wave_sync();
    };

    // rank my sub-tile's 32 staged candidates and merge them into the sorted tail (old before new on
    // equal keys; candidates among themselves by list position).  Reference :774-825, :24-70, :158-192.
    auto merge_batch = [&](int batch_base) __attribute__((always_inline)) { // batch_base: list index of the batch's first entry
        const int lane_m = fresh_lane();
        const int s_m = lane_m >> 4;
        const int n_new = __popc((unsigned int)(((s_m & 1) ? balB : balA) >> (32 * (s_m >> 1)))); // my sub-tile's survivors
        if (n_new == 0) return;
        STP_ROW_VIEW(lane_m)
        const int n_old = n_tail;
        const bool va = x < n_new, vb = x + 16 < n_new;     // my (up to) two new entries
        float ka = va ? nk[x] : 0.0f, kb = vb ? nk[x + 16] : 0.0f;
        int ia = va ? ni[x] : -1, ib = vb ? ni[x + 16] : -1;
        // Counting every candidate against every old entry and every old entry against every candidate costs two slow VALU
        // instructions per pair -- 2 x (32 + 32) pairs per lane at full queues, a quarter of the kernel.  The old entries are
        // SORTED, so (a) a candidate's number of old entries in front of it (c = #old <= key) is a six-probe search of the
        // tail (slots beyond the last old entry hold +inf), and (b) an old entry's number of candidates in front of it
        // (#new < its key = #candidates with c <= its index) is the running sum of a histogram of the c's -- one LDS add per
        // candidate, one 16-lane scan.  Only the candidates' ranks among themselves are still counted pair by pair.
        int* const cnt = ni; // (the staged payloads are in registers now; every lane clears the two slots it has just read)
        ni[x] = 0; ni[x + 16] = 0;
        if (x >= n_old) tk[x] = INFINITY;
        if (x + 16 >= n_old) tk[x + 16] = INFINITY;
        wave_sync();
        int ra = 0, rb = 0;
        int ca = 0, cb = 0; // upper bounds in tk[0..32): five halving probes over slots 0..30, then slot 31
        // (strict compares only: candidates with EQUAL keys -- a handful of batches per frame -- collide on one rank, which
        // is how they are found below; such a batch is redone with the reference's network anyway)
        // A batch leaves a sub-tile eleven candidates on average (C2-full): where no row of the wave has more than sixteen, no lane holds a
        // second candidate and everything computed for it -- half of the counting loop's compares, half of the probes -- is dropped.
        if (__all(n_new <= 16)) { // (wave-uniform; rows without candidates have left)
            for (int j = 0; j < n_new; j++) ra += (int)(nk[j] < ka);
            const float last = tk[31];
#pragma unroll
            for (int step = 16; step >= 1; step >>= 1) ca += tk[ca + step - 1] <= ka ? step : 0;
            ca += (int)(last <= ka);
        } else {
            for (int j = 0; j < n_new; j++) {
                const float kj = nk[j];
                ra += (int)(kj < ka);
                rb += (int)(kj < kb);
            }
            const float last = tk[31];
#pragma unroll
            for (int step = 16; step >= 1; step >>= 1) {
                const float pa = tk[ca + step - 1], pb = tk[cb + step - 1];
                ca += pa <= ka ? step : 0;
                cb += pb <= kb ? step : 0;
            }
            ca += (int)(last <= ka);
            cb += (int)(last <= kb);
        }
        if (va && ca < 32) atomicAdd(&cnt[ca], 1);
        if (vb && cb < 32) atomicAdd(&cnt[cb], 1);
        wave_sync();
        // old entries 2x and 2x + 1 are mine in this phase
        const bool ova = 2 * x < n_old, ovb = 2 * x + 1 < n_old;
        const float2 ok2 = *reinterpret_cast<const float2*>(tk + 2 * x);
        const int2 oi2 = *reinterpret_cast<const int2*>(ti + 2 * x);
        const int2 cn2 = *reinterpret_cast<const int2*>(cnt + 2 * x);
        const float oka = ok2.x, okb = ok2.y;
        const int oia = oi2.x, oib = oi2.y;
        int run = cn2.x + cn2.y; // inclusive scan over the row's 16 lanes (DPP row_shr, zeros shifted in)
        run += __builtin_amdgcn_update_dpp(0, run, 0x111, 0xF, 0xF, false); // row_shr:1
        run += __builtin_amdgcn_update_dpp(0, run, 0x112, 0xF, 0xF, false); // row_shr:2
        run += __builtin_amdgcn_update_dpp(0, run, 0x114, 0xF, 0xF, false); // row_shr:4
        run += __builtin_amdgcn_update_dpp(0, run, 0x118, 0xF, 0xF, false); // row_shr:8
        const int pa_old = 2 * x + run - cn2.y, pb_old = 2 * x + 1 + run; // index + #candidates in front
        wave_sync(); // all reads done
        float* const nkw = nk;
        int* const niw = ni;
        const int fa = ra + ca, fb = rb + cb;
        if (va) { tk[fa] = ka; ti[fa] = ia; }
        if (vb) { tk[fb] = kb; ti[fb] = ib; }
        if (ova) { tk[pa_old] = oka; ti[pa_old] = oia; }
        if (ovb) { tk[pb_old] = okb; ti[pb_old] = oib; }
        n_tail = n_old + n_new;
        wave_sync();
        // Exact ties among the batch's candidates.  The reference sorts the 32 slots of a batch with a Batcher odd-even
        // merge network (:158-192), which is not stable -- where two candidates of a sub-tile have bit-identical depths (a
        // handful of batches per C2 frame) its result depends on the slots the two sit in.  The strict ranks above give
        // such candidates the same rank, i.e. the same slot of the tail: the loser finds a foreign payload there (one LDS
        // read per candidate instead of a tie-break term in every compare of the counting loop).  Such a batch is redone the
        // reference's way: the 32 slots in list order, culled entries as (FLT_MAX, -1), the network with this row's 16
        // lanes as its 16 workers; the sorted array then IS the order of the candidates, which are written to the tail
        // once more (they occupy the same set of positions: only candidates with equal keys trade places).
        const bool tie = (va && ti[fa] != ia) || (vb && ti[fb] != ib); // somebody else's payload in my slot: equal keys
        if (__builtin_expect(__any(tie), 0)) {
            wave_sync();
            // (the colliding candidates left slots of the merged tail unwritten: every slot becomes "not an old entry" first,
            // then the old entries take their places again; the candidates follow at the end)
            for (int p = x; p < n_tail; p += 16) ti[p] = 0x7fffffff;
            wave_sync();
            if (ova) { tk[pa_old] = oka; ti[pa_old] = oia; }
            if (ovb) { tk[pb_old] = okb; ti[pb_old] = oib; }
            nkw[x] = FLT_MAX; nkw[x + 16] = FLT_MAX; niw[x] = -1; niw[x + 16] = -1;
            wave_sync();
            const int slot0 = batch_base - (int)range.x; // payload (list position) of the batch's slot 0
            if (va) { nkw[ia - slot0] = ka; niw[ia - slot0] = ia; }
            if (vb) { nkw[ib - slot0] = kb; niw[ib - slot0] = ib; }
            wave_sync();
            auto exchange = [&](int p, int q) __attribute__((always_inline)) { // strict '>' (reference :171,185)
                const float kp = nkw[p], kq = nkw[q];
                const int ip = niw[p], iq = niw[q];
                if (kp > kq) { nkw[p] = kq; nkw[q] = kp; niw[p] = iq; niw[q] = ip; }
            };
            for (int size = 2; size <= 32; size *= 2) {
                int stride = size / 2;
                exchange(2 * x - (x & (stride - 1)), 2 * x - (x & (stride - 1)) + stride);
                wave_sync();
                const int first_stride = stride;
                for (stride = first_stride / 2; stride > 0; stride /= 2) {
                    const int pos = 2 * x - (x & (stride - 1));
                    if ((x & (first_stride - 1)) >= stride) exchange(pos - stride, pos);
                    wave_sync();
                }
            }
            // the candidate of rank r is sorted slot r; its tail position is r + #(old keys <= its key), counted on the
            // merged tail (old entries = payload below this batch's first list position)
            ka = va ? nkw[x] : 0.0f; kb = vb ? nkw[x + 16] : 0.0f;
            ia = va ? niw[x] : -1; ib = vb ? niw[x + 16] : -1;
            ca = 0; cb = 0;
            for (int i = 0; i < n_tail; i++) {
                const bool is_old = ti[i] < slot0;
                const float ki = tk[i];
                ca += (int)(is_old && ki <= ka);
                cb += (int)(is_old && ki <= kb);
            }
            wave_sync();
            if (va) { tk[x + ca] = ka; ti[x + ca] = ia; }
            if (vb) { tk[x + 16 + cb] = kb; ti[x + 16 + cb] = ib; }
            wave_sync();
        }
    };

    // ---- main loop: stream the tile list in batches of 32, then drain tail -> mid -> head ---------
    // Streaming: after each batch, while a tail holds more than 32 entries its 16 front entries are emitted
    // (at most twice, reference :827-846).  Draining (list exhausted): emit until tail and mid are empty
    // (reference :855-918); the last emissions are all-pad groups that flush the mid queues.
    //
    // With 4x4 culling the four sub-tiles of a wave fill their tails at different rates, so their emissions
    // would fall on different batches and the expensive mid/head work would run for one 16-lane row at a time.
    // Emission and consumption are therefore decoupled: an emitted group of 16 is parked in a small per-sub-tile
    // FIFO, and groups are consumed in rounds in which every row that has a parked group takes part.  The
    // order in which a sub-tile's groups pass through its mid and head queues is unchanged.
    constexpr bool USE_FIFO = CULL;
    int fifo_head = 0, fifo_count = 0; // row-uniform
    int base_idx = (int)range.x;
    for (;;) {
        const bool draining = base_idx >= (int)range.y; // workgroup-uniform
        if constexpr (BACKWARD) {
            // the four waves stage batches together (barriers inside stage_batch): streaming ends for all of them at
            // once; a wave without live pixels keeps taking part in the staging but skips its own depth work
            if (!draining) { if (!__syncthreads_or((int)__any(active))) break; }
            else if (!__any(active)) break;
        } else {
            if (!__any(active)) break;
        }
        if (!draining) {
            stage_batch(base_idx);
            merge_batch(base_idx);
            base_idx += 32;
            staged += 32;
            if constexpr (USE_FIFO) {
                const unsigned long long act0 = __ballot(active);
                const bool live0 = ((act0 >> (lane & ~15)) & 0xFFFFull) != 0ull; // a sub-tile without live pixels just discards
#pragma unroll 1
                for (int rep = 0; rep < 2; rep++)
                    if (n_tail > 32) { // park the 16 front entries (the count stays below FIFO_GROUPS, see below)
                        if (live0) {
                            STP_ROW_VIEW(fresh_lane())
                            fifo[((fifo_head + fifo_count) & (FIFO_GROUPS - 1)) * 16 + x] = ti[x];
                            fifo_count++;
                        }
                        tail_drop16();
                    }
            }
        }
        // consume: rounds of one group per row.  Streaming: a round runs when every row that still has live
        // pixels has a parked group (full convergence), or when some row is about to run out of FIFO space
        // (count >= FIFO_GROUPS - 2; a batch adds at most two).  Draining: until nothing is left.
#pragma unroll 1
        for (;;) {
            int want = 0; // 1: parked group, 2: straight from the tail
            if (USE_FIFO && fifo_count > 0) want = 1;
            else if (draining ? (n_tail > 0 || mid_pending > 0) : (!USE_FIFO && n_tail > 32)) want = 2;
            bool go;
            if constexpr (USE_FIFO) {
                if (draining) go = __any(want != 0);
                else {
                    const unsigned long long act = __ballot(active);
                    const bool row_live = ((act >> (lane & ~15)) & 0xFFFFull) != 0ull;
                    go = __any(fifo_count >= FIFO_GROUPS - 2) || (__all(fifo_count > 0 || !row_live) && __any(fifo_count > 0));
                }
            } else go = __any(want != 0);
            // (head-level FIFOs: once the list is exhausted and nothing is left above them, one last pass empties them)
            const bool last = !BACKWARD && draining && !go;
            if (!go && !last) break;
#ifdef STP_HIER_STATS
            {   // consumption rounds by number of participating sub-tile rows, and live lanes in them
                const unsigned long long wm = __ballot(want != 0);
                const int nrows = __popcll(wm) >> 4;
                const int live = __popcll(__ballot(want != 0 && active));
                if (lane == 0) { atomicAdd(&g_hier_stats[nrows], 1ull); atomicAdd(&g_hier_stats[8], (unsigned long long)live); atomicAdd(&g_hier_stats[9], draining ? 1ull : 0ull); }
            }
#endif
            if (last) {
            } else if (want == 1) {
                wave_sync();
                STP_ROW_VIEW(fresh_lane())
                process16(fifo + fifo_head * 16, 16);
                fifo_head = (fifo_head + 1) & (FIFO_GROUPS - 1);
                fifo_count--;
            } else if (want == 2) {
                {
                    STP_ROW_VIEW(fresh_lane())
                    process16(ti, n_tail);
                }
                tail_drop16();
            }
            if constexpr (!BACKWARD) head_rounds(last); // (all 64 lanes again; the one call site of the head steps)
            if (last) break;
        }
        if (draining) break;
    }
    if constexpr (BACKWARD) {
        while (active && head.num > 0) { blend_front(); refresh_front(); } // reference :919-923
        flush_all();
    } else {
        // drain: pads that sort LAST push the remaining real entries to the front, one per step
#pragma unroll 1
        for (int it = 0; it < HEAD; it++) {
            pop_forward();
            head.replace_front(false, FLT_MAX, 0, 0.0f);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ch++) fp.C[ch] = fmaf(pend_w, pend_c[ch], fp.C[ch]); // the last popped entry
        if constexpr (INVD) { // the last two popped entries
            inv_D = fmaf(pend_w2, pend_z, inv_D);
            const float zl = a.invz[__float_as_int(pend_idf)];
            inv_D = fmaf(pend_w, pend_w != 0.0f ? zl : 0.0f, inv_D);
        }
    }

    if constexpr (RECORD) {
        // the reference leaves n_contrib unwritten in this mode; we keep the pixel's number of blended entries there
        const int nrec = log_records();
        if (inside) a.n_contrib[(size_t)a.W * py + px] = (uint32_t)nrec;
        finish_blend_log(a, tile, nrec, (int)(range.y - range.x));
    }
    if constexpr (!BACKWARD) {
        if (inside) write_forward_pixel<DEPTHVIZ, false>(a, px, py, fp, depth_acc, 0u); // (n_contrib: not by the plain forward, reference :1019; the recording forward's is above)
        if constexpr (INVD) { if (inside) a.out_invdepth[(size_t)a.W * py + px] = inv_D; }
    }
}

template <int HEAD, int MID, bool CULL, int MODE, bool FRCP = false>
hipError_t launch_hier_one(const FrameParams& f, const RenderArgs& a, hipStream_t st)
{
    const dim3 grid(f.gx * (f.ty1 - f.ty0)), block(256);
    hipLaunchKernelGGL((render_hier_kernel<HEAD, MID, CULL, MODE, FRCP>), grid, block, HierLds::total(MID, MODE), st, a);
    return hipGetLastError();
}

} // namespace

} // namespace stp
