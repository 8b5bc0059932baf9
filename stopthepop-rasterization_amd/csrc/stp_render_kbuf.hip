// stp_render_kbuf.hip -- PPX_KBUFFER forward passes (plain, recording, depth visualisation) on the wave64 machinery of the
// hierarchical kernel's head level.
//
// Replaces renderkBufferCUDA<3, W, false> (reference stopthepop/resorted_render.cuh:17-221): per pixel a sorted window of W
// entries keyed by the depth along the pixel's own ray; every entry of the tile's list is looked at in list order -- "if the
// window is full, blend its front; then, if the entry passes the tests, insert it" -- and the window is drained at the end.
//
// What the result depends on, and what it does not (the same argument as stp_render_hier.inc, filter_push): an entry that
// FAILS the tests can only cost the pixel a pop of the window's front -- which the next passing entry would have popped
// anyway before being inserted, and which a second failing entry no longer finds.  The sequence of blended entries is
// therefore the same whichever of the failing entries a pixel is shown, and a pixel's work is "its passing entries, in list
// order".  The previous kernel (stp_render_tile.hip, still the re-sorting BACKWARD; STP_KBUFFER=tile selects its forward) walked the whole
// list with all 64 lanes of a wave on the same entry: 600 cycles for every entry that reached any of the wave's 64 pixels,
// a third of the lanes doing anything.  Here:
//
//   * thread -> pixel as in the hierarchical and replay kernels (wave = row of four 4x4 sub-tiles, sub-tile = 16-lane DPP
//     row, 2x2 quad = DPP quad), so the recording forward writes the same blend log and the replay kernel is its backward;
//   * a batch of 32 list entries is tested against the wave's four sub-tiles by the 64 lanes together (lane = entry x pair of
//     sub-tiles): the EXACT minimum of the exponent's quadratic form over the sub-tile's rectangle, with a margin that
//     covers every rounding of the per-pixel evaluation -- a bound, unlike the reference's max-contribution estimate;
//     survivors are compacted per sub-tile with ballots, in list order;
//   * each quad tests a sub-tile's survivors against its own four pixels (lane q takes survivor 4g + q; quad_can_blend) and
//     parks what is left in its FIFO; head steps then run on groups of four parked entries with every quad of the wave on
//     its OWN entries -- the step itself (entry record fetched by one lane of the quad, DPP-operand evaluation, always-full
//     window with fused pop + insert) is the hierarchical head level's with HEAD = W.
//
// n_contrib: the reference counts the entries a pixel looked at before it saturated.  A pop that saturates is either the
// pop in front of the entry that follows the insertion which filled the window (count = that insertion's position + 1) or a
// pop of the final drain (count = the whole list); both are known here without having looked at the entries in between.
#include "stp_internal.h"
#include "stp_render_wave.h"

#include <cstdlib>
#include <cstring>

namespace stp {

#ifdef STP_KB_STATS
// debug build only: where in the window do candidates land?  [0..15] passing candidates by the number of window slots they pass on their way
// in from the back (0 = appended behind everything), [16..31] candidate steps by the LARGEST such distance among the wave's 64 lanes,
// [32] candidate steps (per wave), [33] passing (lane, candidate) pairs, [34] live lanes in those steps
static __device__ unsigned long long g_kb_stats[40];
extern "C" int stp_debug_kb_stats(unsigned long long* out40)
{
    hipError_t e = hipMemcpyFromSymbol(out40, HIP_SYMBOL(g_kb_stats), sizeof(unsigned long long) * 40);
    unsigned long long z[40] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_kb_stats), z, sizeof(z));
    return (int)e;
}
#endif

namespace {

// MODE (here and below): a forward pass of stp_render_pass.h.
// What the kernel body and a window policy share of a pixel: its blend state, its lists' record rows, and the record rows of the entry
// at the FRONT of its window.  Neither window carries alpha: it is evaluated again at the pop, from the same record with the same
// operations, hence to the same bits as when the entry passed its tests.  What the pop needs of the front entry -- mean, conic +
// opacity, colour -- is fetched when the entry BECOMES the front, one step earlier.
template <int MODE> struct KbPixel {
    static_assert(!pass_backward(MODE), "the wave64 k-buffer kernels are forward passes");
    static constexpr bool RECORD = pass_records(MODE), DEPTHVIZ = pass_depthviz(MODE);
    // INVD: a fourth accumulator D += alpha T / z.  1 / z comes by Gaussian id (the front entry's record row C carries it) from the geometry
    // buffer: the load is issued at the entry's blend and its product is added one blend later (or in the epilogue), like the hierarchical
    // kernel's colour.  A lane that does not blend keeps (0, 0): the row it read may be a stand-in's.
    static constexpr bool INVD = pass_invdepth(MODE);
    const float* invz;
    float D, pend_w, pend_z;
    int lane, px, py;
    bool active;
    int total, list_last;
    const float4 *eC, *eD, *eF;
    float3 pix_dir;
    FwdPixel fp;
    float depth_acc;
    int contrib; // n_contrib of the plain / depth forward (see the header)
    int cfull;   // what it becomes if the NEXT pop saturates the pixel
    BlockedLogCursor logc; // blend log (recording forward): blocked layout, whole pieces from blending lanes only (stp_blend.h)
    float4 frC, frD, frF;
    __device__ __forceinline__ void fetch_front(const int pos) { frC = ent_row(eC, pos); frD = ent_row(eD, pos); frF = ent_row(eF, pos); }
    // blend the front entry (depth `depth0`, list position `pay`) where `doing` holds (reference blend_one, resorted_render.cuh:74-119)
    __device__ __forceinline__ void blend_front(const bool doing, const float depth0, const int pay)
    {
        const float alpha0 = fminf(0.99f, frD.w * exp_blend(blend_power(frC.y - (float)px, frC.z - (float)py, frD)));
        const float test_T = fp.T * (1.0f - alpha0);
        const bool upd = doing && !(test_T < T_THRESHOLD);
        const float wgt = upd ? alpha0 * fp.T : 0.0f;
        fp.C[0] = fmaf(wgt, frF.x, fp.C[0]); fp.C[1] = fmaf(wgt, frF.y, fp.C[1]); fp.C[2] = fmaf(wgt, frF.z, fp.C[2]);
        if constexpr (DEPTHVIZ) depth_acc += upd ? depth0 * alpha0 * fp.T : 0.0f; // reference resorted_render.cuh:107
        if constexpr (INVD) {
            D = fmaf(pend_w, pend_z, D);
            const float zl = invz[__float_as_int(frC.w)];
            pend_z = upd ? zl : 0.0f;
            pend_w = wgt;
        }
        fp.T = upd ? test_T : fp.T;
        if constexpr (RECORD) logc.append(upd, pay);
        else contrib = (doing && !upd) ? cfull : contrib;
        active = active && (upd || !doing); // a saturated pixel retires
    }
};

// ---- the window in REGISTERS: Window<WIN>'s always-full form, the hierarchical head level's step with HEAD = WIN ----------------------
template <int WIN, int MODE, bool FRCP> struct KbRegWindow {
    static constexpr int FIFO_CAP = 32; // list positions a quad's FIFO may hold (one round of 16 survivors adds up to 16)
    // waves per SIMD the kernel is compiled for; the inverse-depth variants (four more registers per lane) one fewer, so that none spills
    static constexpr int WAVES = KbPixel<MODE>::INVD ? (WIN <= 4 ? 3 : 2) : WIN <= 4 ? 4 : WIN <= 16 ? 3 : 2;
    static constexpr bool DOUBLE_ROUND = WIN <= 8; // (two copies of the group step: fewer register shuffles per step)
    using Pixel = KbPixel<MODE>;
    Window<WIN> head;
    __device__ __forceinline__ void init(Pixel& k) { head.init_padded(); }
    __device__ __forceinline__ void fetch_front(Pixel& k) { k.fetch_front(head.id[0]); } // (a pad carries position 0: a harmless read)
    // consumes slot 0 of the always-full window; replace_front() follows.  A pad in front = the reference's window is not full: nothing to blend
    __device__ __forceinline__ void pop_forward(Pixel& k) { k.blend_front(k.active && !(head.depth[0] < 0.0f), head.depth[0], head.id[0]); }
#ifdef STP_KB_STATS
    __device__ __forceinline__ void stat(const Pixel& k, const bool pass, const float depth)
    {
        int disp = 0;
        for (int s_ = 1; s_ < WIN; s_++) disp += (int)(depth < head.depth[s_]);
        disp = pass ? disp : -1;
        int mx = disp;
        for (int o_ = 1; o_ < 64; o_ <<= 1) mx = max(mx, __shfl_xor(mx, o_));
        if (disp >= 0) atomicAdd(&g_kb_stats[min(disp, 15)], 1ull);
        const int np_ = __popcll(__ballot(pass)), na_ = __popcll(__ballot(k.active));
        if (k.lane == 0) { atomicAdd(&g_kb_stats[16 + min(max(mx, 0), 15)], 1ull); atomicAdd(&g_kb_stats[32], 1ull);
                           atomicAdd(&g_kb_stats[33], (unsigned long long)np_); atomicAdd(&g_kb_stats[34], (unsigned long long)na_); }
    }
#endif
    // candidate I of a group of four (rows fetched by lane I of the quad from the clamped position pf): pop, look, fused pop + insert
    template <int I> __device__ __forceinline__ void step(Pixel& k, const int fid, const int pf, const float4 eAq, const float4 eBq, const float4 eCq, float4& eDq)
    {
        pop_forward(k);
        const int cid = quad_bcast_i<I>(pf);
        const HeadCandidate c = head_candidate<I, FRCP>(fid, eAq, eBq, eCq, eDq, k.pix_dir, k.px, k.py, k.active);
#ifdef STP_KB_STATS
        stat(k, c.pass, c.depth);
#endif
        head.replace_front(c.pass, c.pass ? c.depth : -FLT_MAX, cid, 0.0f);
        fetch_front(k);
        if constexpr (!Pixel::RECORD) k.cfull = c.pass ? cid + 1 : k.cfull;
    }
    // drain: fillers that sort LAST push the remaining real entries to the front, one per step
    __device__ __forceinline__ void drain(Pixel& k)
    {
#pragma unroll 1
        for (int it = 0; it < WIN; it++) {
            pop_forward(k);
            head.replace_front(false, FLT_MAX, 0, 0.0f);
            fetch_front(k);
            k.cfull = k.total; // (only the drain's first pop can be the one "in front of the next entry")
        }
    }
};


// ---- the window as a per-lane RING in LDS ----------------------------------------------------------------------------------------------
// Where do candidates land in a pixel's window?  Measured on C3 (3M Gaussians, window 16; tools/kb_stats.py, profiles/r05_experiments/kb_stats_c3.txt):
// 92.7 % of the passing candidates are appended BEHIND every entry of the window, 6.6 % pass one entry, 0.7 % two or more; the LARGEST distance
// among the 64 lanes of a wave is 0 in 38 % of the candidate steps, 1 in 52 %, 2 in 9 %, above 2 in 1 %.  The register window above pays for the
// general case in every step: the front is consumed and all W slots move (15 compares, 14 tie terms, 30 payload selects, 16 medians at W = 16 --
// 75 half-rate instructions, 32 VGPRs, three waves per SIMD).  Here the window of a pixel is a ring of (depth, list position) records in the
// lane's own LDS column ([slot][thread]: the bank of an access is the lane, whatever the slot -- every lane may sit at its own ring position
// without a bank conflict), with a per-lane head and count:
//   * a candidate that fails its tests is a no-op for its pixel (the argument of this file's header: pop only in front of a passing candidate);
//   * a pop advances the head: nothing moves;
//   * an insertion walks in from the back while the entry in front of it is deeper (strict: a new entry goes behind equals, like the
//     reference's swap loop, resorted_render.cuh:187-196) -- one LDS round per entry passed, 0.74 rounds per step on average for the wave;
//   * the reference's swap loop is not a plain insertion when it carries an entry past EQUAL depths (the carried entry does not swap with
//     its equals: every run of equal depths among the displaced entries ends up rotated by one): such a step is detected while walking
//     (two consecutive displaced entries of equal depth) and its payloads are rotated afterwards, in a branch that is almost never entered.
// What the pop needs of the front entry is fetched when the entry becomes the front, as above; alpha is evaluated again at the pop.
template <int WIN, int MODE, bool FRCP> struct KbRingWindow {
    static constexpr int FIFO_CAP = 24; // (a round of 16 survivors adds up to 16; not a power of two: 40 KB of LDS = four workgroups per CU)
    static constexpr int WAVES = KbPixel<MODE>::INVD ? 3 : WIN <= 16 ? 4 : 3; // (LDS: 40 KB per workgroup at 16 entries, 48 / 56 KB at 20 / 24; the inverse-depth variants: three, none spills)
    static constexpr size_t RING_BYTES = (size_t)WIN * 256 * 8; // (depth, list position) [WIN][256]: slot-major, 8 bytes per thread
    static constexpr size_t LDS_BYTES = RING_BYTES + 16 * 32 * 4 + 64 * FIFO_CAP * 4;
    static constexpr bool DOUBLE_ROUND = false;
    static constexpr bool POW2 = (WIN & (WIN - 1)) == 0;
    using Pixel = KbPixel<MODE>;
    // the ring: logical entry k of my window lives in slot (rh + k) mod WIN of my column
    char* ring;
    uint32_t col;
    int rn, rh;          // entries in my window, slot of its front
    float back_d;        // my window's LAST entry (-FLT_MAX: the window is empty) and the one in front of it (-FLT_MAX: none): nine candidates
    int back_i;          // in ten are placed against these two without an LDS access
    float back2_d;
    int back2_i;
    int fr_id;           // the front entry the pixel's front rows belong to
    float fr_depth;
    __device__ __forceinline__ void init(Pixel& k)
    {
        col = (uint32_t)threadIdx.x * 8u;
        rn = 0; rh = 0;
        back_d = -FLT_MAX; back_i = 0; back2_d = -FLT_MAX; back2_i = 0;
        fr_id = 0; fr_depth = 0.0f;
    }
    static __device__ __forceinline__ int wrap(int p) // p in [0, 2 WIN) -> [0, WIN)
    {
        if constexpr (POW2) return p & (WIN - 1);
        else return p - (p >= WIN ? WIN : 0);
    }
    static __device__ __forceinline__ int prev_slot(int p) // p in [0, WIN) -> the slot in front of it
    {
        if constexpr (POW2) return (p - 1) & (WIN - 1);
        else return (p == 0 ? WIN : p) - 1;
    }
    __device__ __forceinline__ char* slot_addr(int p) const { return ring + (((uint32_t)p << 11) + col); }
    __device__ __forceinline__ float2 rd(int p) const { return *reinterpret_cast<const float2*>(slot_addr(p)); } // (.x depth, .y the position's bits)
    __device__ __forceinline__ void wr(int p, float d, int i) const { *reinterpret_cast<float2*>(slot_addr(p)) = make_float2(d, __int_as_float(i)); }

    __device__ __forceinline__ void fetch_front(Pixel& k) // (an empty window reads a stale slot: a harmless, clamped load)
    {
        const float2 r = rd(rh);
        fr_id = min(max(__float_as_int(r.y), 0), k.list_last);
        if constexpr (Pixel::DEPTHVIZ) fr_depth = r.x;
        k.fetch_front(fr_id);
    }
    // blend my window's front where `popping` holds and advance the ring's head
    __device__ __forceinline__ void pop_front(Pixel& k, const bool popping)
    {
        k.blend_front(popping, fr_depth, fr_id);
        rh = wrap(rh + (popping ? 1 : 0));
        rn -= popping ? 1 : 0;
        back_d = rn == 0 ? -FLT_MAX : back_d;
        back2_d = rn <= 1 ? -FLT_MAX : back2_d;
    }
    // insert (depth, cid) into my window where `ins` holds; returns the logical index it took
    __device__ __forceinline__ int ring_insert(const bool ins, const float depth, const int cid)
    {
        int j = rn;                       // the logical index the candidate takes: behind everything, for a start
        int p = wrap(rh + rn);            // ... and its slot
        const bool mv1 = ins && depth < back_d;   // the last entry is deeper than the candidate (strictly: a new entry goes behind its equals): it moves up
        const bool mv2 = mv1 && depth < back2_d;  // ... and so is the one in front of it
        bool tie = mv2 && back_d == back2_d;      // two displaced entries of equal depth: the reference's swap loop leaves them in another order
        if (__builtin_amdgcn_ballot_w64(mv1) != 0ull) {
            if (mv1) { wr(p, back_d, back_i); p = prev_slot(p); j--; }
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(mv2) != 0ull, 0)) { // one step in ten
                float prev_moved = back2_d;
                bool mv = mv2;
                if (mv) { wr(p, back2_d, back2_i); p = prev_slot(p); j--; }
                float cur_d = -FLT_MAX; int cur_i = 0;
                mv = mv && j > 0;
                if (mv) { const float2 r = rd(prev_slot(p)); cur_d = r.x; cur_i = __float_as_int(r.y); mv = depth < cur_d; }
                while (__builtin_amdgcn_ballot_w64(mv) != 0ull) {
                    if (mv) {
                        wr(p, cur_d, cur_i);
                        tie = tie || cur_d == prev_moved;
                        prev_moved = cur_d;
                        p = prev_slot(p);
                        j--;
                        mv = j > 0;
                        if (mv) { const float2 r = rd(prev_slot(p)); cur_d = r.x; cur_i = __float_as_int(r.y); mv = depth < cur_d; }
                    }
                }
            }
        }
        if (ins) {
            wr(p, depth, cid);
            // the window's last two entries afterwards: (back, candidate) when nothing moved, (candidate, back) when the last entry did, unchanged otherwise
            const bool none = !mv1, one = mv1 && !mv2;
            back2_d = none ? back_d : one ? depth : back2_d;
            back2_i = none ? back_i : one ? cid : back2_i;
            back_d = none ? depth : back_d;
            back_i = none ? cid : back_i;
            rn++;
        }
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(tie) != 0ull, 0)) {
            // reference resorted_render.cuh:187-196: the carried entry swaps only with strictly deeper ones, so it travels past its equals, which
            // keep their slots -- among the displaced entries [j + 1, rn) every run of equal depths ends up rotated left by one
            if (tie) {
                int k = j + 1;
                while (k < rn) {
                    const float2 rk = rd(wrap(rh + k));
                    int e = k;
                    while (e + 1 < rn && rd(wrap(rh + e + 1)).x == rk.x) e++;
                    if (e > k) {
                        for (int u = k; u < e; u++) wr(wrap(rh + u), rk.x, __float_as_int(rd(wrap(rh + u + 1)).y));
                        wr(wrap(rh + e), rk.x, __float_as_int(rk.y));
                    }
                    k = e + 1;
                }
                back_i = __float_as_int(rd(wrap(rh + rn - 1)).y);
                back2_i = __float_as_int(rd(wrap(rh + rn - 2)).y); // (a tie displaced at least two entries: rn >= 3)
            }
        }
        return j;
    }
    // candidate I of a group of four (rows fetched by lane I of the quad from the clamped position pf)
    template <int I> __device__ __forceinline__ void step(Pixel& k, const int fid, const int pf, const float4 eAq, const float4 eBq, const float4 eCq, float4& eDq)
    {
        const int cid = quad_bcast_i<I>(pf);
        const HeadCandidate c = head_candidate<I, FRCP>(fid, eAq, eBq, eCq, eDq, k.pix_dir, k.px, k.py, k.active);
        pop_front(k, c.pass && rn == WIN); // a full window gives up its front before the candidate goes in
        wave_sync();
        fetch_front(k);                    // the front behind it: needed at the next pop, a candidate step from now
        const bool ins = c.pass && k.active; // (a pixel that saturated at that pop is done)
        const int at = ring_insert(ins, c.depth, cid);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(ins && at == 0) != 0ull, 0)) { // the candidate IS the front now (a window that was empty, mostly)
            wave_sync();
            fetch_front(k);
        }
        if constexpr (!Pixel::RECORD) k.cfull = ins ? cid + 1 : k.cfull;
    }
    // drain: what is left in the window, front first.  Only a pop of a FULL window can be the reference's pop "in front of the next entry"
    __device__ __forceinline__ void drain(Pixel& k)
    {
        if (rn != WIN) k.cfull = k.total;
#pragma unroll 1
        for (int it = 0; it < WIN; it++) {
            if (!__any(k.active && rn > 0)) break;
            pop_front(k, k.active && rn > 0);
            wave_sync();
            fetch_front(k);
            k.cfull = k.total;
        }
    }
};

// ---- the kernel body: prologue, batch staging, quad pre-test and FIFO, head rounds, drain, epilogue -- whichever way the window is kept ----
template <int MODE, class WINDOW>
__device__ __forceinline__ void render_kbuffer_body(const RenderArgs& a, WINDOW& win, int* const s_stage /* [sub-tile][survivor] */, int* const s_fifo /* [quad][slot] */)
{
    constexpr bool RECORD = KbPixel<MODE>::RECORD;
    constexpr bool DEPTHVIZ = KbPixel<MODE>::DEPTHVIZ;
    constexpr bool INVD = KbPixel<MODE>::INVD;
    constexpr int CAP = WINDOW::FIFO_CAP;

    const WavePixel wp = wave_pixel_map(a);
    const int lane = wp.lane, w = wp.w, s = wp.s, m = wp.m, q = wp.q, px = wp.px, py = wp.py;
    const int total = (int)(wp.range.y - wp.range.x);
    KbPixel<MODE> k;
    k.lane = lane; k.px = px; k.py = py;
    k.active = wp.inside;
    if (total <= 0) { // an empty tile is background (and its "entry 0" -- what pads and stand-ins read -- may not exist: stp_render_hier.inc)
        if (wp.inside) write_background_pixel<DEPTHVIZ, true>(a, px, py);
        if constexpr (INVD) { if (wp.inside) a.out_invdepth[(size_t)a.W * py + px] = 0.0f; }
        return;
    }

    const float3 cam = make_float3(a.cam[0], a.cam[1], a.cam[2]);
    k.pix_dir = view_ray(a.inv_vp, cam, (float)px, (float)py, a.W, a.H);

    const float4* const eA = a.entA + wp.range.x;
    const float4* const eB = a.entB + wp.range.x;
    const float4* const eC = a.entC + wp.range.x;
    const float4* const eD = a.entD + wp.range.x;
    const float4* const eF = a.entF + wp.range.x;
    const int list_last = max(total - 1, 0);
    k.eC = eC; k.eD = eD; k.eF = eF;
    k.total = total; k.list_last = list_last;
    k.logc = BlockedLogCursor{RECORD ? log_wave_slice(a.blend_log, wp.tile, w, a.log_depth) : nullptr, 2u * (uint32_t)a.log_depth, (uint32_t)lane << LOG_PIECE_SHIFT};

    win.init(k);
    init_fwd_pixel(k.fp);
    k.depth_acc = 0.0f;
    if constexpr (INVD) { k.invz = a.invz; k.D = 0.0f; k.pend_w = 0.0f; k.pend_z = 0.0f; }
    k.contrib = total;
    k.cfull = total;
    k.frC = make_float4(0, 0, 0, 0); k.frD = k.frC; k.frF = k.frC;

    // four candidates per quad, lane q brings candidate q (list position, -1 = none)
    auto feed4_from = [&](const int fid) __attribute__((always_inline)) {
        const int pf = min(max(fid, 0), list_last);
        float4 eAq = ent_row(eA, pf), eBq = ent_row(eB, pf), eCq = ent_row(eC, pf), eDq = ent_row(eD, pf);
        win.template step<0>(k, fid, pf, eAq, eBq, eCq, eDq);
        win.template step<1>(k, fid, pf, eAq, eBq, eCq, eDq);
        win.template step<2>(k, fid, pf, eAq, eBq, eCq, eDq);
        win.template step<3>(k, fid, pf, eAq, eBq, eCq, eDq);
    };

    int* const hfifo = s_fifo + ((w * 4 + s) * 4 + m) * CAP;
    QuadFifo<CAP> hf;
    auto head_round = [&](const bool force) __attribute__((always_inline)) -> bool { // false: nothing (more) to do now
        if (!hf.round_due(force, quad_live(__ballot(k.active), lane))) return false;
        wave_sync();
        feed4_from(hf.take4(hfifo, q));
        return true;
    };
    auto head_rounds = [&](const bool force) __attribute__((always_inline)) {
#pragma unroll 1
        for (;;) {
            if (!head_round(force)) break;
            if constexpr (WINDOW::DOUBLE_ROUND) { if (!head_round(force)) break; }
        }
    };

    // ---- main loop: batches of 32 list entries -----------------------------------------------------------------------
    const int half = lane >> 5, e = lane & 31;
    int* const stA = s_stage + (w * 4 + 2 * half) * 32; // my half's two sub-tiles: [0..32) and [32..64)
    const int* const st_row = s_stage + (w * 4 + s) * 32;
    const float qxc = (float)(px - (q & 1)) + 0.5f, qyc = (float)(py - (q >> 1)) + 0.5f; // centre of my 2x2 quad
#pragma unroll 1
    for (int base = 0; base < total; base += 32) {
        if (!__any(k.active)) break;
        // stage: lane = entry e of the batch x the sub-tile pair of my half
        const int ep = base + e;
        bool keepA = false, keepB = false;
        if (ep < total) {
            // (the sixteen sub-tile verdicts of this entry were computed by the entry gather, stp_tilesort.hip: subtile_keep_mask_kbuffer)
            const uint32_t mask = __float_as_uint(*reinterpret_cast<const float*>(reinterpret_cast<const char*>(eF) + ((uint32_t)ep << 4) + 12));
            const uint32_t mine = mask >> (4 * w + 2 * half);
            keepA = (mine & 1u) != 0u;
            keepB = (mine & 2u) != 0u;
        }
        const unsigned long long balA = __ballot(keepA), balB = __ballot(keepB);
        const unsigned int mA = (unsigned int)(balA >> (32 * half)), mB = (unsigned int)(balB >> (32 * half));
        const unsigned int below = (1u << e) - 1u;
        wave_sync(); // (the previous batch's readers are done)
        if (keepA) stA[__popc(mA & below)] = ep;
        if (keepB) stA[32 + __popc(mB & below)] = ep;
        wave_sync();
        const int n_s = __popc((unsigned int)(((s & 1) ? balB : balA) >> (32 * (s >> 1)))); // my sub-tile's survivors
        // feed: groups of four survivors per quad, head steps after every 16
        int n_max = n_s;
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) n_max = max(n_max, __shfl_xor(n_max, o));
#pragma unroll 1
        for (int g0 = 0; g0 < n_max; g0 += 16) {
#pragma unroll 1
            for (int g = g0; g < min(g0 + 16, n_max); g += 4) {
                const int i = g + q;
                int fid = -1;
                if (i < n_s) fid = st_row[i];
                bool keep = false;
                const bool qlive = quad_live(__ballot(k.active), lane); // (a ballot: every lane takes part, with or without an entry)
                if (fid >= 0 && qlive) keep = quad_can_blend(ent_row(eC, fid), ent_row(eD, fid), qxc, qyc);
                hf.push(hfifo, q, keep, fid);
            }
            head_rounds(false);
        }
    }
    head_rounds(true);
    win.drain(k);

    if constexpr (RECORD) k.logc.flush();
    if (wp.inside) write_forward_pixel<DEPTHVIZ, true>(a, px, py, k.fp, k.depth_acc, RECORD ? (uint32_t)k.logc.records() : (uint32_t)k.contrib); // (recording forward: the pixel's number of log records)
    if constexpr (INVD) { if (wp.inside) a.out_invdepth[(size_t)a.W * py + px] = fmaf(k.pend_w, k.pend_z, k.D); } // (+ the last blended entry)
    if constexpr (RECORD) finish_blend_log(a, wp.tile, k.logc.records(), total);
}

template <int WIN, int MODE, bool FRCP>
__global__ void __launch_bounds__(256, (KbRegWindow<WIN, MODE, FRCP>::WAVES)) render_kbuffer_wave_kernel(const RenderArgs a)
{
    __shared__ int s_stage[16 * 32];
    __shared__ int s_fifo[64 * KbRegWindow<WIN, MODE, FRCP>::FIFO_CAP];
    KbRegWindow<WIN, MODE, FRCP> win;
    render_kbuffer_body<MODE>(a, win, s_stage, s_fifo);
}

template <int WIN, int MODE, bool FRCP>
__global__ void __launch_bounds__(256, (KbRingWindow<WIN, MODE, FRCP>::WAVES)) render_kbuffer_ring_kernel(const RenderArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    KbRingWindow<WIN, MODE, FRCP> win;
    win.ring = smem;
    int* const s_stage = reinterpret_cast<int*>(smem + win.RING_BYTES);
    render_kbuffer_body<MODE>(a, win, s_stage, s_stage + 16 * 32);
}

template <int WIN, int MODE> hipError_t launch_kb_ring(const FrameParams& f, const RenderArgs& a, hipStream_t st)
{
    const dim3 grid(f.gx * (f.ty1 - f.ty0)), block(256);
    constexpr size_t lds = KbRingWindow<WIN, MODE, true>::LDS_BYTES;
    if (f.wild_cov) hipLaunchKernelGGL((render_kbuffer_ring_kernel<WIN, MODE, false>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((render_kbuffer_ring_kernel<WIN, MODE, true>), grid, block, lds, st, a);
    return hipGetLastError();
}

template <int WIN, int MODE> hipError_t launch_kb_win(const FrameParams& f, const RenderArgs& a, hipStream_t st)
{
    const dim3 grid(f.gx * (f.ty1 - f.ty0)), block(256);
    if (f.wild_cov) hipLaunchKernelGGL((render_kbuffer_wave_kernel<WIN, MODE, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((render_kbuffer_wave_kernel<WIN, MODE, true>), grid, block, 0, st, a);
    return hipGetLastError();
}


// One forward pass over the window ladder.  Every window size of the reference's ladder (forward.cu:409-425: the next supported window) has a
// kernel here: four waves per SIMD up to 4 entries, three up to 16, two for 20 and 24 (164-187 VGPRs, no scratch).  Windows of 8 entries and
// more: the ring-in-LDS kernel (STP_KBUFFER=wave keeps the register window for them too).
template <int MODE> hipError_t launch_kb_pass(const FrameParams& f, const RenderArgs& a, hipStream_t st)
{
    const int w = f.s.queue_per_pixel;
    const bool ring = switches().kbuffer != Switches::KBUFFER_WAVE;
#define STP_KBW(WIN) if (w <= WIN) return launch_kb_win<WIN, MODE>(f, a, st)
#define STP_KBR(WIN) if (w <= WIN) return ring ? launch_kb_ring<WIN, MODE>(f, a, st) : launch_kb_win<WIN, MODE>(f, a, st)
    STP_KBW(1); STP_KBW(2); STP_KBW(4);
    STP_KBR(8); STP_KBR(12); STP_KBR(16); STP_KBR(20);
    return ring ? launch_kb_ring<24, MODE>(f, a, st) : launch_kb_win<24, MODE>(f, a, st);
#undef STP_KBW
#undef STP_KBR
}

} // namespace

// pass: a forward pass of stp_render_pass.h
hipError_t launch_kbuffer_wave(int pass, const FrameParams& f, const RenderArgs& a, hipStream_t st)
{
    switch (pass) {
    case PASS_FWD: return launch_kb_pass<PASS_FWD>(f, a, st);
    case PASS_FWD_RECORD: return launch_kb_pass<PASS_FWD_RECORD>(f, a, st);
    case PASS_FWD_DEPTH: return launch_kb_pass<PASS_FWD_DEPTH>(f, a, st);
    case PASS_FWD_INVD: return launch_kb_pass<PASS_FWD_INVD>(f, a, st);
    case PASS_FWD_RECORD_INVD: return launch_kb_pass<PASS_FWD_RECORD_INVD>(f, a, st);
    default: return hipErrorInvalidValue;
    }
}

} // namespace stp
