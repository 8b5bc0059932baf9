// stp_forward.hip -- stp_forward of the C ABI (include/stp_raster.h): the host orchestration of one frame.  Replaces
// CudaRasterizer::Rasterizer::forward (reference cuda_rasterizer/rasterizer_impl.cu:221-413).
// Stage order of a forward is the reference's: preprocess -> inclusive scan -> (one host read-back of num_rendered) -> duplicate -> sort ->
// tile ranges -> render, where "sort" is by default a radix sort on the tile bits followed by the per-tile (depth, id) sort fused with the entry
// gather (stp_tilesort.hip; STP_SORT selects the alternatives, see stp_forward).  Everything is enqueued on the caller's stream; the only host
// synchronisation is the read-back.  The call is re-entrant: the scratch buffers belong to the caller, and the per-device helpers (mailbox ring,
// side stream, binning-size guesses) are created once behind acquire/release flags.  The environment switches are read ONCE (stp_switches.h).
#include "stp_internal.h"

#include <atomic>
#include <cstring>
#include <mutex>
#include <string>

using namespace stp;

// ---- num_rendered mailbox: host-mapped pinned words + an event, a small ring per device (concurrent forwards on one
// ---- device -- several streams or threads -- each get their own slot)
namespace {
// (`done`: recorded on the side stream behind this forward's SH -> RGB kernel -- one per slot, so that concurrent forwards
// on one device do not re-record each other's event)
struct Mailbox { volatile uint32_t* host = nullptr; uint32_t* dev = nullptr; hipEvent_t ev = nullptr; hipEvent_t done = nullptr; int device = 0; uint32_t ticket = 0; };
constexpr int MAILBOX_RING = 8;
struct MailboxRing { Mailbox slot[MAILBOX_RING]; std::atomic<unsigned> next{0}; std::atomic<bool> ready{false};
                     uint32_t* log_need = nullptr; /* device words, one per guess slot: report_log_need (stp_blend.h) */ };
MailboxRing g_mailboxes[MAX_DEVICES];
std::mutex g_mailbox_mutex;
// Binning-size guesses: tile-list entries of the previous forward OF THE SAME KIND on each device.  "Kind" = (P, width,
// height, tile-row window, sort mode): a small frame that follows a 4K frame (an eval render between training steps, a
// second rasterizer module) does not inherit the big frame's count.  Direct-mapped, 16 kinds per device; a collision only
// costs the second allocator call.
constexpr int GUESS_SLOTS = 16;
struct SizeGuess { std::atomic<uint64_t> key{0}; std::atomic<uint32_t> R{0}; std::atomic<uint32_t> log_need{0}; }; // log_need: blends per pixel the kind's recording forwards needed
SizeGuess g_guess[MAX_DEVICES][GUESS_SLOTS];
uint64_t guess_key(const FrameParams& f)
{
    uint64_t k = 0x9E3779B97F4A7C15ull;
    for (uint64_t v : {(uint64_t)f.P, (uint64_t)f.W, (uint64_t)f.H, (uint64_t)f.ty0, (uint64_t)f.ty1, (uint64_t)f.s.sort_mode,
                       (uint64_t)(f.s.tile_based_culling * 8 + f.s.rect_bounding * 4 + f.s.tight_opacity_bounding * 2 + (f.s.sort_order == ORDER_PTD_MAX))})
        k = (k ^ v) * 0xBF58476D1CE4E5B9ull, k ^= k >> 29;
    return k | 1ull;
}

// A second stream per device for the SH -> RGB kernel: nothing before the entry gather needs the colours, so the kernel (a
// pure HBM stream, 70 us at C2) runs BESIDE the host hand-over, duplicate and the tile-bit sort (atomics, small launches and
// 1.6 TB/s radix passes) instead of in front of them.  It starts behind the mailbox event and is joined back into the
// caller's stream before the first reader of the colours -- and on every early return, so the caller's buffers are never
// touched by work the caller's stream does not know about.  STP_SIDE_STREAM=0: everything on the caller's stream.
struct SideStream { hipStream_t stream = nullptr; std::atomic<bool> ready{false}; };
SideStream g_side[MAX_DEVICES];
SideStream* side_stream(int device)
{
    if (!switches().side_stream || device < 0 || device >= MAX_DEVICES) return nullptr;
    SideStream& s = g_side[device];
    if (!s.ready.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lock(g_mailbox_mutex);
        if (!s.ready.load(std::memory_order_relaxed)) {
            if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            s.ready.store(true, std::memory_order_release);
        }
    }
    return &s;
}
struct SideJoin { // joins the side stream's work into `st` when it goes out of scope, unless done earlier
    hipEvent_t done; hipStream_t st; bool pending;
    hipError_t join() { if (!pending) return hipSuccess; pending = false; return hipStreamWaitEvent(st, done, 0); }
    ~SideJoin() { (void)join(); }
};

inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::atomic_signal_fence(std::memory_order_seq_cst);
#endif
}

// run-ahead forward: 0 = never, 1 = whenever a size guess exists, 2 (default) = for SMALL frames only (guess below RUN_AHEAD_AUTO_MAX entries)
constexpr uint32_t RUN_AHEAD_AUTO_MAX = 1u << 18;
std::atomic<int> g_run_ahead{[] { const char* e = std::getenv("STP_RUN_AHEAD"); return (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : 2; }()};

// Depth of this frame's blend log: the largest blend count per pixel that the recording forwards of this kind reported (slowly forgotten:
// read_mailbox), + 12.5 % + 4, rounded up to 16 records; a frame nothing is known about gets the default.  STP_LOG_DEPTH=n fixes it.
int log_depth_for(const SizeGuess& slot, uint64_t key)
{
    const int fixed = switches().fixed_log_depth;
    if (fixed > 0) return blend_log_clamp_depth((fixed + 1) & ~1);
    const uint32_t need = slot.key.load(std::memory_order_acquire) == key ? slot.log_need.load(std::memory_order_relaxed) : 0u;
    if (need == 0) return blend_log_default_depth();
    return blend_log_clamp_depth((int)((need + need / 8 + 4 + 15) & ~15u));
}

int acquire_mailbox(Mailbox* out)
{
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= MAX_DEVICES) return fail(STP_ERR_HIP, "hipGetDevice failed");
    MailboxRing& ring = g_mailboxes[device];
    if (!ring.ready.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lock(g_mailbox_mutex);
        if (!ring.ready.load(std::memory_order_relaxed)) {
            for (int i = 0; i < MAILBOX_RING; i++) {
                void* h = nullptr; void* d = nullptr;
                if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess ||
                    hipEventCreateWithFlags(&ring.slot[i].ev, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&ring.slot[i].done, hipEventDisableTiming) != hipSuccess)
                    return fail(STP_ERR_HIP, "cannot create the num_rendered mailbox");
                std::memset(h, 0, 64); // (a recycled pinned page may hold an old ticket: the first tickets are the small integers 1..8)
                ring.slot[i].host = static_cast<volatile uint32_t*>(h);
                ring.slot[i].dev = static_cast<uint32_t*>(d);
                ring.slot[i].device = device;
            }
            if (hipMalloc(reinterpret_cast<void**>(&ring.log_need), sizeof(uint32_t) * 64) != hipSuccess || hipMemset(ring.log_need, 0, sizeof(uint32_t) * 64) != hipSuccess)
                return fail(STP_ERR_HIP, "cannot create the blend-log depth words");
            ring.ready.store(true, std::memory_order_release);
        }
    }
    const unsigned seq = ring.next.fetch_add(1u);
    *out = ring.slot[seq % MAILBOX_RING];
    out->ticket = seq + 1u == 0u ? 1u : seq + 1u; // what the kernel writes LAST into the slot's third word: unique per use of the slot
    return 0;
}

// One stp_forward call: what its stages share, and the stages behind the argument checks as member functions, in the order stp_forward runs them.
struct ForwardCall {
    const hipStream_t st; const int debug; // (under the names STP_DEBUG_SYNC uses)
    FrameParams f;
    GeometryState g{}; ImageState img{}; char* img_ptr = nullptr; char* geom_base = nullptr; float* sh_stash = nullptr; // (sh_stash: stp_set_forward_sh_stash, else nullptr)
    Mailbox mb;
    SizeGuess* gslot = nullptr; uint64_t gkey = 0; // the guess slot of this kind of frame
    uint32_t* log_need_word = nullptr; uint32_t log_tag = 0; int log_depth = 0; bool with_log = false;
    SideStream* side = nullptr;
    bool colour_started = true; // (false: the SH -> RGB kernel starts behind duplicate_kernel, see launch_up_to_mailbox)
    char* bin_ptr = nullptr; size_t bin_have = 0; // the binning buffer requested on the size guess (request_binning) ...
    uint32_t cap = 0; bool ahead = false, run_ahead = false; // ... its entries, and is the whole forward launched on it
    int* radii; float* const out_color;
    // Whatever happens to the call, on EVERY return path: the side stream's work is joined into the caller's stream (`colours`), and only THEN is the
    // caller's split event (stp_set_forward_split) recorded, behind everything this call enqueued.  `split` is declared BEFORE `colours`, so it is
    // destroyed AFTER it; stp_forward makes the ForwardCall in front of its first check.
    struct Split { const ForwardSplit s; hipStream_t st; bool recorded; ~Split() { if (s.armed && !recorded) (void)hipEventRecord(s.event, st); } } split;
    SideJoin colours; // the SH -> RGB kernel on the side stream

    ForwardCall(hipStream_t stream, int debug_, const ForwardSplit& split_, int* radii_, float* out_color_)
        : st(stream), debug(debug_), radii(radii_), out_color(out_color_), split{split_, stream, false}, colours{nullptr, stream, false} {}
    int carve_geometry_and_image(stp_alloc_fn geometry_alloc, void* geometry_user, stp_alloc_fn image_alloc, void* image_user, bool with_inv, bool with_stash);
    int launch_up_to_mailbox(); int colour_on_side();
    int request_binning(stp_alloc_fn binning_alloc, void* binning_user);
    int wait_mailbox(); int read_mailbox(int* R_out, bool* wild_out);
    int binning_and_render(const GeometryState& gd, const BinningState& b, int L, uint32_t dup_cap);
};

int ForwardCall::carve_geometry_and_image(stp_alloc_fn geometry_alloc, void* geometry_user, stp_alloc_fn image_alloc, void* image_user, bool with_inv, bool with_stash)
{
    size_t geom_bytes = 0;
    carve_geometry(nullptr, (size_t)f.P, with_inv, &geom_bytes, nullptr, nullptr, with_stash ? &sh_stash : nullptr);
    char* geom_ptr = (char*)geometry_alloc(geometry_user, geom_bytes);
    if (!geom_ptr) return fail(STP_ERR_ALLOC, "geometry allocator returned NULL");
    g = carve_geometry(geom_ptr, (size_t)f.P, with_inv, nullptr, nullptr, nullptr, with_stash ? &sh_stash : nullptr);
    geom_base = geom_ptr;
    if (!radii) radii = g.internal_radii;

    // (the mailbox is taken here already: the device's guess slots size the blend log)
    if (int rc = acquire_mailbox(&mb)) return rc;
    colours.done = mb.done;
    gkey = guess_key(f);
    const unsigned gidx = (unsigned)((gkey >> 1) % GUESS_SLOTS);
    gslot = &g_guess[mb.device][gidx];
    log_need_word = g_mailboxes[mb.device].log_need + gidx;
    size_t img_bytes = 0;
    with_log = uses_blend_log(f.s);
    log_depth = with_log ? log_depth_for(*gslot, gkey) : 0;
    f.log_depth = log_depth;
    f.log_need = with_log ? log_need_word : nullptr;
    log_tag = (uint32_t)((gkey >> 40) & 0xFFFFu) | 1u; // (never 0: an empty word carries no tag)
    f.log_tag = log_tag;
    carve_image(nullptr, f.W, f.H, f.ty0, f.ty1, log_depth, &img_bytes); // (the tile-row window's share: see carve_image)
    img_ptr = (char*)image_alloc(image_user, img_bytes);
    if (!img_ptr) return fail(STP_ERR_ALLOC, "image allocator returned NULL");
    img = carve_image(img_ptr, f.W, f.H, f.ty0, f.ty1, log_depth, nullptr);
    // (the buffer's own header is written by frame_init_kernel; the host-side cache entry follows when num_rendered is known)
    return 0;
}

// frame init -> preprocess -> scan -> the mailbox kernel, and where the colour kernel goes
int ForwardCall::launch_up_to_mailbox()
{
    const bool atomic_bin = switches().atomic_bin, two_level_scan = switches().two_level_scan;
    timer_begin_forward();
    timer_mark(0, st);
    STP_TRY(launch_frame_init(g, img, f.gx * f.ty0, f.gx * (f.ty1 - f.ty0), with_log, atomic_bin, st), "frame init launch");
    STP_TRY(launch_preprocess(f, g, radii, atomic_bin ? img.tile_counts : nullptr, st), "preprocess launch");
    STP_DEBUG_SYNC("preprocess");
    if (!two_level_scan) STP_TRY(launch_scan(f, g, st), "inclusive scan");
    STP_DEBUG_SYNC("scan");
    if (atomic_bin) STP_TRY(launch_tile_scan(f, img, st), "tile scan"); // counters -> ranges + cursors (no host value needed)

    // The one mandatory host hand-over: num_rendered sizes the binning buffers (reference :317, a blocking 4-byte copy into
    // pageable memory).  Here a one-thread kernel drops the two words into host-mapped pinned memory and an event marks
    // the spot; the SH -> RGB kernel -- which nothing before the render stage depends on -- is enqueued BEHIND it, so
    // the GPU keeps working while the host wakes up, sizes the buffer and launches duplicate / sort.
    if (two_level_scan) STP_TRY(launch_block_prefix_mailbox(f, g, mb.dev, mb.ticket, log_need_word, st), "workgroup prefixes + mailbox launch");
    else STP_TRY(launch_mailbox(g.point_offsets + (f.P - 1), g.status + 1, mb.dev, mb.ticket, log_need_word, st), "mailbox launch");
    STP_TRY(hipEventRecord(mb.ev, st), "record mailbox event");
    side = side_stream(mb.device);
    // Where the colour kernel starts on the side stream.  Rounds 2-3: behind the mailbox, i.e. in the host's hand-over bubble and then beside
    // duplicate_kernel -- two bandwidth-bound kernels that slow each other down (duplicate 61 us alone, 98 us beside it).  Since the host watches the
    // mailbox word the bubble is a few microseconds, and the kernel now starts behind duplicate_kernel, beside the tile-bit sort, whose radix
    // passes run at 1.6 TB/s and leave it room (late round 3, one box, alternating: duplicate 0.098 -> 0.058 ms, sort stage 0.289 -> 0.337, the
    // step -6 .. -10 us at C2-full, -40 .. -70 us at C5, C3 / C4 / C2-min unchanged).  STP_COLOUR_LATE=0 restores the earlier start.
    colour_started = !(side && switches().colour_late);
    if (side) {
        if (colour_started) { if (int rc = colour_on_side()) return rc; }
    } else STP_TRY(launch_sh_color(f, g, radii, sh_stash, st), "SH colour launch");
    return 0;
}

int ForwardCall::colour_on_side()
{
    STP_TRY(hipStreamWaitEvent(side->stream, mb.ev, 0), "side stream wait");
    STP_TRY(launch_sh_color(f, g, radii, sh_stash, side->stream), "SH colour launch");
    // from here on the side stream works on the caller's buffers: every return path joins it (SideJoin); should the
    // event that the join waits for fail to record, the side stream is drained on the spot instead
    if (hipError_t e = hipEventRecord(mb.done, side->stream); e != hipSuccess) {
        (void)hipStreamSynchronize(side->stream);
        return fail_hip(e, "record colour event");
    }
    colours.pending = true;
    return 0;
}

// The binning buffer is requested BEFORE num_rendered is known, sized by the counts of the previous frames of the same kind on this
// device (+12.5 %): in the steady state of training or serving no allocator callback runs between the kernels.  The exact-size
// request of the reference follows only when the guess was too small (STP_BINNING=exact: always) -- so binning_alloc may be called
// TWICE per forward, the second time with the larger size (include/stp_raster.h).
// RUN-AHEAD (round 4; by default for small frames only: STP_RUN_AHEAD=0 / 1 in the environment or stp_set_run_ahead(0 / 1 / 2) say never / always / auto).  The reference -- and the
// default path here -- stop the host after the scan until num_rendered has come back, and only then enqueue duplicate / sort / render:
// a stall of the launching thread there is GPU idle time.  With a size guess the whole forward is enqueued at once ON THE GUESSED
// CAPACITY: the sub-arrays are carved for `cap` entries, duplicate_kernel guards its writes and pads [num_rendered, cap) with entries
// that sort behind every tile, the sort / range passes run over `cap`, the render kernels are the ones for a tame Sigma^-1 -- and the
// host reads the mailbox AFTER the last launch, when the word has long arrived.  Only a frame that does not fit (or whose status word
// asks for the checked reciprocal) is redone from duplicate_kernel on with the exact size, before the call returns: results never
// depend on the guess (tests/test_gpu_parity.py::test_run_ahead_overflow_is_redone; every GpuRun of the tests renders its frame both ways).
// MEASURED (one box, alternating, profiles/r04_run_ahead_ab.txt): the padding costs the device-wide passes what it weighs -- C2-full sort
// stage 0.325 -> 0.343 ms, step 2.410 -> 2.422 ms; C5 +0.04 ms; C4 +0.03 ms -- and nothing comes back: the hand-over bubble was already
// hidden (mailbox word + colour kernel behind it), `ms_per_step - sum(stages)` stays at 0.04 ms, and C1 is bound by the ~25 launches of a
// step, not by the round trip.  Hence off for large frames by default; what it does buy there is a frame whose GPU time no longer depends on
// the launching thread being scheduled in the middle of it.
// Small frames are the exception (mode 2, the default: guesses below 2^18 entries): there the padding weighs nothing and the round trip is
// a tenth of the frame -- C1 0.179 -> 0.167 ms per step (profiles/r04_host_profile_c1.txt).
int ForwardCall::request_binning(stp_alloc_fn binning_alloc, void* binning_user)
{
    const Switches& sw = switches();
    const int run_ahead_mode = g_run_ahead.load(std::memory_order_relaxed);
    run_ahead = run_ahead_mode != 0;
    const uint32_t guess = (sw.speculative_binning && gslot->key.load(std::memory_order_acquire) == gkey) ? gslot->R.load(std::memory_order_relaxed) : 0u;
    ahead = run_ahead && guess > 0 && (run_ahead_mode == 1 || guess < RUN_AHEAD_AUTO_MAX) && sw.two_level_scan && !sw.atomic_bin && !debug;
    cap = guess + guess / 8 + (ahead ? 1024u : 0u);
    if (guess > 0) {
        carve_binning(nullptr, (size_t)cap, &bin_have);
        bin_ptr = (char*)binning_alloc(binning_user, bin_have);
        if (!bin_ptr) return fail(STP_ERR_ALLOC, "binning allocator returned NULL");
    }
    return 0;
}

// The host watches the slot itself: the kernel's last store (the ticket) is visible a microsecond after it was made, the event behind the
// kernel is signalled by a barrier packet some microseconds later, and hipEventSynchronize's wake-up adds its own.  The event is still
// polled now and then: it completes if the kernel has, and it is how a device fault surfaces (STP_MAILBOX=event: wait on the event only).
int ForwardCall::wait_mailbox()
{
    const bool mbx_spin = switches().mailbox_spin;
    if (mbx_spin) {
        for (unsigned it = 1;; it++) {
            if (mb.host[2] == mb.ticket) break;
            if ((it & 255u) == 0u) {
                const hipError_t q = hipEventQuery(mb.ev);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) return fail_hip(q, "query (num_rendered)");
                if (it > (1u << 22)) { STP_TRY(hipEventSynchronize(mb.ev), "synchronize (num_rendered)"); break; } // (seconds of spinning: stop burning a core)
            }
            cpu_relax();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    } else STP_TRY(hipEventSynchronize(mb.ev), "synchronize (num_rendered)");
    return 0;
}

int ForwardCall::read_mailbox(int* R_out, bool* wild_out)
{
    if (int rc = wait_mailbox()) return rc;
    const uint32_t host_status[2] = {mb.host[0], mb.host[1]};
    const uint32_t word = mb.host[3]; // (tag << 16 | blends per pixel): the report of the last recording forward(s) that used this slot's word
    if (const uint32_t reported = (word >> 16) == log_tag ? (word & 0xFFFFu) : 0u) { // of THIS kind: never less than 31/32 of what was known
        const uint32_t known = gslot->key.load(std::memory_order_acquire) == gkey ? gslot->log_need.load(std::memory_order_relaxed) : 0u;
        const uint32_t keep = known - known / 32;
        gslot->log_need.store(reported > keep ? reported : keep, std::memory_order_relaxed);
    } else if (gslot->key.load(std::memory_order_acquire) != gkey) gslot->log_need.store(0u, std::memory_order_relaxed); // (the slot changes hands)
    if (host_status[1] & 1u) return fail(STP_ERR_PREFILTERED, "Point is filtered although prefiltered is set. This shouldn't happen!");
    *wild_out = (host_status[1] & 2u) != 0;
    *R_out = (int)host_status[0];
    // next frame's guess: this frame's count, but never less than 31/32 of the last guess -- with a moving camera the count jumps from
    // frame to frame, and a guess that follows every dip overflows at the next peak (a redone frame costs far more than padding)
    const uint32_t prev = gslot->key.load(std::memory_order_acquire) == gkey ? gslot->R.load(std::memory_order_relaxed) : 0u;
    const uint32_t keep = run_ahead ? prev - prev / 32 : 0u;
    gslot->R.store((uint32_t)*R_out > keep ? (uint32_t)*R_out : keep, std::memory_order_relaxed);
    gslot->key.store(gkey, std::memory_order_release);
    return 0;
}

// everything behind the hand-over: duplicate -> (colour kernel on the side stream) -> sort -> ranges -> per-tile sort + gather -> render.
// L = entries the device-wide passes run over: num_rendered, or the capacity of a run-ahead launch (dup_cap = the same value then)
int ForwardCall::binning_and_render(const GeometryState& gd, const BinningState& b, int L, uint32_t dup_cap)
{
    const bool atomic_bin = switches().atomic_bin, tile_local_sort = switches().tile_local_sort;
    uint32_t* zero_ptr = nullptr; size_t zero_words = 0; // (the tile-bit sort's histograms / look-back states / block counters: cleared here, once)
    if (!atomic_bin && tile_local_sort) sort_zero_region(b, (size_t)L, (uint32_t)(f.gx * f.gy), &zero_ptr, &zero_words);
    STP_TRY(launch_duplicate(f, gd, radii, b, atomic_bin ? img.tile_cursor : nullptr, dup_cap, (uint32_t)L, zero_ptr, zero_words, st), "duplicate launch");
    STP_DEBUG_SYNC("duplicate");
    timer_mark(2, st);
    if (!colour_started) {
        STP_TRY(hipEventRecord(mb.ev, st), "record event behind duplicate");
        if (int rc = colour_on_side()) return rc;
        colour_started = true;
    }
    if (atomic_bin) {
        STP_TRY(launch_bin_pad(b, img, L, st), "pad entries");
    } else {
        STP_TRY(launch_sort(f, b, L, tile_local_sort, zero_words != 0, st), "radix sort");
        STP_DEBUG_SYNC("sort");
        STP_TRY(launch_ranges(f, b, img, L, st), "tile ranges");
        STP_DEBUG_SYNC("ranges");
    }
    // The tile order (one workgroup: 7 us at 1080p, 31 us at 4K) needs the ranges and is needed by the render kernel only: on the side stream it
    // runs beside the entry gather.  The mailbox's two events serve a second time: `ev` marks "ranges done" for the side stream, `done` -- re-recorded
    // behind the order kernel AFTER the caller's stream has been told to wait for its first recording, the colour kernel's -- is joined in front of
    // the render launch.  MEASURED (one box, alternating, sort stage ms): 4K 0.489 -> 0.473; 1080p 0.324 -> 0.329 (C2L, C5 likewise: the two event
    // operations and the company of the gather cost more than seven microseconds hidden) -- so only frames of 16 384 tiles and more take the side stream.
    const bool order_wanted = !atomic_bin && tile_order_used(f);
#ifdef STP_ORDER_MAIN   // (A/B builds: the order kernel on the caller's stream, in front of the gather)
    const bool order_on_side = false;
#else
    const bool order_on_side = order_wanted && side != nullptr && gather_order_mode() == 0 && f.gx * (f.ty1 - f.ty0) >= 16384;
#endif
    if (order_on_side) {
        STP_TRY(hipEventRecord(mb.ev, st), "record event behind the ranges");
        STP_TRY(hipStreamWaitEvent(side->stream, mb.ev, 0), "side stream wait (ranges)");
        STP_TRY(launch_tile_order(f, img, side->stream), "tile order");
    } else if (order_wanted) STP_TRY(launch_tile_order(f, img, st), "tile order");
    STP_TRY(colours.join(), "join colour stream"); // (the entry gather -- or, in GLOBAL mode, the render kernel -- reads the colours)
    SideJoin ordering{mb.done, st, false};
    if (order_on_side) {
        if (hipError_t e = hipEventRecord(mb.done, side->stream); e != hipSuccess) {
            (void)hipStreamSynchronize(side->stream);
            return fail_hip(e, "record tile-order event");
        }
        ordering.pending = true;
    }
    if (tile_local_sort) STP_TRY(launch_tile_sort_gather(f, g, b, img, L, atomic_bin, st), "tile sort + entry gather");
    else STP_TRY(launch_gather_entries(f, g, b, L, st), "entry gather");
    STP_DEBUG_SYNC("entry gather");
    STP_TRY(ordering.join(), "join tile order");
    timer_mark(3, st);
    std::string err;
    hipError_t e;
    if (split.s.armed && split.s.row > f.ty0 && split.s.row < f.ty1 && f.s.debug_visualization == 0) {
        // two launches, tile rows [ty0, row) and [row, ty1), the caller's event between them: a tile-row shard sends the first half of its
        // strip while the second half renders (include/stp_raster.h: stp_set_forward_split).  Same kernels, same per-tile work, same pixels.
        FrameParams f1 = f, f2 = f;
        f1.ty1 = split.s.row; f2.ty0 = split.s.row;
        f1.split_launch = f2.split_launch = 1;
        e = launch_render_forward(f1, g, b, img, out_color, st, &err);
        if (e == hipSuccess) { e = hipEventRecord(split.s.event, st); split.recorded = e == hipSuccess; }
        if (e == hipSuccess) e = launch_render_forward(f2, g, b, img, out_color, st, &err);
    } else e = launch_render_forward(f, g, b, img, out_color, st, &err);
    if (e != hipSuccess) {
        if (!err.empty()) return fail(STP_ERR_QUEUE_SIZE, err);
        return fail_hip(e, "render launch");
    }
    STP_DEBUG_SYNC("render");
    STP_TRY(launch_render_debug_finish(f, img, out_color, st), "debug visualisation");
    timer_mark(4, st);
    return 0;
}
} // namespace

extern "C" {

void stp_set_run_ahead(int mode) { g_run_ahead.store(mode < 0 ? 0 : (mode > 2 ? 2 : mode), std::memory_order_relaxed); }
int stp_get_run_ahead(void) { return g_run_ahead.load(std::memory_order_relaxed); }
void stp_reset_size_guesses(void)
{
    for (auto& dev : g_guess)
        for (auto& slot : dev) { slot.key.store(0, std::memory_order_release); slot.R.store(0u, std::memory_order_relaxed); slot.log_need.store(0u, std::memory_order_relaxed); }
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return;
    for (int d = 0; d < MAX_DEVICES; d++) // ... and what recording forwards have reported but no forward has collected yet
        if (g_mailboxes[d].ready.load(std::memory_order_acquire) && g_mailboxes[d].log_need && hipSetDevice(d) == hipSuccess) {
            (void)hipDeviceSynchronize();
            (void)hipMemset(g_mailboxes[d].log_need, 0, sizeof(uint32_t) * 64);
        }
    (void)hipSetDevice(cur);
}

int stp_forward(stp_alloc_fn geometry_alloc, void* geometry_user, stp_alloc_fn binning_alloc, void* binning_user,
                stp_alloc_fn image_alloc, void* image_user, int P, int D, int M, const float* background, int width, int height,
                const StpSettings* settings, const float* means3D, const float* shs, const float* colors_precomp,
                const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* inv_viewprojmatrix,
                const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* radii, int debug,
                void* stream)
{
    const ForwardRequests req = take_forward_requests(); // (one forward per request, whatever becomes of this call)
    ForwardCall c((hipStream_t)stream, debug, req.split, radii, out_color); // (from here on every return records the caller's split event)
    const ForwardBackground& fbg = req.background;
    if (!settings || !geometry_alloc || !binning_alloc || !image_alloc) return fail(STP_ERR_INVALID_ARGUMENT, "null settings or allocator");
    if (P < 0 || width <= 0 || height <= 0) return fail(STP_ERR_INVALID_ARGUMENT, "bad sizes");
    if (P == 0) return 0; // reference rasterize_points.cu:93 -- nothing launched, caller's zero image stands
    if (!means3D || !opacities || !background || !viewmatrix || !projmatrix || !inv_viewprojmatrix || !cam_pos || !out_color)
        return fail(STP_ERR_INVALID_ARGUMENT, "null required input");
    if (int rc = check_settings(*settings, false)) return rc;
    if ((fbg.bg_image || fbg.out_alpha) && settings->debug_visualization == STP_DEBUG_DEPTH)
        return fail(STP_ERR_INVALID_ARGUMENT, "alpha output / per-pixel background (stp_set_forward_background) are not available with the debug depth visualisation: its image is not C + T * background");
    if (req.out_invdepth && settings->debug_visualization == STP_DEBUG_DEPTH)
        return fail(STP_ERR_INVALID_ARGUMENT, "the inverse-depth output (stp_set_forward_invdepth) is not available with the debug depth visualisation");
    if (int rc = check_raw_params(req.raw_params, opacities, scales, rotations)) return rc; // stp_set_forward_raw_params
    const float* const sh_dc = colors_precomp ? nullptr : req.sh_dc; // stp_set_forward_split_sh (precomputed colours win)
    if (sh_dc && M > 1 && !shs) return fail(STP_ERR_INVALID_ARGUMENT, "split SH (stp_set_forward_split_sh): M > 1 needs the rest of the coefficients in shs");
    if (!colors_precomp && !shs && !sh_dc) return fail(STP_ERR_INVALID_ARGUMENT, "neither SHs nor precomputed colours given");
    if (!cov3D_precomp && !(scales && rotations)) return fail(STP_ERR_INVALID_ARGUMENT, "neither scale/rotation nor precomputed covariance given");
    const bool with_inv = requires_depth_along_ray(*settings);
    if (with_inv && !(scales && rotations)) return fail(STP_ERR_NEEDS_SCALE_ROTATION, "sorted modes need scales and rotations");

    FrameParams& f = c.f;
    fill_frame(f, P, D, M, background, width, height, *settings, means3D, shs, colors_precomp, opacities, scales, scale_modifier,
               rotations, cov3D_precomp, viewmatrix, projmatrix, inv_viewprojmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered);
    f.out_invdepth = req.out_invdepth;
    f.sh_dc = sh_dc;
    f.raw_params = req.raw_params;
    f.bg_image = fbg.bg_image; f.out_alpha = fbg.out_alpha; // (every render launch of the call: both halves of a split forward, a redone run-ahead frame)
    // stp_set_forward_sh_stash: only a forward that runs the SH colour kernel has anything to stash (launch_sh_color's own test)
    const bool with_stash = req.sh_stash && !colors_precomp && (shs || sh_dc) && M > 0;
    if (int rc = c.carve_geometry_and_image(geometry_alloc, geometry_user, image_alloc, image_user, with_inv, with_stash)) return rc;

    // How the (tile, depth) order is established:
    //   default           device-wide radix sort on the tile bits only (two passes), then the tile's own workgroup sorts its
    //                     segment by (depth, Gaussian id) in LDS
    //   STP_SORT=radix    the reference's single device-wide radix sort on (tile, depth)
    //   STP_SORT=counters no device-wide sort: preprocess counts every tile's entries, duplicate writes each entry straight
    //                     into its tile's segment through an atomic cursor, then the same per-tile sort.  Measured SLOWER on
    //                     MI355X (the 2 x R device-scope atomics cost more than the two radix passes they replace: C2
    //                     preprocess + duplicate + sort 0.54 ms against 0.50 ms); kept selectable and tested.
    // (like every path switch STP_SORT is read ONCE, stp_switches.h: it selects code paths, not per-call behaviour)
    const Switches& sw = switches();
    // The tile sort + entry gather of lists up to TS_SMALL entries runs inside the hierarchical forward's workgroups, in front of rendering the
    // tile, instead of in a launch of its own: the render's other workgroups on the CU hide the gather's memory latency.
    // Not in STP_SORT=counters (segments not in id order), STP_SORT=radix, the k-buffer and GLOBAL modes or the debug depth forward.
    // STP_FUSED_GATHER=0: the separate launch.
    f.fused_gather = sw.fused_gather && sw.tile_local_sort && !sw.atomic_bin && f.s.sort_mode == MODE_HIER && f.s.debug_visualization != STP_DEBUG_DEPTH ? 1 : 0;
    // STP_SCAN=rocprim: the device-wide scan of round 1-2 (rocPRIM inclusive_scan + a one-thread mailbox kernel) instead of the two-level scan
    // folded into preprocess_kernel / duplicate_kernel
    if (!sw.two_level_scan) { c.g.block_sums = nullptr; c.g.block_prefix = nullptr; }

    if (int rc = c.launch_up_to_mailbox()) return rc;
    if (int rc = c.request_binning(binning_alloc, binning_user)) return rc;

    const hipStream_t st = c.st; // (STP_TRY / STP_DEBUG_SYNC)
    int R = 0;
    bool wild = false;
    GeometryState g_dup = c.g; // what duplicate_kernel sees (a redone frame finds the finished scan in point_offsets: no second level)
    if (c.ahead) { // the whole forward on the guessed capacity; the mailbox is read behind the last launch
        f.wild_cov = 0; // (every sane frame; the status word says otherwise afterwards)
        timer_mark(1, st);
        const BinningState b = carve_binning(c.bin_ptr, (size_t)c.cap, nullptr);
        if (int rc = c.binning_and_render(g_dup, b, (int)c.cap, c.cap)) return rc;
        if (int rc = c.read_mailbox(&R, &wild)) return rc;
        if ((uint32_t)R <= c.cap && !wild) {
            remember_stash(c.geom_base, with_stash, R);
            remember_layout(c.bin_ptr, c.cap, R);
            remember_log_depth(c.img_ptr, (uint32_t)c.log_depth, R);
            return R;
        }
        // the frame did not fit its guess (or needs the checked reciprocal): once more from duplicate_kernel on, exact this time
        g_dup.block_prefix = nullptr; g_dup.block_sums = nullptr;
        STP_TRY(launch_frame_init(c.g, c.img, f.gx * f.ty0, f.gx * (f.ty1 - f.ty0), c.with_log, sw.atomic_bin, st), "frame init launch"); // ranges and tile flags of the discarded pass
        STP_TRY(launch_stash_mark(f, c.g, c.sh_stash, st), "stash mark launch"); // (... and the status block, where a stashing colour kernel had left its mark)
    } else { // the hand-over: the host waits for num_rendered
        if (int rc = c.read_mailbox(&R, &wild)) return rc;
        STP_DEBUG_SYNC("SH colour");
        timer_mark(1, st);
    }
    f.wild_cov = wild ? 1 : 0;
    size_t bin_bytes = 0;
    carve_binning(nullptr, (size_t)R, &bin_bytes);
    if (bin_bytes > c.bin_have) {
        c.bin_ptr = (char*)binning_alloc(binning_user, bin_bytes);
        if (!c.bin_ptr) return fail(STP_ERR_ALLOC, "binning allocator returned NULL");
    }
    const BinningState b = carve_binning(c.bin_ptr, (size_t)R, nullptr);
    if (int rc = c.binning_and_render(g_dup, b, R, 0xFFFFFFFFu)) return rc;
    remember_stash(c.geom_base, with_stash, R);
    if (c.bin_ptr) remember_layout(c.bin_ptr, (uint32_t)R, R);
    remember_log_depth(c.img_ptr, (uint32_t)c.log_depth, R);
    return R;
}
} // extern "C"
