// stp_switches.h -- the environment switches that select code paths, parsed in ONE place to what the code branches on.
// All are read ONCE, at the first library call that needs any of them: changing the environment afterwards has no effect.  What each path is and
// what was measured stands beside the code that branches.  (STP_RUN_AHEAD is not here: it initialises a run-time setting, stp_forward.hip.)
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace stp {

struct Switches {
    bool tile_local_sort;     // STP_SORT is not "radix": tile-bit radix sort + per-tile (depth, id) sort
    bool atomic_bin;          // STP_SORT=counters: binning by tile counters, no device-wide sort
    bool fused_gather;        // STP_FUSED_GATHER does not start with 0: short tile lists are sorted + gathered inside the hierarchical forward
    bool two_level_scan;      // STP_SCAN is not "rocprim": the scan folded into preprocess_kernel / duplicate_kernel
    bool colour_late;         // STP_COLOUR_LATE does not start with 0: the SH -> RGB kernel starts behind duplicate_kernel
    bool speculative_binning; // STP_BINNING is not "exact": the binning buffer is requested on the size guess
    bool mailbox_spin;        // STP_MAILBOX is not "event": the host watches the mailbox word itself
    bool side_stream;         // STP_SIDE_STREAM is not "0": a second stream per device
    int fixed_log_depth;      // STP_LOG_DEPTH=n (atoi; <= 0: the depth is chosen per frame)
    size_t carve_skew;        // STP_CARVE_SKEW=n (strtoull, any base), rounded down to a multiple of 256 (stp_internal.h: ALIGN)
    bool tile_order;          // STP_TILE_ORDER does not start with 0: longest-list-first order of the render workgroups
    int gather_order;         // STP_GATHER_ORDER=n (atoi): 0 / 1 / 2, stp_preprocess.hip
    enum TileSort { TILE_SORT_AUTO, TILE_SORT_ROCPRIM, TILE_SORT_OWN } tile_sort; // STP_TILE_SORT=rocprim / own
    enum KBuffer { KBUFFER_RING, KBUFFER_TILE, KBUFFER_WAVE } kbuffer;            // STP_KBUFFER=tile / wave
};

inline const Switches& switches()
{
    static const Switches table = [] {
        const auto is = [](const char* name, const char* value) { const char* e = std::getenv(name); return e && std::strcmp(e, value) == 0; };
        const auto starts_with_0 = [](const char* name) { const char* e = std::getenv(name); return e && e[0] == '0'; };
        const auto number = [](const char* name) { const char* e = std::getenv(name); return e ? std::atoi(e) : 0; };
        Switches s{};
        s.tile_local_sort = !is("STP_SORT", "radix");
        s.atomic_bin = is("STP_SORT", "counters");
        s.fused_gather = !starts_with_0("STP_FUSED_GATHER");
        s.two_level_scan = !is("STP_SCAN", "rocprim");
        s.colour_late = !starts_with_0("STP_COLOUR_LATE");
        s.speculative_binning = !is("STP_BINNING", "exact");
        s.mailbox_spin = !is("STP_MAILBOX", "event");
        s.side_stream = !is("STP_SIDE_STREAM", "0");
        s.fixed_log_depth = number("STP_LOG_DEPTH");
        const char* skew = std::getenv("STP_CARVE_SKEW");
        s.carve_skew = skew ? ((size_t)std::strtoull(skew, nullptr, 0) & ~(size_t)255) : (size_t)0;
        s.tile_order = !starts_with_0("STP_TILE_ORDER");
        s.gather_order = number("STP_GATHER_ORDER");
        s.tile_sort = is("STP_TILE_SORT", "rocprim") ? Switches::TILE_SORT_ROCPRIM : is("STP_TILE_SORT", "own") ? Switches::TILE_SORT_OWN : Switches::TILE_SORT_AUTO;
        s.kbuffer = is("STP_KBUFFER", "tile") ? Switches::KBUFFER_TILE : is("STP_KBUFFER", "wave") ? Switches::KBUFFER_WAVE : Switches::KBUFFER_RING;
        return s;
    }();
    return table;
}

} // namespace stp
