// stp_render_hier.hip -- dispatch of the hierarchical kernel over the queue-size ladder
// (reference forward.cu:445-494, backward.cu:739-767); the kernels themselves are instantiated in
// slices by stp_render_hier_inst.hip.
#include "stp_internal.h"
#include "stp_blend.h"

namespace stp {

// the slices' entry points, one per (pass, MID) of stp_render_pass.h's list
using HierSliceFn = hipError_t(const FrameParams& f, const RenderArgs& a, hipStream_t st, bool* handled);
#define STP_SLICE(PASS, MID) HierSliceFn STP_HIER_SLICE_FN(PASS, MID);
STP_HIER_SLICES(STP_SLICE)
#undef STP_SLICE
static constexpr struct { int pass, mid; HierSliceFn* fn; } HIER_SLICES[] = {
#define STP_SLICE(PASS, MID) {PASS, MID, STP_HIER_SLICE_FN(PASS, MID)},
    STP_HIER_SLICES(STP_SLICE)
#undef STP_SLICE
};

// pass: a render pass of stp_render_pass.h
hipError_t launch_hier(int pass, const FrameParams& f, const RenderArgs& a, hipStream_t st, std::string* err)
{
    const bool backward = pass_backward(pass);
    const int head = f.s.queue_per_pixel, mid = f.s.queue_tile_2x2;
    bool handled = false, mid_ok = false;
    for (const auto& s : HIER_SLICES) {
        if (s.mid != mid) continue;
        mid_ok = true;
        if (s.pass != pass) continue;
        const hipError_t e = s.fn(f, a, st, &handled);
        if (handled) return e;
    }
    if (err) {
        if (!mid_ok) *err = "Not supported mid queue size" + (backward ? " " + std::to_string(mid) : std::string());
        else *err = "Not supported head queue size" + (backward ? " " + std::to_string(head) : std::string());
    }
    return hipErrorInvalidValue;
}

} // namespace stp
