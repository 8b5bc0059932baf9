// stp_render_hier_inst.hip -- one slice of the hierarchical kernel's instantiation ladder.
// Compiled once per (pass, MID) of stp_render_pass.h's list by the Makefile, with -DSTP_INST_MODE=<pass id> -DSTP_INST_MID={8,12,20}, so the
// template instantiations (HEAD x CULL per slice) build in parallel.  Queue-size ladders follow the
// reference: forward HEAD in {4,8,16} (forward.cu:465-472), backward HEAD in {4,8,12,16}
// (backward.cu:745-752), MID in {8,12,20}.  -DSTP_FASTBUILD keeps only HEAD 4 (with MID 8), the
// counterpart of the reference's STOPTHEPOP_FASTBUILD (rasterizer.h:15-17,50-58).
#include "stp_render_hier.inc"

#ifndef STP_INST_MID
#error "STP_INST_MID must be defined"
#endif
#ifndef STP_INST_MODE
#error "STP_INST_MODE must be defined"
#endif
#define STP_SLICE(PASS, MID) || (STP_INST_MODE == PASS && STP_INST_MID == MID)
#if !(0 STP_HIER_SLICES(STP_SLICE))
#error "(STP_INST_MODE, STP_INST_MID) is not in STP_HIER_SLICES"
#endif
#undef STP_SLICE

namespace stp {

// returns hipErrorInvalidValue with *handled = false when this slice has no kernel for `head`
hipError_t STP_HIER_SLICE_FN(STP_INST_MODE, STP_INST_MID)(const FrameParams& f, const RenderArgs& a, hipStream_t st, bool* handled)
{
    constexpr int MID = STP_INST_MID;
    constexpr int MODE = STP_INST_MODE;
    constexpr bool BWD = pass_backward(MODE);
    const int head = f.s.queue_per_pixel;
    const bool cull = f.s.hierarchical_4x4_culling != 0;
    *handled = true;
#define STP_GO(H) return cull ? launch_hier_one<H, MID, true, MODE>(f, a, st) : launch_hier_one<H, MID, false, MODE>(f, a, st)
    // the default queue sizes' forward passes also exist without the reciprocal's domain check, for frames whose Sigma^-1
    // entries are all tame (every frame of a sane scene: FrameParams::wild_cov, from preprocess_kernel's status word)
    if constexpr (!BWD && MID == 8) {
        if (head == 4 && !f.wild_cov) return cull ? launch_hier_one<4, MID, true, MODE, true>(f, a, st) : launch_hier_one<4, MID, false, MODE, true>(f, a, st);
    }
    if (head == 4) STP_GO(4);
#ifndef STP_FASTBUILD
    if (head == 8) STP_GO(8);
    if constexpr (BWD) { if (head == 12) STP_GO(12); } // (the backward's ladder only: a forward slice has no HEAD = 12 kernel)
    if (head == 16) STP_GO(16);
#endif
#undef STP_GO
    *handled = false;
    return hipErrorInvalidValue;
}

} // namespace stp
