// stp_render_pass.h -- the render passes: THE list every render kernel family (global, k-buffer tile / wave / ring, hierarchical) instantiates
// and dispatches by.  No HIP include: plain C++ (tests/cpp/render_pass_check.cpp compiles it with g++).
//
// A pass is the kernels' `int MODE` template parameter.  The values are fixed: the Makefile's slice list, tools/check_dpp_hazards.py and
// tools/flag_variants.sh pass them as -DSTP_INST_MODE=n, and they are part of the kernels' mangled names.
#pragma once

namespace stp {

constexpr int PASS_FWD = 0;             // forward
constexpr int PASS_BWD = 1;             // backward that re-runs the sort (the reference's scheme; with a blend log only the fallback for tiles whose log overflowed)
constexpr int PASS_FWD_RECORD = 2;      // training forward: also records every pixel's blend order in the blend log (its backward: stp_render_replay.hip)
constexpr int PASS_FWD_DEPTH = 3;       // forward of the debug depth visualisation: accumulates depth * alpha * T instead of colour
constexpr int PASS_FWD_INVD = 4;        // PASS_FWD with the inverse-depth output (stp_set_forward_invdepth): a fourth accumulator D += alpha T / z
constexpr int PASS_FWD_RECORD_INVD = 5; // PASS_FWD_RECORD with the inverse-depth output
constexpr int PASS_BWD_INVD = 6;        // PASS_BWD with the fourth channel's gradient (stp_set_backward_invdepth)
constexpr int PASS_COUNT = 7;

constexpr bool pass_backward(int p) { return p == PASS_BWD || p == PASS_BWD_INVD; }
constexpr bool pass_records(int p) { return p == PASS_FWD_RECORD || p == PASS_FWD_RECORD_INVD; } // writes the blend log
constexpr bool pass_depthviz(int p) { return p == PASS_FWD_DEPTH; }
constexpr bool pass_invdepth(int p) { return p == PASS_FWD_INVD || p == PASS_FWD_RECORD_INVD || p == PASS_BWD_INVD; }

// The pass of a launch.  `record`: the frame keeps a blend log (uses_blend_log) -- a forward then records it; the re-sorting backward is the same
// kernel with or without one.  Negative: a combination the API has refused before any launch (the depth visualisation has neither an
// inverse-depth output nor a backward).
constexpr int render_pass(bool backward, bool record, bool depthviz, bool invdepth)
{
    if (depthviz) return (backward || invdepth) ? -1 : PASS_FWD_DEPTH;
    if (backward) return invdepth ? PASS_BWD_INVD : PASS_BWD;
    if (record) return invdepth ? PASS_FWD_RECORD_INVD : PASS_FWD_RECORD;
    return invdepth ? PASS_FWD_INVD : PASS_FWD;
}

static_assert(PASS_FWD == 0 && PASS_BWD == 1 && PASS_FWD_RECORD == 2 && PASS_FWD_DEPTH == 3 && PASS_FWD_INVD == 4 && PASS_FWD_RECORD_INVD == 5 &&
              PASS_BWD_INVD == 6 && PASS_COUNT == 7, "the pass ids are command-line values and part of the kernels' names");
constexpr bool pass_roundtrips(int p) { return render_pass(pass_backward(p), pass_records(p), pass_depthviz(p), pass_invdepth(p)) == p; }
static_assert(pass_roundtrips(0) && pass_roundtrips(1) && pass_roundtrips(2) && pass_roundtrips(3) && pass_roundtrips(4) && pass_roundtrips(5) &&
              pass_roundtrips(6), "the predicates invert the selector");

} // namespace stp

// The slices of the hierarchical kernel: one translation unit (stp_render_hier_inst.hip, -DSTP_INST_MODE=pass -DSTP_INST_MID=mid) and one entry
// point per (pass, MID).  X(pass, mid) with literal numbers, so that they can be pasted into the entry point's name; stp_render_hier.hip
// declares and picks the entry points from this list, the slice derives its own name from it, the Makefile builds hier_<tag><mid>.o per pair.
#define STP_HIER_PASSES(X, MID) X(0, MID) X(1, MID) X(2, MID) X(3, MID) X(4, MID) X(5, MID) X(6, MID)
#ifdef STP_FASTBUILD
#define STP_HIER_SLICES(X) STP_HIER_PASSES(X, 8)
#else
#define STP_HIER_SLICES(X) STP_HIER_PASSES(X, 8) STP_HIER_PASSES(X, 12) STP_HIER_PASSES(X, 20)
#endif
#define STP_HIER_SLICE_FN_(PASS, MID) launch_hier_pass##PASS##_mid##MID
#define STP_HIER_SLICE_FN(PASS, MID) STP_HIER_SLICE_FN_(PASS, MID) // (the arguments may be macros: expanded before the paste)

namespace stp {
#define STP_SLICE(PASS, MID) static_assert(pass_roundtrips(PASS) && (MID == 8 || MID == 12 || MID == 20), "a slice of an unknown pass or queue size");
STP_HIER_SLICES(STP_SLICE)
#undef STP_SLICE
} // namespace stp
