// render_pass_check.cpp -- the render passes' ids, predicates and selector (csrc/stp_render_pass.h) against tables written out here, on the host alone.
//     g++ -O1 -std=c++17 -fsanitize=address,undefined -I stopthepop-rasterization_amd/csrc tests/cpp/render_pass_check.cpp -o render_pass_check && ./render_pass_check
#include "stp_render_pass.h"

#include <cstdio>
#include <string_view>

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

int main()
{
    // the selector, all 16 combinations: index = backward * 8 + record * 4 + depth visualisation * 2 + inverse depth
    static const int SELECT[16] = {
        0,  // forward
        4,  // forward, inverse depth
        3,  // depth visualisation
        -1, // depth visualisation with inverse depth: refused
        2,  // recording forward
        5,  // recording forward, inverse depth
        3,  // depth visualisation (a frame with a log request: the visualisation records none)
        -1, // refused
        1,  // backward
        6,  // backward, inverse depth
        -1, // depth visualisation in a backward: refused
        -1, // refused
        1,  // backward of a frame with a blend log (the re-sorting kernel: the fallback of the replay)
        6,  // the same, inverse depth
        -1, // refused
        -1, // refused
    };
    for (int i = 0; i < 16; i++) {
        const int got = stp::render_pass((i & 8) != 0, (i & 4) != 0, (i & 2) != 0, (i & 1) != 0);
        if (got != SELECT[i]) { std::printf("FAILED: render_pass of combination %d = %d, expected %d\n", i, got, SELECT[i]); failures++; }
    }

    // the ids
    CHECK(stp::PASS_FWD == 0 && stp::PASS_BWD == 1 && stp::PASS_FWD_RECORD == 2 && stp::PASS_FWD_DEPTH == 3);
    CHECK(stp::PASS_FWD_INVD == 4 && stp::PASS_FWD_RECORD_INVD == 5 && stp::PASS_BWD_INVD == 6 && stp::PASS_COUNT == 7);

    // the predicates on the seven ids: {backward, records, depth visualisation, inverse depth}
    static const bool PRED[7][4] = {
        {false, false, false, false}, // 0 forward
        {true, false, false, false},  // 1 re-sorting backward
        {false, true, false, false},  // 2 recording forward
        {false, false, true, false},  // 3 depth visualisation
        {false, false, false, true},  // 4 forward, inverse depth
        {false, true, false, true},   // 5 recording forward, inverse depth
        {true, false, false, true},   // 6 re-sorting backward, inverse depth
    };
    for (int p = 0; p < 7; p++) {
        const bool got[4] = {stp::pass_backward(p), stp::pass_records(p), stp::pass_depthviz(p), stp::pass_invdepth(p)};
        for (int k = 0; k < 4; k++)
            if (got[k] != PRED[p][k]) { std::printf("FAILED: predicate %d of pass %d = %d\n", k, p, (int)got[k]); failures++; }
    }
    // no predicate holds for a value that is not a pass
    for (int p : {-1, 7}) CHECK(!stp::pass_backward(p) && !stp::pass_records(p) && !stp::pass_depthviz(p) && !stp::pass_invdepth(p));

    // the hierarchical slices' list: every pass once per queue size, the entry point's name from the pair
    int n_slices = 0, per_pass[7] = {};
#define STP_SLICE(PASS, MID) n_slices++; per_pass[PASS] += (MID == 8 || MID == 12 || MID == 20) ? 1 : 100;
    STP_HIER_SLICES(STP_SLICE)
#undef STP_SLICE
    CHECK(n_slices == 21);
    for (int p = 0; p < 7; p++) CHECK(per_pass[p] == 3);
#define STP_STR2(x) #x
#define STP_STR(x) STP_STR2(x)
#define STP_CHECK_PASS 5
#define STP_CHECK_MID 12
    const char* const name = STP_STR(STP_HIER_SLICE_FN(STP_CHECK_PASS, STP_CHECK_MID)); // (arguments that are macros, as in the slice's translation unit)
    CHECK(std::string_view(name) == "launch_hier_pass5_mid12");

    if (failures == 0) std::printf("ok\n");
    return failures == 0 ? 0 : 1;
}
