// photometric_args_check.cpp -- calls the three C functions of the fused photometric loss (include/stp_raster.h:
// stp_photometric_workspace_floats, stp_photometric_forward, stp_photometric_backward) with the invalid and the empty argument sets.
// Validation precedes any launch, so this needs no GPU: the pointers are host addresses that are never followed.  Built with the
// command line of tests/cpp/Makefile's rule (tests/test_photometric_cpu.py builds and runs it):
//     hipcc -std=c++17 -O1 -Wall -I include tests/cpp/photometric_args_check.cpp -o photometric_args_check.bin -L <library dir> -lstp_raster -Wl,-rpath,<library dir>
// Prints "ok <number of calls checked>" and exits 0, or the first failed expectation and exits 1.
#include <cstdio>
#include <cstring>

#include "stp_raster.h"

static int g_checked = 0;

static bool expect(const char* what, int got, int want, const char* needle)
{
    g_checked++;
    if (got != want) {
        std::printf("%s: returned %d, expected %d (%s)\n", what, got, want, stp_last_error());
        return false;
    }
    if (needle && !std::strstr(stp_last_error(), needle)) {
        std::printf("%s: last error \"%s\" does not name \"%s\"\n", what, stp_last_error(), needle);
        return false;
    }
    return true;
}

int main()
{
    static float buf[64];
    float *p = buf, *null = nullptr;
    const int bad = STP_ERR_INVALID_ARGUMENT;
    bool ok = stp_abi_version() == 7;
    if (!ok) std::printf("ABI version %d, expected 7\n", stp_abi_version());
    // refused: negative sizes
    ok = ok && expect("forward planes < 0", stp_photometric_forward(-1, 4, 4, p, p, p, p, p, nullptr), bad, "negative size");
    ok = ok && expect("forward H < 0", stp_photometric_forward(3, -4, 4, p, p, p, p, p, nullptr), bad, "negative size");
    ok = ok && expect("forward W < 0", stp_photometric_forward(3, 4, -4, p, p, p, null, p, nullptr), bad, "negative size");
    ok = ok && expect("backward planes < 0", stp_photometric_backward(-3, 4, 4, p, p, p, p, p, nullptr), bad, "negative size");
    ok = ok && expect("backward W < 0", stp_photometric_backward(3, 4, -1, p, p, p, p, p, nullptr), bad, "negative size");
    ok = ok && expect("negative size and a zero", stp_photometric_forward(0, -1, 4, p, p, p, p, p, nullptr), bad, "negative size");
    // refused: planes * H * W >= 2^31 (also where an int product would wrap)
    ok = ok && expect("forward 2^31", stp_photometric_forward(2, 32768, 32768, p, p, p, p, p, nullptr), bad, ">= 2^31");
    ok = ok && expect("forward 2^31 - 1 planes * 2", stp_photometric_forward(2147483647, 2, 1, p, p, p, p, p, nullptr), bad, ">= 2^31");
    ok = ok && expect("forward wraps to 0", stp_photometric_forward(65536, 65536, 65536, p, p, p, p, p, nullptr), bad, ">= 2^31");
    ok = ok && expect("forward all large", stp_photometric_forward(2147483647, 2147483647, 2147483647, p, p, p, p, p, nullptr), bad, ">= 2^31");
    ok = ok && expect("backward 2^31", stp_photometric_backward(1, 65536, 32768, p, p, p, p, p, nullptr), bad, ">= 2^31");
    // refused: null pointers
    ok = ok && expect("forward null image", stp_photometric_forward(3, 4, 4, null, p, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("forward null target", stp_photometric_forward(3, 4, 4, p, null, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("forward null out2", stp_photometric_forward(3, 4, 4, p, p, null, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("forward null workspace", stp_photometric_forward(3, 4, 4, p, p, p, null, null, nullptr), bad, "null pointer");
    ok = ok && expect("backward null maps", stp_photometric_backward(3, 4, 4, p, p, null, p, p, nullptr), bad, "null maps");
    ok = ok && expect("backward null image", stp_photometric_backward(3, 4, 4, null, p, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("backward null target", stp_photometric_backward(3, 4, 4, p, null, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("backward null dL_dout2", stp_photometric_backward(3, 4, 4, p, p, p, null, p, nullptr), bad, "null pointer");
    ok = ok && expect("backward null dL_dimage", stp_photometric_backward(3, 4, 4, p, p, p, p, null, nullptr), bad, "null pointer");
    // empty work: 0, nothing touched (not even looked at: every pointer may be null)
    ok = ok && expect("forward planes == 0", stp_photometric_forward(0, 4, 4, null, null, null, null, null, nullptr), 0, nullptr);
    ok = ok && expect("forward H == 0", stp_photometric_forward(3, 0, 4, p, p, p, p, p, nullptr), 0, nullptr);
    ok = ok && expect("forward W == 0", stp_photometric_forward(3, 4, 0, p, p, p, null, p, nullptr), 0, nullptr);
    ok = ok && expect("forward W == 0, large", stp_photometric_forward(2147483647, 2147483647, 0, p, p, p, null, p, nullptr), 0, nullptr);
    ok = ok && expect("backward planes == 0", stp_photometric_backward(0, 4, 4, null, null, null, null, null, nullptr), 0, nullptr);
    ok = ok && expect("backward H == 0", stp_photometric_backward(3, 0, 4, p, p, null, p, p, nullptr), 0, nullptr);
    ok = ok && expect("backward W == 0", stp_photometric_backward(3, 4, 0, p, p, p, p, p, nullptr), 0, nullptr);
    for (int i = 0; ok && i < 64; i++)
        if (buf[i] != 0.0f) { std::printf("buffer touched at %d\n", i); ok = false; }
    // the workspace: two floats per workgroup (a tile of STP_PHOTOMETRIC_TILE_W x STP_PHOTOMETRIC_TILE_H pixels of one plane)
    const int TW = STP_PHOTOMETRIC_TILE_W, TH = STP_PHOTOMETRIC_TILE_H;
    struct { int planes, H, W; size_t want; } ws[] = {
        {1, 1, 1, 2}, {3, TH, TW, 6}, {3, TH + 1, TW + 1, 24}, {1, 5, 3 * TW - 1, 6}, {6, 37, 53, 2 * 6 * (size_t)((37 + TH - 1) / TH) * ((53 + TW - 1) / TW)},
        {3, 1080, 1920, 2 * 3 * (size_t)((1080 + TH - 1) / TH) * ((1920 + TW - 1) / TW)}, {0, 4, 4, 0}, {3, 0, 4, 0}, {3, 4, 0, 0}, {-1, 4, 4, 0},
        {2, 32768, 32768, 0}, {2147483647, 1, 1, 2 * (size_t)2147483647}};
    for (const auto& w : ws) {
        g_checked++;
        const size_t got = stp_photometric_workspace_floats(w.planes, w.H, w.W);
        if (ok && got != w.want) {
            std::printf("workspace_floats(%d, %d, %d) = %zu, expected %zu\n", w.planes, w.H, w.W, got, w.want);
            ok = false;
        }
    }
    if (!ok) return 1;
    std::printf("ok %d\n", g_checked);
    return 0;
}
