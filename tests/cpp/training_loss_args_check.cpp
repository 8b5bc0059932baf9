// training_loss_args_check.cpp -- calls the three C functions of the training loss (include/stp_raster.h: stp_training_loss_workspace_floats,
// stp_training_loss_forward, stp_training_loss_backward) with the invalid and the empty argument sets.  Validation precedes any launch, so
// this needs no GPU: the pointers are host addresses that are never followed.  Built like photometric_args_check.cpp
// (tests/test_training_loss_cpu.py builds and runs it):
//     hipcc -std=c++17 -O1 -Wall -I include tests/cpp/training_loss_args_check.cpp -o training_loss_args_check.bin -L <library dir> -lstp_raster -Wl,-rpath,<library dir>
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

static float buf[64];

static int fwd(int planes, int H, int W, const StpTrainingLoss* x) { return stp_training_loss_forward(planes, H, W, buf, buf, x, buf, buf, buf, nullptr); }
static int bwd(int planes, int H, int W, const StpTrainingLoss* x, float* dE = nullptr, float* dD = nullptr, float* ws = buf)
{
    return stp_training_loss_backward(planes, H, W, buf, buf, x, buf, buf, buf, dE, dD, ws, nullptr);
}

int main()
{
    float *p = buf, *null = nullptr;
    const int bad = STP_ERR_INVALID_ARGUMENT;
    bool ok = stp_abi_version() == 7;
    if (!ok) std::printf("ABI version %d, expected 7\n", stp_abi_version());
    StpTrainingLoss none{}, full{p, p, p, p, p, 1, 0, 0, 3, 1};
    // refused: sizes
    ok = ok && expect("forward planes < 0", fwd(-1, 4, 4, &full), bad, "negative size");
    ok = ok && expect("forward W < 0", fwd(3, 4, -4, nullptr), bad, "negative size");
    ok = ok && expect("backward H < 0", bwd(3, -4, 4, &full), bad, "negative size");
    ok = ok && expect("forward 2^31", fwd(2, 32768, 32768, &none), bad, ">= 2^31");
    ok = ok && expect("backward wraps to 0", bwd(65536, 65536, 65536, nullptr), bad, ">= 2^31");
    {
        StpTrainingLoss x = full;
        x.depth_planes = -1;
        ok = ok && expect("depth_planes < 0", fwd(3, 4, 4, &x), bad, "negative size");
        x.depth_planes = 1 << 30;
        ok = ok && expect("depth planes * H * W >= 2^31", fwd(3, 4, 4, &x), bad, ">= 2^31");
        x = full;
        x.channels = -3;
        ok = ok && expect("channels < 0", fwd(3, 4, 4, &x), bad, "negative size");
    }
    // refused: the extras
    {
        StpTrainingLoss x = full;
        x.clamp = 2;
        ok = ok && expect("clamp = 2", fwd(3, 4, 4, &x), bad, "must be 0 or 1");
        x = full;
        x.exposure_batched = -1;
        ok = ok && expect("exposure_batched = -1", bwd(3, 4, 4, &x), bad, "must be 0 or 1");
        ok = ok && expect("exposure with 4 planes", fwd(4, 4, 4, &full), bad, "exposure needs three channels");
        x = full;
        x.channels = 1;
        ok = ok && expect("exposure with channels = 1", fwd(3, 4, 4, &x), bad, "exposure needs three channels");
        x = none;
        x.alpha_mask = p;
        x.channels = 2;
        ok = ok && expect("mask, planes no multiple of channels", fwd(3, 4, 4, &x), bad, "no multiple of channels");
        x = full;
        x.mono_invdepth = nullptr;
        ok = ok && expect("invdepth without mono_invdepth", fwd(3, 4, 4, &x), bad, "come together");
        x = full;
        x.invdepth = nullptr;
        ok = ok && expect("mono_invdepth without invdepth", bwd(3, 4, 4, &x), bad, "come together");
        x = none;
        x.depth_mask = p;
        ok = ok && expect("depth_mask alone", fwd(3, 4, 4, &x), bad, "without invdepth");
        x = none;
        x.depth_planes = 1;
        ok = ok && expect("depth_planes alone", fwd(3, 4, 4, &x), bad, "without invdepth");
        x = full;
        x.depth_planes = 0;
        ok = ok && expect("invdepth with depth_planes = 0", fwd(3, 4, 4, &x), bad, "depth_planes = 0");
        ok = ok && expect("dL_dexposure without exposure", bwd(3, 4, 4, &none, p), bad, "dL_dexposure without exposure");
        ok = ok && expect("dL_dinvdepth without invdepth", bwd(3, 4, 4, nullptr, null, p), bad, "dL_dinvdepth without invdepth");
    }
    // refused: null pointers
    ok = ok && expect("forward null image", stp_training_loss_forward(3, 4, 4, null, p, &full, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("forward null target", stp_training_loss_forward(3, 4, 4, p, null, &full, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("forward null out3", stp_training_loss_forward(3, 4, 4, p, p, nullptr, null, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("forward null workspace", stp_training_loss_forward(3, 4, 4, p, p, &full, p, null, null, nullptr), bad, "null pointer");
    ok = ok && expect("backward null maps", stp_training_loss_backward(3, 4, 4, p, p, &full, null, p, p, p, p, p, nullptr), bad, "null maps");
    ok = ok && expect("backward null image", stp_training_loss_backward(3, 4, 4, null, p, &full, p, p, p, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("backward null target", stp_training_loss_backward(3, 4, 4, p, null, &full, p, p, p, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("backward null dL_dout3", stp_training_loss_backward(3, 4, 4, p, p, nullptr, p, null, p, null, null, null, nullptr), bad, "null pointer");
    ok = ok && expect("backward null dL_dimage", stp_training_loss_backward(3, 4, 4, p, p, &full, p, p, null, p, p, p, nullptr), bad, "null pointer");
    ok = ok && expect("backward dL_dexposure without workspace", bwd(3, 4, 4, &full, p, p, null), bad, "null pointer");
    // empty work: 0, nothing touched
    ok = ok && expect("forward planes == 0", stp_training_loss_forward(0, 4, 4, null, null, nullptr, null, null, null, nullptr), 0, nullptr);
    ok = ok && expect("forward H == 0", fwd(3, 0, 4, &full), 0, nullptr);
    ok = ok && expect("forward W == 0", fwd(3, 4, 0, &none), 0, nullptr);
    ok = ok && expect("backward planes == 0", stp_training_loss_backward(0, 4, 4, null, null, nullptr, null, null, null, null, null, null, nullptr), 0, nullptr);
    ok = ok && expect("backward H == 0", bwd(3, 0, 4, &full, p, p), 0, nullptr);
    ok = ok && expect("backward W == 0", bwd(3, 4, 0, &full), 0, nullptr);
    for (int i = 0; ok && i < 64; i++)
        if (buf[i] != 0.0f) { std::printf("buffer touched at %d\n", i); ok = false; }
    // the workspace: the larger of the forward's (two floats per colour workgroup + one per depth workgroup) and the backward's (twelve per workgroup)
    const int TW = STP_PHOTOMETRIC_TILE_W, TH = STP_PHOTOMETRIC_TILE_H;
    struct { int planes, H, W, depth; size_t want; } ws[] = {
        {3, 1, 1, 0, 36}, {3, 1, 1, 1, 36}, {3, TH + 1, TW + 1, 1, 144}, {1, 5, 3 * TW - 1, 40, 2 * 3 + 40 * 3}, {0, 4, 4, 0, 0}, {3, 0, 4, 1, 0}, {-1, 4, 4, 0, 0},
        {3, 4, 4, -1, 0}, {2, 32768, 32768, 0, 0}, {3, 4, 4, 1 << 30, 0}};
    for (const auto& w : ws) {
        g_checked++;
        const size_t got = stp_training_loss_workspace_floats(w.planes, w.H, w.W, w.depth);
        if (ok && got != w.want) {
            std::printf("workspace_floats(%d, %d, %d, %d) = %zu, expected %zu\n", w.planes, w.H, w.W, w.depth, got, w.want);
            ok = false;
        }
    }
    if (!ok) return 1;
    std::printf("ok %d\n", g_checked);
    return 0;
}
