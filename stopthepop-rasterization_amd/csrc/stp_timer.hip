// stp_timer.hip -- the optional stage timer of libstp_raster.so (stp_timing_* of include/stp_raster.h): one instance PER DEVICE behind a
// mutex.  A backward is attributed to the latest forward of its device: meant for one timed caller per device -- bench.py, the viewer's
// timings text.  The forward and the backward reach it through timer_begin_forward / timer_begin_backward / timer_mark (stp_internal.h).
#include "stp_internal.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

namespace stp {

static bool g_timing = false;

// Counterpart of the reference's Timer (rasterizer_impl.h:77-147): hipEvents around the stages of every call,
// recorded on the call's stream.  A ring of event sets lets a whole timed region run without any extra host
// synchronisation; spans are harvested lazily and averaged (mean over the calls since stp_timing_enable(1)).
struct StageTimer {
    static constexpr int SETS = 64, EV = 8; // events 0..4: forward stage boundaries, 5..7: backward
    static constexpr int HIST = 1024;       // per-call stage times kept since the last reset (stp_timing_history)
    struct Set { hipEvent_t ev[EV]; bool have[EV]; bool used; long seq; std::chrono::steady_clock::time_point host[EV]; };
    Set sets[SETS] = {};
    bool created = false;
    int cur = 0;
    double sum[6] = {};
    long cnt[6] = {};
    long failures = 0; // hipEventCreate / Record failures since the last reset (surfaced by stp_timing_read)
    long calls = 0;    // forwards begun since the last reset
    float hist[HIST][6]; // stage times of call (seq mod HIST), -1 = not measured
    float hist_host[HIST][6]; // ... and the HOST time between recording the stage's two events (the launching thread's own time in that part of the call)
    void ensure()
    {
        if (created) return;
        for (auto& s : sets) { for (auto& e : s.ev) if (hipEventCreate(&e) != hipSuccess) failures++; for (auto& h : s.have) h = false; s.used = false; }
        created = true;
    }
    void harvest(Set& s)
    {
        if (!s.used) return;
        static const int from[6] = {0, 1, 2, 3, 5, 6}, to[6] = {1, 2, 3, 4, 6, 7};
        for (int i = 0; i < 6; i++) {
            if (!(s.have[from[i]] && s.have[to[i]])) continue;
            if (hipEventSynchronize(s.ev[to[i]]) != hipSuccess) continue;
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, s.ev[from[i]], s.ev[to[i]]) == hipSuccess) {
                sum[i] += ms; cnt[i]++; hist[s.seq % HIST][i] = ms;
                hist_host[s.seq % HIST][i] = std::chrono::duration<float, std::milli>(s.host[to[i]] - s.host[from[i]]).count();
            }
        }
        for (auto& h : s.have) h = false;
        s.used = false;
    }
    void begin_forward()
    {
        if (!g_timing) return;
        ensure();
        cur = (cur + 1) % SETS;
        harvest(sets[cur]); // only blocks if the ring wrapped around unharvested work
        sets[cur].used = true;
        sets[cur].seq = calls++;
        for (auto& v : hist[sets[cur].seq % HIST]) v = -1.0f;
        for (auto& v : hist_host[sets[cur].seq % HIST]) v = -1.0f;
    }
    void begin_backward()
    {
        if (!g_timing) return;
        ensure();
        sets[cur].used = true;
        for (int i = 5; i < EV; i++) sets[cur].have[i] = false;
    }
    void mark(int i, hipStream_t st)
    {
        if (!g_timing) return;
        ensure();
        if (hipEventRecord(sets[cur].ev[i], st) != hipSuccess) { failures++; return; }
        sets[cur].host[i] = std::chrono::steady_clock::now();
        sets[cur].have[i] = true;
    }
    void reset()
    {
        if (created) for (auto& s : sets) { for (auto& h : s.have) h = false; s.used = false; }
        for (auto& v : sum) v = 0.0;
        for (auto& c : cnt) c = 0;
        failures = 0;
        calls = 0;
    }
};
// One timer per device (its events live on that device; a backward is attributed to the latest forward OF ITS DEVICE), all
// behind one mutex: timing is a debugging aid, the lock is uncontended in the single-threaded use the reference knows.
static StageTimer g_timers[MAX_DEVICES];
static std::mutex g_timer_mutex;
static StageTimer& current_timer()
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MAX_DEVICES) d = 0;
    return g_timers[d];
}
// (the call sites stay short: lock, then the current device's timer)
void timer_begin_forward() { if (!g_timing) return; std::lock_guard<std::mutex> l(g_timer_mutex); current_timer().begin_forward(); }
void timer_begin_backward() { if (!g_timing) return; std::lock_guard<std::mutex> l(g_timer_mutex); current_timer().begin_backward(); }
void timer_mark(int i, hipStream_t st) { if (!g_timing) return; std::lock_guard<std::mutex> l(g_timer_mutex); current_timer().mark(i, st); }

} // namespace stp

using namespace stp;

extern "C" {

void stp_timing_enable(int enabled)
{
    std::lock_guard<std::mutex> l(g_timer_mutex);
    g_timing = enabled != 0;
    if (g_timing) {
        for (auto& t : g_timers) t.reset();
        current_timer().ensure(); // the calling thread's device: its 512 events exist before the first timed call (creating them inside it
                                  // put 2-3 ms of driver calls into the first step of a timed region)
    }
}

int stp_timing_read(float* ms6) // the calling thread's current device
{
    if (!ms6) return fail(STP_ERR_INVALID_ARGUMENT, "null output");
    for (int i = 0; i < 6; i++) ms6[i] = -1.0f;
    std::lock_guard<std::mutex> l(g_timer_mutex);
    StageTimer& t = current_timer();
    if (!t.created) return 0;
    for (auto& s : t.sets) t.harvest(s);
    // 0 Preprocess (+scan+read-back), 1 Duplicate, 2 Sort (+ranges), 3 Render, 4 BwdRender, 5 BwdPreprocess
    for (int i = 0; i < 6; i++)
        if (t.cnt[i] > 0) ms6[i] = (float)(t.sum[i] / (double)t.cnt[i]);
    if (t.failures > 0) return fail(STP_ERR_HIP, "stage timer: " + std::to_string(t.failures) + " hipEvent create/record call(s) failed; timings are incomplete");
    return 0;
}

static int timing_history(float* ms6, int capacity, bool host);
int stp_timing_history(float* ms6, int capacity) { return timing_history(ms6, capacity, false); } // the calling thread's current device
int stp_timing_history_host(float* ms6, int capacity) { return timing_history(ms6, capacity, true); }
static int timing_history(float* ms6, int capacity, bool host)
{
    if (!ms6 || capacity < 0) return fail(STP_ERR_INVALID_ARGUMENT, "null output");
    std::lock_guard<std::mutex> l(g_timer_mutex);
    StageTimer& t = current_timer();
    if (!t.created) return 0;
    for (auto& s : t.sets) t.harvest(s);
    const long n = std::min<long>(std::min<long>(t.calls, StageTimer::HIST), capacity);
    for (long k = 0; k < n; k++) // chronological: the last n calls
        std::memcpy(ms6 + 6 * k, (host ? t.hist_host : t.hist)[(t.calls - n + k) % StageTimer::HIST], 6 * sizeof(float));
    return (int)n;
}

size_t stp_timing_text(char* buf, size_t size)
{
    float ms[6];
    (void)stp_timing_read(ms);
    static const char* names[6] = {"Preprocess", "Duplicate", "Sort", "Render", "BwdRender", "BwdPreprocess"};
    std::string text = "Timings: \n";
    float total = 0.0f;
    char line[96];
    for (int i = 0; i < 4; i++) {
        const float v = ms[i] >= 0.0f ? ms[i] : 0.0f;
        std::snprintf(line, sizeof(line), " - %s: %gms\n", names[i], v);
        text += line;
        total += v;
    }
    std::snprintf(line, sizeof(line), " - Total: %gms\n", total); // reference Timer::total (rasterizer_impl.h:79,131-134)
    text += line;
    for (int i = 4; i < 6; i++)
        if (ms[i] >= 0.0f) {
            std::snprintf(line, sizeof(line), " - %s: %gms\n", names[i], ms[i]);
            text += line;
        }
    if (buf && size > 0) {
        const size_t n = text.size() < size - 1 ? text.size() : size - 1;
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return text.size();
}

} // extern "C"
