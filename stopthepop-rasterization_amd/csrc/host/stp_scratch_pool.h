// stp_scratch_pool.h -- the buffers a forward hands to the library: the resize callback, the pool for the two large ones (tile lists with their
// list-ordered entry records, image state with the blend log), and the memory of which allocation each buffer is.
//
// The scratch pool.  Cycling a GB-sized block through torch's caching allocator every step invites splitting: smaller
// requests carve pieces off the free block, the next forward finds no hole of that size and the allocator falls back to
// hipMalloc (tens of ms per step -- observed on MI355X).  Buffers of >= 256 MiB are therefore kept on a small free list per
// device: handed out by the forward, handed back by the backward (release_scratch), capacities in steps of 64 MiB so that a
// buffer whose size follows num_rendered finds its predecessor.  Reuse across streams is ordered by an event recorded on
// the releasing stream; a generation counter per address lets the autograd function detect a backward that comes after
// its buffers were recycled (check_scratch).
#pragma once

#include <torch/extension.h>

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <map>
#include <mutex>
#include <unordered_map>

#include "stp_exports.h"

namespace {
constexpr int64_t BIG_BYTES = 256ll << 20, BIG_STEP = 64ll << 20;

struct Pooled { torch::Tensor t; hipEvent_t ev; }; // ev: recorded on the releasing stream (owned by g_events, never destroyed: creating an
                                                   // event can cost a driver call when the runtime's signal pool grows -- not per step)
std::mutex g_mutex;
std::map<int, std::vector<Pooled>> g_free;          // device -> free buffers (oldest first)
std::unordered_map<uintptr_t, int64_t> g_generation; // data_ptr -> how often the buffer at this address was handed out
std::unordered_map<uintptr_t, hipEvent_t> g_events;  // data_ptr -> the event that orders reuse of the buffer at this address
int g_keep = 4;                                       // free buffers kept per device
int64_t g_max_bytes = -1;                             // optional cap on the pooled bytes per device

// A pooled buffer is used on whichever stream is current when it is handed out, not only on the stream torch::empty allocated it on: the caching
// allocator must know, or it could re-issue the block -- once the pool evicts it -- while kernels of another stream still read it.  (A no-op for
// the allocation stream itself, i.e. for single-stream training.)
void note_stream_use(const torch::Tensor& buf)
{
    c10::hip::HIPCachingAllocator::recordStream(buf.storage().data_ptr(), c10::hip::getCurrentHIPStream(buf.get_device()));
}

void put_back(const torch::Tensor& buf) // caller holds g_mutex
{
    auto& fl = g_free[buf.get_device()];
    for (auto& p : fl)
        if (p.t.data_ptr() == buf.data_ptr()) return;
    note_stream_use(buf);
    g_api.forget_buffer(buf.data_ptr()); // (its next tenant is described by what a forward carves there, or by the header a copy brings along)
    hipEvent_t& ev = g_events[(uintptr_t)buf.data_ptr()];
    if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
    const hipStream_t stream = c10::hip::getCurrentHIPStream(buf.get_device()).stream();
    const bool recorded = ev && hipEventRecord(ev, stream) == hipSuccess;
    if (!recorded) (void)hipStreamSynchronize(stream); // (no event: order reuse the slow way)
    fl.push_back({buf, recorded ? ev : nullptr});
    auto total = [&]() { int64_t s = 0; for (auto& p : fl) s += p.t.numel(); return s; };
    while ((int)fl.size() > g_keep || (g_max_bytes >= 0 && fl.size() > 1 && total() > g_max_bytes)) fl.erase(fl.begin());
}

// Which allocation a scratch buffer IS: the library caches (address, num_rendered) -> layout for the buffers its forwards carved, and
// an address alone does not say whose memory it is now -- a buffer is freed, a clone of ANOTHER forward's buffer lands on its address with the same
// num_rendered (static views repeat it exactly), and the stale entry would describe it.  The binding knows more than the address: it remembers the
// StorageImpl of every binning / image buffer its forwards returned (weak reference); a backward that is handed a tensor with another storage at a
// known address, or one whose storage has died since, tells the library to forget the address first, and the library reads the header the
// buffer carries (include/stp_raster.h: stp_forget_buffer).
std::unordered_map<uintptr_t, c10::weak_intrusive_ptr<c10::StorageImpl>> g_storage_of; // behind g_mutex
void remember_storage(const torch::Tensor& t)
{
    if (!t.defined() || t.numel() == 0) return;
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_storage_of.size() > 4096) // forwards whose buffers nobody came back for
        for (auto it = g_storage_of.begin(); it != g_storage_of.end();) it = it->second.expired() ? g_storage_of.erase(it) : std::next(it);
    g_storage_of.insert_or_assign((uintptr_t)t.data_ptr(), t.storage().getWeakStorageImpl());
}
void forget_unless_same_storage(const torch::Tensor& t)
{
    if (!t.defined() || t.numel() == 0) return;
    std::lock_guard<std::mutex> lock(g_mutex);
    const auto it = g_storage_of.find((uintptr_t)t.data_ptr());
    if (it != g_storage_of.end() && !it->second.expired() && it->second._unsafe_get_target() == t.storage().unsafeGetStorageImpl()) return;
    if (it != g_storage_of.end()) g_storage_of.erase(it);
    g_api.forget_buffer(t.data_ptr());
}

// Placement experiment (profiles/EXPERIMENTS.md, round 6: the k-buffer ring kernel's speed follows WHERE the frame's scratch buffers lie):
// STP_SCRATCH_OFFSET_GEOM / _BINNING / _IMAGE = bytes (multiple of 256, below 64 MiB) the buffer of that kind starts behind the start of its
// allocation.  Read at every request; unset or 0 = the allocation's own start.
constexpr int64_t OFFSET_SLACK = 64ll << 20;
int64_t scratch_offset(int kind)
{
    static const char* const names[3] = {"STP_SCRATCH_OFFSET_GEOM", "STP_SCRATCH_OFFSET_BINNING", "STP_SCRATCH_OFFSET_IMAGE"};
    const char* e = kind >= 0 && kind < 3 ? std::getenv(names[kind]) : nullptr;
    if (!e) return 0;
    const int64_t v = std::strtoll(e, nullptr, 0) & ~255ll;
    return v < 0 ? 0 : (v >= OFFSET_SLACK ? OFFSET_SLACK - 256 : v);
}
torch::Tensor empty_at_offset(int64_t n, const torch::TensorOptions& opt, int64_t off)
{
    return off ? torch::empty({n + OFFSET_SLACK}, opt).narrow(0, off, n) : torch::empty({n}, opt);
}

// The reference's resizeFunctional (rasterize_points.cu:33-41): grows a byte tensor on request.  The library may call the
// binning one twice per forward (a size guess before the num_rendered hand-over, the exact size afterwards if the guess
// was short: include/stp_raster.h): a request the current buffer already covers returns the same pointer.
struct Resizer {
    torch::Tensor t;
    bool pooled = false, from_pool = false;
    int kind = -1;
    static void* call(void* user, size_t nbytes_)
    {
        auto* self = static_cast<Resizer*>(user);
        try {
            const int64_t nbytes = (int64_t)nbytes_;
            if (nbytes > 0 && nbytes <= self->t.numel()) return self->t.data_ptr();
            const int64_t off = scratch_offset(self->kind);
            if (self->pooled && nbytes >= BIG_BYTES) {
                std::lock_guard<std::mutex> lock(g_mutex);
                if (self->from_pool) put_back(self->t); // the guess was too small: the buffer goes back, a larger one comes
                const int64_t cap = (nbytes + BIG_STEP - 1) / BIG_STEP * BIG_STEP;
                auto& fl = g_free[self->t.get_device()];
                int hit = -1;
                for (int i = 0; i < (int)fl.size(); i++) {
                    const int64_t n = fl[i].t.numel();
                    if (n >= nbytes && n <= cap + cap / 4 && fl[i].t.storage_offset() == off && (hit < 0 || n < fl[hit].t.numel())) hit = i;
                }
                if (hit >= 0) {
                    Pooled p = fl[hit];
                    fl.erase(fl.begin() + hit);
                    if (p.ev) // the releasing stream's kernels may still be reading it: order this stream behind them
                        (void)hipStreamWaitEvent(c10::hip::getCurrentHIPStream(p.t.get_device()).stream(), p.ev, 0);
                    self->t = p.t;
                    note_stream_use(self->t);
                } else self->t = empty_at_offset(cap, self->t.options(), off);
                self->from_pool = true;
                g_generation[(uintptr_t)self->t.data_ptr()]++;
                return self->t.data_ptr();
            }
            if (off && nbytes) self->t = empty_at_offset(nbytes, self->t.options(), off);
            else self->t.resize_({nbytes});
            return nbytes ? self->t.data_ptr() : nullptr;
        } catch (...) { // surfaces as STP_ERR_ALLOC on the C side
            return nullptr;
        }
    }
};

// ---- the pool's surface in the module ---------------------------------------------------------------------------------
int64_t scratch_generation(const torch::Tensor& buf) // token the autograd function keeps with a pooled buffer (0 for ordinary ones)
{
    if (buf.numel() < BIG_BYTES) return 0;
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = g_generation.find((uintptr_t)buf.data_ptr());
    return it == g_generation.end() ? 0 : it->second;
}

void check_scratch(const torch::Tensor& buf, int64_t generation)
{
    if (generation && scratch_generation(buf) != generation)
        throw std::runtime_error("a scratch buffer of this forward (tile lists / blend log) was recycled by a later forward pass; run the forward "
                                 "again before this backward");
}

void release_scratch(const torch::Tensor& buf) // hand a pooled buffer back after the backward that consumed it
{
    if (buf.numel() < BIG_BYTES || !buf.is_cuda()) return;
    const c10::hip::HIPGuard guard(buf.get_device());
    std::lock_guard<std::mutex> lock(g_mutex);
    put_back(buf);
}

int64_t clear_scratch_pool(int device) // device < 0: all devices; returns the bytes released
{
    std::lock_guard<std::mutex> lock(g_mutex);
    int64_t freed = 0;
    for (auto it = g_free.begin(); it != g_free.end();) {
        if (device >= 0 && it->first != device) { ++it; continue; }
        for (auto& p : it->second) freed += p.t.numel();
        it = g_free.erase(it);
    }
    return freed;
}

void set_scratch_pool_limit(int max_buffers, int64_t max_bytes)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    g_keep = max_buffers;
    g_max_bytes = max_bytes;
}

std::vector<int64_t> pooled_sizes(int device)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    std::vector<int64_t> out;
    auto it = g_free.find(device);
    if (it != g_free.end()) for (auto& p : it->second) out.push_back(p.t.numel());
    return out;
}
} // namespace
