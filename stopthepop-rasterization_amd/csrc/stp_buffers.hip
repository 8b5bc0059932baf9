// stp_buffers.hip -- the three scratch buffers of libstp_raster.so: how they are carved (the state carving of the reference's
// rasterizer_impl.cu:175-217, our own SoA layout), the size and layout queries of include/stp_raster.h built on the carving, and the
// headers / host cache that tell a backward what a buffer was carved with.
#include "stp_internal.h"
#include "stp_layout_cache.h"

#include <cstring>
#include <mutex>
#include <string>

namespace stp {

GeometryState carve_geometry(char* base, size_t P, bool with_inv, size_t* total, NamedOffset* names, int* n_names, float** sh_stash)
{
    Carver c(base);
    GeometryState g{};
    size_t off;
    int n = 0;
    auto note = [&](const char* nm, size_t o, size_t cnt) { if (names) names[n] = {nm, o, cnt}; n++; };
    g.status = c.take<uint32_t>(64, &off);
    g.depths = c.take<float>(P, &off); note("depths", off, P);
    g.clamped = c.take<uint8_t>(3 * P, &off); note("clamped", off, 3 * P);
    g.internal_radii = c.take<int32_t>(P, &off); note("radii", off, P);
    g.rects2D = c.take<float2>(P, &off); note("rects2D", off, 2 * P);
    g.means2D = c.take<float2>(P, &off); note("means2D", off, 2 * P);
    g.cov3D = c.take<float>(6 * P, &off); note("cov3D", off, 6 * P);
    if (with_inv) { g.cov3D_inv = c.take<float4>(3 * P, &off); note("cov3D_inv", off, 12 * P); }
    if (with_inv) { g.gpack = c.take<float4>(4 * P, &off); note("gpack", off, 16 * P); }
    g.conic_opacity = c.take<float4>(P, &off); note("conic_opacity", off, 4 * P);
    g.rgb = c.take<float>(3 * P, &off); note("rgb", off, 3 * P);
    g.tiles_touched = c.take<uint32_t>(P, &off); note("tiles_touched", off, P);
    g.point_offsets = c.take<uint32_t>(P, &off); note("point_offsets", off, P);
    g.block_sums = c.take<uint32_t>((P + 255) / 256, &off);
    g.block_prefix = c.take<uint32_t>((P + 255) / 256, &off);
    g.scan_temp_bytes = scan_temp_bytes(P);
    g.scan_temp = c.take<char>(g.scan_temp_bytes);
    g.invz = c.take<float>(P, &off); note("invz", off, P); // (behind everything else: the other sub-arrays are where they were)
    // the SH stash (stp_set_forward_sh_stash), LAST: a buffer carved without it ends here, and its size is the one it has always been.  A layout query
    // names the place in either case (the sub-array exists only in a buffer of a forward that asked)
    {
        const Carver before_stash = c;
        float* const stash = c.take<float>(9 * P, &off); note("sh_stash", off, 9 * P);
        if (sh_stash) *sh_stash = stash;
        else c = before_stash;
    }
    if (total) *total = c.total();
    if (n_names) *n_names = n;
    return g;
}

// The image-side state covers the frame's TILE-ROW WINDOW only (StpSettings::tile_y0 / tile_y1; the whole frame by default): a rank of a
// tile-row shard holds 1 / N of the per-pixel arrays and of the blend log (4.3 GB per frame at 4K), not the whole frame's.  The kernels keep
// indexing by frame coordinates (pixel id W * y + x, tile id gx * ty + tx): the sub-array pointers handed to them are shifted back by the
// window's first pixel row / tile, so that index -> address is unchanged inside the window and nothing outside it is ever touched (every
// loop over tiles runs over [gx * ty0, gx * ty1), every kernel's grid over the window's tiles).
ImageState carve_image(char* base, int W, int H, int ty0, int ty1, int log_depth, size_t* total, NamedOffset* names, int* n_names)
{
    Carver c(base);
    ImageState s{};
    size_t off;
    int n = 0;
    auto note = [&](const char* nm, size_t o, size_t cnt) { if (names) names[n] = {nm, o, cnt}; n++; };
    const int gx = (W + TILE - 1) / TILE;
    const int py0 = ty0 * TILE < H ? ty0 * TILE : H, py1 = ty1 * TILE < H ? ty1 * TILE : H;
    const size_t N = (size_t)W * (size_t)(py1 > py0 ? py1 - py0 : 0), T = (size_t)gx * (size_t)(ty1 > ty0 ? ty1 - ty0 : 0);
    s.header = c.take<uint32_t>(64, &off); note("header", off, 4); // first 256 bytes of the buffer, whatever the frame and the log's depth
    s.final_T = c.take<float>(N, &off); note("final_T", off, N);
    s.n_contrib = c.take<uint32_t>(N, &off); note("n_contrib", off, N);
    s.ranges = c.take<uint2>(T, &off); note("ranges", off, 2 * T);
    s.dbg_minmax = c.take<uint32_t>(2, &off); note("dbg_minmax", off, 2);
    s.tile_counts = c.take<uint32_t>(T, &off); note("tile_counts", off, T);
    s.tile_cursor = c.take<uint32_t>(T, &off); note("tile_cursor", off, T);
    s.bin_total = c.take<uint32_t>(2, &off); note("bin_total", off, 2);
    // tile_flags is ALWAYS there: a forward that records no log marks every tile "no valid log" (0xFFFFFFFF), so a backward
    // that is (wrongly) told a log exists -- e.g. after a render_depth forward -- replays nothing and re-sorts every tile
    // instead of reading a log that was never allocated.
    s.tile_flags = c.take<uint32_t>(T, &off); note("tile_flags", off, T);
    const size_t recs_per_tile = 4 * (size_t)blend_log_rows(log_depth) * 64; // 4 waves x (depth + spare) records x 64 lanes, 2 B each
    s.log_depth = log_depth;
    if (log_depth > 0) { // blend log of the recording forward: [tile][wave][record][lane]
        const size_t recs = T * recs_per_tile;
        s.blend_log = c.take<uint32_t>(recs / 2, &off); note("blend_log", off, recs);
    }
    if (total) *total = c.total();
    if (n_names) *n_names = n;
    if (base) { // frame-coordinate indexing (see above)
        const size_t pix0 = (size_t)W * (size_t)py0, tile0 = (size_t)gx * (size_t)ty0;
        s.final_T -= pix0; s.n_contrib -= pix0;
        s.ranges -= tile0; s.tile_counts -= tile0; s.tile_cursor -= tile0; s.tile_flags -= tile0;
        if (s.blend_log) s.blend_log -= tile0 * (recs_per_tile / 2);
    }
    return s;
}

BinningState carve_binning(char* base, size_t R, size_t* total, NamedOffset* names, int* n_names)
{
    Carver c(base);
    BinningState b{};
    size_t off;
    int n = 0;
    auto note = [&](const char* nm, size_t o, size_t cnt) { if (names) names[n] = {nm, o, cnt}; n++; };
    b.header = c.take<uint32_t>(64, &off); note("header", off, 4);
    b.point_list = c.take<uint32_t>(R, &off); note("point_list", off, R);
    b.point_list_unsorted = c.take<uint32_t>(R, &off); note("point_list_unsorted", off, R);
    b.keys = c.take<uint64_t>(R, &off); note("keys", off, R);
    b.keys_unsorted = c.take<uint64_t>(R, &off); note("keys_unsorted", off, R);
    b.sort_temp_bytes = sort_temp_bytes(R);
    b.sort_temp = c.take<char>(b.sort_temp_bytes);
    b.entA = c.take<float4>(R, &off); note("entA", off, 4 * R);
    b.entB = c.take<float4>(R, &off); note("entB", off, 4 * R);
    b.entC = c.take<float4>(R, &off); note("entC", off, 4 * R);
    b.entD = c.take<float4>(R, &off); note("entD", off, 4 * R);
    b.entF = c.take<float4>(R, &off); note("entF", off, 4 * R);
    if (total) *total = c.total();
    if (n_names) *n_names = n;
    return b;
}

// the tile-row window of a frame (fill_frame, and the size / layout queries of a window)
void clamp_tile_rows(int height, int& y0, int& y1)
{
    const int gy = (height + TILE - 1) / TILE;
    if (y1 <= 0) { y0 = 0; y1 = gy; return; }
    y0 = y0 < 0 ? 0 : (y0 > gy ? gy : y0);
    y1 = y1 > gy ? gy : y1;
    if (y1 < y0) y1 = y0;
}

// Which entry count a binning buffer was CARVED with, and which depth an image buffer's blend log.  A run-ahead forward (stp_forward) carves
// and launches on a capacity before num_rendered is known; the sub-arrays of the buffer then sit at the offsets of that capacity, not of the
// count stp_forward returns; and the blend log's depth is chosen per frame.  The backward and the introspection helpers are handed (pointer,
// num_rendered) only, as in the reference -- whose buffers are self-contained blobs.  Ours are too: every forward writes a HEADER into the
// buffer itself (device side, no extra launch: duplicate_kernel / frame_init_kernel) --
//     binning: first 256 bytes  {STP_HEADER_MAGIC_BINNING, capacity, ~capacity, 0}
//     image:   first 256 bytes  {STP_HEADER_MAGIC_IMAGE, depth of the blend log (0: none), ~depth, 0}
// -- and the HOST keeps a cache pointer -> value so that the backward of the same process needs no read-back (one entry per buffer address,
// overwritten whenever a forward carves that address again; least-recently-used entries are dropped in batches).  An entry also remembers the
// num_rendered of its forward, and the backward -- which is handed num_rendered -- takes it only if that matches: an address the allocator has
// re-issued for somebody else's buffer (a clone of another forward's buffers) does not get the previous tenant's layout.  A pointer the cache
// does not know -- a buffer that was cloned, copied, moved, or whose entry was dropped -- is looked up in the buffer's own header (one blocking
// 16-byte copy: the rare path); a buffer without a valid header is REFUSED (STP_ERR_INVALID_ARGUMENT) instead of being carved on a guess.
static std::mutex g_layout_mutex;
static LayoutCache g_layout, g_log_depth, g_stash;
void remember_layout(const void* binning, uint32_t count, int64_t R) { std::lock_guard<std::mutex> l(g_layout_mutex); g_layout.put(binning, count, R); }
void remember_log_depth(const void* image, uint32_t depth, int64_t R) { std::lock_guard<std::mutex> l(g_layout_mutex); g_log_depth.put(image, depth, R); }
void remember_stash(const void* geometry, bool stash, int64_t R) { std::lock_guard<std::mutex> l(g_layout_mutex); g_stash.put(geometry, stash ? 1u : 0u, R); }
// the header a forward left in the buffer: 0 and *value on success, else a negative STP_ERR_* (message set)
// (the copy is ordered on the CALLER's stream -- a clone made on a non-blocking stream is not visible to the null stream's copy -- and waited for;
//  introspection calls have no stream: they wait for the device first)
static int read_buffer_header(const uint32_t* dev_header, uint32_t magic, const char* what, uint32_t* value, hipStream_t st, bool have_stream)
{
    uint32_t h[4] = {0, 0, 0, 0};
    if (!have_stream) (void)hipDeviceSynchronize();
    if (hipMemcpyAsync(h, dev_header, sizeof(h), hipMemcpyDeviceToHost, have_stream ? st : nullptr) != hipSuccess ||
        hipStreamSynchronize(have_stream ? st : nullptr) != hipSuccess) { (void)hipGetLastError(); return fail(STP_ERR_HIP, std::string("could not read the header of the ") + what + " buffer"); }
    if (h[0] != magic || h[2] != ~h[1])
        return fail(STP_ERR_INVALID_ARGUMENT, std::string("the ") + what + " buffer does not carry a header of this library: it was not written by stp_forward (or has been overwritten)");
    *value = h[1];
    return 0;
}
// entries the binning buffer was carved for: cache, else the buffer's own header
int layout_of(const char* binning, uint32_t R, uint32_t* cap, hipStream_t st, bool have_stream)
{
    {
        std::lock_guard<std::mutex> l(g_layout_mutex);
        if (g_layout.get(binning, (int64_t)R, cap) && *cap >= R) return 0;
    }
    if (int rc = read_buffer_header(reinterpret_cast<const uint32_t*>(binning), STP_HEADER_MAGIC_BINNING, "binning", cap, st, have_stream)) return rc;
    if (*cap < R) return fail(STP_ERR_INVALID_ARGUMENT, "the binning buffer was carved for fewer entries than num_rendered");
    remember_layout(binning, *cap, (int64_t)R);
    return 0;
}

// depth the image buffer's blend log was carved with: cache, else the buffer's own header (whose offset does not depend on the depth)
int log_depth_of(const char* image, int64_t R, uint32_t* depth, hipStream_t st, bool have_stream)
{
    {
        std::lock_guard<std::mutex> l(g_layout_mutex);
        if (g_log_depth.get(image, R, depth)) return 0;
    }
    if (int rc = read_buffer_header(reinterpret_cast<const uint32_t*>(image), STP_HEADER_MAGIC_IMAGE, "image", depth, st, have_stream)) return rc;
    if (*depth != 0u && (int)*depth != blend_log_clamp_depth((int)*depth)) return fail(STP_ERR_INVALID_ARGUMENT, "the image buffer's header holds an impossible blend-log depth");
    remember_log_depth(image, *depth, R);
    return 0;
}

// does the geometry buffer carry an SH stash (stp_set_forward_sh_stash): cache, else the three words the stashing forward left in the buffer's status
// block.  A buffer without them -- a forward that did not ask, a library that did not know -- has none and takes the legacy path: nothing is refused.
int stash_of(const char* geometry, int P, int64_t R, bool* stash, hipStream_t st, bool have_stream)
{
    uint32_t v = 0;
    {
        std::lock_guard<std::mutex> l(g_layout_mutex);
        if (g_stash.get(geometry, R, &v)) { *stash = v != 0u; return 0; }
    }
    uint32_t h[4] = {0, 0, 0, 0};
    if (!have_stream) (void)hipDeviceSynchronize();
    if (hipMemcpyAsync(h, reinterpret_cast<const uint32_t*>(geometry) + STP_STASH_WORD, sizeof(h), hipMemcpyDeviceToHost, have_stream ? st : nullptr) != hipSuccess ||
        hipStreamSynchronize(have_stream ? st : nullptr) != hipSuccess) { (void)hipGetLastError(); return fail(STP_ERR_HIP, "could not read the status block of the geometry buffer"); }
    *stash = h[0] == STP_HEADER_MAGIC_STASH && h[1] == (uint32_t)P && h[2] == ~(uint32_t)P;
    remember_stash(geometry, *stash, R);
    return 0;
}

} // namespace stp

using namespace stp;

extern "C" {

size_t stp_geometry_buffer_size(int P, const StpSettings* settings)
{
    size_t total = 0;
    carve_geometry(nullptr, (size_t)P, settings ? requires_depth_along_ray(*settings) : true, &total);
    return total;
}
size_t stp_geometry_buffer_size_stash(int P, const StpSettings* settings)
{
    size_t total = 0;
    float* stash = nullptr;
    carve_geometry(nullptr, (size_t)P, settings ? requires_depth_along_ray(*settings) : true, &total, nullptr, nullptr, &stash);
    return total;
}
size_t stp_binning_buffer_size(int R)
{
    size_t total = 0;
    carve_binning(nullptr, (size_t)(R > 0 ? R : 0), &total);
    return total;
}
size_t stp_image_buffer_size(int width, int height)
{
    size_t total = 0;
    carve_image(nullptr, width, height, 0, (height + TILE - 1) / TILE, 0, &total);
    return total;
}

static size_t blend_log_bytes_of(int width, int height, int tile_y0, int tile_y1, int depth) // what a log of that depth adds to the window's image buffer
{
    clamp_tile_rows(height, tile_y0, tile_y1);
    size_t plain = 0, with_log = 0;
    carve_image(nullptr, width, height, tile_y0, tile_y1, 0, &plain);
    carve_image(nullptr, width, height, tile_y0, tile_y1, depth, &with_log);
    return with_log - plain;
}
size_t stp_blend_log_bytes_rows(int width, int height, int tile_y0, int tile_y1)
{
    return blend_log_bytes_of(width, height, tile_y0, tile_y1, blend_log_default_depth()); // (a frame nothing is known about: see stp_raster.h)
}
size_t stp_blend_log_bytes(int width, int height) { return stp_blend_log_bytes_rows(width, height, 0, 0); }
size_t stp_blend_log_bytes_depth(int width, int height, int tile_y0, int tile_y1, int depth) // depth <= 0: the deepest log a forward may carve
{
    return blend_log_bytes_of(width, height, tile_y0, tile_y1, depth > 0 ? blend_log_clamp_depth(depth) : blend_log_clamp_depth(1 << 30));
}

static int find_name(const NamedOffset* names, int n, const char* name, size_t* offset, size_t* count)
{
    for (int i = 0; i < n; i++)
        if (std::strcmp(names[i].name, name) == 0) {
            if (offset) *offset = names[i].offset;
            if (count) *count = names[i].count;
            return 0;
        }
    return fail(STP_ERR_INVALID_ARGUMENT, std::string("unknown sub-array name: ") + name);
}
int stp_geometry_layout(int P, const StpSettings* settings, const char* name, size_t* offset, size_t* count)
{
    NamedOffset names[24]; int n = 0;
    carve_geometry(nullptr, (size_t)P, settings ? requires_depth_along_ray(*settings) : true, nullptr, names, &n);
    return find_name(names, n, name, offset, count);
}
int stp_binning_layout(int R, const char* name, size_t* offset, size_t* count)
{
    NamedOffset names[16]; int n = 0;
    carve_binning(nullptr, (size_t)(R > 0 ? R : 0), nullptr, names, &n);
    return find_name(names, n, name, offset, count);
}
void stp_forget_buffer(const void* buffer)
{
    if (!buffer) return;
    std::lock_guard<std::mutex> l(g_layout_mutex);
    g_layout.map.erase(buffer);
    g_log_depth.map.erase(buffer);
    g_stash.map.erase(buffer);
}
int stp_blend_log_depth(const void* image_buffer)
{
    if (!image_buffer) return fail(STP_ERR_INVALID_ARGUMENT, "null image buffer");
    uint32_t d = 0;
    if (int rc = log_depth_of((const char*)image_buffer, -1, &d)) return rc;
    return (int)d;
}
int stp_binning_layout_count(const void* binning_buffer, int R)
{
    if (!binning_buffer) return fail(STP_ERR_INVALID_ARGUMENT, "null binning buffer");
    uint32_t cap = 0;
    if (int rc = layout_of((const char*)binning_buffer, (uint32_t)(R > 0 ? R : 0), &cap)) return rc;
    return (int)cap;
}
static int image_layout_of(int width, int height, int tile_y0, int tile_y1, int depth, const char* name, size_t* offset, size_t* count)
{
    NamedOffset names[16]; int n = 0;
    clamp_tile_rows(height, tile_y0, tile_y1);
    carve_image(nullptr, width, height, tile_y0, tile_y1, depth, nullptr, names, &n);
    return find_name(names, n, name, offset, count);
}
int stp_image_layout_rows(int width, int height, int tile_y0, int tile_y1, const char* name, size_t* offset, size_t* count)
{
    return image_layout_of(width, height, tile_y0, tile_y1, blend_log_default_depth(), name, offset, count);
}
int stp_image_layout(int width, int height, const char* name, size_t* offset, size_t* count)
{
    return stp_image_layout_rows(width, height, 0, 0, name, offset, count);
}
int stp_image_layout_depth(int width, int height, int tile_y0, int tile_y1, int log_depth, const char* name, size_t* offset, size_t* count)
{
    return image_layout_of(width, height, tile_y0, tile_y1, log_depth > 0 ? blend_log_clamp_depth(log_depth) : 0, name, offset, count);
}

} // extern "C"
