// Frames delivered to host memory (include/course5_hip.h): c5_render, and the ring of c5_render_host_async frames that
// a copy stream carries to the caller's buffers behind the render stream.
#include "context.hpp"

using namespace c5api;

extern "C" {

// (the file's helpers are declared inside extern "C": their unmangled names are part of the library's symbol table)
namespace {
bool is_pinned(const void* p) {
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // an ordinary (pageable) pointer: not an error here
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

// Device image -> host.  Pinned destination: one asynchronous copy.  Pageable destination: 4 MB chunks
// through two pinned staging buffers, each copied out on the host threads while the next is in flight
// (a plain hipMemcpy into pageable memory ran at 7.7 GB/s: 4.5 ms for a 2400x1800 image).
int copy_image_to_host(c5_context* ctx, const void* dev, void* host, size_t bytes) {
    hipStream_t cs = ctx->copy_stream;
    if (is_pinned(host)) {
        C5_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, cs));
        C5_HIP(ctx, hipStreamSynchronize(cs));
        return C5_OK;
    }
    for (int k = 0; k < 2; ++k)
        if (!ctx->stage[k]) C5_HIP(ctx, hipHostMalloc(&ctx->stage[k], kStageChunk, hipHostMallocDefault));
    const size_t n_chunks = (bytes + kStageChunk - 1) / kStageChunk;
    for (size_t i = 0; i <= n_chunks; ++i) {
        if (i < n_chunks) {
            const size_t off = i * kStageChunk, n = std::min(kStageChunk, bytes - off);
            C5_HIP(ctx, hipMemcpyAsync(ctx->stage[i & 1], static_cast<const char*>(dev) + off, n, hipMemcpyDeviceToHost, cs));
            C5_HIP(ctx, hipEventRecord(ctx->stage_ev[i & 1], cs));
        }
        if (i > 0) {
            const size_t off = (i - 1) * kStageChunk, n = std::min(kStageChunk, bytes - off);
            C5_HIP(ctx, hipEventSynchronize(ctx->stage_ev[(i - 1) & 1]));
            c5::parallel_copy(static_cast<char*>(host) + off, ctx->stage[(i - 1) & 1], n);
        }
    }
    return C5_OK;
}
}  // namespace

int c5_render(c5_context* ctx, float* out_host) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (!out_host) return fail(ctx, C5_ERR_INVALID, "null output pointer");
    if (ctx->hr_count) return fail(ctx, C5_ERR_STATE, "c5_render while c5_render_host_async frames are outstanding");
    for (int attempt = 0; attempt < 3; ++attempt) {
        int rc = enqueue_frame(ctx, ctx->out.as<float2>());
        if (rc) return rc;
        rc = c5_synchronize(ctx);
        if (rc == C5_RETRY) continue;
        if (rc) return rc;
        const size_t bytes = image_bytes(ctx);
        return copy_image_to_host(ctx, ctx->out.ptr, out_host, bytes);
    }
    return fail(ctx, C5_ERR_STATE, "entry buffer kept overflowing");
}

namespace {
// Copy the local strip (device) to the host: either as it is, or every row tile to its place in the full image.
int enqueue_strip_copy(c5_context* ctx, const void* strip, float* host, bool into_full_frame) {
    const c5::ImageParams& im = ctx->im;
    const size_t row_bytes = static_cast<size_t>(im.res_x) * 2 * sizeof(float);
    hipStream_t cs = ctx->copy_stream;
    if (!into_full_frame) {
        C5_HIP(ctx, hipMemcpyAsync(host, strip, row_bytes * im.n_local_rows, hipMemcpyDeviceToHost, cs));
        return C5_OK;
    }
    char* const frame = reinterpret_cast<char*>(host);
    const char* const src = static_cast<const char*>(strip);
    if (im.world == 1) {  // one contiguous block of rows
        C5_HIP(ctx, hipMemcpyAsync(frame + row_bytes * im.row_begin, src, row_bytes * im.n_local_rows, hipMemcpyDeviceToHost, cs));
        return C5_OK;
    }
    // cyclic tiles: local tile t is global tile t * world + rank (counted from row_begin): ONE 2-D copy for the
    // whole tiles (a "row" of the 2-D copy = one tile of tile_rows image rows) and one for a short last tile
    const size_t tile_bytes = row_bytes * im.tile_rows;
    const int whole = im.n_local_rows / im.tile_rows, rest = im.n_local_rows - whole * im.tile_rows;
    char* const first = frame + row_bytes * im.row_begin + tile_bytes * im.rank;
    if (whole > 0)
        C5_HIP(ctx, hipMemcpy2DAsync(first, tile_bytes * im.world, src, tile_bytes, tile_bytes, static_cast<size_t>(whole),
                                     hipMemcpyDeviceToHost, cs));
    if (rest > 0)
        C5_HIP(ctx, hipMemcpyAsync(first + tile_bytes * im.world * whole, src + tile_bytes * whole, row_bytes * rest,
                                   hipMemcpyDeviceToHost, cs));
    return C5_OK;
}

int render_host_async(c5_context* ctx, float* out_host, bool into_full_frame) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (!out_host) return fail(ctx, C5_ERR_INVALID, "null output pointer");
    if (ctx->hr_count >= C5_HOST_RING)
        return fail(ctx, C5_ERR_STATE, "%d frames outstanding: call c5_render_host_wait first", C5_HOST_RING);
    int rc = bind_device(ctx);
    if (rc) return rc;
    c5_context::HostFrame& h = ctx->hring[ctx->hr_next];
    const size_t bytes = image_bytes(ctx);
    C5_HIP(ctx, h.img.ensure(((bytes + 8191) / 8192) * 8192));
    C5_HIP(ctx, h.counters.ensure(kCountersBytes));
    // (the slot's previous copy is complete: its c5_render_host_wait has returned)
    rc = enqueue_frame(ctx, h.img.as<float2>(), h.counters.as<c5::FrameCounters>());
    if (rc) return rc;
    C5_HIP(ctx, hipEventRecord(h.rendered, ctx->stream));
    C5_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, h.rendered, 0));
    rc = enqueue_strip_copy(ctx, h.img.ptr, out_host, into_full_frame);
    if (rc) return rc;
    // THIS frame's failure words (walk_overflow, entry_overflow: adjacent in shard 0 of its own counters, cleared by its
    // own first kernel): the wait can tell without touching the render stream, and no frame enqueued later adds to them.
    // (Rounds 2-3 copied the context's cumulative sticky words here: a snapshot that depended on how a NULL-stream
    // hipMemset of c5_create was ordered against this copy stream, and that a later frame's raster could add to.)
    static_assert(offsetof(c5::FrameCounters, entry_overflow) == offsetof(c5::FrameCounters, walk_overflow) + sizeof(unsigned) &&
                  offsetof(c5::FrameCounters, overlap_rays) == offsetof(c5::FrameCounters, walk_overflow) + 2 * sizeof(unsigned), "status = adjacent words");
    C5_HIP(ctx, hipMemcpyAsync(h.status, reinterpret_cast<const char*>(h.counters.ptr) + offsetof(c5::FrameCounters, walk_overflow),
                               kStatusWords * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->copy_stream));
    C5_HIP(ctx, hipEventRecord(h.copied, ctx->copy_stream));
    ctx->hr_next = (ctx->hr_next + 1) % C5_HOST_RING;
    ctx->hr_count += 1;
    return C5_OK;
}
}  // namespace

int c5_render_host_async(c5_context* ctx, float* out_host) { return render_host_async(ctx, out_host, false); }
int c5_render_frame_rows_async(c5_context* ctx, float* frame_host) { return render_host_async(ctx, frame_host, true); }

int c5_render_host_wait(c5_context* ctx) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (ctx->hr_count == 0) return fail(ctx, C5_ERR_STATE, "no c5_render_host_async frame is outstanding");
    int rc = bind_device(ctx);
    if (rc) return rc;
    c5_context::HostFrame& h = ctx->hring[ctx->hr_head];
    C5_HIP(ctx, hipEventSynchronize(h.copied));
    ctx->hr_head = (ctx->hr_head + 1) % C5_HOST_RING;
    ctx->hr_count -= 1;
    if (ctx->hr_retry_left > 0) {  // enqueued before an overflow was noticed: rendered with the buffers that were too small
        ctx->hr_retry_left -= 1;
        return fail(ctx, C5_RETRY, "frame was enqueued before an internal buffer was grown: render it again");
    }
    if (h.status[0] == 0 && h.status[1] == 0 && h.status[2] == 0) return C5_OK;
    // this frame failed: settle it (waits for the render stream, grows what was too small); every frame enqueued behind
    // it used the same buffers
    const unsigned lost = h.status[0], refused = h.status[1], overlapping = h.status[2];
    ctx->hr_retry_left = ctx->hr_count;
    rc = wait_and_collect(ctx);
    if (rc == C5_OK)
        rc = fail(ctx, C5_RETRY, "frame incomplete (%u boundary entries without a pool slot, %u rays over the step bound, %u rays through "
                  "interpenetrating cells by its own counters; the context's cumulative words read %u / %u / %u when the stream was waited "
                  "for; pool now %lld records): render again",
                  refused, lost, overlapping, ctx->host_sticky[0], ctx->host_sticky[1], ctx->host_sticky[2],
                  static_cast<long long>(ctx->slots[0].entry_capacity));
    return rc;
}

int c5_host_alloc(c5_context* ctx, size_t bytes, void** out_ptr) {
    if (!ctx || !out_ptr) return fail(ctx, C5_ERR_INVALID, "null argument");
    int rc = bind_device(ctx);
    if (rc) return rc;
    *out_ptr = nullptr;
    // portable: several contexts (one per GPU) copy their rows into the same frame (c5_render_frame_rows_async)
    C5_HIP(ctx, hipHostMalloc(out_ptr, bytes ? bytes : 1, hipHostMallocPortable));
    return C5_OK;
}

int c5_host_free(c5_context* ctx, void* ptr) {
    if (!ctx) return fail(nullptr, C5_ERR_INVALID, "null context");
    if (!ptr) return C5_OK;
    C5_HIP(ctx, hipHostFree(ptr));
    return C5_OK;
}

}  // extern "C"
