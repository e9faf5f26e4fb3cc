// ------------------------------------------------------------------------------------------
// Derivative renders, host side: what derivative_setup.hip, scalar_derivatives.hip, geometry_derivatives.hip and
// ray_matrix.hip share (the kernels: scalar_derivative_kernels.hip, geometry_derivative_kernels.hip, ray_matrix_kernels.hip).
// A derivative is the frame c5_render would produce now, differentiated.  All share one per-view setup on the context's
// stream into slot 0's buffers - records of "integration" 0 (the reference's order, whatever the option says), whole rays (no
// "depth_split"), the entry lists, the solid mask; or bin_sort_resolve's lists - then run their own kernels.  They leave the
// options alone and the frames' statistics and failure words too (counters and sticky words of their own); the slot's
// per-view data are marked stale, so the next frame builds its own ("view_cache").
//
// The entry heads.  After the setup slot 0's per-pixel entry heads are live.  A walk either leaves them in place (the
// adjoint's pass 1, an exact pass E, the products' pass A, the ray matrix's count: for the walk that follows) or hands them
// back cleared, and FrameSlot::head_clean tells the next setup whether it may skip its memset.  The view keeps that state
// and commit_derivative hands it to the slot: a launch that may hand the heads back takes its keep_entries from
// DerivativeView::keep, one that always does says keep(false), and one that never does says nothing.
// ------------------------------------------------------------------------------------------
#pragma once
#include "context.hpp"

namespace c5api __attribute__((visibility("hidden"))) {

struct DerivativeView {
    bool no_cells = false;  // a scene of solids only: nothing was set up (there is no cell to differentiate)
    bool bin_sort = false;  // "algorithm" 1: bin_sort_resolve's lists in ctx->offs64 / ctx->segs; else the walk's in w
    bool heads_cleared = false;  // the last walk launched handed the heads back cleared (the lists: as the setup found them)
    hipStream_t s = nullptr;        // the context's stream: everything of a derivative runs on it
    int64_t n_px = 0, padded = 0;   // pixels of the context's rows; rounded up to the scan's 1024
    const int32_t* perm = nullptr;  // cell_perm on the device (device order -> the caller's), or nullptr: the identity
    const uint32_t* mask = nullptr;  // solid-marked pixels, or nullptr
    c5::WalkParams w{};
    c5::ResolveParams r{};     // (bin_sort) what every *_resolve kernel reads
    c5::MotionGeometry geo{};  // the cells' vertices in view space

    // keep_entries of the walk about to be launched: it leaves the heads in place where another walk follows
    bool keep(bool more_follows) {
        heads_cleared = !more_follows;
        return more_follows;
    }
};

// ---- derivative_setup.hip
int setup_derivative(c5_context* ctx, DerivativeView& v);
// After a derivative's kernels: its status words to the host for finish_adjoint, at the next wait, and the heads' state to
// the slot.
int commit_derivative(c5_context* ctx, const DerivativeView& v, const char* what);
// commit_derivative for a call that ran pass S: the misfit word (on the device: the scalar sums' or the vertex sums')
// travels to the host behind the status words
int commit_exact(c5_context* ctx, const DerivativeView& v, const unsigned* misfits, const char* what);
// The adjoint's parameters over the view's walk, with Lambda's buffer (pass 1 -> pass 2); the weights and where the sums
// go are the caller's to fill in.
int adjoint_params(c5_context* ctx, const DerivativeView& v, c5::AdjointParams& ap);
// The exact sums' word width m for an image of res_x x res_y pixels (exact_sum.hpp), refused where it leaves too few bits.
// ctx may be null (the pure host functions).
int exact_word_bits(c5_context* ctx, int res_x, int res_y, int& m);
// nothing but solids: n tangent images do not depend on any cell
int zero_tangents(c5_context* ctx, const DerivativeView& v, int n, float2* out);
// Batches: the chunk width (4 or 8 directions / upstream images per walk; "batch_width").
int batch_width(const c5_context* ctx, int n);

// Row j of a caller's [.][stride] array, or the null pointer the caller gave
template <class T>
T* row_of(T* p, int64_t j, int64_t stride) { return p ? p + j * stride : nullptr; }

// n items in chunks of up to `width`: for (const Chunk c : Chunks{n, width}); c.more is what DerivativeView::keep wants
struct Chunk {
    int k0, n_used;
    bool more;  // another chunk follows
};
struct Chunks {
    int n, width;
    struct Iterator {
        int k0, n, width;
        Chunk operator*() const { return {k0, std::min(width, n - k0), n - k0 > width}; }
        void operator++() { k0 += width; }
        bool operator!=(const Iterator&) const { return k0 < n; }
    };
    Iterator begin() const { return {0, n, width}; }
    Iterator end() const { return {n, n, width}; }
};

// ---- the exact passes (pass E: the exponents; pass S: the words against them) of every family of exact sums
enum ExactFlags : unsigned {
    kBounds = 1,      // pass E into x.exps, cleared here first
    kSums = 2,        // pass S against x.exps into x.words, cleared here first
    kHaveLambda = 4,  // Lambda is there (an earlier image's pass 1, or a product's pass A): pass 1 is not launched
    kKeep = 8,        // the walk's pass S leaves the entry heads in place (another image follows)
    kFirst = 16,      // the misfit word is cleared with the words (the call's first pass S)
};

// Image k of a call of n_total upstream images through passes E and S: pass 1 only before the call's first image unless
// Lambda is there, the heads kept unless it is the last, the misfit word cleared at the first.
inline unsigned exact_image_flags(int k, int n_total, bool have_lambda) {
    return kBounds | kSums | (have_lambda || k > 0 ? kHaveLambda : 0u) | (k + 1 < n_total ? kKeep : 0u) | (k == 0 ? kFirst : 0u);
}

// The exact passes over the view for one upstream image.  A family (the adjoint, the Gauss-Newton diagonal, the
// Hessian-vector render, the vertex adjoint) brings its sums' type and four launchers over parameters it has set up:
// clear(v, x, n_cells, flags) (kBounds: the exponents; kSums: the words, and with kFirst the misfit word), pass1(v),
// walk(v, x, sums), resolve(v, x, sums).  Without pass S the heads stay in place, and the next per-view setup clears them.
template <class Family>
void exact_passes(c5_context* ctx, DerivativeView& v, const Family& f, typename Family::Sums x, unsigned flags) {
    const bool bounds = flags & kBounds, sums = flags & kSums;
    f.clear(v, x, ctx->n_cells, flags);
    if (v.bin_sort) {
        if (bounds) f.resolve(v, x, false);
        if (sums) f.resolve(v, x, true);
        return;
    }
    if (!(flags & kHaveLambda)) f.pass1(v);
    if (bounds) f.walk(v, x, false);
    if (sums) {
        x.keep_entries = v.keep(flags & kKeep);
        f.walk(v, x, true);
    }
}

// ---- the entry points' checks and the host-pointer forms

// What the derivative entry points check before anything else, in this order: the context; a batch's size; the call's own
// pointers (`required_ok`, and `per_cell_ok` where the grid has cells); no c5_render_host_async frame outstanding; and for
// the host-pointer forms the image, after which the device is bound.
struct DerivativeCall {
    const char* name;         // as the messages spell it: "c5_render_tangent_batch" also for its _device form
    bool host;                // a host-pointer form
    int n;                    // a batch's size (1: not a batch)
    const char* batch_of;     // "direction" / "upstream image"
    bool required_ok, per_cell_ok;
    const char* pointer_msg;
    bool refuse_async = true;
};
int check_derivative(c5_context* ctx, const DerivativeCall& c);

// One block of a host-pointer derivative call's staging buffer: uploaded from `src` before the work, downloaded to `dst`
// after it (either may be null).  dev: its place on the device, or nullptr where the caller gave neither - the enqueue
// then sees the null pointer the caller passed.
struct Staged {
    const void* src;
    void* dst;
    size_t bytes;
    char* dev = nullptr;
    template <class T>
    T* as() const { return reinterpret_cast<T*>(dev); }
};

// The host-pointer form of a derivative: the blocks laid out in the staging buffer (256-byte aligned), the uploads on the
// context's stream, `enqueue` and c5_synchronize - again while the entry pool had to grow (C5_RETRY) - and the downloads.
template <size_t N, class Enqueue>
int run_staged(c5_context* ctx, const char* what, Staged (&blocks)[N], Enqueue enqueue) {
    auto room = [](const Staged& b) { return (b.bytes + 255) / 256 * 256; };
    size_t total = 0;
    for (const Staged& b : blocks) total += room(b);
    C5_HIP(ctx, ctx->deriv.io.ensure(total + 256));
    char* at = ctx->deriv.io.as<char>();
    for (Staged& b : blocks) {
        if (b.src || b.dst) b.dev = at;
        at += room(b);
        if (b.src && b.bytes > 0) C5_HIP(ctx, hipMemcpyAsync(b.dev, b.src, b.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    for (int attempt = 0; attempt < 3; ++attempt) {
        int rc = enqueue();
        if (rc) return rc;
        rc = c5_synchronize(ctx);
        if (rc == C5_RETRY) continue;
        if (rc) return rc;
        for (const Staged& b : blocks)
            if (b.dst && b.bytes > 0) C5_HIP(ctx, hipMemcpy(b.dst, b.dev, b.bytes, hipMemcpyDeviceToHost));
        return C5_OK;
    }
    return fail(ctx, C5_ERR_STATE, "%s: entry buffer kept overflowing", what);
}

inline size_t cells_bytes(const c5_context* ctx) { return static_cast<size_t>(ctx->n_cells) * sizeof(double); }

}  // namespace c5api
