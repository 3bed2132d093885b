// gsr_api_common.h — what the translation units of the C ABI layer (gsr_api.hip, api_train.hip,
// api_mesh.hip, api_eval.hip, api_tnt.hip, api_data.hip, api_model.hip) share: the error report, the checking macros and the three host
// idioms of an entry point (pinned readback, per-stage event times, scratch carve).  Host code
// only; not part of the public ABI (include/gsr.h) and included by nothing else.
#pragma once

#include <mutex>
#include <vector>

#include "../../include/gsr.h"
#include "gsr_kernels.h"

#define GSR_INTERNAL __attribute__((visibility("hidden")))

namespace gsr {

// Sets the calling thread's gsr_last_error message and returns `code` (defined in gsr_api.hip,
// next to the thread_local string).
GSR_INTERNAL int fail(int code, const char* what, hipError_t e = hipSuccess);

#define GSR_CHECK(expr, what)                                     \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return fail(GSR_ERR_HIP, what, _e); \
    } while (0)

// GSR_CHECK for entry points with a `debug` argument: debug synchronises `stream` after each step
#define GSR_TRY(expr, what)                                       \
    do {                                                          \
        GSR_CHECK(expr, what);                                    \
        if (debug) GSR_CHECK(hipStreamSynchronize(stream), what); \
    } while (0)

// The forward's one host synchronisation (K sizes the binning buffer, as
// rasterizer_impl.cu:384) waits on an event recorded right after the counts
// are copied into pinned host memory, not on the whole stream: work queued
// behind the event (the depth sort) keeps the GPU busy while the host reads
// K and allocates.  The pinned words and the event come from a process-wide
// per-device pool: a forward leases a slot for its readback and returns it,
// so slots are created only up to the number of concurrent forwards and are
// reused by every thread (no per-thread slots left behind by short-lived
// threads; no hipHostMalloc / hipHostFree, which synchronise, per call).
struct HostReadback {
    uint32_t* pinned = nullptr;  // 8 words
    hipEvent_t ev = nullptr;
    int dev = 0;
};
constexpr int kMaxReadbackDevices = 64;

class GSR_INTERNAL ReadbackPool {
  public:
    hipError_t acquire(HostReadback*& rb) {
        rb = nullptr;
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= kMaxReadbackDevices) return hipErrorInvalidDevice;
        {
            std::lock_guard<std::mutex> lock(m_);
            if (!free_[dev].empty()) {
                rb = free_[dev].back();
                free_[dev].pop_back();
                return hipSuccess;
            }
        }
        auto* slot = new HostReadback();
        slot->dev = dev;
        if ((e = hipHostMalloc(reinterpret_cast<void**>(&slot->pinned), 8 * sizeof(uint32_t),
                               hipHostMallocDefault)) != hipSuccess) {
            delete slot;
            return e;
        }
        if ((e = hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming)) != hipSuccess) {
            (void)hipHostFree(slot->pinned);
            delete slot;
            return e;
        }
        rb = slot;
        return hipSuccess;
    }
    void release(HostReadback* rb) {
        std::lock_guard<std::mutex> lock(m_);
        free_[rb->dev].push_back(rb);
    }

  private:
    std::mutex m_;
    std::vector<HostReadback*> free_[kMaxReadbackDevices];
};
GSR_INTERNAL extern ReadbackPool g_readback_pool;  // (gsr_api.hip)

namespace {

// 256-B alignment of the carve base (callbacks may return any alignment)
inline void* aligned_base(void* p) {
    return reinterpret_cast<void*>(align_up(reinterpret_cast<uintptr_t>(p), 256));
}

// A pool slot leased for one call's readbacks, returned on every exit path: begin() leases it,
// copy() queues a device-to-host copy into pinned word `word`, commit() records the slot's event
// behind the copies queued so far and wait() blocks the host on that event; then rb[k] is word k.
// Work queued between commit() and wait() runs while the host waits, and copy / commit / wait may
// repeat.  An exit with a copy queued and no event recorded behind it drains the stream instead;
// a slot whose copies cannot be proven finished is never returned to the pool (another call could
// otherwise lease it while a late copy lands).
class Readback {
  public:
    Readback() = default;
    Readback(const Readback&) = delete;
    Readback& operator=(const Readback&) = delete;
    hipError_t begin(hipStream_t stream) {
        stream_ = stream;
        return g_readback_pool.acquire(rb_);
    }
    hipError_t copy(int word, const void* src, size_t bytes) {
        state_ = kQueued;
        return hipMemcpyAsync(rb_->pinned + word, src, bytes, hipMemcpyDeviceToHost, stream_);
    }
    hipError_t commit() {
        const hipError_t e = hipEventRecord(rb_->ev, stream_);
        if (e == hipSuccess) state_ = kRecorded;
        return e;
    }
    hipError_t wait() { return hipEventSynchronize(rb_->ev); }
    uint32_t operator[](int word) const { return rb_->pinned[word]; }
    ~Readback() {
        if (!rb_) return;
        hipError_t e = hipSuccess;
        if (state_ == kRecorded) e = hipEventSynchronize(rb_->ev);
        else if (state_ == kQueued) e = hipStreamSynchronize(stream_);
        if (e == hipSuccess) g_readback_pool.release(rb_);  // (else the slot is leaked, not reused)
    }

  private:
    enum State { kIdle, kQueued, kRecorded };
    HostReadback* rb_ = nullptr;
    hipStream_t stream_ = nullptr;
    State state_ = kIdle;
};

// Optional per-stage GPU times of one call (measurement only; the float stage_ms[8] of gsr.h): a
// begin and an end event around each stage, read by collect() after the call's last kernel.
// Construction zeroes stage_ms; with stage_ms NULL no event is created or recorded.
class StageTimes {
  public:
    static constexpr int kStages = 7;
    StageTimes(float* stage_ms, hipStream_t stream) : ms_(stage_ms), stream_(stream) { zero(); }
    StageTimes(const StageTimes&) = delete;
    StageTimes& operator=(const StageTimes&) = delete;
    hipError_t begin(int k) {
        if (!ms_) return hipSuccess;
        hipError_t e = hipEventCreate(&ev_[k][0]);
        if (e == hipSuccess) e = hipEventCreate(&ev_[k][1]);
        if (e == hipSuccess) e = hipEventRecord(ev_[k][0], stream_);
        used_[k] = e == hipSuccess;
        return e;
    }
    hipError_t end(int k) { return ms_ ? hipEventRecord(ev_[k][1], stream_) : hipSuccess; }
    hipError_t collect() {
        if (!ms_) return hipSuccess;
        hipError_t e = hipStreamSynchronize(stream_);
        zero();
        for (int k = 0; k < kStages && e == hipSuccess; k++)
            if (used_[k]) e = hipEventElapsedTime(&ms_[k], ev_[k][0], ev_[k][1]);
        return e;
    }
    ~StageTimes() {
        for (auto& p : ev_)
            for (hipEvent_t x : p)
                if (x) (void)hipEventDestroy(x);
    }

  private:
    void zero() {
        if (ms_)
            for (int k = 0; k < kStages + 1; k++) ms_[k] = 0.f;
    }
    float* ms_;
    hipStream_t stream_;
    hipEvent_t ev_[kStages][2] = {};
    bool used_[kStages] = {};
};

// one launch as stage k of `times` (a stage of several steps brackets them with begin / end itself)
#define GSR_TIMED(times, k, expr, what)        \
    do {                                       \
        GSR_CHECK((times).begin(k), "event");  \
        GSR_CHECK(expr, what);                 \
        GSR_CHECK((times).end(k), "event");    \
    } while (0)

// Scratch carve: the size pass of `carve` (base NULL), the allocation, and the carve proper at the
// block's aligned base.  `args` are carve's arguments after the base.  GSR_OK, or GSR_ERR_ALLOC
// with `what` as the message when the callback returns NULL.
template <class... P, class... A>
int carve_alloc(gsr_alloc_fn alloc, void* ctx, const char* what, size_t (*carve)(void*, P...), A&&... args) {
    void* buf = alloc(ctx, carve(nullptr, args...));
    if (!buf) return fail(GSR_ERR_ALLOC, what);
    carve(aligned_base(buf), args...);
    return GSR_OK;
}

// carve_alloc for a carve whose last parameter, after `args`, is `Carver* tmp`: where its forward-only
// fields go.  With `scratch` they come out of a block of their own, requested after the buffer itself and
// carved from its aligned base; with `scratch` NULL tmp is NULL and they sit at the end of the buffer.
template <class Carve, class... A>
int carve_alloc_scratch(gsr_alloc_fn alloc, void* ctx, const char* what, gsr_alloc_fn scratch, void* scratch_ctx,
                        Carve carve, A&&... args) {
    Carver tmp(nullptr);
    Carver* t = scratch ? &tmp : nullptr;
    void* buf = alloc(ctx, carve(nullptr, args..., t));
    if (!buf) return fail(GSR_ERR_ALLOC, what);
    if (scratch) {
        void* sbuf = scratch(scratch_ctx, tmp.off + 256);
        if (!sbuf) return fail(GSR_ERR_ALLOC, "scratch allocation failed");
        tmp = Carver(aligned_base(sbuf));
    }
    carve(aligned_base(buf), args..., t);
    return GSR_OK;
}

}  // namespace
}  // namespace gsr
