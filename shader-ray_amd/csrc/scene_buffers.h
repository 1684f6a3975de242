// scene_buffers.h -- the device allocations a scene owns, and the one rule that says when a buffer launches have read may be
// reused or freed.  scene_internal.h's struct shray_scene, dispatch_order.h and view_cache.h hold these by value.
// Host-only, internal to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <utility>
#include <vector>

namespace shray {

struct DeviceBuffer {
    void *p = nullptr;
    ~DeviceBuffer() { release(); }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
    }
    hipError_t upload(const void *src, size_t bytes)
    {
        release();
        if (bytes == 0)
            bytes = 16;   // keep a valid pointer for empty scenes
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess)
            return e;
        if (src)
            return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        e = hipMemset(p, 0, bytes);
        // the fill runs on the null stream, which non-blocking streams do not wait for: finish it here, before
        // any kernel or copy on another stream can touch the buffer
        return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
    }
    // `bytes` of device memory, uninitialised, or a copy of device memory (shray_scene_create_from_device; null stream)
    hipError_t reserve(size_t bytes)
    {
        release();
        return hipMalloc(&p, bytes ? bytes : 16);
    }
    hipError_t copy_of(const void *device_src, size_t bytes)
    {
        const hipError_t e = reserve(bytes);
        return (e != hipSuccess || !bytes) ? e : hipMemcpyAsync(p, device_src, bytes, hipMemcpyDeviceToDevice, nullptr);
    }
};

// shray_render_batch_device: per-frame FrameViews travel through a small ring of slots (pinned staging -> device); a slot is
// reused only after the launch that read it has finished.  Launch number q (shray_scene::launch_seq, 1-based) uses slot
// (q - 1) % kBatchSlots and first waits for the launch that used it before (render_api.hip: launch_stack_views).
constexpr int kBatchSlots = 16;

// THE rule for every buffer that launches read: launch `mark` is known to be over while launch `seq` is being enqueued once
// kBatchSlots further launches have been enqueued -- seq's slot wait has returned, and with it every launch up to
// seq - kBatchSlots is over (each was waited for by its slot's next user).  What was given to, or taken from, the launches up
// to `mark` may then be rewritten, handed out again or freed, and nothing has to synchronise with the device to know it.
inline bool launch_is_over(unsigned long long mark, unsigned long long seq) { return seq >= mark + kBatchSlots; }

// Buffer pairs that were set aside while launches might still read them: an evicted dispatch order's (cost, ring), a view-cache
// entry's (rays, sky).  `size` is what the pair was allocated for -- patches or pixels, the list does not care --, `set_aside_at`
// the scene's launch number at that moment: the pair is "aged" once that launch is over.  Dropping an entry frees its buffers
// (hipFree waits for the device), so WHEN the two callers take and free stays each one's own policy.
struct RetiredPairs {
    struct Pair {
        DeviceBuffer a, b;
        size_t size = 0;
        unsigned long long set_aside_at = 0;
    };
    std::vector<std::unique_ptr<Pair>> held;

    // takes *a and *b (left null) into the list
    void push(void **a, void **b, size_t size, unsigned long long seq)
    {
        std::unique_ptr<Pair> r(new Pair);
        std::swap(r->a.p, *a);
        std::swap(r->b.p, *b);
        r->size = size;
        r->set_aside_at = seq;
        held.push_back(std::move(r));
    }
    // the first aged pair whose size satisfies fits(size) leaves the list into *a, *b (both null before); returns its size, 0: none
    template <typename Fits>
    size_t take_first(unsigned long long seq, Fits &&fits, void **a, void **b)
    {
        for (size_t k = 0; k < held.size(); k++) {
            Pair &r = *held[k];
            if (launch_is_over(r.set_aside_at, seq) && fits(r.size)) {
                const size_t size = r.size;
                std::swap(*a, r.a.p);
                std::swap(*b, r.b.p);
                held.erase(held.begin() + (long)k);
                return size;
            }
        }
        return 0;
    }
    // frees aged pairs, in the list's order, while more than `keep` pairs are held
    void free_aged(unsigned long long seq, size_t keep = 0)
    {
        for (size_t k = 0; held.size() > keep && k < held.size();) {
            if (launch_is_over(held[k]->set_aside_at, seq))
                held.erase(held.begin() + (long)k);
            else
                k++;
        }
    }
    size_t total_size() const
    {
        size_t sum = 0;
        for (const auto &r : held)
            sum += r->size;
        return sum;
    }
};

}   // namespace shray
