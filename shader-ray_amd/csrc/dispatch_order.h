// dispatch_order.h -- the dispatch order of the convergent batch kernels, per launch shape (dispatch_order.hip): what a scene
// keeps for one shape, and the two steps of a launch that use it (render_api.hip: launch_stack_views).
// Host-only, internal to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.h"
#include "scene_buffers.h"

struct shray_scene;

namespace shray {

// Dispatch order of the convergent batch kernels: heaviest patches first, learnt from the frames before.
// A frame's few long-running waves (rays grazing the silhouette, caught between the ears) last as long as a whole
// frame of average waves; in row-major order many of them start when a launch is almost over, and a launch that is
// not followed at once by another -- a rank's share of a step on 8 GPUs, the last launches of a short run -- waits
// for them with the machine empty (profiles/history/r03/dispatch_order_ab.txt: a rank's 20-frame share at N = 8 takes 0.64
// instead of 0.91 ms).  The waves of the launches a re-sort follows (of every one-frame launch) leave their running
// time in `cost` (per patch, the longest); every few launches a one-workgroup kernel behind the launch, on its
// stream, turns the costs into the next permutation (launch_dispatch_order); launches take a permutation up once it
// is complete (`ready[entry]`, polled: no other stream ever waits for it, and no stream of the library's own competes
// with the caller's for hardware queues).
// A ring entry is never rewritten while a launch may still read it: every entry remembers the last launch that was
// given it (`last_reader`, in the scene's launch numbers) and is written again only when that launch is known to be
// over (scene_buffers.h: launch_is_over) and when it is neither the entry new launches read nor one that is still being
// written; otherwise the re-sort is skipped (the next due launch tries again).
struct DispatchOrder {
    static constexpr int kRing = kBatchSlots + 2;
    DeviceBuffer cost, ring;            // 2 n words (costs, the order kernel's copy); kRing * n words
    size_t capacity = 0;                // patches the two buffers were sized for
    uint32_t n = 0;                     // 0: the slot holds no shape
    long long key[8] = {};              // the launch shape the costs belong to
    int current = -1;                   // ring entry new launches read; -1: none yet (identity)
    int written = -1;                   // ring entry the order kernel last wrote (or is writing)
    int pending_first = 0, pending_count = 0;   // entries pending_first .. written (ring order) are enqueued, not known complete
    unsigned long long launches = 0;    // since the shape was set
    hipStream_t written_on = nullptr;   // the stream the pending order kernels were enqueued on: launches enqueued on it
                                        // afterwards are ordered behind them and may read `written` at once
    hipEvent_t ready[kRing] = {};       // recorded behind the order kernel that wrote the entry
    unsigned long long last_reader[kRing] = {};   // scene launch number of the last launch given the entry (0: none)
    unsigned long long last_use = 0;    // (of the scene's dispatch clock: the least recently used shape makes room)
};

// What launch_stack_views finds out about a launch before it picks the stack kernel's instance; whether the launch reads a
// dispatch order depends on the same facts.
struct LaunchKind {
    bool all_plain;   // every frame is a plain which == 0 frame (device_types.h: plain_view)
    bool all_metal;   // every frame's diffuse colour is zero in some component (metal)
    bool pair;        // the instances that test both children of a node per turn (render_api.hip: pair_policy)
    bool deal;        // the instances with the dealt leaf stage (leaf_stage_policy)
    bool tally;       // the tallying twins (shray_render_counters_timed)
};

// A launch's step 2: decides whether launch `seq` of `count` frames (`views`, copied to `staged`) reads a dispatch order,
// and if so finds or starts its shape's slot and gives the staged views the order and the cost buffer.  *ordered: the launch
// runs the instances that read them.
int dispatch_order_attach(shray_scene *scene, const FrameView *views, int count, FrameView *staged, const LaunchKind &kind,
                          unsigned long long seq, hipStream_t stream, bool *ordered);

// A launch's step 7, for an ordered launch only: counts it and, when one is due and a ring entry is free, enqueues the kernel
// that writes the shape's next permutation behind the launch on `stream`.
int dispatch_order_resort(shray_scene *scene, unsigned long long seq, hipStream_t stream);

}   // namespace shray
