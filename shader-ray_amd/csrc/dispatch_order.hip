// dispatch_order.hip -- the dispatch order of the convergent batch kernels (dispatch_order.h): which launches read one, the
// slot a launch shape's costs and permutations live in, and the re-sort behind a launch.  Host code only; the kernel that sorts
// is kernel_assemble.hip's (launch_dispatch_order).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "dispatch_order.h"
#include "error_internal.h"
#include "launch.h"
#include "scene_internal.h"

using namespace shray;

namespace {

// SHRAY_DISPATCH_ORDER: heaviest patches first in the convergent batch kernels (dispatch_order.h: DispatchOrder);
// the environment variable SHRAY_DISPATCH_ORDER=0 turns it off at run time (A/B, profiles/r03_dispatch_order_ab.sh)
// launches of a shape between two re-sorts (tuning: SHRAY_DISPATCH_PERIOD)
unsigned long long dispatch_period()
{
    static const unsigned long long period = [] {
        const char *e = getenv("SHRAY_DISPATCH_PERIOD");
        const long long v = e ? atoll(e) : 32;
        return (unsigned long long)(v < 1 ? 1 : v);
    }();
    return period;
}
bool dispatch_order_enabled()
{
    static const bool on = [] {
        const char *e = getenv("SHRAY_DISPATCH_ORDER");
        return !(e && e[0] == '0');
    }();
    return on;
}

// A re-sort follows a shape's first three launches, then launches 4, 8, 16 ... up to the period, and every dispatch_period()-th
// from then on.  Round 6 (profiles/r06/dispatch_period_ab.txt): the costs between two re-sorts are the maximum over the launches
// between them and halve at every re-sort, so eight launches between re-sorts made the order follow the last eight views -- on
// an orbit of twenty that is the half the next frames are NOT in -- and cost a 10-40 us kernel per eight frames; thirty-two cover
// the orbit (a lone frame of it 0.400 -> 0.387 ms), the doubling start keeps a new shape's first orders coming as fast as before.
bool dispatch_sorts_after(unsigned long long launch_number)
{
    if (launch_number <= 3 || launch_number % dispatch_period() == 0)
        return true;
    return launch_number < dispatch_period() && (launch_number & (launch_number - 1)) == 0;
}

// costs below (16 - bulk) / 16 of a shape's largest keep their row-major order among themselves (tuning: SHRAY_DISPATCH_BULK)
int dispatch_bulk_class()
{
    static const int bulk = [] {
        const char *e = getenv("SHRAY_DISPATCH_BULK");
        return e ? atoi(e) : 1 << 20;    // every class of its own (measured: profiles/history/r03/dispatch_bulk_ab.txt)
    }();
    return bulk;
}

// A dispatch-order slot starts over for a new launch shape.  Launches of the shape it held may still be running and
// reading its buffers: those are set aside (shray_scene::retired) and handed out again only when every launch that was
// enqueued before the eviction is over (launch_is_over), so nothing here
// synchronises with the device.  `seq`: the current launch's number; `stream`: its stream (the new costs are zeroed on it:
// a launch of the shape on ANOTHER stream that reports before the fill has run loses its report, which the next one
// repeats).  A caller that rotates more shapes than there are slots would evict on every launch: shapes that come back
// after their eviction are counted, and after kThrashLimit of them the scene's launches keep row-major order for a while
// (shray_scene::dispatch_paused_until; the slot is then left as it is).
int dispatch_slot_start(shray_scene *scene, DispatchOrder &d, const long long key[8], uint32_t patches,
                        unsigned long long seq, hipStream_t stream)
{
    // a shape that was evicted not long ago and is back: the caller rotates more shapes than there are slots
    for (int k = 0; k < shray_scene::kEvictedKeys; k++)
        if (memcmp(scene->evicted_keys[k], key, sizeof(scene->evicted_keys[k])) == 0 && key[7] != 0) {
            if (++scene->dispatch_returns >= shray_scene::kThrashLimit) {
                scene->dispatch_returns = 0;
                scene->dispatch_paused_until = seq + shray_scene::kThrashPause;
                scene->dispatch_last = -1;
                return SHRAY_OK;
            }
            break;
        }
    if (d.n) {
        memcpy(scene->evicted_keys[scene->evicted_next], d.key, sizeof(d.key));
        scene->evicted_next = (scene->evicted_next + 1) % shray_scene::kEvictedKeys;
        d.n = 0;                                   // from here on the slot matches no key, whatever fails below
        scene->retired.push(&d.cost.p, &d.ring.p, d.capacity, seq);
        d.capacity = 0;
    }
    // (a start that failed behind its allocations -- the memset, an event -- left the slot unused, d.n == 0, WITH buffers of the
    // capacity that start asked for: no launch has read them; they serve this start only if they are large enough.  ADVICE round 4)
    if ((d.cost.p || d.ring.p) && d.capacity < patches) {
        d.cost.release();
        d.ring.release();
        d.capacity = 0;
    }
    // buffers: a retired pair that is large enough and no longer read, else new ones
    if (!d.cost.p)
        if (const size_t fits = scene->retired.take_first(seq, [&](size_t capacity) { return capacity >= patches; }, &d.cost.p, &d.ring.p))
            d.capacity = fits;
    if (!d.cost.p || !d.ring.p) {
        d.cost.release();      // (an earlier allocation that failed half-way leaves nothing behind)
        d.ring.release();
        d.capacity = 0;
        // more than a handful set aside: free the ones nobody reads any more (hipFree waits for the device: rare, and only here)
        scene->retired.free_aged(seq, 8);
        HIP_TRY(hipMalloc(&d.cost.p, (size_t)patches * 4 * 2));              // costs + the order kernel's copy of them
        HIP_TRY(hipMalloc(&d.ring.p, (size_t)patches * 4 * DispatchOrder::kRing));
        d.capacity = patches;
    }
    HIP_TRY(hipMemsetAsync(d.cost.p, 0, (size_t)patches * 4 * 2, stream));
    for (hipEvent_t &e : d.ready)
        if (!e)
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    memcpy(d.key, key, sizeof(d.key));
    d.current = d.written = -1;
    d.pending_first = d.pending_count = 0;
    d.launches = 0;
    d.written_on = nullptr;
    memset(d.last_reader, 0, sizeof(d.last_reader));
    d.n = patches;
    return SHRAY_OK;
}

}   // namespace

namespace shray {

int dispatch_order_attach(shray_scene *scene, const FrameView *views, int count, FrameView *staged, const LaunchKind &kind,
                          unsigned long long seq, hipStream_t stream, bool *ordered)
{
    *ordered = false;
    // plain frames of the stack kernel's convergent instances
    const bool plain = (scene->kernel_id == 0 || scene->kernel_id == 3) && kind.all_plain;
    // Where it pays (profiles/history/r03/dispatch_order_ab.txt): a launch that is not followed at once by more of the same -- one
    // frame per launch (a lone frame: 0.54 -> 0.45 ms), a tile set (a rank's share of a multi-GPU step: 0.92 -> 0.74 ms for
    // 20 frames at N = 8; within 3 % either way once steps follow each other without a gap).  Several whole frames per
    // launch over several streams (the N = 1 throughput form) run 6 % SLOWER heaviest-first -- the long divergent waves
    // of every launch then crowd the machine together -- and keep their row-major order.
    const bool lone_kind = count == 1 || views[0].tile_stride != 0;
    // (the instances that read an order exist for zero-diffuse frames: kernel_stack.hip)
    // ... and for the instances that deal their leaves: every 1 spp launch, and multi-sample frames of a tree larger than
    // an L2 share (config 4: 3.00 -> 2.74 ms); a cache-resident multi-sample frame (config 5) is 5 % SLOWER re-ordered
    const bool dealing = views[0].spp == 1 || kind.deal;
    if (!(plain && !kind.tally && lone_kind && kind.all_metal && dealing && !kind.pair && dispatch_order_enabled() &&
          seq >= scene->dispatch_paused_until))
        return SHRAY_OK;
    const FrameView &f = views[0];
    const long long key[8] = {f.width, f.height, f.spp, f.tile_w, f.tile_h, f.tile_stride,
                              ((long long)f.tile_phase << 32) | (unsigned int)f.tile_phase_count, (long long)f.total_patches};
    int which = -1, lru = 0;
    for (int k = 0; k < shray_scene::kDispatchShapes; k++) {
        if (scene->dispatch[k].n && memcmp(key, scene->dispatch[k].key, sizeof(key)) == 0)
            which = k;
        if (scene->dispatch[k].last_use < scene->dispatch[lru].last_use)
            lru = k;
    }
    if (which >= 0) {
        scene->dispatch_returns = 0;
    } else {
        // a shape not seen (lately) takes the least recently used slot
        const int rc = dispatch_slot_start(scene, scene->dispatch[lru], key, f.total_patches, seq, stream);
        if (rc)
            return rc;
        which = seq < scene->dispatch_paused_until ? -1 : lru;   // (-1: too many shapes in rotation, row-major for a while)
    }
    if (which < 0)
        return SHRAY_OK;
    scene->dispatch_last = which;
    DispatchOrder &d = scene->dispatch[which];
    d.last_use = ++scene->dispatch_clock;
    // permutations that have become complete, oldest first (the pending order kernels sit on one stream, in order)
    while (d.pending_count > 0 && hipEventQuery(d.ready[d.pending_first]) == hipSuccess) {
        d.current = d.pending_first;
        d.pending_first = (d.pending_first + 1) % DispatchOrder::kRing;
        d.pending_count--;
    }
    const int use = (d.pending_count > 0 && stream == d.written_on) ? d.written : d.current;
    if (use >= 0)
        d.last_reader[use] = seq;
    // only the launches a re-sort follows report their waves' running times: reporting costs a launch 3 % (a late
    // scalar load of the buffer's address and an atomic per wave, profiles/history/r03/dispatch_mechanism_ab.txt)
    // (the two launches before a re-sort: a loop that alternates long and short steps reports both)
    // A launch of one frame always reports: its views change from launch to launch and the union of the last few is
    // the better predictor (0.474 against 0.480 ms on the orbit).
    const bool reports = count == 1 || dispatch_sorts_after(d.launches + 1) || dispatch_sorts_after(d.launches + 2);
    for (int k = 0; k < count; k++) {
        staged[k].dispatch_cost = reports ? (uint32_t *)d.cost.p : nullptr;
        staged[k].dispatch_order = use >= 0 ? (const uint32_t *)d.ring.p + (size_t)use * d.n : nullptr;
    }
    *ordered = true;
    return SHRAY_OK;
}

// the next permutation: after each of the first launches of a shape, then every dispatch_period() launches
int dispatch_order_resort(shray_scene *scene, unsigned long long seq, hipStream_t stream)
{
    DispatchOrder &d = scene->dispatch[scene->dispatch_last];
    d.launches++;
    // (an update that is still pending on ANOTHER stream is not overtaken; on the same stream the kernels queue up)
    if (!((d.pending_count == 0 || stream == d.written_on) && dispatch_sorts_after(d.launches)))
        return SHRAY_OK;
    const int next = (d.written + 1) % DispatchOrder::kRing;
    // `next` must be free: not the entry launches read, not one still being written, and not read by a launch that
    // may still be running (launch_is_over says when its last reader is not);
    // if it is not, this re-sort is skipped and the next due launch tries again
    const bool ring_full = (d.current >= 0 ? 1 : 0) + d.pending_count >= DispatchOrder::kRing;
    const bool still_read = d.last_reader[next] != 0 && !launch_is_over(d.last_reader[next], seq);
    if (ring_full || still_read)
        return SHRAY_OK;
    const hipError_t oe = launch_dispatch_order((uint32_t *)d.cost.p, (uint32_t *)d.ring.p + (size_t)next * d.n, d.n, stream, dispatch_bulk_class());
    if (oe != hipSuccess)
        return fail(SHRAY_ERR_DEVICE, "dispatch-order kernel launch failed: %s", hipGetErrorString(oe));
    HIP_TRY(hipEventRecord(d.ready[next], stream));
    if (d.pending_count == 0)
        d.pending_first = next;
    d.pending_count++;
    d.written = next;
    d.written_on = stream;
    d.last_reader[next] = 0;
    return SHRAY_OK;
}

}   // namespace shray
