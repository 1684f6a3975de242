// first_k_query.h -- the host side that the counted, first-K queries share (the all-hits ray query, multihit/multihit.hip,
// its instanced form, instance_multihit/instance_multihit.hip, the within-radius query, near/near.hip, and the box-overlap
// query, overlap/overlap.hip): per item a count and the first K records in order.  How such a query is refused, which
// instance of its kernel a K and the outputs asked for select, the launches of its device form and its blocking form are
// here once; a library keeps its kernel, its Work struct, its params check, its alignment refusal and the table of its nouns.
// Host-only, internal to the libraries; no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include "client_internal.h"
#include "packed_walk.h"

namespace {

constexpr int kSlotsInMemory = 0;   // SLOTS of the kernel instance that keeps its K best in the item's own output slots

// The ladder from K to a kernel's SLOTS: registers for 1, 2, 4 and 8 slots, the item's output slots for no record and
// for more than 8.
constexpr int slots_for(int k) { return k <= 0 || k > 8 ? kSlotsInMemory : k == 1 ? 1 : k == 2 ? 2 : k <= 4 ? 4 : 8; }
static_assert(slots_for(0) == 0 && slots_for(1) == 1 && slots_for(2) == 2 && slots_for(3) == 4 && slots_for(4) == 4, "the ladder");
static_assert(slots_for(5) == 8 && slots_for(8) == 8 && slots_for(9) == 0 && slots_for(64) == 0, "the ladder");

// whether K records are kept, and in the item's output slots
constexpr bool kept_in_memory(int k) { return k > 0 && slots_for(k) == kSlotsInMemory; }
static_assert(!kept_in_memory(0) && !kept_in_memory(8) && kept_in_memory(9), "in memory: above 8");

// f(std::integral_constant<int, SLOTS>) for k's SLOTS
template <typename F>
void with_slots(int k, F &&f)
{
    switch (slots_for(k)) {
    case kSlotsInMemory: return f(std::integral_constant<int, kSlotsInMemory>());
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
    }
}

// The form of a walk that may skip what cannot reach the first K: the work counters count the walk that skips nothing,
// a count needs every member, and without either the walk prunes.
struct Form {
    bool prune, count;
};
constexpr Form form_for(bool counters, bool counts, int k)
{
    return counters ? Form{false, true} : counts || k == 0 ? Form{false, false} : Form{true, false};
}
static_assert(!form_for(true, false, 8).prune && form_for(true, false, 8).count, "counters: <S, false, true>");
static_assert(!form_for(true, true, 0).prune && form_for(true, true, 0).count, "counters: <S, false, true>");
static_assert(!form_for(false, true, 8).prune && !form_for(false, true, 8).count, "counts: <S, false, false>");
static_assert(!form_for(false, false, 0).prune && !form_for(false, false, 0).count, "K = 0: <S, false, false>");
static_assert(form_for(false, false, 8).prune && !form_for(false, false, 8).count, "everything else: <S, true, false>");

// f(std::bool_constant<PRUNE>, std::bool_constant<COUNT>) for the form
template <typename F>
void with_form(Form form, F &&f)
{
    if (form.count)
        f(std::false_type(), std::true_type());
    else if (!form.prune)
        f(std::false_type(), std::false_type());
    else
        f(std::true_type(), std::false_type());
}

// a library's words for what it is given and what it returns, as its refusals use them
struct Nouns {
    const char *item, *items;   // "ray", "rays"
    const char *owner;          // "scene"
    const char *out;            // "hits"
    const char *k;              // "max_hits"
    const char *query;          // "all-hits ray query": the name of a launch
};

// The refusals every form makes after its params check and before it touches the owner or a device.  `extra` is a
// library's own refusal, at its place in the order.
template <typename Extra>
int check_first_k(const Nouns &n, const void *owner, const void *items, int64_t count, int k, const void *out, const void *counts, Extra &&extra)
{
    if (count < 0)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "negative %s count %lld", n.item, (long long)count);
    if (!owner || !items)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "%s or %s is NULL", n.owner, n.items);
    if (const int rc = extra())
        return rc;
    if (k > 0 && !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "%s is NULL with %s %d", n.out, n.k, k);
    if (k == 0 && !counts)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "nothing is asked for: %s is 0 and counts is NULL", n.k);
    return SHRAY_OK;
}

inline int check_first_k(const Nouns &n, const void *owner, const void *items, int64_t count, int k, const void *out, const void *counts)
{
    return check_first_k(n, owner, items, count, k, out, counts, [] { return (int)SHRAY_OK; });
}

// the entries of a lane's stack column: one per edge of the tree's height, one for a tree that is a single leaf
inline size_t stack_levels(int height) { return (size_t)(height > 0 ? height : 1); }

// The launches of a device form: `count` items, one lane each, in launches of at most kPointsPerLaunch; launch(grid) with
// w.first set to the launch's first item, up to the first error.
template <typename Work, typename Launch>
int first_k_launches(const Nouns &n, Work &w, int64_t count, Launch &&launch)
{
    return for_each_launch(((uint64_t)count + kBlock - 1) / kBlock, kPointsPerLaunch / kBlock, [&](uint64_t first, dim3 grid) {
        w.first = first * kBlock;
        launch(grid);
        return launched(n.query);
    });
}

// the host memory of a blocking form
struct FirstKHost {
    const void *items;
    size_t item_bytes;
    void *out;         // k records per item
    size_t record_bytes;
    int32_t *second;   // k more words per item (the instances of an instance set), or nullptr
    int32_t *counts;   // one per item, or nullptr
};

// The blocking form, after the library's check of its arguments: the tallies zeroed, nothing more for no item, enter()
// (the owner's errors come before any allocation), then the items to the device, device(items, out, second, counts,
// shards) -- the device form on the null stream -- and the records, counts (and tallies) back.
template <typename Enter, typename Device>
int first_k_blocking(const FirstKHost &h, int64_t count, int k, shray_counters *tallies, Enter &&enter, Device &&device)
{
    if (tallies) {
        memset(tallies, 0, sizeof(*tallies));
        tallies->samples = (uint64_t)count;
    }
    if (count == 0)
        return SHRAY_OK;
    if (const int rc = enter())
        return rc;
    const size_t n = (size_t)count, per_item = (size_t)k;
    return run_blocking({{h.items, n * h.item_bytes}},
                        {{h.out, n * per_item * h.record_bytes},
                         {h.second, h.second ? n * per_item * sizeof(int32_t) : 0},
                         {h.counts, h.counts ? n * sizeof(int32_t) : 0}},
                        tallies, [&](DeviceBuffer *d_items, DeviceBuffer *d_out, shray::DeviceCounters *shards) {
                            return device(d_items->p, d_out[0].p, d_out[1].as<int32_t>(), d_out[2].as<int32_t>(), shards);
                        });
}

// the refusal of a form that returns the work counters
inline int check_counters(const void *counters)
{
    return counters ? (int)SHRAY_OK : fail(SHRAY_ERR_INVALID_ARGUMENT, "counters is NULL");
}

}   // namespace
