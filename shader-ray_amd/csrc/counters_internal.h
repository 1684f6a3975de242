// counters_internal.h -- the host's sum of the kCounterShards tallies a counting kernel leaves (device_types.h), for render_api.hip's
// counting renders and the client libraries' blocking forms (client_internal.h).  Host-only, internal to the libraries; not
// part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "error_internal.h"

namespace {

// Copies the shards at `d_shards` back and sets the seven tallies of *out to their sums; out->samples is the caller's.
inline int sum_counter_shards(const shray::DeviceCounters *d_shards, shray_counters *out)
{
    shray::DeviceCounters shards[shray::kCounterShards];
    HIP_TRY(hipMemcpy(shards, d_shards, sizeof(shards), hipMemcpyDeviceToHost));
    shray_counters sum = {};
    for (const shray::DeviceCounters &s : shards) {
        sum.node_visits += s.node_visits;
        sum.leaf_visits += s.leaf_visits;
        sum.triangle_tests += s.triangle_tests;
        sum.shaded_hits += s.shaded_hits;
        sum.env_lookups += s.env_lookups;
        sum.traversals += s.traversals;
        sum.bad_hits += s.bad_hits;
    }
    sum.samples = out->samples;
    *out = sum;
    return SHRAY_OK;
}

}   // namespace
