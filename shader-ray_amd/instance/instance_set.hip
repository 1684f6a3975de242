// instance_set.hip -- the instance set of include/shader_ray_instance.h and its host build: the transforms' inverses and world
// boxes (set_internal.h's invert and place_box), a small top-level BVH over the boxes (object median splits, one instance
// per leaf), the upload, the host update, and the accessors through which the tests and the other instanced libraries read
// the set.  DESIGN.md section 10 argues the box margin.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <map>
#include <numeric>

#include "error_internal.h"
#include "scene_access_internal.h"
#include "set_internal.h"

using namespace shray;
using namespace shray_set;

namespace {

void free_device(SetDevice &d)
{
    for (void *p : {(void *)d.nodes, (void *)d.records, (void *)d.views})
        if (p)
            (void)hipFree(p);
    d = SetDevice{};
}

// the top level over boxes[ids[first .. first + n)], node `at` (its children are allocated together)
void build_top(std::vector<TopNode> &nodes, std::vector<BoxRef> &boxes, std::vector<int32_t> &ids, size_t first, size_t n, size_t at)
{
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double k = 0.0;
    for (size_t j = first; j < first + n; ++j) {
        const BoxRef &b = boxes[ids[j]];
        for (int c = 0; c < 3; ++c) {
            lo[c] = std::min(lo[c], b.lo[c]);
            hi[c] = std::max(hi[c], b.hi[c]);
            clo[c] = std::min(clo[c], b.centre[c]);
            chi[c] = std::max(chi[c], b.centre[c]);
        }
        k = std::max(k, b.k);
    }
    TopNode node;
    for (int c = 0; c < 3; ++c) {
        node.lo[c] = round_down(lo[c]);
        node.hi[c] = round_up(hi[c]);
    }
    node.k = round_up(k);
    if (n == 1) {
        node.link = kLeafBit | (uint32_t)ids[first];
        nodes[at] = node;
        return;
    }
    int axis = 0;
    for (int c = 1; c < 3; ++c)
        if (chi[c] - clo[c] > chi[axis] - clo[axis])
            axis = c;
    const size_t half = n / 2;
    std::nth_element(ids.begin() + first, ids.begin() + first + half, ids.begin() + first + n, [&](int32_t x, int32_t y) {
        const double cx = boxes[x].centre[axis], cy = boxes[y].centre[axis];
        return cx < cy || (cx == cy && x < y);
    });
    const size_t left = nodes.size();
    nodes.resize(left + 2);
    node.link = (uint32_t)axis << 29 | (uint32_t)left;
    nodes[at] = node;
    build_top(nodes, boxes, ids, first, half, left);
    build_top(nodes, boxes, ids, first + half, n - half, left + 1);
}

int prepare(const std::vector<shray_scene *> &scenes, const float *object_to_world, Prepared &p)
{
    const size_t n = scenes.size();
    p.object_to_world.assign(object_to_world, object_to_world + 12 * n);
    p.world_to_object.assign(12 * n, 0.0f);
    std::map<const shray_scene *, uint32_t> slot;
    std::vector<std::array<float, 6>> root_box;
    std::vector<BoxRef> boxes(n);
    p.records.assign(4 * n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (size_t i = 0; i < n; ++i) {
        const float *m = &p.object_to_world[12 * i];
        double condition = 0.0;
        if (!invert(m, &p.world_to_object[12 * i], &condition))
            return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance %zu: the transform is non-finite or singular, or its inverse is not finite", i);
        auto found = slot.find(scenes[i]);
        if (found == slot.end()) {
            ShrayQueryScene q;
            if (!scenes[i])
                return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance %zu: the scene is NULL", i);
            const int rc = shrayi_scene_query_view(scenes[i], &q);
            if (rc)
                return rc;
            if (!q.packed_ok)
                return fail(SHRAY_ERR_BAD_TREE, "instance %zu: the scene has no packed tree (instances walk the packed stack traversal)", i);
            if (p.device < 0) {
                p.device = q.device;
                HIP_TRY(hipSetDevice(p.device));
                // work enqueued before this call on any stream (a refit of a member) completes before its root box is read
                HIP_TRY(hipDeviceSynchronize());
            } else if (q.device != p.device) {
                return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance %zu: its scene is on device %d, the set's on %d", i, q.device, p.device);
            }
            std::array<float, 6> box;
            const size_t root = 3u * (size_t)q.view.tree_root;
            HIP_TRY(hipMemcpy(box.data(), q.view.boxmin + root, 3 * sizeof(float), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(box.data() + 3, q.view.boxmax + root, 3 * sizeof(float), hipMemcpyDeviceToHost));
            found = slot.emplace(scenes[i], (uint32_t)p.views.size()).first;
            p.views.push_back(q.view);
            root_box.push_back(box);
            p.stack_levels = std::max(p.stack_levels, q.stack_levels);
        }
        place_box(m, root_box[found->second].data(), condition, boxes[i]);
        const float *wrow = &p.world_to_object[12 * i];
        for (int r = 0; r < 3; ++r)
            p.records[4 * i + r] = make_float4(wrow[4 * r], wrow[4 * r + 1], wrow[4 * r + 2], wrow[4 * r + 3]);
        uint32_t s = found->second;
        float sbits;
        memcpy(&sbits, &s, sizeof(s));
        p.records[4 * i + 3].x = sbits;
    }
    std::vector<int32_t> ids(n);
    std::iota(ids.begin(), ids.end(), 0);
    p.nodes.assign(1, TopNode{});
    build_top(p.nodes, boxes, ids, 0, n, 0);
    return SHRAY_OK;
}

int upload(const Prepared &p, SetDevice &d)
{
    struct Guard {
        SetDevice &d;
        bool keep = false;
        ~Guard() { if (!keep) free_device(d); }
    } guard{d};
    HIP_TRY(hipMalloc(&d.nodes, p.nodes.size() * sizeof(TopNode)));
    HIP_TRY(hipMalloc(&d.records, p.records.size() * sizeof(float4)));
    HIP_TRY(hipMalloc(&d.views, p.views.size() * sizeof(SceneView)));
    HIP_TRY(hipMemcpy(d.nodes, p.nodes.data(), p.nodes.size() * sizeof(TopNode), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.records, p.records.data(), p.records.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.views, p.views.data(), p.views.size() * sizeof(SceneView), hipMemcpyHostToDevice));
    guard.keep = true;
    return SHRAY_OK;
}

int make_set(const std::vector<shray_scene *> &scenes, const float *object_to_world, Prepared &p, SetDevice &d)
{
    int rc = prepare(scenes, object_to_world, p);
    if (rc)
        return rc;
    return upload(p, d);
}

}   // namespace

namespace shray_set {

// `bytes` of host memory to device memory at `dst` on `stream`, through pinned memory that is reused once its copy is done
// (no host wait)
int stage(std::vector<Staging> &staging, hipStream_t stream, void *dst, const void *src, size_t bytes)
{
    Staging *s = nullptr;
    for (Staging &c : staging) {
        const hipError_t q = hipEventQuery(c.copied);
        if (q == hipSuccess && c.bytes >= bytes) {
            s = &c;
            break;
        }
        if (q != hipSuccess)
            (void)hipGetLastError();   // (hipErrorNotReady is an answer here, not an error for the launches after this)
    }
    if (!s) {
        Staging c;
        c.bytes = bytes;
        HIP_TRY(hipHostMalloc(&c.host, bytes, hipHostMallocDefault));
        const hipError_t e = hipEventCreateWithFlags(&c.copied, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipHostFree(c.host);
            return fail(SHRAY_ERR_DEVICE, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        staging.push_back(c);
        s = &staging.back();
    }
    memcpy(s->host, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, s->host, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->copied, stream));
    return SHRAY_OK;
}

// The device copy of the set's object-to-world maps, current for work enqueued on `stream` after this call: made on first
// use (12 n floats, nothing else), uploaded from the host copy on `stream` when it is behind it, else `stream` waits for the
// last upload, which may have run on another stream.  No host wait.  (The set's device is current.)
int current_maps(shray_instance_set *set, hipStream_t stream)
{
    if (!set->maps) {
        auto m = std::make_unique<ForwardMaps>();
        HIP_TRY(m->transforms.alloc(12 * set->scenes.size() * sizeof(float)));
        HIP_TRY(hipEventCreateWithFlags(&m->uploaded, hipEventDisableTiming));
        set->maps = std::move(m);
    }
    ForwardMaps &m = *set->maps;
    if (m.stale) {
        const int rc = stage(m.staging, stream, m.transforms.p, set->host.object_to_world.data(), 12 * set->scenes.size() * sizeof(float));
        if (rc)
            return rc;
        HIP_TRY(hipEventRecord(m.uploaded, stream));
        m.recorded = true;
        m.stale = false;
    } else if (m.recorded) {
        HIP_TRY(hipStreamWaitEvent(stream, m.uploaded, 0));
    }
    return SHRAY_OK;
}

}   // namespace shray_set

namespace {

// the host copies of the transforms and W after a device update: waits for it and downloads them
int refresh_host(shray_instance_set *set)
{
    if (!set->host_stale)
        return SHRAY_OK;
    int rc = use_device(set->host.device);
    if (rc)
        return rc;
    const size_t n = set->scenes.size();
    std::vector<float4> records(4 * n);
    std::vector<float> transforms(12 * n);
    HIP_TRY(hipEventSynchronize(set->update->finished));
    HIP_TRY(hipMemcpy(records.data(), set->dev.records, records.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(transforms.data(), set->maps->transforms.p, transforms.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) {
            const float4 &w = records[4 * i + r];
            float *out = &set->host.world_to_object[12 * i + 4 * r];
            out[0] = w.x;
            out[1] = w.y;
            out[2] = w.z;
            out[3] = w.w;
        }
    set->host.object_to_world = std::move(transforms);
    set->host.records = std::move(records);
    set->host_stale = false;
    return SHRAY_OK;
}

}   // namespace

extern "C" {

int shray_instance_set_create(const shray_instance *instances, int32_t count, shray_instance_set **out)
{
    if (!instances || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "instances or out is NULL");
    *out = nullptr;
    if (count <= 0 || count > SHRAY_INSTANCE_MAX)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance count %d is outside [1, 2^20]", count);
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0)
        return fail(SHRAY_ERR_NO_DEVICE, "no HIP device is visible");
    std::vector<shray_scene *> scenes((size_t)count);
    std::vector<float> transforms(12 * (size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        scenes[i] = instances[i].scene;
        memcpy(&transforms[12 * (size_t)i], instances[i].object_to_world, 12 * sizeof(float));
    }
    shray_instance_set *set = new shray_instance_set;
    set->scenes = std::move(scenes);
    for (shray_scene *s : set->scenes)
        if (std::find(set->distinct.begin(), set->distinct.end(), s) == set->distinct.end())
            set->distinct.push_back(s);
    const int rc = make_set(set->scenes, transforms.data(), set->host, set->dev);
    if (rc) {
        delete set;
        return rc;
    }
    *out = set;
    return SHRAY_OK;
}

int shray_instance_set_update(shray_instance_set *set, const float *object_to_world)
{
    if (!set)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set is NULL");
    int rc = object_to_world ? SHRAY_OK : refresh_host(set);   // (the transforms of a device update)
    if (rc)
        return rc;
    Prepared p;
    SetDevice d;
    rc = make_set(set->scenes, object_to_world ? object_to_world : set->host.object_to_world.data(), p, d);
    if (rc)
        return rc;
    // queries in flight read the old arrays
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        free_device(d);
        return fail(SHRAY_ERR_DEVICE, "hipDeviceSynchronize failed: %s", hipGetErrorString(e));
    }
    free_device(set->dev);
    set->host = std::move(p);
    set->dev = d;
    set->host_stale = false;
    if (set->maps)
        set->maps->stale = true;
    return SHRAY_OK;
}

void shray_instance_set_destroy(shray_instance_set *set)
{
    if (!set)
        return;
    if (set->host.device >= 0 && hipSetDevice(set->host.device) == hipSuccess)
        free_device(set->dev);
    delete set;
}

int shray_instance_set_count(const shray_instance_set *set, int32_t *count)
{
    if (!set || !count)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or count is NULL");
    *count = (int32_t)set->scenes.size();
    return SHRAY_OK;
}

int shray_instance_set_world_to_object(const shray_instance_set *set, float *out)
{
    if (!set || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or out is NULL");
    const int rc = refresh_host(const_cast<shray_instance_set *>(set));
    if (rc)
        return rc;
    memcpy(out, set->host.world_to_object.data(), set->host.world_to_object.size() * sizeof(float));
    return SHRAY_OK;
}

// For tests, not in the header: the set's top-level nodes (2 count - 1 of 32 bytes: lo.xyz, k, hi.xyz, link) and records
// (count * 4 float4: W's rows, then the scene slot) as the next query reads them, after any device update has finished.
// nodes and records may be NULL; *node_count, unless NULL, gets the node count.
int shrayi_instance_set_arrays(const shray_instance_set *set, void *nodes, void *records, int32_t *node_count)
{
    if (!set)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set is NULL");
    const size_t n = set->scenes.size();
    if (node_count)
        *node_count = (int32_t)(2 * n - 1);
    if (!nodes && !records)
        return SHRAY_OK;
    const int rc = use_device(set->host.device);
    if (rc)
        return rc;
    if (set->update && set->update->enqueued)
        HIP_TRY(hipEventSynchronize(set->update->finished));
    if (nodes)
        HIP_TRY(hipMemcpy(nodes, set->dev.nodes, (2 * n - 1) * sizeof(TopNode), hipMemcpyDeviceToHost));
    if (records)
        HIP_TRY(hipMemcpy(records, set->dev.records, 4 * n * sizeof(float4), hipMemcpyDeviceToHost));
    return SHRAY_OK;
}

// top_level.h declares this and the next one, for the other instanced libraries: nothing is copied or waited for
int shrayi_instance_set_device_arrays(const shray_instance_set *set, ShrayInstanceSetDevice *out)
{
    if (!set || !out)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or out is NULL");
    out->nodes = set->dev.nodes;
    out->records = set->dev.records;
    out->views = set->dev.views;
    out->scenes = set->distinct.data();
    out->count = (int32_t)set->scenes.size();
    out->scene_count = (int32_t)set->distinct.size();
    out->device = set->host.device;
    return SHRAY_OK;
}

int shrayi_instance_set_forward_maps(shray_instance_set *set, void *hip_stream, const float **d_maps)
{
    if (!set || !d_maps)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or d_maps is NULL");
    *d_maps = nullptr;
    int rc = use_device(set->host.device);
    if (rc)
        return rc;
    if ((rc = current_maps(set, (hipStream_t)hip_stream)))
        return rc;
    *d_maps = set->maps->transforms.as<const float>();
    return SHRAY_OK;
}

int shrayi_instance_set_member_scene(const shray_instance_set *set, int32_t instance, shray_scene **scene)
{
    if (!set || !scene)
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "set or scene is NULL");
    if (instance < 0 || (size_t)instance >= set->scenes.size())
        return fail(SHRAY_ERR_INVALID_ARGUMENT, "instance %d is not among the set's %zu", instance, set->scenes.size());
    *scene = set->scenes[(size_t)instance];
    return SHRAY_OK;
}

}   // extern "C"
