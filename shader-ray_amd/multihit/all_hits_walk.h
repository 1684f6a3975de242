// all_hits_walk.h -- one lane's all-hits walk of one scene, shared by multihit.hip (one scene per ray)
// and instance_multihit/instance_multihit.hip (one walk per instance a ray reaches): the ray's divisors
// and slab test, the K best and their sorted insertion, the leaf loop, and the branch and pop logic over the level-major LDS
// column stack.  Internal to the libraries; no kernel is defined here.
//
// The K best are kept by sorted insertion: in registers for K <= 8 (instances for 1, 2, 4 and 8 slots; every index is a
// compile-time constant, so there is no scratch), in the ray's own K output slots for larger K.  INST: the records carry an
// instance index as a fifth field, and the key is (t, instance, triangle) instead of (t, triangle).
#pragma once

#include <hip/hip_runtime.h>

#include "exact_div.h"
#include "first_k_query.h"
#include "packed_walk.h"
#include "shader_ray_multihit.h"
#include "trace_common.h"

namespace {

using namespace shray;

constexpr float kDetEps = 0.0000001f;             // fs:311

// the key of the header: t as a float comparison, then the triangle index
__device__ __forceinline__ bool before(float t, int tri, float slot_t, int slot_tri)
{
    return t < slot_t || (t == slot_t && tri < slot_tri);
}
__device__ __forceinline__ bool before(float t, int tri, float4 slot) { return before(t, tri, slot.x, __float_as_int(slot.w)); }
// the key of an instance set (include/shader_ray_instance_multihit.h): t, then the instance index, then the triangle index
__device__ __forceinline__ bool before(float t, int inst, int tri, float slot_t, int slot_inst, int slot_tri)
{
    return t < slot_t || (t == slot_t && (inst < slot_inst || (inst == slot_inst && tri < slot_tri)));
}

// a ray's divisors: its direction, and where exact_div.h's conditions hold the correctly rounded reciprocals
struct Slab {
    float o[3], d[3], y[3], yl[3];
    bool exact;   // every quotient of this ray may take div_by_constant4
};

__device__ __forceinline__ Slab make_slab(const SceneView &sc, V3 P, V3 D)
{
    Slab s;
    s.o[0] = P.x, s.o[1] = P.y, s.o[2] = P.z;
    s.d[0] = D.x, s.d[1] = D.y, s.d[2] = D.z;
    s.exact = sc.exact_div_ok != 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        s.exact = s.exact && divisor_in_range(s.d[a]) && coordinate_in_range(s.o[a]);
        s.y[a] = reciprocal_in_range(s.d[a]);   // (not looked at when the ray is not exact)
        s.yl[a] = reciprocal_residual(s.d[a], s.y[a]);
    }
    return s;
}

// range_intersect_box over [0, 1e8] (fs:200-217): true divisions, or their exact_div.h equals
__device__ __forceinline__ void slab_range(const Slab &s, const Box &b, float &r0, float &r1)
{
    float ta[3], tb[3];
    if (s.exact) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            ta[a] = div_by_constant4(b.lo[a] - s.o[a], s.d[a], s.y[a], s.yl[a]);
            tb[a] = div_by_constant4(b.hi[a] - s.o[a], s.d[a], s.y[a], s.yl[a]);
        }
    } else {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            ta[a] = (b.lo[a] - s.o[a]) / s.d[a];
            tb[a] = (b.hi[a] - s.o[a]) / s.d[a];
        }
    }
    r0 = 0.0f, r1 = kRangeMax;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const bool forward = s.d[a] >= 0.0f;
        r0 = sel_max(r0, forward ? ta[a] : tb[a]);
        r1 = sel_min(r1, forward ? tb[a] : ta[a]);
    }
}

// One ray's K best and its crossing count.  SLOTS: the register slots (k <= SLOTS), kSlotsInMemory: they live in the ray's
// own output slots, `slots` (and `inst_slots` with INST), any k, also 0.
template <int SLOTS, bool INST>
struct KBest {
    static constexpr int R = SLOTS > 0 ? SLOTS : 1;
    float held_t[R], held_u[R], held_v[R];   // (plain scalars: every index below is a constant once unrolled)
    int held_tri[R];
    int held_inst[INST ? R : 1];
    float4 *slots;         // this ray's own k records (dereferenced only when live and k > 0)
    int32_t *inst_slots;   // INST and kSlotsInMemory: this ray's own k instance indices
    int k;
    // the k-th smallest t held; tmax while fewer than k are held (an accepted t is below tmax, and so is an entered r0)
    float tk;
    int n;

    __device__ __forceinline__ void init(float tmax, int records, float4 *ray_slots, int32_t *ray_inst_slots, bool live)
    {
        slots = ray_slots;
        inst_slots = ray_inst_slots;
        k = records;
#pragma unroll
        for (int i = 0; i < R; i++)
            held_t[i] = tmax, held_u[i] = 0.0f, held_v[i] = 0.0f, held_tri[i] = SHRAY_HIT_MISS;
        if constexpr (INST) {
#pragma unroll
            for (int i = 0; i < R; i++)
                held_inst[i] = -1;
        }
        if (SLOTS == kSlotsInMemory && live) {
            const float4 empty = make_float4(tmax, 0.0f, 0.0f, __int_as_float(SHRAY_HIT_MISS));
            for (int i = 0; i < k; i++)
                slots[i] = empty;
            if constexpr (INST)
                for (int i = 0; i < k; i++)
                    inst_slots[i] = -1;
        }
        tk = tmax;
        n = 0;
    }

    // slot i against the candidate
    __device__ __forceinline__ bool sorts_before(float dist, int inst, int tri, int i) const
    {
        if constexpr (INST)
            return before(dist, inst, tri, held_t[i], held_inst[i], held_tri[i]);
        else
            return before(dist, tri, held_t[i], held_tri[i]);
    }

    // a member of the crossing set: counted, and kept where it sorts among the first k
    __device__ __forceinline__ void insert(float dist, float u, float bw, int tri, int inst)
    {
        n++;
        if (SLOTS != kSlotsInMemory) {
            // the record moves in where it sorts, the rest move down, the last falls off
#pragma unroll
            for (int i = R - 1; i >= 0; i--) {
                constexpr int kNone = 0;
                const int up = i > 0 ? i - 1 : kNone;
                const bool here = sorts_before(dist, inst, tri, i);
                const bool above = i > 0 && sorts_before(dist, inst, tri, up);
                held_t[i] = above ? held_t[up] : (here ? dist : held_t[i]);
                held_u[i] = above ? held_u[up] : (here ? u : held_u[i]);
                held_v[i] = above ? held_v[up] : (here ? bw : held_v[i]);
                held_tri[i] = above ? held_tri[up] : (here ? tri : held_tri[i]);
                if constexpr (INST)
                    held_inst[i] = above ? held_inst[up] : (here ? inst : held_inst[i]);
            }
#pragma unroll
            for (int i = 0; i < R; i++)
                tk = i == k - 1 ? held_t[i] : tk;
        } else if constexpr (INST) {
            if (k > 0) {
                const float4 last = slots[k - 1];
                if (before(dist, inst, tri, last.x, inst_slots[k - 1], __float_as_int(last.w))) {
                    int i = k - 1;
                    while (i > 0) {
                        const float4 s = slots[i - 1];
                        const int s_inst = inst_slots[i - 1];
                        if (!before(dist, inst, tri, s.x, s_inst, __float_as_int(s.w)))
                            break;
                        slots[i] = s;
                        inst_slots[i] = s_inst;
                        i--;
                    }
                    slots[i] = make_float4(dist, u, bw, __int_as_float(tri));
                    inst_slots[i] = inst;
                    tk = slots[k - 1].x;
                }
            }
        } else if (k > 0 && before(dist, tri, slots[k - 1])) {
            int i = k - 1;
            while (i > 0) {
                const float4 s = slots[i - 1];
                if (!before(dist, tri, s))
                    break;
                slots[i] = s;
                i--;
            }
            slots[i] = make_float4(dist, u, bw, __int_as_float(tri));
            tk = slots[k - 1].x;
        }
    }

    // the register slots into the ray's records (the memory form holds them there already)
    __device__ __forceinline__ void store(int32_t *ray_instances) const
    {
        if (SLOTS != kSlotsInMemory) {
#pragma unroll
            for (int i = 0; i < R; i++)
                if (i < k)
                    slots[i] = make_float4(held_t[i], held_u[i], held_v[i], __int_as_float(held_tri[i]));
            if constexpr (INST) {
                if (ray_instances) {
#pragma unroll
                    for (int i = 0; i < R; i++)
                        if (i < k)
                            ray_instances[i] = held_inst[i];
                }
            }
        }
    }
};

// One lane's walk of scene `sc` with the ray (P, D, tmax), tmax > 0: every member of the crossing set goes to best.insert
// with `inst`.  `column` is the lane's LDS stack (node names, level-major, kBlock apart).  PRUNE: skip nodes whose r0 is above
// the k-th smallest t held (nothing in them can reach the first k).
template <int SLOTS, bool PRUNE, bool INST>
__device__ __forceinline__ void all_hits_walk(const SceneView &sc, const V3 &P, const V3 &D, float tmax, int max_leaf_tests, int inst,
                                              uint32_t *column, KBest<SLOTS, INST> &best, RayCounters &rc)
{
    const char *copy = static_cast<const char *>(sc.packed_nodes) + (size_t)kOctant * sc.packed_nodes_bytes;
    const Slab slab = make_slab(sc, P, D);
    rc.traversals += 1;
    Record cur = load_record(copy, sc.packed_root);
    float r0, r1;
    slab_range(slab, cur.box, r0, r1);
    rc.node_visits += 1;
    rc.leaf_visits += (cur.b & kLeafFlag) ? 1 : 0;
    int sp = 0;
    bool go = !(r0 >= r1) && r0 < tmax;
    while (go) {
        if (cur.b & kLeafFlag) {
            const uint32_t first = cur.a, in_leaf = cur.b & ~kLeafFlag;
            const uint32_t tests = in_leaf < (uint32_t)max_leaf_tests ? in_leaf : (uint32_t)max_leaf_tests;
            for (uint32_t j = 0; j < tests; j++) {
                rc.triangle_tests++;
                const int tri = (int)(first + j);
                const float *v = sc.positions + 9ull * (uint32_t)tri;
                const V3 v0 = mk(v[0], v[1], v[2]), v1 = mk(v[3], v[4], v[5]), v2 = mk(v[6], v[7], v[8]);
                const V3 e0 = v1 - v0, e1 = v0 - v2;
                const V3 M = cross3(e1, D);
                const float det = dot3(e0, M);
                if (det > -kDetEps && det < kDetEps)
                    continue;
                const float inv_det = 1.0f / det;
                const V3 T = P - v0;
                const V3 Q = cross3(T, e0);
                const float dist = -dot3(e1, Q) * inv_det;
                if (dist > tmax || dist < r0 || dist > r1)
                    continue;
                const float u = dot3(T, M) * inv_det;
                if (u < 0.0f || u > 1.0f)
                    continue;
                const float bw = dot3(D, Q) * inv_det;
                if (bw < 0.0f || u + bw > 1.0f)
                    continue;
                if (!(dist < tmax))   // the report rule; NaN ends here too
                    continue;
                best.insert(dist, u, bw, tri, inst);
            }
        } else {
            const uint32_t n0 = cur.a & kChildNameMask, n1 = cur.b;
            const Record c0 = load_record(copy, n0), c1 = load_record(copy, n1);
            float a0, b0, a1, b1;
            slab_range(slab, c0.box, a0, b0);
            slab_range(slab, c1.box, a1, b1);
            rc.node_visits += 2;
            rc.leaf_visits += ((c0.b & kLeafFlag) ? 1 : 0) + ((c1.b & kLeafFlag) ? 1 : 0);
            // entered (the header); skipped when nothing in it can reach the first k: an accepted t is never below
            // its leaf's r0, a descendant's r0 never below this one (a NaN r0 compares false: visited)
            const bool e0 = !(a0 >= b0) && a0 < tmax && !(PRUNE && a0 > best.tk);
            const bool e1 = !(a1 >= b1) && a1 < tmax && !(PRUNE && a1 > best.tk);
            const bool second = a1 < a0;   // the child with the smaller r0 first
            const bool go_near = second ? e1 : e0, go_far = second ? e0 : e1;
            if (go_near || go_far) {
                if (go_near && go_far) {
                    column[(size_t)sp * kBlock] = second ? n0 : n1;
                    sp++;
                }
                const bool take1 = go_near ? second : !second;
                cur = take1 ? c1 : c0;
                r0 = take1 ? a1 : a0;
                r1 = take1 ? b1 : b0;
                continue;
            }
        }
        // the next pending node; the stack holds at most one entry per level of the current path
        go = false;
        while (sp > 0) {
            sp--;
            cur = load_record(copy, column[(size_t)sp * kBlock]);
            slab_range(slab, cur.box, r0, r1);   // (the values that entered it)
            if (PRUNE && r0 > best.tk)   // t_K has dropped below it since it was pushed
                continue;
            go = true;
            break;
        }
    }
}

}   // namespace
