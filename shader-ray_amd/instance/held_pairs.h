// held_pairs.h -- a lane's K smallest (instance, triangle) pairs, as the instanced box-overlap and triangle-intersection
// walks keep them (instance_overlap/, instance_intersect/): in registers for K <= 8 (one 64-bit key a slot, every index a
// compile-time constant, no scratch), else the triangles in the item's own K output slots and the instances in the instance
// buffer beside them.  It needs point/first_k_query.h's kSlotsInMemory, so, like enter_set.h, it is not for
// libshray_instance.so's own units, which are built without -Ipoint.  Internal to the libraries; no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>

#include "first_k_query.h"
#include "shader_ray_query.h"

namespace {

constexpr unsigned long long kEmptyKey = ~0ull;   // after every (instance, triangle)

__device__ __forceinline__ unsigned long long key_of(int inst, uint32_t tri) { return ((unsigned long long)(uint32_t)inst << 32) | tri; }

// A lane's K smallest.  SLOTS > 0: the keys in registers, ascending; kSlotsInMemory: the triangles in the item's own output
// slots and their instances beside them (any k, also 0).  The two kernels spell out its initialisation and its write-out
// themselves: as members they changed the kernels' register allocation.
template <int SLOTS>
struct Held {
    static constexpr int R = SLOTS > 0 ? SLOTS : 1;
    unsigned long long key[R];   // (plain scalars: every index is a constant once unrolled)
    int32_t *slots;              // in memory: this item's own triangles and instances (dereferenced only when live and k > 0)
    int32_t *slot_inst;
    int k;

    // the pair sinks to where it sorts, the largest falls off
    __device__ __forceinline__ void insert(int inst, uint32_t t)
    {
        if (SLOTS != kSlotsInMemory) {
            unsigned long long carry = key_of(inst, t);
#pragma unroll
            for (int i = 0; i < R; i++) {
                const unsigned long long low = carry < key[i] ? carry : key[i];
                carry = carry < key[i] ? key[i] : carry;
                key[i] = low;
            }
        } else if (k > 0 && before(inst, t, slot_inst[k - 1], slots[k - 1])) {
            int i = k - 1;
            while (i > 0) {
                const int32_t st = slots[i - 1], si = slot_inst[i - 1];
                if (!before(inst, t, si, st))
                    break;
                slots[i] = st, slot_inst[i] = si;
                i--;
            }
            slots[i] = (int32_t)t, slot_inst[i] = inst;
        }
    }

    // the key of the header against a slot in memory; an empty slot (triangle < 0) is after every pair
    static __device__ __forceinline__ bool before(int inst, uint32_t t, int32_t slot_inst, int32_t slot_tri)
    {
        return slot_tri < 0 || inst < slot_inst || (inst == slot_inst && t < (uint32_t)slot_tri);
    }

    // whether K pairs are held and every one of them is of an instance below `inst`: no pair of `inst` can be among the K
    // smallest, because the key leads with the instance
    __device__ __forceinline__ bool full_below(int inst) const
    {
        if (SLOTS != kSlotsInMemory) {
            unsigned long long last = kEmptyKey;
#pragma unroll
            for (int i = 0; i < R; i++)
                last = i == k - 1 ? key[i] : last;
            return last != kEmptyKey && (uint32_t)inst > (uint32_t)(last >> 32);
        }
        return k > 0 && slots[k - 1] >= 0 && inst > slot_inst[k - 1];
    }
};

}   // namespace
