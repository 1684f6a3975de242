// scene_tree.h -- the proof that the eight (hit, miss) tables shray_scene_create receives are one threaded binary tree, and that
// tree's pre-order arrays (scene_create.hip hands them to the device).  Index arithmetic on arrays that come from outside the
// library: plain C++ with no HIP in it, so that tests/native_scene_tree.cpp runs it under AddressSanitizer and
// UndefinedBehaviorSanitizer on a machine without a GPU.  Host-only, internal to the library.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "shader_ray_hip.h"

namespace shray {

constexpr float kTerminatorF = 16777215.0f;   // raytracer.es.fs:384

// The shader carries every index as float32 (raytracer.es.fs:239-245, :384): exact only below 2^24, and node links at or above
// 16777215 mean "stop".  false: the scene is too large (SHRAY_ERR_INDEX_RANGE), *why says by how much.
inline bool check_index_range(const shray_scene_desc &d, std::string *why)
{
    const uint64_t stride = (uint64_t)d.data_texture_width * (uint64_t)d.group_data_rows;
    if (stride * 8 > 16777216ull || d.vertex_count > 16777216u) {
        char buf[160];
        snprintf(buf, sizeof(buf), "scene too large for float32 indices (%llu link texels, %u vertices; limit 2^24)",
                 (unsigned long long)(stride * 8), d.vertex_count);
        *why = buf;
        return false;
    }
    return true;
}

// host copies of a tree's pre-order arrays (TreeBuilder::preorder)
struct PreorderTree {
    std::vector<int32_t> negative, positive, start, triangles, index_of;
    std::vector<float> direction;
};

// Validation + reconstruction of the tree from the eight (hit, miss) tables, and its pre-order arrays.  The caller has checked
// the counts (0 <= tree_root < group_count <= stride, vertex_count % 3 == 0) and calls links_are_safe, recover_children,
// tables_match and preorder in that order, each only after the one before has answered true.
struct TreeBuilder {
    const shray_scene_desc &d;
    uint32_t n, stride, tri_count;
    std::vector<int32_t> neg, pos;      // per reference node; -1 for leaves
    std::vector<uint8_t> axis;
    std::string why;

    explicit TreeBuilder(const shray_scene_desc &desc)
        : d(desc), n((uint32_t)desc.group_count), stride(desc.data_texture_width * (uint32_t)desc.group_data_rows),
          tri_count(desc.vertex_count / 3)
    {
    }

    const float *link(int code, uint32_t node) const { return d.group_hitmiss + 2 * ((size_t)stride * code + node); }

    // every link is END or a node index; every leaf names existing triangles
    bool links_are_safe()
    {
        for (int code = 0; code < 8; code++) {
            for (uint32_t g = 0; g < n; g++) {
                for (int k = 0; k < 2; k++) {
                    const float v = link(code, g)[k];
                    if (v >= kTerminatorF)
                        continue;
                    if (!(v >= 0.0f) || v != floorf(v) || v >= (float)n) {
                        why = "a hit/miss link is neither a node index nor a terminator";
                        return false;
                    }
                }
                const bool leaf = link(code, g)[0] == link(code, g)[1];
                if (leaf) {
                    const float s = d.group_objects[2 * (size_t)g], c = d.group_objects[2 * (size_t)g + 1];
                    if (!(s >= 0.0f) || !(c >= 0.0f) || s != floorf(s) || c != floorf(c) ||
                        (double)s + (double)c > (double)tri_count) {
                        why = "a leaf's (start, count) does not name existing triangles";
                        return false;
                    }
                }
            }
        }
        return true;
    }

    // children + split axis of every branch, from the hit links alone
    bool recover_children()
    {
        neg.assign(n, -1);
        pos.assign(n, -1);
        axis.assign(n, 0);
        for (uint32_t g = 0; g < n; g++) {
            const float h0 = link(0, g)[0];
            bool leaf = h0 == link(0, g)[1];
            for (int code = 1; code < 8; code++)
                if ((link(code, g)[0] == link(code, g)[1]) != leaf)
                    return false;
            if (leaf)
                continue;
            // code 0 (all components <= 0) goes to the positive child first, code 7 to the negative
            const float p = h0, m = link(7, g)[0];
            if (p >= kTerminatorF || m >= kTerminatorF || p == m)
                return false;
            int found = -1;
            for (int k = 0; k < 3 && found < 0; k++) {
                bool ok = true;
                for (int code = 0; code < 8 && ok; code++)
                    ok = link(code, g)[0] == (((code >> k) & 1) ? m : p);
                if (ok)
                    found = k;
            }
            if (found < 0)
                return false;
            axis[g] = (uint8_t)found;
            neg[g] = (int32_t)m;
            pos[g] = (int32_t)p;
        }
        return true;
    }

    // Re-threads the recovered tree for each direction code and compares with
    // the tables given; also checks it is a tree that reaches all n nodes.
    bool tables_match(int *depth_out)
    {
        std::vector<uint32_t> stack;
        int depth = 0;
        for (int code = 0; code < 8; code++) {
            uint32_t visited = 0;
            stack.clear();
            int64_t g = d.tree_root;
            while (g >= 0) {
                if (++visited > n)
                    return false;   // a cycle
                const int64_t next_subtree = stack.empty() ? -1 : (int64_t)stack.back();
                const float expect_miss = next_subtree < 0 ? -1.0f : (float)next_subtree;
                const float got_hit = link(code, (uint32_t)g)[0], got_miss = link(code, (uint32_t)g)[1];
                auto same = [](float got, float expect) { return expect < 0 ? got >= kTerminatorF : got == expect; };
                int64_t go;
                if (neg[g] < 0) {
                    if (!same(got_hit, expect_miss) || !same(got_miss, expect_miss))
                        return false;
                    go = next_subtree;
                    if (!stack.empty())
                        stack.pop_back();
                } else {
                    const bool neg_first = (code >> axis[g]) & 1;
                    const int32_t near_child = neg_first ? neg[g] : pos[g];
                    const int32_t far_child = neg_first ? pos[g] : neg[g];
                    if (got_hit != (float)near_child || !same(got_miss, expect_miss))
                        return false;
                    stack.push_back((uint32_t)far_child);
                    depth = std::max(depth, (int)stack.size());
                    if (stack.size() > 64)
                        return false;   // hitmiss_max_stack_size, world.cpp:228
                    go = near_child;
                }
                g = go;
            }
            if (visited != n)
                return false;
        }
        *depth_out = depth;
        return true;
    }

    // The tree as ShrayDeviceTreeView holds it: pre-order (a node, its negative subtree, its positive subtree; the root at 0),
    // a branch's children as pre-order indices and its split direction as the unit vector of its axis, a leaf's (start,
    // count), and index_of[k] = the reference node at k.  Pre-order is the packed order (packed_layout.h).
    void preorder(PreorderTree &t) const
    {
        t.negative.assign(n, -1);
        t.positive.assign(n, -1);
        t.start.assign(n, 0);
        t.triangles.assign(n, 0);
        t.direction.assign(3 * (size_t)n, 0.0f);
        // (a node, where its parent names it): a node is numbered when it is taken, its negative subtree is taken next
        std::vector<std::pair<uint32_t, int32_t *>> todo(1, {(uint32_t)d.tree_root, nullptr});
        while (!todo.empty()) {
            const auto [g, named_at] = todo.back();
            todo.pop_back();
            const int32_t k = (int32_t)t.index_of.size();
            t.index_of.push_back((int32_t)g);
            if (named_at)
                *named_at = k;
            if (neg[g] >= 0) {
                t.direction[3 * (size_t)k + axis[g]] = 1.0f;
                todo.push_back({(uint32_t)pos[g], &t.positive[k]});
                todo.push_back({(uint32_t)neg[g], &t.negative[k]});
            } else {
                t.start[k] = (int32_t)d.group_objects[2 * (size_t)g];
                t.triangles[k] = (int32_t)d.group_objects[2 * (size_t)g + 1];
            }
        }
    }
};

}   // namespace shray
