// tree_order.h -- the packed tree's topology in height order: what the refit (refit/refit.hip), the winding-number derivation
// (winding/winding.hip) and the one-lane walks (point/packed_walk.h) learn from one octant copy read back to the host.  A node's
// HEIGHT is 0 for a leaf and one above its taller child for a branch: a branch reads only nodes of lower heights, and fewer
// nodes have height h than h - 1, so a bottom-up pass gives every wide height a launch and the narrow rest one workgroup that
// steps through them behind barriers (for_each_level).  The root's height is the tree's: the depth of a walk's stack.
// Plain C++17 over packed_layout.h: no HIP, and a refusal is a message for the caller's fail(SHRAY_ERR_BAD_TREE, ...), so that
// a host compiler can build this file alone (tests/native_tree_order.cpp).  Host-only, internal to the libraries.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "packed_layout.h"

namespace {

// topology of a packed node: a leaf {first triangle, count | kLeafFlag}, a branch {negative child, positive child} (indices).
// A kernel parameter type of the libraries that upload it: its name, layout and namespace are part of their kernels' names.
struct Topo {
    uint32_t x, y;
};

struct TreeOrder {
    std::vector<Topo> topo;               // per node
    std::vector<uint32_t> order;          // the nodes by ascending height
    std::vector<uint32_t> height_start;   // order[height_start[h] .. height_start[h + 1]) have height h; tallest + 2 entries
    uint32_t leaves = 0;                  // nodes of height 0
    uint32_t tallest = 0;                 // the largest height
    uint32_t tail_height = 1;             // the first height >= 1 with at most tail_width nodes (tallest + 1: there is none)
    int height = 0;                       // the root's height (every node is reached from it, so it is the tallest)
};

// The order of `n` records of octant copy `octant`, whose root has the name `root` (packed_layout.h: a name is a byte offset
// / 8), over a scene of `nt` triangles.  In copy 0 a' names the positive child and b' the negative, in copy 7 a' the negative
// and b' the positive; the other copies order their children by the node's axis and are not read here.  Returns "" and fills
// *out, or why the words are not a tree: the root or a child name that is not a record's or lies beyond the tree, a leaf's
// range beyond the triangles, a node reached twice, a node not reached.  The last refuses nothing a scene can hold: the packed
// tree is only ever written by scene creation, which numbers exactly the nodes it reaches from the root.
inline std::string tree_order(const shray::DeviceNode *nodes, uint32_t n, uint32_t root, uint32_t nt, int octant, uint32_t tail_width,
                              TreeOrder *out)
{
    using namespace shray;
    const auto text = [](const char *what, uint32_t a, uint32_t b) { return what + std::to_string(a) + " of " + std::to_string(b); };
    if (octant != 0 && octant != 7)
        return "only octant copies 0 and 7 order every node's children alike; asked for copy " + std::to_string(octant);
    const uint32_t per = (uint32_t)(sizeof(DeviceNode) >> kNodeNameShift);   // names per record
    if (root % per || root / per >= n)
        return text("the packed root is not a node: name ", root, n);
    std::vector<Topo> &topo = out->topo;
    topo.assign(n, Topo{0, 0});
    for (uint32_t k = 0; k < n; k++) {
        const DeviceNode &d = nodes[k];
        if (d.b & kLeafFlag) {
            if ((uint64_t)d.a + (d.b & ~kLeafFlag) > nt)
                return text("a packed leaf names triangles beyond the scene's: node ", k, n);
            topo[k] = {d.a, d.b};
        } else {
            const uint32_t first = d.a & kChildNameMask, other = d.b;
            const uint32_t neg = octant == 7 ? first : other, pos = octant == 7 ? other : first;
            if (neg % per || pos % per || neg / per >= n || pos / per >= n)
                return text("a packed node names a child that is not a node: node ", k, n);
            topo[k] = {neg / per, pos / per};
        }
    }
    // heights, by a post-order walk from the root (which also proves every node is reached once)
    std::vector<uint32_t> height(n, 0);
    std::vector<uint8_t> seen(n, 0);
    std::vector<std::pair<uint32_t, bool>> todo{{root / per, false}};
    uint32_t reached = 0, tallest = 0;
    while (!todo.empty()) {
        const auto [k, expanded] = todo.back();
        todo.pop_back();
        if (expanded) {
            height[k] = 1 + std::max(height[topo[k].x], height[topo[k].y]);
            tallest = std::max(tallest, height[k]);
            continue;
        }
        if (seen[k]++)
            return text("a packed node is reached twice: node ", k, n);
        reached++;
        if (!(topo[k].y & kLeafFlag)) {
            todo.push_back({k, true});
            todo.push_back({topo[k].x, false});
            todo.push_back({topo[k].y, false});
        }
    }
    if (reached != n)
        return text("the packed tree does not reach all its nodes: ", reached, n);
    // counting sort by height
    std::vector<uint32_t> &start = out->height_start;
    start.assign(tallest + 2, 0);
    for (uint32_t k = 0; k < n; k++)
        start[height[k] + 1]++;
    for (uint32_t h = 0; h <= tallest; h++)
        start[h + 1] += start[h];
    std::vector<uint32_t> next(start.begin(), start.end() - 1);
    out->order.resize(n);
    for (uint32_t k = 0; k < n; k++)
        out->order[next[height[k]]++] = k;
    out->leaves = start[1];
    out->tallest = tallest;
    out->tail_height = 1;
    while (out->tail_height <= tallest && start[out->tail_height + 1] - start[out->tail_height] > tail_width)
        out->tail_height++;
    out->height = (int)height[root / per];
    return std::string();
}

// The bottom-up schedule over a TreeOrder: leaves(count), then wide(begin, count) for the slice of `order` of each height
// below tail_height, then tail(first height, heights) for the rest when there is one.  Each returns an error code; the first
// that is not 0 ends the schedule and is returned.
template <typename Leaves, typename Wide, typename Tail>
int for_each_level(const TreeOrder &t, Leaves &&leaves, Wide &&wide, Tail &&tail)
{
    if (const int rc = leaves(t.leaves))
        return rc;
    for (uint32_t h = 1; h < t.tail_height; h++)
        if (const int rc = wide(t.height_start[h], t.height_start[h + 1] - t.height_start[h]))
            return rc;
    return t.tail_height <= t.tallest ? tail(t.tail_height, t.tallest + 1) : 0;
}

}   // namespace
