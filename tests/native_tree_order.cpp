// The checks of tests/test_tree_order_cpu.py on csrc/tree_order.h: hand-built DeviceNode arrays in both octant conventions
// against a plain recursive height computation.  Usage: native_tree_order shapes | edges | random SEED COUNT | refusals.
// Prints one line per failed check and exits 1, or "ok" and exits 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "tree_order.h"

using namespace shray;

namespace {

constexpr uint32_t kTailWidth = 1024;
constexpr uint32_t kPer = sizeof(DeviceNode) >> kNodeNameShift;
int failures = 0;

#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            failures++;                                     \
            printf("FAILED %s: ", #cond);                   \
            printf(__VA_ARGS__);                            \
            printf("\n");                                   \
        }                                                   \
    } while (0)

// a tree as the test describes it: per node, a leaf's triangle range or a branch's children
struct Plain {
    struct Node {
        bool leaf;
        uint32_t x, y;   // leaf: first, count; branch: negative, positive
        int axis;
    };
    std::vector<Node> nodes;
    uint32_t root = 0, triangles = 0;
};

std::vector<DeviceNode> encode(const Plain &t, int octant)
{
    std::vector<DeviceNode> out(t.nodes.size());
    for (size_t k = 0; k < out.size(); k++) {
        const Plain::Node &n = t.nodes[k];
        DeviceNode d{};
        if (n.leaf) {
            d.a = n.x;
            d.b = kLeafFlag | n.y;
        } else {
            const uint32_t first = octant == 7 ? n.x : n.y, other = octant == 7 ? n.y : n.x;
            d.a = (1u << (kAxisHotShift + n.axis)) | (first * kPer);
            d.b = other * kPer;
        }
        out[k] = d;
    }
    return out;
}

// the reference: a node's height by plain recursion
uint32_t height_of(const Plain &t, uint32_t k, std::vector<uint32_t> &height)
{
    const Plain::Node &n = t.nodes[k];
    return height[k] = n.leaf ? 0 : 1 + std::max(height_of(t, n.x, height), height_of(t, n.y, height));
}

void check_tree(const Plain &t, const char *what)
{
    const uint32_t n = (uint32_t)t.nodes.size();
    std::vector<uint32_t> want(n, ~0u);
    height_of(t, t.root, want);
    const uint32_t tallest = *std::max_element(want.begin(), want.end());
    std::vector<uint32_t> width(tallest + 1, 0);
    for (uint32_t h : want)
        width[h]++;
    uint32_t tail_height = 1;
    while (tail_height <= tallest && width[tail_height] > kTailWidth)
        tail_height++;

    TreeOrder got[2];
    for (int c = 0; c < 2; c++) {
        const int octant = c ? 7 : 0;
        const std::vector<DeviceNode> nodes = encode(t, octant);
        TreeOrder &r = got[c];
        const std::string refused = tree_order(nodes.data(), n, t.root * kPer, t.triangles, octant, kTailWidth, &r);
        CHECK(refused.empty(), "%s, copy %d: %s", what, octant, refused.c_str());
        if (!refused.empty())
            return;
        // the topology as the test described it
        CHECK(r.topo.size() == n, "%s", what);
        for (uint32_t k = 0; k < n; k++) {
            const Plain::Node &p = t.nodes[k];
            CHECK(r.topo[k].x == p.x && r.topo[k].y == (p.leaf ? (p.y | kLeafFlag) : p.y), "%s, copy %d, node %u", what, octant, k);
        }
        // order is a permutation, along which the heights ascend; height_start brackets each height
        CHECK(r.order.size() == n && r.height_start.size() == tallest + 2, "%s", what);
        CHECK(r.height_start.front() == 0 && r.height_start.back() == n, "%s", what);
        std::vector<uint32_t> height(n, ~0u), times(n, 0);
        for (uint32_t h = 0; h <= tallest; h++) {
            CHECK(r.height_start[h + 1] - r.height_start[h] == width[h], "%s, copy %d, height %u", what, octant, h);
            for (uint32_t i = r.height_start[h]; i < r.height_start[h + 1] && i < n; i++) {
                CHECK(r.order[i] < n, "%s", what);
                times[r.order[i] % n]++;
                height[r.order[i] % n] = h;
            }
        }
        for (uint32_t i = 1; i < n; i++)
            CHECK(height[r.order[i - 1]] <= height[r.order[i]], "%s, copy %d, position %u", what, octant, i);
        for (uint32_t k = 0; k < n; k++) {
            CHECK(times[k] == 1, "%s, copy %d: node %u is in the order %u times", what, octant, k, times[k]);
            CHECK(height[k] == want[k], "%s, copy %d: node %u at height %u, recursion says %u", what, octant, k, height[k], want[k]);
            // every branch sits one above its taller child
            if (!t.nodes[k].leaf)
                CHECK(height[k] == 1 + std::max(height[r.topo[k].x], height[r.topo[k].y]), "%s, copy %d, node %u", what, octant, k);
        }
        CHECK(r.leaves == width[0], "%s: %u leaves, %u counted", what, r.leaves, width[0]);
        CHECK(r.tallest == tallest && r.height == (int)want[t.root], "%s: tallest %u, height %d", what, r.tallest, r.height);
        CHECK(r.tail_height == tail_height, "%s: tail_height %u, expected %u", what, r.tail_height, tail_height);
        // the schedule: the leaves, each wide height's slice, the rest
        uint32_t leaves = ~0u, next_height = 1, tail_first = 0, tail_heights = 0, tails = 0;
        const int rc = for_each_level(
            r, [&](uint32_t count) { return leaves = count, 0; },
            [&](uint32_t begin, uint32_t count) {
                CHECK(begin == r.height_start[next_height] && count == width[next_height] && count > kTailWidth, "%s, height %u", what,
                      next_height);
                next_height++;
                return 0;
            },
            [&](uint32_t first, uint32_t heights) { return tails++, tail_first = first, tail_heights = heights, 0; });
        CHECK(rc == 0 && leaves == width[0] && next_height == tail_height, "%s: the schedule", what);
        CHECK(tail_height <= tallest ? (tails == 1 && tail_first == tail_height && tail_heights == tallest + 1) : tails == 0, "%s: the tail", what);
        CHECK(for_each_level(r, [](uint32_t) { return 5; }, [](uint32_t, uint32_t) { return 6; }, [](uint32_t, uint32_t) { return 7; }) == 5,
              "%s: the first error ends the schedule", what);
    }
    // conventions 0 and 7 give the same Topo
    CHECK(got[0].topo.size() == got[1].topo.size() &&
              !memcmp(got[0].topo.data(), got[1].topo.data(), got[0].topo.size() * sizeof(Topo)), "%s: the copies' topologies differ", what);
    CHECK(got[0].order == got[1].order && got[0].height_start == got[1].height_start, "%s: the copies' orders differ", what);
}

// `leaves` leaves under node `at` (already allocated), split by `split(leaves)` -> the negative side's share
template <typename Split>
void grow(Plain &t, uint32_t at, uint32_t leaves, Split &&split, const std::vector<uint32_t> &name, uint32_t &next)
{
    if (leaves == 1) {
        const uint32_t count = at % 5;   // (empty leaves too)
        t.nodes[name[at]] = {true, t.triangles, count, 0};
        t.triangles += count;
        return;
    }
    const uint32_t neg = next++, pos = next++, share = split(leaves);
    t.nodes[name[at]] = {false, name[neg], name[pos], (int)(at % 3)};
    grow(t, neg, share, split, name, next);
    grow(t, pos, leaves - share, split, name, next);
}

template <typename Split>
Plain tree_of(uint32_t leaves, Split &&split, std::mt19937 *shuffle = nullptr)
{
    Plain t;
    const uint32_t n = 2 * leaves - 1;
    t.nodes.resize(n);
    std::vector<uint32_t> name(n);
    for (uint32_t k = 0; k < n; k++)
        name[k] = k;
    if (shuffle)
        std::shuffle(name.begin(), name.end(), *shuffle);
    uint32_t next = 1;
    t.root = name[0];
    grow(t, 0, leaves, split, name, next);
    return t;
}

void shapes()
{
    const auto halves = [](uint32_t leaves) { return leaves / 2; };
    const auto one = [](uint32_t) { return 1u; };
    TreeOrder r;
    {
        const Plain t = tree_of(1, halves);
        check_tree(t, "a single leaf");
        tree_order(encode(t, 7).data(), 1, 0, t.triangles, 7, kTailWidth, &r);
        CHECK(r.height == 0 && r.leaves == 1 && r.tail_height == 1, "a single leaf: height %d, leaves %u, tail %u", r.height, r.leaves, r.tail_height);
    }
    {
        const Plain t = tree_of(2, halves);
        check_tree(t, "three nodes");
        tree_order(encode(t, 0).data(), 3, 0, t.triangles, 0, kTailWidth, &r);
        CHECK(r.height == 1 && r.leaves == 2 && r.tail_height == 1 && r.order[2] == 0, "three nodes");
    }
    for (int side = 0; side < 2; side++) {
        // one-sided, 130 edges deep: above SHRAY_POINT_MAX_HEIGHT (128); the height is reported, not refused here
        const Plain t = side ? tree_of(131, one) : tree_of(131, [](uint32_t leaves) { return leaves - 1; });
        check_tree(t, "a chain");
        tree_order(encode(t, 7).data(), 261, 0, t.triangles, 7, kTailWidth, &r);
        CHECK(r.height == 130 && r.leaves == 131 && r.tail_height == 1, "a chain: height %d", r.height);
    }
    {
        // complete, 4096 leaves: 2048 branches of height 1 (above the tail width), exactly 1024 of height 2 (not above it)
        const Plain t = tree_of(4096, halves);
        check_tree(t, "a complete tree");
        tree_order(encode(t, 0).data(), 8191, 0, t.triangles, 0, kTailWidth, &r);
        CHECK(r.height == 12 && r.leaves == 4096 && r.tail_height == 2, "a complete tree: height %d, tail %u", r.height, r.tail_height);
        CHECK(r.height_start[2] - r.height_start[1] == 2048 && r.height_start[3] - r.height_start[2] == 1024, "a complete tree's widths");
    }
}

// a new root over two trees: node 0, then `neg`'s nodes, then `pos`'s (their roots must be their node 0)
Plain join(const Plain &neg, const Plain &pos)
{
    Plain t;
    t.nodes.push_back({false, 1, 1 + (uint32_t)neg.nodes.size(), 0});
    const auto append = [&](const Plain &from) {
        const uint32_t nodes = (uint32_t)t.nodes.size(), triangles = t.triangles;
        for (Plain::Node n : from.nodes) {
            if (n.leaf)
                n.x += triangles;
            else
                n.x += nodes, n.y += nodes;
            t.nodes.push_back(n);
        }
        t.triangles += from.triangles;
    };
    append(neg);
    append(pos);
    return t;
}

// The schedule of a tree shaped to its edges (tests/tree_shapes.py builds the same shapes for the GPU tests): the leaves, the
// tallest height, where the tail starts, and exactly the wide(begin, count) and tail(first, heights) calls for_each_level
// makes for a tail of kTailWidth threads.
void check_schedule(const Plain &t, const char *what, uint32_t leaves, uint32_t tallest, uint32_t tail_height,
                    const std::vector<uint32_t> &wide_counts)
{
    check_tree(t, what);
    const uint32_t n = (uint32_t)t.nodes.size();
    for (int octant : {0, 7}) {
        TreeOrder r;
        const std::string refused = tree_order(encode(t, octant).data(), n, t.root * kPer, t.triangles, octant, kTailWidth, &r);
        CHECK(refused.empty(), "%s, copy %d: %s", what, octant, refused.c_str());
        if (!refused.empty())
            return;
        CHECK(r.leaves == leaves && r.tallest == tallest && r.height == (int)tallest && r.tail_height == tail_height,
              "%s, copy %d: %u leaves, tallest %u, height %d, tail_height %u", what, octant, r.leaves, r.tallest, r.height, r.tail_height);
        CHECK(r.height_start.size() == tallest + 2, "%s, copy %d: %zu entries of height_start", what, octant, r.height_start.size());
        std::vector<std::pair<uint32_t, uint32_t>> wide, tail;
        uint32_t leaf_calls = 0, leaf_count = 0;
        const int rc = for_each_level(
            r, [&](uint32_t count) { return leaf_calls++, leaf_count = count, 0; },
            [&](uint32_t begin, uint32_t count) { return wide.push_back({begin, count}), 0; },
            [&](uint32_t first, uint32_t heights) { return tail.push_back({first, heights}), 0; });
        CHECK(rc == 0 && leaf_calls == 1 && leaf_count == leaves, "%s, copy %d: the leaves' call", what, octant);
        CHECK(wide.size() == wide_counts.size(), "%s, copy %d: %zu wide calls, expected %zu", what, octant, wide.size(), wide_counts.size());
        uint32_t begin = leaves;
        for (size_t i = 0; i < wide.size() && i < wide_counts.size(); i++) {
            CHECK(wide[i].first == begin && wide[i].second == wide_counts[i], "%s, copy %d: wide call %zu is (%u, %u), expected (%u, %u)",
                  what, octant, i, wide[i].first, wide[i].second, begin, wide_counts[i]);
            begin += wide_counts[i];
        }
        if (tail_height <= tallest) {
            CHECK(tail.size() == 1 && tail[0].first == tail_height && tail[0].second == tallest + 1,
                  "%s, copy %d: %zu tail calls, the first (%u, %u)", what, octant, tail.size(), tail.empty() ? 0 : tail[0].first,
                  tail.empty() ? 0 : tail[0].second);
            // the tail picks up where the wide launches stopped, and its first height fits the workgroup
            CHECK(r.height_start[tail_height] == begin && r.height_start[tail_height + 1] - begin <= kTailWidth, "%s, copy %d: the tail's start",
                  what, octant);
        } else {
            CHECK(tail.empty(), "%s, copy %d: a tail call for a tree without a tail", what, octant);
        }
    }
}

void edge_shapes()
{
    const auto halves = [](uint32_t leaves) { return leaves / 2; };
    const auto perfect = [&](int k) { return tree_of(1u << k, halves); };
    check_schedule(perfect(1), "one_branch", 2, 1, 1, {});
    check_schedule(perfect(11), "tail_full", 2048, 11, 1, {});                       // height 1: exactly 1024
    check_schedule(join(perfect(11), perfect(1)), "wide_by_one", 2050, 12, 2, {1025});
    check_schedule(perfect(13), "two_wide", 8192, 13, 3, {4096, 2048});              // height 3: exactly 1024
    Plain spine = perfect(0);
    for (int i = 0; i < 13; i++)
        spine = join(perfect(i), spine);
    check_schedule(spine, "lopsided", 8192, 13, 3, {4096, 2048});
    spine = perfect(12);
    for (int k : {1, 2, 1, 2})
        spine = join(perfect(k), spine);
    check_schedule(spine, "mixed_spine", 4108, 16, 3, {2054, 1026});
    {
        // the widths the shapes are built around
        TreeOrder r;
        const Plain t = perfect(11), w = join(perfect(11), perfect(1));
        tree_order(encode(t, 0).data(), (uint32_t)t.nodes.size(), 0, t.triangles, 0, kTailWidth, &r);
        CHECK(r.height_start[2] - r.height_start[1] == kTailWidth, "tail_full: %u branches of height 1", r.height_start[2] - r.height_start[1]);
        tree_order(encode(w, 0).data(), (uint32_t)w.nodes.size(), 0, w.triangles, 0, kTailWidth, &r);
        CHECK(r.height_start[2] - r.height_start[1] == kTailWidth + 1, "wide_by_one: %u branches of height 1", r.height_start[2] - r.height_start[1]);
    }
}

void random_trees(uint32_t seed, int count)
{
    std::mt19937 rng(seed);
    for (int i = 0; i < count; i++) {
        const uint32_t leaves = 1 + rng() % 1000;          // up to 1999 nodes
        const int lean = (int)(rng() % 4);                 // balanced-ish ... nearly a chain
        const auto split = [&](uint32_t l) {
            const uint32_t span = lean == 3 ? std::min(l - 1, 3u) : l - 1;
            const uint32_t share = 1 + rng() % span;
            return (lean & 1) ? l - share : share;
        };
        const Plain t = tree_of(leaves, split, &rng);
        check_tree(t, ("random tree " + std::to_string(i) + " of seed " + std::to_string(seed)).c_str());
    }
}

void refusals()
{
    Plain t;   // 0: (1: (2, 3), 4: (5, 6))
    t.nodes = {{false, 1, 4, 0}, {false, 2, 3, 1}, {true, 0, 2, 0}, {true, 2, 1, 0}, {false, 5, 6, 2}, {true, 3, 0, 0}, {true, 3, 2, 0}};
    t.triangles = 5;
    const uint32_t n = 7;
    TreeOrder r;
    for (int c = 0; c < 2; c++) {
        const int octant = c ? 7 : 0;
        const std::vector<DeviceNode> good = encode(t, octant);
        const auto refused = [&](const std::vector<DeviceNode> &nodes, uint32_t root, uint32_t triangles) {
            return !tree_order(nodes.data(), (uint32_t)nodes.size(), root, triangles, octant, kTailWidth, &r).empty();
        };
        CHECK(!refused(good, 0, t.triangles), "the tree itself, copy %d", octant);
        std::vector<DeviceNode> bad = good;
        bad[1].b += 1;
        CHECK(refused(bad, 0, t.triangles), "a child name that is not a multiple of the record size, copy %d", octant);
        bad = good;
        bad[4].a = (bad[4].a & ~kChildNameMask) | (n * kPer);
        CHECK(refused(bad, 0, t.triangles), "a child beyond the tree (a'), copy %d", octant);
        bad = good;
        bad[4].b = n * kPer;
        CHECK(refused(bad, 0, t.triangles), "a child beyond the tree (b'), copy %d", octant);
        CHECK(t.triangles > 0 && refused(good, 0, t.triangles - 1), "a leaf range beyond the triangle count, copy %d", octant);
        bad = good;
        bad[4].b = bad[1].b;
        CHECK(refused(bad, 0, t.triangles), "a node named by two parents, copy %d", octant);
        Plain shared;   // ... and with every node reached: 0: (1, 2), 1: (2, 3)
        shared.nodes = {{false, 1, 2, 0}, {false, 2, 3, 1}, {true, 0, 1, 0}, {true, 1, 1, 0}};
        CHECK(refused(encode(shared, octant), 0, 2), "a node named by two parents, all reached, copy %d", octant);
        bad = good;
        bad.push_back(good[6]);
        CHECK(refused(bad, 0, t.triangles), "a tree with an unreachable node, copy %d", octant);
        CHECK(refused(good, 2, t.triangles) && refused(good, n * kPer, t.triangles), "a root that is not a node, copy %d", octant);
    }
    CHECK(!tree_order(encode(t, 7).data(), n, 0, t.triangles, 3, kTailWidth, &r).empty(), "a copy that orders its children by axis");
}

}   // namespace

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "shapes")
        shapes();
    else if (what == "edges")
        edge_shapes();
    else if (what == "random" && argc == 4)
        random_trees((uint32_t)atoi(argv[2]), atoi(argv[3]));
    else if (what == "refusals")
        refusals();
    else
        return 2;
    if (!failures)
        printf("ok\n");
    return failures ? 1 : 0;
}
