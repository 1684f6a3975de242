// The checks of tests/test_scene_tree_cpu.py on csrc/scene_tree.h: trees built here and threaded into the eight (hit, miss)
// tables by plain recursion, an independent restatement of what TreeBuilder proves.  Built with AddressSanitizer and
// UndefinedBehaviorSanitizer; every array has exactly the size the scene description states, so an index that strays is
// caught.  Usage: native_scene_tree shapes | random SEED | refusals.
// Prints one line per failed check and exits 1, or "ok" and exits 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "scene_tree.h"

using namespace shray;

namespace {

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

constexpr float kEnd = 16777215.0f;   // the shader's terminator, restated
const char *const kBadLink = "a hit/miss link is neither a node index nor a terminator";
const char *const kBadLeaf = "a leaf's (start, count) does not name existing triangles";

// a tree as the test describes it: per node, a leaf's triangle range or a branch's children and split axis
struct Plain {
    struct Node {
        bool leaf;
        uint32_t x, y;   // leaf: start, count; branch: negative, positive
        int axis;
    };
    std::vector<Node> nodes;
    uint32_t root = 0, triangles = 0;
};

// the arrays a scene description points to, each exactly as large as the description says
struct Tables {
    uint32_t width = 16, rows = 0, stride = 0;
    std::vector<float> hitmiss, objects;
    shray_scene_desc desc{};

    float *link(int code, uint32_t node) { return hitmiss.data() + 2 * ((size_t)stride * code + node); }
    const shray_scene_desc &describe(uint32_t n, uint32_t root, uint32_t triangles)
    {
        desc = shray_scene_desc{};
        desc.struct_size = sizeof(desc);
        desc.data_texture_width = width;
        desc.vertex_count = 3 * triangles;
        desc.group_count = (int32_t)n;
        desc.group_data_rows = (int32_t)rows;
        desc.tree_root = (int32_t)root;
        desc.group_hitmiss = hitmiss.data();
        desc.group_objects = objects.data();
        return desc;
    }
};

// the restatement: under direction code `code`, `node` is visited with `next` as the place to go when its subtree is done
void thread_tables(const Plain &t, Tables &out, int code, uint32_t node, float next)
{
    const Plain::Node &n = t.nodes[node];
    float *l = out.link(code, node);
    if (n.leaf) {
        l[0] = l[1] = next;
        return;
    }
    const bool negative_first = (code >> n.axis) & 1;
    const uint32_t near_child = negative_first ? n.x : n.y, far_child = negative_first ? n.y : n.x;
    l[0] = (float)near_child;
    l[1] = next;
    thread_tables(t, out, code, near_child, (float)far_child);
    thread_tables(t, out, code, far_child, next);
}

Tables tables_of(const Plain &t)
{
    Tables out;
    const uint32_t n = (uint32_t)t.nodes.size();
    out.rows = (n + out.width - 1) / out.width;
    out.stride = out.width * out.rows;
    out.hitmiss.assign((size_t)out.stride * 8 * 2, -7.0f);   // (the padding behind node n - 1 is never a valid link)
    out.objects.assign(2 * (size_t)n, 0.0f);
    for (int code = 0; code < 8; code++)
        thread_tables(t, out, code, t.root, kEnd);
    for (uint32_t k = 0; k < n; k++)
        if (t.nodes[k].leaf) {
            out.objects[2 * k] = (float)t.nodes[k].x;
            out.objects[2 * k + 1] = (float)t.nodes[k].y;
        }
    return out;
}

// pending far children while `node` is visited with `held` of them already waiting
int depth_of(const Plain &t, int code, uint32_t node, int held)
{
    const Plain::Node &n = t.nodes[node];
    if (n.leaf)
        return held;
    const bool negative_first = (code >> n.axis) & 1;
    const uint32_t near_child = negative_first ? n.x : n.y, far_child = negative_first ? n.y : n.x;
    return std::max(held + 1, std::max(depth_of(t, code, near_child, held + 1), depth_of(t, code, far_child, held)));
}

int32_t number_preorder(const Plain &t, uint32_t node, PreorderTree &p)
{
    const int32_t k = (int32_t)p.index_of.size();
    p.index_of.push_back((int32_t)node);
    const Plain::Node &n = t.nodes[node];
    if (n.leaf) {
        p.start[k] = (int32_t)n.x;
        p.triangles[k] = (int32_t)n.y;
    } else {
        p.direction[3 * (size_t)k + n.axis] = 1.0f;
        p.negative[k] = number_preorder(t, n.x, p);
        p.positive[k] = number_preorder(t, n.y, p);
    }
    return k;
}

// every accepted tree: the children and axes that were built, the recursion's depth, the recursion's pre-order arrays
void check_accepted(const Plain &t, const char *what, int expect_depth = -1)
{
    const uint32_t n = (uint32_t)t.nodes.size();
    Tables tab = tables_of(t);
    TreeBuilder tb(tab.describe(n, t.root, t.triangles));
    CHECK(tb.links_are_safe(), "%s: %s", what, tb.why.c_str());
    CHECK(tb.why.empty(), "%s: why is '%s'", what, tb.why.c_str());
    const bool recovered = tb.recover_children();
    CHECK(recovered, "%s", what);
    if (!recovered)
        return;
    CHECK(tb.neg.size() == n && tb.pos.size() == n && tb.axis.size() == n, "%s", what);
    for (uint32_t k = 0; k < n; k++) {
        const Plain::Node &p = t.nodes[k];
        if (p.leaf)
            CHECK(tb.neg[k] == -1 && tb.pos[k] == -1, "%s: leaf %u has children (%d, %d)", what, k, tb.neg[k], tb.pos[k]);
        else
            CHECK(tb.neg[k] == (int32_t)p.x && tb.pos[k] == (int32_t)p.y && tb.axis[k] == p.axis,
                  "%s: branch %u is (%d, %d) on axis %d, built (%u, %u) on axis %d", what, k, tb.neg[k], tb.pos[k], tb.axis[k], p.x, p.y, p.axis);
    }
    int depth = -1, want_depth = 0;
    const bool matched = tb.tables_match(&depth);
    CHECK(matched, "%s: the tables do not match", what);
    if (!matched)
        return;
    for (int code = 0; code < 8; code++)
        want_depth = std::max(want_depth, depth_of(t, code, t.root, 0));
    CHECK(depth == want_depth, "%s: depth %d, the recursion says %d", what, depth, want_depth);
    if (expect_depth >= 0)
        CHECK(depth == expect_depth, "%s: depth %d, expected %d", what, depth, expect_depth);

    PreorderTree got, want;
    tb.preorder(got);
    want.negative.assign(n, -1);
    want.positive.assign(n, -1);
    want.start.assign(n, 0);
    want.triangles.assign(n, 0);
    want.direction.assign(3 * (size_t)n, 0.0f);
    number_preorder(t, t.root, want);
    CHECK(got.index_of == want.index_of, "%s: index_of", what);
    CHECK(got.negative == want.negative && got.positive == want.positive, "%s: the children in pre-order", what);
    CHECK(got.start == want.start && got.triangles == want.triangles, "%s: the leaves' ranges", what);
    CHECK(got.direction == want.direction, "%s: the split directions", what);
}

// `leaves` leaves under node `at` (already allocated), split by `split(leaves)` -> the negative side's share
template <typename Split, typename Axis>
void grow(Plain &t, uint32_t at, uint32_t leaves, Split &&split, Axis &&axis, const std::vector<uint32_t> &name, uint32_t &next)
{
    if (leaves == 1) {
        const uint32_t count = at % 5;   // (empty leaves too)
        t.nodes[name[at]] = {true, t.triangles, count, 0};
        t.triangles += count;
        return;
    }
    const uint32_t neg = next++, pos = next++, share = split(leaves);
    t.nodes[name[at]] = {false, name[neg], name[pos], axis(at)};
    grow(t, neg, share, split, axis, name, next);
    grow(t, pos, leaves - share, split, axis, name, next);
}

template <typename Split, typename Axis>
Plain tree_of(uint32_t leaves, Split &&split, Axis &&axis, std::mt19937 *shuffle = nullptr)
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
    grow(t, 0, leaves, split, axis, name, next);
    return t;
}

// a one-sided chain of `branches` branches, the chain on the negative or the positive side, the axes in rotation
Plain chain_of(uint32_t branches, bool negative_side)
{
    const auto by_turns = [](uint32_t at) { return (int)(at % 3); };
    return negative_side ? tree_of(branches + 1, [](uint32_t leaves) { return leaves - 1; }, by_turns)
                         : tree_of(branches + 1, [](uint32_t) { return 1u; }, by_turns);
}

void shapes()
{
    const auto halves = [](uint32_t leaves) { return leaves / 2; };
    check_accepted(tree_of(1, halves, [](uint32_t) { return 0; }), "a single leaf", 0);
    for (int a = 0; a < 3; a++)
        check_accepted(tree_of(2, halves, [a](uint32_t) { return a; }), ("three nodes, axis " + std::to_string(a)).c_str(), 1);
    for (int side = 0; side < 2; side++)
        check_accepted(chain_of(64, side != 0), side ? "a chain 64 deep on the negative side" : "a chain 64 deep on the positive side", 64);
}

void random_trees(uint32_t seed)
{
    std::mt19937 rng(seed);
    for (int i = 0; i < 12; i++) {
        const uint32_t leaves = 100 + rng() % 200;         // 199 .. 597 nodes
        const int lean = (int)(rng() % 3);                 // any split; near the middle; lopsided, an eighth at the least
        const auto split = [&](uint32_t l) {               // (with these seeds every tree stays within the 64 levels)
            const uint32_t low = lean == 0 ? 1u : std::max(1u, lean == 1 ? l / 3 : l / 8), high = lean == 0 ? l - 1 : std::max(low, l / 2);
            const uint32_t share = low + rng() % (high - low + 1);
            return (rng() & 1) ? l - share : share;
        };
        const Plain t = tree_of(leaves, split, [&](uint32_t) { return (int)(rng() % 3); }, &rng);
        check_accepted(t, ("random tree " + std::to_string(i) + " of seed " + std::to_string(seed)).c_str());
    }
}

enum Stage { kLinks, kChildren, kTables };

// `tab` must be refused at `stage`, every stage before it passing, with `why` (empty for the stages that give none)
void check_refused(Tables &tab, uint32_t n, uint32_t root, uint32_t triangles, Stage stage, const char *why, const char *what)
{
    TreeBuilder tb(tab.describe(n, root, triangles));
    const bool safe = tb.links_are_safe();
    if (stage == kLinks) {
        CHECK(!safe, "%s: the links passed", what);
        CHECK(tb.why == why, "%s: why is '%s'", what, tb.why.c_str());
        return;
    }
    CHECK(safe && tb.why.empty(), "%s: refused too early, '%s'", what, tb.why.c_str());
    if (!safe)
        return;
    const bool recovered = tb.recover_children();
    if (stage == kChildren) {
        CHECK(!recovered, "%s: the children were recovered", what);
        CHECK(tb.why == why, "%s: why is '%s'", what, tb.why.c_str());
        return;
    }
    CHECK(recovered, "%s: refused too early, by recover_children", what);
    if (!recovered)
        return;
    int depth = -1;
    CHECK(!tb.tables_match(&depth), "%s: the tables matched, depth %d", what, depth);
    CHECK(tb.why == why, "%s: why is '%s'", what, tb.why.c_str());
}

void refusals()
{
    for (int side = 0; side < 2; side++) {
        const Plain t = chain_of(65, side != 0);
        Tables tab = tables_of(t);
        check_refused(tab, (uint32_t)t.nodes.size(), t.root, t.triangles, kTables, "", "a chain that needs 65 levels");
    }

    Plain t;   // 0: (1: (2, 3), 4: (5, 6)), the branches on axes 0, 1, 2
    t.nodes = {{false, 1, 4, 0}, {false, 2, 3, 1}, {true, 0, 2, 0}, {true, 2, 1, 0}, {false, 5, 6, 2}, {true, 3, 0, 0}, {true, 3, 2, 0}};
    t.triangles = 5;
    const uint32_t n = 7;
    check_accepted(t, "the tree the refusals start from", 2);
    const Tables good = tables_of(t);

    // links that are no node index: in a hit and in a miss, in the first and in the last table
    const float bad_links[] = {-1.0f, std::numeric_limits<float>::quiet_NaN(), 2.5f, (float)n, (float)(n + 9), -std::numeric_limits<float>::infinity()};
    for (float v : bad_links)
        for (int code : {0, 7})
            for (int k = 0; k < 2; k++) {
                Tables bad = good;
                bad.link(code, 4)[k] = v;
                check_refused(bad, n, 0, t.triangles, kLinks, kBadLink, ("a link of " + std::to_string(v)).c_str());
            }
    // leaves that name no existing triangles: (start, count) of leaf 6 is (3, 2), of 5 triangles
    const float bad_leaves[][2] = {{3.0f, 3.0f}, {4.0f, 2.0f}, {-1.0f, 2.0f}, {3.0f, -1.0f}, {2.5f, 2.0f}, {3.0f, 1.5f},
                                   {std::numeric_limits<float>::quiet_NaN(), 1.0f}, {0.0f, std::numeric_limits<float>::infinity()}, {16777216.0f, 16777216.0f}};
    for (const float *leaf : bad_leaves) {
        Tables bad = good;
        bad.objects[2 * 6] = leaf[0];
        bad.objects[2 * 6 + 1] = leaf[1];
        check_refused(bad, n, 0, t.triangles, kLinks, kBadLeaf, ("a leaf of (" + std::to_string(leaf[0]) + ", " + std::to_string(leaf[1]) + ")").c_str());
    }
    {
        Tables ok = good;   // (a branch's entry of group_objects is not a leaf's range: it is not read)
        ok.objects[2 * 4] = -3.5f;
        TreeBuilder tb(ok.describe(n, 0, t.triangles));
        CHECK(tb.links_are_safe(), "a branch's unused (start, count): %s", tb.why.c_str());
    }
    {
        Tables bad = good;   // a leaf under seven direction codes, a branch under code 3
        bad.link(3, 2)[0] = 5.0f;
        check_refused(bad, n, 0, t.triangles, kChildren, "", "a node that is a leaf under one code and a branch under another");
        bad = good;          // ... and a branch that is a leaf under code 5
        bad.link(5, 4)[0] = bad.link(5, 4)[1];
        check_refused(bad, n, 0, t.triangles, kChildren, "", "a node that is a branch under one code and a leaf under another");
    }
    {
        Tables bad = good;   // node 1's hit links: its positive child under codes 0, 1, 2 and 4, which no axis explains
        for (int code : {1, 2, 4})
            bad.link(code, 1)[0] = bad.link(0, 1)[0];
        check_refused(bad, n, 0, t.triangles, kChildren, "", "a branch whose hit links fit no axis");
    }
    {
        Tables bad = good;   // p == m
        const float p = bad.link(0, 4)[0];
        for (int code = 0; code < 8; code++)
            bad.link(code, 4)[0] = p;
        check_refused(bad, n, 0, t.triangles, kChildren, "", "a branch with p == m");
    }
    {
        Tables bad = good;   // the last leaf of every code's walk goes back to the root instead of stopping
        for (int code = 0; code < 8; code++)
            for (uint32_t g = 0; g < n; g++)
                if (bad.link(code, g)[0] >= kEnd && bad.link(code, g)[1] >= kEnd)
                    bad.link(code, g)[0] = bad.link(code, g)[1] = 0.0f;
        check_refused(bad, n, 0, t.triangles, kTables, "", "a miss link that closes a cycle");
        bad = good;          // a branch's miss link back to its own parent: every table still has its terminator
        for (int code = 0; code < 8; code++)
            if (bad.link(code, 1)[1] < kEnd)
                bad.link(code, 1)[1] = 0.0f;
        check_refused(bad, n, 0, t.triangles, kTables, "", "a branch's miss link that closes a cycle");
    }
    {
        Plain more = t;      // an eighth node that nothing names
        more.nodes.push_back({true, 0, 0, 0});
        Tables bad = tables_of(more);
        for (int code = 0; code < 8; code++)
            bad.link(code, 7)[0] = bad.link(code, 7)[1] = kEnd;
        check_refused(bad, n + 1, 0, t.triangles, kTables, "", "a tree that does not reach all its nodes");
        // ... and the subtree under node 1 taken as the whole: three of the seven nodes
        Tables sub = good;
        check_refused(sub, n, 1, t.triangles, kTables, "", "a root whose tree does not reach all the nodes");
    }
    {
        std::string why;     // the float32 index range: 2^24 link texels and 2^24 vertices pass, one more row or vertex does not
        shray_scene_desc d{};
        d.data_texture_width = 2048;
        d.group_data_rows = 1024;
        d.vertex_count = 16777216u;
        CHECK(check_index_range(d, &why) && why.empty(), "the largest scene: %s", why.c_str());
        d.group_data_rows = 1025;
        CHECK(!check_index_range(d, &why) && why.find("16793600 link texels") != std::string::npos, "one row too many: '%s'", why.c_str());
        d.group_data_rows = 1024;
        d.vertex_count = 16777217u;
        why.clear();
        CHECK(!check_index_range(d, &why) && why.find("16777217 vertices") != std::string::npos, "one vertex too many: '%s'", why.c_str());
    }
}

}   // namespace

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "shapes")
        shapes();
    else if (what == "random" && argc == 3)
        random_trees((uint32_t)atoi(argv[2]));
    else if (what == "refusals")
        refusals();
    else
        return 2;
    if (!failures)
        printf("ok\n");
    return failures ? 1 : 0;
}
