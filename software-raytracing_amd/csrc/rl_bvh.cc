// Host BVH builder: binned-SAH BVH2 over triangle bounds, emitted as 64-byte
// two-box nodes (rl_device.h DNode).
//
// The reference builds three nested levels of random-axis median-split trees with
// a std::sort per node (reference geom/bvh.cc:10-80, geom/static_mesh.cc:80-95,
// loader/obj_loader.cc:236-245, geom/scene.cc:23-31).  Tree topology is not part
// of results parity -- closest hit is the minimum t over all triangles whichever
// way they are grouped -- so this builder is free to produce
// ONE flat tree whose shape suits a GPU: SAH splits (fewer nodes touched per
// ray), <= 4 triangles per leaf stored contiguously, both child boxes in the
// parent so a lane decides two children per 64-byte fetch.
#include "rl_host.h"
#include "rl_oracle.h"   // TriangleM1Host, and rl_slack.h's RL_BOX_WIDEN
#include "rl_grid.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <thread>

namespace rl {
namespace {

struct Box {
	f3 mn, mx;
	void reset() { mn = F3(FLT_MAX, FLT_MAX, FLT_MAX); mx = F3(-FLT_MAX, -FLT_MAX, -FLT_MAX); }
	void grow(const f3& p) { mn = fmin3(mn, p); mx = fmax3(mx, p); }
	void grow(const Box& b) { mn = fmin3(mn, b.mn); mx = fmax3(mx, b.mx); }
	float halfArea() const {
		f3 d = mx - mn;
		if (d.x < 0 || d.y < 0 || d.z < 0) return 0.0f;
		return d.x * d.y + d.y * d.z + d.z * d.x;
	}
};
inline float axisOf(const f3& v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }

struct TmpNode {
	Box box;
	int32_t left = -1, right = -1;   // TmpNode indices; -1 => leaf
	uint32_t first = 0, count = 0;
	// soft: a leaf of the binary builder (<= kMaxLeaf triangles, first / count) that carries a split of its triangles below it for the 8-wide plan to open where a
	// node has slots to spare (SplitLeaves); dead: below a soft node the plan left closed (not part of any tree)
	uint8_t soft = 0, dead = 0;
};

constexpr int kBins = 16;
constexpr uint32_t kMaxLeaf = 4;
constexpr float kCostTraverse = 1.0f, kCostTri = 1.0f;

// Work shared by the build threads.  The tree is the one a single thread would build, whatever the thread count:
// bin boxes and counts are min/max/integer sums (order-free), the partition is the serial std::partition on the same
// input order, sub-trees below a size threshold are built as independent tasks on disjoint ranges of `order`, and the
// final node array is re-emitted in the serial build's pre-order.
struct Shared {
	std::vector<uint8_t> kind;      // per primitive: PRIM_TRIANGLE / PRIM_SPHERE / PRIM_CUBE
	std::vector<Box> triBox;
	std::vector<f3> centroid;
	std::vector<uint32_t> order;
	unsigned threads = 1;
	uint32_t taskSize = 0;          // ranges of at most this many primitives become tasks (0: no tasks)
};

struct Task { uint32_t b, e, depth; };

struct Ctx {
	std::vector<TmpNode> tmp;
	std::vector<Task>* tasks = nullptr;   // only the top-level context spawns tasks
};

struct BinSet {
	Box box[3][kBins]; uint32_t count[3][kBins];
	void reset() { for (int a = 0; a < 3; ++a) for (int k = 0; k < kBins; ++k) { box[a][k].reset(); count[a][k] = 0; } }
	void merge(const BinSet& o) { for (int a = 0; a < 3; ++a) for (int k = 0; k < kBins; ++k) { box[a][k].grow(o.box[a][k]); count[a][k] += o.count[a][k]; } }
};

constexpr size_t kLeafListMax = 4 * RL_LEAFLIST_RECORDS;   // leaves of the leaf list (rl_device.h)
constexpr uint32_t kMedianSplitDepth = 36;      // see build(): SAH splits above, median splits from here on -> depth <= 36 + 25 < 64
constexpr uint32_t kParallelRange = 1u << 17;   // ranges at least this long are scanned by all threads
// below these sizes a stage runs on the calling thread: the build (primitives), the grid copy of the 4-wide tree and the emission of the 8-wide one (nodes)
constexpr size_t kThreadedBuild = 1u << 16, kThreadedQuantize = 1u << 16, kThreadedEmit8 = 1u << 15;

// threads of a stage over `count` items: RAYLIB_BUILD_THREADS, else the host's (capped at 32; a host that does not say how many it has counts as one);
// stages under their threshold run on the calling thread
unsigned ThreadsFor(size_t count, size_t threshold)
{
	if (count < threshold) return 1u;
	unsigned threads = std::thread::hardware_concurrency();
	if (const char* e = getenv("RAYLIB_BUILD_THREADS")) { int v = atoi(e); if (v > 0) threads = (unsigned)v; }
	return std::max(1u, std::min(32u, threads));
}

// fn(cb, ce, t) on the chunks of ceil(n / threads) items of [b, e), chunk t on thread t: chunk 0 on the caller, the others on threads that are joined before
// this returns.  No caller's result depends on where the chunk boundaries fall.
template <typename F>
void ParallelFor(unsigned threads, size_t b, size_t e, F&& fn)
{
	const size_t n = e - b;
	if (threads <= 1) { fn(b, e, 0u); return; }
	std::vector<std::thread> pool;
	const size_t per = (n + threads - 1) / threads;
	for (unsigned t = 1; t < threads; ++t) {
		const size_t cb = b + std::min(n, t * per), ce = b + std::min(n, (t + 1) * per);
		if (cb < ce) pool.emplace_back([&fn, cb, ce, t]() { fn(cb, ce, t); });
	}
	fn(b, b + std::min(n, per), 0u);
	for (std::thread& th : pool) th.join();
}

// build()'s scans: short ranges are not worth the threads
template <typename F>
void ParallelChunks(unsigned threads, uint32_t b, uint32_t e, F&& fn)
{
	if (e - b < kParallelRange) { fn(b, e, 0u); return; }
	ParallelFor(threads, b, e, [&fn](size_t cb, size_t ce, unsigned t) { fn((uint32_t)cb, (uint32_t)ce, t); });
}

// a leaf is either <= kMaxLeaf triangles or exactly one analytic primitive
bool leafAllowed(const Shared& S, uint32_t b, uint32_t e)
{
	if (e - b == 1) return true;
	if (e - b > kMaxLeaf) return false;
	for (uint32_t i = b; i < e; ++i) if (S.kind[S.order[i]] != PRIM_TRIANGLE) return false;
	return true;
}

int32_t build(Shared& S, Ctx& C, uint32_t b, uint32_t e, uint32_t depth)
{
	const uint32_t n = e - b;
	const int32_t self = (int32_t)C.tmp.size();
	C.tmp.push_back(TmpNode());
	if (C.tasks && n <= S.taskSize && n > 1) {
		// built later by a worker; the placeholder keeps this node's place in the pre-order
		C.tmp[self].left = -2 - (int32_t)C.tasks->size();
		C.tasks->push_back({ b, e, depth });
		return self;
	}
	const unsigned threads = C.tasks ? S.threads : 1u;

	// long ranges of the top levels are scanned by all threads (per-thread partial results, merged in thread order:
	// min / max / integer sums, so the merge order does not matter)
	const bool wide = threads > 1 && n >= kParallelRange;

	// bounds of the boxes and of the centroids
	Box nodeBox, cb;
	if (!wide) {
		nodeBox.reset(); cb.reset();
		for (uint32_t i = b; i < e; ++i) { nodeBox.grow(S.triBox[S.order[i]]); cb.grow(S.centroid[S.order[i]]); }
	} else {
		std::vector<Box> nb(threads), cbs(threads);
		for (unsigned t = 0; t < threads; ++t) { nb[t].reset(); cbs[t].reset(); }
		ParallelChunks(threads, b, e, [&](uint32_t lo, uint32_t hi, unsigned t) {
			Box x, y; x.reset(); y.reset();
			for (uint32_t i = lo; i < hi; ++i) { x.grow(S.triBox[S.order[i]]); y.grow(S.centroid[S.order[i]]); }
			nb[t] = x; cbs[t] = y;
		});
		nodeBox = nb[0]; cb = cbs[0];
		for (unsigned t = 1; t < threads; ++t) { nodeBox.grow(nb[t]); cb.grow(cbs[t]); }
	}
	C.tmp[self].box = nodeBox;

	auto makeLeaf = [&]() {
		C.tmp[self].first = b; C.tmp[self].count = n;
		return self;
	};
	if (n <= 1) return makeLeaf();

	// binned SAH over the three axes, one pass over the range
	float lo[3], scale[3]; bool live[3];
	for (int a = 0; a < 3; ++a) {
		lo[a] = axisOf(cb.mn, a); const float hi = axisOf(cb.mx, a);
		live[a] = hi > lo[a];
		scale[a] = live[a] ? (float)kBins / (hi - lo[a]) : 0.0f;
	}
	BinSet bins; bins.reset();
	auto scan = [&](BinSet& bs, uint32_t cbeg, uint32_t cend) {
		for (uint32_t i = cbeg; i < cend; ++i) {
			const uint32_t p = S.order[i];
			const f3& c = S.centroid[p]; const Box& bx = S.triBox[p];
			for (int a = 0; a < 3; ++a) {
				if (!live[a]) continue;
				int k = (int)((axisOf(c, a) - lo[a]) * scale[a]);
				k = k < 0 ? 0 : (k >= kBins ? kBins - 1 : k);
				bs.box[a][k].grow(bx); bs.count[a][k]++;
			}
		}
	};
	if (!wide) scan(bins, b, e);
	else {
		std::vector<BinSet> sets(threads);
		for (BinSet& bs : sets) bs.reset();
		ParallelChunks(threads, b, e, [&](uint32_t cbeg, uint32_t cend, unsigned t) { scan(sets[t], cbeg, cend); });
		for (unsigned t = 0; t < threads; ++t) bins.merge(sets[t]);
	}

	float bestCost = FLT_MAX; int bestAxis = -1; int bestBin = -1;
	const float parentArea = std::max(nodeBox.halfArea(), 1e-30f);
	for (int a = 0; a < 3; ++a) {
		if (!live[a]) continue;
		float rightArea[kBins]; uint32_t rightCount[kBins];
		Box acc; acc.reset(); uint32_t cnt = 0;
		for (int k = kBins - 1; k >= 1; --k) { acc.grow(bins.box[a][k]); cnt += bins.count[a][k]; rightArea[k] = acc.halfArea(); rightCount[k] = cnt; }
		acc.reset(); cnt = 0;
		for (int k = 0; k < kBins - 1; ++k) {
			acc.grow(bins.box[a][k]); cnt += bins.count[a][k];
			if (cnt == 0 || rightCount[k + 1] == 0) continue;
			float cost = kCostTraverse + kCostTri * (acc.halfArea() * cnt + rightArea[k + 1] * rightCount[k + 1]) / parentArea;
			if (cost < bestCost) { bestCost = cost; bestAxis = a; bestBin = k; }
		}
	}

	uint32_t mid;
	if (depth >= kMedianSplitDepth) {
		// A SAH tree has no depth bound (a pathological input can peel one primitive per level) and the traversal stacks hold
		// 64 entries: from this depth on the range is halved by count along the longest centroid axis, which ends within
		// log2(n) <= 25 more levels (kMaxPrimitives), i.e. below 64.  Deterministic for any thread count (nth_element on a range
		// whose order is already fixed).
		if (leafAllowed(S, b, e)) return makeLeaf();
		int axis = 0;
		const float ex = cb.mx.x - cb.mn.x, ey = cb.mx.y - cb.mn.y, ez = cb.mx.z - cb.mn.z;
		if (ey > ex && ey >= ez) axis = 1; else if (ez > ex && ez > ey) axis = 2;
		mid = b + n / 2;
		std::nth_element(S.order.begin() + b, S.order.begin() + mid, S.order.begin() + e, [&](uint32_t x, uint32_t y) {
			const float cx = axisOf(S.centroid[x], axis), cy = axisOf(S.centroid[y], axis);
			return cx < cy || (cx == cy && x < y);
		});
	} else if (bestAxis < 0) {
		// all centroids coincide: split by index
		if (leafAllowed(S, b, e)) return makeLeaf();
		mid = b + n / 2;
	} else {
		if (leafAllowed(S, b, e) && bestCost >= kCostTri * n) return makeLeaf();
		const float l0 = lo[bestAxis], sc = scale[bestAxis];
		auto it = std::partition(S.order.begin() + b, S.order.begin() + e, [&](uint32_t t) {
			int k = (int)((axisOf(S.centroid[t], bestAxis) - l0) * sc);
			k = k < 0 ? 0 : (k >= kBins ? kBins - 1 : k);
			return k <= bestBin;
		});
		mid = (uint32_t)(it - S.order.begin());
		if (mid == b || mid == e) mid = b + n / 2;
	}
	const int32_t l = build(S, C, b, mid, depth + 1);
	const int32_t r = build(S, C, mid, e, depth + 1);
	C.tmp[self].left = l; C.tmp[self].right = r;
	return self;
}

// pre-order copy of (top tree + task sub-trees) into one array: the order a single-threaded build pushes nodes in
int32_t Splice(const std::vector<Ctx>& sub, const std::vector<std::pair<uint32_t, int32_t>>& where, const Ctx& src, int32_t idx, std::vector<TmpNode>& dst)
{
	const TmpNode& n = src.tmp[idx];
	if (n.left <= -2) { const auto& w = where[(size_t)(-2 - n.left)]; return Splice(sub, where, sub[w.first], w.second, dst); }
	const int32_t self = (int32_t)dst.size();
	dst.push_back(n);
	if (n.left >= 0) {
		const int32_t l = Splice(sub, where, src, n.left, dst);
		const int32_t r = Splice(sub, where, src, n.right, dst);
		dst[self].left = l; dst[self].right = r;
	}
	return self;
}

inline void storeBox(float* mn, float* mx, const Box& b) {
	mn[0] = b.mn.x; mn[1] = b.mn.y; mn[2] = b.mn.z;
	mx[0] = b.mx.x; mx[1] = b.mx.y; mx[2] = b.mx.z;
}
inline int32_t leafRef(uint32_t first, uint32_t kind, uint32_t count) { return ~(int32_t)((first << LEAF_FIRST_SHIFT) | (kind << LEAF_KIND_SHIFT) | (count - 1)); }

// nodes4 -> nodes4q (DNode4Q, rl_device.h) by rl_grid.h's rule.
static void QuantizeWide(BVH& out)
{
	out.nodes4q.assign(out.nodes4.size(), DNode4Q());
	const size_t count = out.nodes4.size();
	ParallelFor(ThreadsFor(count, kThreadedQuantize), 0, count, [&](size_t i0, size_t i1, unsigned) { for (size_t i = i0; i < i1; ++i) {
		out.nodes4q[i] = QuantizeNode4(out.nodes4[i]);
	} });
}

// ---- the 8-wide tree (DNode8, rl_device.h) ---------------------------------------------------------------------------------------------------------
// Collapse: starting from a node's two children, the inner child with the largest surface area is replaced by its own two children until there are eight (or
// only leaves) -- the BVH4's rule.  Slots: child c goes to the slot whose three bits (bit 0: +x, bit 1: +y, bit 2: +z) point from the node's centre towards
// the child's, assigned greedily by the largest dot product of (child centre - node centre) with the slot's (+-1, +-1, +-1): a ray then visits the slots in the
// order slot XOR (signs of its direction) without sorting anything.  Nodes are numbered breadth first, so the inner children of a node are consecutive; the
// leaf children of a node, taken in slot order, define the order of the triangle slots (BuildBVH assigns them in W.leafOrder's order).
struct Wide8Node { int32_t kid[8]; uint32_t firstChild; };   // TmpNode index per slot (-1: none); node index of the first inner child
struct Wide8 { std::vector<Wide8Node> nodes; std::vector<int32_t> leafOrder; uint32_t depth = 0; double sah = 0.0; };

// Which binary nodes become 8-wide nodes is decided for the whole tree at once (the dynamic programme of Ylitie, Karras, Laine, "Efficient incoherent ray
// traversal on GPUs through compressed wide BVHs", HPG 2017, section 3.1, without its leaf merging: the binary tree's leaves stay what they are), minimising the
// sum of the 8-wide nodes' surface areas -- the node steps a random ray is expected to take.  c[n][i - 1]: the least cost of the sub-tree under n when it may
// occupy i slots of its parent 8-wide node (i = 1: n is itself an 8-wide node, or a leaf).  Opening the largest child first (what the 4-wide tree does; here
// RAYLIB_WIDE_GREEDY=1) leaves 4.1 of the 8 slots used on the 298 k-triangle room -- 63 655 nodes, an expected 39.5 steps; the plan: 45 455 nodes, 5.4 slots used,
// 38.5 steps, and frames 0.3 ... 4.7 % shorter (tools/gpu_w8_plan_ab.py).  For the 4-wide tree the same plan buys 0.7 ... 2 % of expected steps and a deeper
// worst-case stack (colonnade 29 -> 33 entries: the next kernel instance): not used there.
template <int W> struct WidePlan {
	float c[W - 1];
	uint32_t bits;   // k (slots of the left sub-tree) when n's children share j = 2 ... W slots: 3 bits each from bit 0; bit 21 + i: c[i - 1] is c[i - 2] (i = 2 ... W - 1)
	int kAt(int j) const { return (int)((bits >> (3 * (j - 2))) & 7u); }
	bool sameAsFewer(int i) const { return ((bits >> (21 + i)) & 1u) != 0u; }
};
template <int W>
static void PlanWide(const std::vector<TmpNode>& T, int32_t root, std::vector<WidePlan<W>>& plan, float triCost)
{
	plan.assign(T.size(), WidePlan<W>());
	const double rootArea = std::max((double)T[root].box.halfArea(), 1e-30);
	for (size_t t = T.size(); t-- > 0;) {   // children follow their parent in T: a reverse sweep sees them first
		WidePlan<W>& P = plan[t];
		// a leaf child costs its expected triangle tests: (its box's area / the root's) x its triangles x triCost node steps
		const float leafCost = triCost * (float)((double)T[t].box.halfArea() / rootArea) * (float)T[t].count;
		if (T[t].left < 0) { for (int i = 0; i < W - 1; ++i) P.c[i] = leafCost; P.bits = 0; continue; }
		const WidePlan<W>& L = plan[T[t].left]; const WidePlan<W>& R = plan[T[t].right];
		float d[W + 1]; uint32_t bits = 0;   // d[j]: n's two children share j slots
		for (int j = 2; j <= W; ++j) {
			float best = FLT_MAX; int bestK = 1;
			for (int k = 1; k < j; ++k) { if (k > W - 1 || j - k > W - 1) continue; const float v = L.c[k - 1] + R.c[j - k - 1]; if (v < best) { best = v; bestK = k; } }
			d[j] = best; bits |= (uint32_t)bestK << (3 * (j - 2));
		}
		// one slot: an 8-wide node of its own -- or, for a split leaf (soft), the leaf as the binary builder made it
		P.c[0] = T[t].soft ? leafCost : (float)((double)T[t].box.halfArea() / rootArea) + d[W];
		for (int i = 2; i <= W - 1; ++i) {
			if (d[i] < P.c[i - 2]) P.c[i - 1] = d[i];
			else { P.c[i - 1] = P.c[i - 2]; bits |= 1u << (21 + i); }
		}
		P.bits = bits;
	}
}
// the planned children of the W-wide node rooted at t: its two sub-trees share W slots as the plan says; a sub-tree given i slots is either opened (its own two
// children share them) or, with one slot, a child of this node.  Returns their number.
template <int W>
static int PlannedChildren(std::vector<TmpNode>& T, const std::vector<WidePlan<W>>& plan, int32_t t, int32_t* kids)
{
	struct Share { int32_t t; int slots; } todo[2 * W]; int top = 0, nk = 0;
	{ const int k = plan[t].kAt(W); todo[top++] = { T[t].right, W - k }; todo[top++] = { T[t].left, k }; }
	while (top > 0) {
		const Share sh = todo[--top];
		if (T[sh.t].left < 0) { kids[nk++] = sh.t; continue; }
		int i = sh.slots;
		while (i > 1 && plan[sh.t].sameAsFewer(i)) --i;
		if (i == 1) { kids[nk++] = sh.t; continue; }
		const int k = plan[sh.t].kAt(i);
		T[sh.t].soft = 0;   // (a split leaf the plan opens is an inner node from here on: the binary and the 4-wide tree are emitted from the same T)
		todo[top++] = { T[sh.t].right, i - k }; todo[top++] = { T[sh.t].left, k };
	}
	return nk;
}

// The greedy collapse: starting from t's two children, the inner child with the largest surface area is replaced by its own two children until there are `width`
// (or only leaves).  Returns their number.
static int OpenLargestFirst(const std::vector<TmpNode>& T, int32_t t, int32_t* kids, int width)
{
	int nk = 0;
	kids[nk++] = T[t].left; kids[nk++] = T[t].right;
	while (nk < width) {
		int best = -1; float bestArea = -1.0f;
		for (int k = 0; k < nk; ++k) if (T[kids[k]].left >= 0) { const float a = T[kids[k]].box.halfArea(); if (a > bestArea) { bestArea = a; best = k; } }
		if (best < 0) break;
		const int32_t open = kids[best];
		kids[best] = T[open].left; kids[nk++] = T[open].right;
	}
	return nk;
}

// Leaves of the binary tree hold up to kMaxLeaf triangles: below that the surface-area heuristic finds a node not worth its step.  In an 8-wide node a step tests
// eight boxes whether or not eight children exist (5.4 did on the 298 k-triangle room), so a spare slot is a free box: every triangle leaf gets a binary split
// of its triangles (sorted along the longest axis of their centroids; each range cut where the two halves' area x count is least) down to single triangles,
// flagged `soft`; the plan (PlanWide) opens such a node where its parent has slots left and the smaller boxes save expected triangle tests, and leaves it the
// leaf it was elsewhere (CollapseWide8 closes what the plan did not open).  No node is added to the 8-wide tree by this.
static void SplitLeaves(std::vector<TmpNode>& T, Shared& B)
{
	const size_t n0 = T.size();
	for (size_t t = 0; t < n0; ++t) {
		if (T[t].left >= 0 || T[t].count < 2 || B.kind[B.order[T[t].first]] != PRIM_TRIANGLE) continue;
		const uint32_t b = T[t].first, e = b + T[t].count;
		Box cb; cb.reset();
		for (uint32_t i = b; i < e; ++i) cb.grow(B.centroid[B.order[i]]);
		int axis = 0;
		const float ex = cb.mx.x - cb.mn.x, ey = cb.mx.y - cb.mn.y, ez = cb.mx.z - cb.mn.z;
		if (ey > ex && ey >= ez) axis = 1; else if (ez > ex && ez > ey) axis = 2;
		std::sort(B.order.begin() + b, B.order.begin() + e, [&](uint32_t x, uint32_t y) {
			const float cx = axisOf(B.centroid[x], axis), cy = axisOf(B.centroid[y], axis);
			return cx < cy || (cx == cy && x < y);
		});
		// ranges to split, depth first; a range's node exists before its children are appended (children follow their parent in T)
		struct Range { int32_t node; uint32_t b, e; } todo[2 * kMaxLeaf]; int top = 0;
		todo[top++] = { (int32_t)t, b, e };
		while (top > 0) {
			const Range r = todo[--top];
			if (r.e - r.b < 2) continue;
			uint32_t bestCut = r.b + 1; float bestCost = FLT_MAX;
			for (uint32_t cut = r.b + 1; cut < r.e; ++cut) {
				Box l, rr; l.reset(); rr.reset();
				for (uint32_t i = r.b; i < cut; ++i) l.grow(B.triBox[B.order[i]]);
				for (uint32_t i = cut; i < r.e; ++i) rr.grow(B.triBox[B.order[i]]);
				const float cost = l.halfArea() * (float)(cut - r.b) + rr.halfArea() * (float)(r.e - cut);
				if (cost < bestCost) { bestCost = cost; bestCut = cut; }
			}
			TmpNode kids[2];
			const uint32_t lim[3] = { r.b, bestCut, r.e };
			for (int k = 0; k < 2; ++k) {
				kids[k].box.reset();
				for (uint32_t i = lim[k]; i < lim[k + 1]; ++i) kids[k].box.grow(B.triBox[B.order[i]]);
				kids[k].first = lim[k]; kids[k].count = lim[k + 1] - lim[k];
			}
			const int32_t li = (int32_t)T.size(); T.push_back(kids[0]);
			const int32_t ri = (int32_t)T.size(); T.push_back(kids[1]);
			T[r.node].left = li; T[r.node].right = ri; T[r.node].soft = 1;
			todo[top++] = { ri, bestCut, r.e }; todo[top++] = { li, r.b, bestCut };
		}
	}
}

static void CollapseWide8(std::vector<TmpNode>& T, int32_t root, Wide8& W, bool greedy, float triCost)
{
	std::vector<WidePlan<8>> plan;
	if (!greedy) PlanWide<8>(T, root, plan, triCost);
	struct Item { int32_t tmp; uint32_t level; };
	std::vector<Item> queue;
	queue.push_back({ root, 1u });
	W.nodes.clear(); W.leafOrder.clear(); W.depth = 0; W.sah = 0.0;
	const double rootArea = std::max((double)T[root].box.halfArea(), 1e-30);
	for (size_t at = 0; at < queue.size(); ++at) {
		const Item it = queue[at];
		W.depth = std::max(W.depth, it.level);
		W.sah += (double)T[it.tmp].box.halfArea() / rootArea;
		int32_t kids[8]; int nk = 0;
		if (!plan.empty()) nk = PlannedChildren<8>(T, plan, it.tmp, kids);
		else nk = OpenLargestFirst(T, it.tmp, kids, 8);
		const Box& nb = T[it.tmp].box;
		const double cx = 0.5 * ((double)nb.mn.x + nb.mx.x), cy = 0.5 * ((double)nb.mn.y + nb.mx.y), cz = 0.5 * ((double)nb.mn.z + nb.mx.z);
		double cost[8][8];
		for (int c = 0; c < nk; ++c) {
			const Box& b = T[kids[c]].box;
			const double dx = 0.5 * ((double)b.mn.x + b.mx.x) - cx, dy = 0.5 * ((double)b.mn.y + b.mx.y) - cy, dz = 0.5 * ((double)b.mn.z + b.mx.z) - cz;
			for (int sl = 0; sl < 8; ++sl) cost[c][sl] = ((sl & 1) ? dx : -dx) + ((sl & 2) ? dy : -dy) + ((sl & 4) ? dz : -dz);
		}
		Wide8Node nd; for (int sl = 0; sl < 8; ++sl) nd.kid[sl] = -1;
		bool childDone[8] = { false, false, false, false, false, false, false, false };
		for (int round = 0; round < nk; ++round) {
			int bc = -1, bs = -1; double bv = -1e300;
			for (int c = 0; c < nk; ++c) { if (childDone[c]) continue; for (int sl = 0; sl < 8; ++sl) { if (nd.kid[sl] >= 0) continue; if (cost[c][sl] > bv) { bv = cost[c][sl]; bc = c; bs = sl; } } }
			nd.kid[bs] = kids[bc]; childDone[bc] = true;
		}
		nd.firstChild = (uint32_t)queue.size();
		for (int sl = 0; sl < 8; ++sl) {
			const int32_t k = nd.kid[sl];
			if (k < 0) continue;
			if (T[k].left >= 0 && !T[k].soft) queue.push_back({ k, it.level + 1u }); else W.leafOrder.push_back(k);
		}
		W.nodes.push_back(nd);
	}
	// split leaves the plan left closed are leaves again; what hangs below them belongs to no tree
	for (size_t t = 0; t < T.size(); ++t) {
		if (!T[t].soft || T[t].dead) continue;
		int32_t st[4 * kMaxLeaf]; int top = 0;
		st[top++] = T[t].left; st[top++] = T[t].right;
		while (top > 0) { const int32_t k = st[--top]; T[k].dead = 1; if (T[k].left >= 0) { st[top++] = T[k].left; st[top++] = T[k].right; } }
		T[t].left = T[t].right = -1; T[t].soft = 0;
	}
}

// the expected node steps of a random ray through the 4-wide collapse of T (sum of the wide nodes' areas over the root's), without building it: what decides
// whether a scene's rays walk the 8-wide tree by default (rl_device.h RL_BVH8_MIN_STEPS) -- and only then are its leaves split for that tree
static double ExpectedSteps4(const std::vector<TmpNode>& T, int32_t root)
{
	const double rootArea = std::max((double)T[root].box.halfArea(), 1e-30);
	double sum = 0.0;
	std::vector<int32_t> work; work.push_back(root);
	while (!work.empty()) {
		const int32_t t = work.back(); work.pop_back();
		sum += (double)T[t].box.halfArea() / rootArea;
		int32_t kids[4]; const int nk = OpenLargestFirst(T, t, kids, 4);
		for (int k = 0; k < nk; ++k) if (T[kids[k]].left >= 0) work.push_back(kids[k]);
	}
	return sum;
}

// W + the leaf references (first triangle slot, count) -> out.nodes8, and per child the binary tree's box it came from (boxId: EmitBinary's) -> out.boxOf8.
// Grid boxes as in QuantizeWide.
static void EmitWide8(const std::vector<TmpNode>& T, const Wide8& W, const std::vector<int32_t>& leafCode, const std::vector<int32_t>& boxId, BVH& out)
{
	out.nodes8.assign(W.nodes.size(), DNode8());
	out.boxOf8.assign(8 * W.nodes.size(), -1);
	out.depth8 = W.depth; out.sahNodes8 = (float)W.sah;
	const size_t count = W.nodes.size();
	ParallelFor(ThreadsFor(count, kThreadedEmit8), 0, count, [&](size_t i0, size_t i1, unsigned) { for (size_t i = i0; i < i1; ++i) {
		const Wide8Node& w = W.nodes[i];
		DNode8 n; memset(&n, 0, sizeof(n));
		uint32_t imask = 0, leafMask = 0, triBase = 0; bool haveTri = false;
		for (int c = 0; c < 8; ++c) {
			const int32_t k = w.kid[c];
			if (k < 0) continue;
			if (T[k].left >= 0) { imask |= 1u << c; continue; }
			const uint32_t code = (uint32_t)~leafCode[k], first = code >> LEAF_FIRST_SHIFT, count = (code & LEAF_COUNT_MASK) + 1;
			leafMask |= ((1u << count) - 1u) << (4 * c);
			if (!haveTri) { triBase = first; haveTri = true; }
		}
		float lo[3][8], hi[3][8]; uint32_t used = 0;
		for (int c = 0; c < 8; ++c) {
			out.boxOf8[8 * i + (size_t)c] = w.kid[c] < 0 ? -1 : boxId[w.kid[c]];
			if (w.kid[c] < 0) continue;
			used |= 1u << c;
			const Box& b = T[w.kid[c]].box;
			for (int a = 0; a < 3; ++a) { lo[a][c] = axisOf(b.mn, a); hi[a][c] = axisOf(b.mx, a); }
		}
		n.meta = imask << 24;
		QuantizeNode8(lo, hi, used, n);
		n.childBase = w.firstChild; n.triBase = triBase; n.leafMask = leafMask; n.alphaMask = 0;
		out.nodes8[i] = n;
	} });
}

// The binary tree.  Reads the primitives' boxes and kinds; fills B (kinds, boxes, centroids and `order`, the primitives permuted so that every node's are one
// range) and T, the tree's nodes in the pre-order a single-threaded build pushes them in, whatever the thread count; returns the root's index in T.  The top
// levels are built by the caller with all threads scanning the long ranges, the sub-trees below B.taskSize primitives by the workers, one arena each, and
// Splice puts them back in order.  RAYLIB_BUILD_TIMING=1 logs the three phases.
int32_t BuildBinary(const std::vector<PrimRef>& prims, Shared& B, std::vector<TmpNode>& T)
{
	const uint32_t n = (uint32_t)prims.size();
	B.kind.resize(n); B.triBox.resize(n); B.centroid.resize(n); B.order.resize(n);
	for (uint32_t i = 0; i < n; ++i) {
		Box b; b.mn = prims[i].mn; b.mx = prims[i].mx;
		B.kind[i] = prims[i].kind;
		B.triBox[i] = b;
		B.centroid[i] = F3(0.5f * (b.mn.x + b.mx.x), 0.5f * (b.mn.y + b.mx.y), 0.5f * (b.mn.z + b.mx.z));
		B.order[i] = i;
	}
	// threads: RAYLIB_BUILD_THREADS, else the host's (capped at 32); small scenes build on the calling thread
	const unsigned threads = ThreadsFor(n, kThreadedBuild);
	B.threads = threads;
	// sub-trees of at most this many primitives are tasks.  Not far below kParallelRange: between the two sizes a range is
	// binned by ONE thread while the others wait (10 M triangles, 32 threads: 1.3 s of a 2.3 s build went there with n / 16T)
	B.taskSize = threads > 1 ? std::max<uint32_t>(4096u, std::min<uint32_t>(kParallelRange - 1u, n / (threads * 4u))) : 0u;
	// large scenes: everything below the all-thread ranges is a task -- no range is left for one thread to bin while the others wait
	if (threads > 1 && n >= 8u * kParallelRange) B.taskSize = kParallelRange - 1u;

	const auto tb0 = std::chrono::steady_clock::now();
	Ctx top;
	std::vector<Task> tasks;
	if (threads > 1) top.tasks = &tasks;
	top.tmp.reserve(threads > 1 ? 4096 : 2 * (size_t)n);
	const int32_t topRoot = build(B, top, 0, n, 0);
	const auto tb1 = std::chrono::steady_clock::now();
	// every worker appends the sub-trees of the tasks it takes to its own arena (one growing vector per thread: a
	// vector per task meant one mmap/munmap pair per task, and the threads queued on the kernel's mm lock)
	std::vector<Ctx> sub(threads);
	std::vector<std::pair<uint32_t, int32_t>> where(tasks.size());   // task -> (arena, root index in it)
	if (!tasks.empty()) {
		std::atomic<size_t> nextTask{ 0 };
		ParallelFor(threads, 0, threads, [&](size_t, size_t, unsigned me) {   // one chunk per thread: worker `me`
			sub[me].tmp.reserve((size_t)n / threads);
			for (;;) {
				const size_t t = nextTask.fetch_add(1);
				if (t >= tasks.size()) return;
				const int32_t r = build(B, sub[me], tasks[t].b, tasks[t].e, tasks[t].depth);
				where[t] = { me, r };
			}
		});
	}
	const auto tb2 = std::chrono::steady_clock::now();
	int32_t root = topRoot;
	if (!tasks.empty()) {
		T.reserve(2 * (size_t)n);
		root = Splice(sub, where, top, topRoot, T);
	} else {
		T.swap(top.tmp);
	}
	if (getenv("RAYLIB_BUILD_TIMING")) Log("BVH build: %u threads, %zu tasks; top levels %.3f s, tasks %.3f s, merge %.3f s", threads, tasks.size(),
		std::chrono::duration<double>(tb1 - tb0).count(), std::chrono::duration<double>(tb2 - tb1).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - tb2).count());
	return root;
}

// Leaf references.  Triangle leaves index the triangle arrays in leaf order (triOrder lists the original triangle index of every slot); an analytic primitive's leaf carries its index in its own array.
// Reads T's leaves -- those `order` lists, in its order (the 8-wide plan's W.leafOrder), else every leaf in T's order --, B and the primitives' indices; appends
// to triOrder; returns the leaf reference of every node of T it visited (0 elsewhere).
std::vector<int32_t> AssignLeafSlots(const std::vector<TmpNode>& T, const Shared& B, const std::vector<PrimRef>& prims, const std::vector<int32_t>* order, std::vector<uint32_t>& triOrder)
{
	std::vector<int32_t> leafCode(T.size(), 0);
	auto codeLeaf = [&](size_t t) {
		const uint32_t k = B.kind[B.order[T[t].first]];
		if (k == PRIM_TRIANGLE) {
			const uint32_t first = (uint32_t)triOrder.size();
			for (uint32_t i = 0; i < T[t].count; ++i) triOrder.push_back(prims[B.order[T[t].first + i]].index);
			leafCode[t] = leafRef(first, PRIM_TRIANGLE, T[t].count);
		} else {
			leafCode[t] = leafRef(prims[B.order[T[t].first]].index, k, 1);
		}
	};
	if (order) { for (int32_t t : *order) codeLeaf((size_t)t); }
	else for (size_t t = 0; t < T.size(); ++t) if (T[t].left < 0) codeLeaf(t);
	return leafCode;
}

// Emit two-box nodes in depth-first order.  A tree that is a single leaf still gets one inner node (left = the leaf, right = empty).
// Reads T (skipping what CollapseWide8 marked dead) and the leaf references; writes out.nodes, out.depth and out.sahCost (the single-leaf tree: depth 1, no cost).
// Returns, per node of T but the root, the id of the box out.nodes keeps for it (rl_grid.h BoxOfId; -1: none): what the wide formats record per child.
std::vector<int32_t> EmitBinary(const std::vector<TmpNode>& T, int32_t root, const std::vector<int32_t>& leafCode, BVH& out)
{
	std::vector<int32_t> boxId(T.size(), -1);
	if (T[root].left < 0) {
		Box empty; empty.reset();
		DNode nd; memset(&nd, 0, sizeof(nd));
		storeBox(nd.lmin, nd.lmax, T[root].box); storeBox(nd.rmin, nd.rmax, empty);
		nd.left = leafCode[root]; nd.right = DNODE_EMPTY;
		out.nodes.push_back(nd);
		out.depth = 1;
		return boxId;
	}
	std::vector<int32_t> emitIndex(T.size(), -1);
	int32_t next = 0;
	uint32_t maxDepth = 0;
	{
		// (the depth is taken here, from the tree that is emitted: split leaves the 8-wide plan opened are inner nodes of it)
		std::vector<std::pair<int32_t, uint32_t>> st; st.push_back({ root, 0u });
		while (!st.empty()) {
			const int32_t t = st.back().first; const uint32_t d = st.back().second; st.pop_back();
			if (T[t].left < 0) { maxDepth = std::max(maxDepth, d); continue; }
			emitIndex[t] = next++;
			st.push_back({ T[t].right, d + 1u }); st.push_back({ T[t].left, d + 1u });
		}
	}
	out.nodes.resize((size_t)next);
	double sah = 0.0; const float rootArea = std::max(T[root].box.halfArea(), 1e-30f);
	for (size_t t = 0; t < T.size(); ++t) {
		if (T[t].dead) continue;
		if (T[t].left < 0) { sah += kCostTri * T[t].count * T[t].box.halfArea() / rootArea; continue; }
		sah += kCostTraverse * T[t].box.halfArea() / rootArea;
		DNode nd; memset(&nd, 0, sizeof(nd));
		const TmpNode& L = T[T[t].left]; const TmpNode& R = T[T[t].right];
		storeBox(nd.lmin, nd.lmax, L.box); storeBox(nd.rmin, nd.rmax, R.box);
		nd.left = (L.left < 0) ? leafCode[T[t].left] : emitIndex[T[t].left];
		nd.right = (R.left < 0) ? leafCode[T[t].right] : emitIndex[T[t].right];
		out.nodes[emitIndex[t]] = nd;
		boxId[T[t].left] = 2 * emitIndex[t]; boxId[T[t].right] = 2 * emitIndex[t] + 1;
	}
	out.depth = maxDepth;     // leaves at depth d => at most d inner nodes above them
	out.sahCost = (float)sah;
	return boxId;
}

// ---- the wide tree: collapse to <= 4 children per node ----
// Starting from a node's two children, the inner child with the largest surface area is replaced by its own two children until there are four (or only leaves).  Only for scenes the pool schedule can run (triangles only, not tiny).
// Reads T, the leaf references and the boxes' ids; writes out.nodes4, out.boxOf4, out.stackNeed4 (the entries a walk can leave on its stack along the worst path) and out.sahNodes4.
void EmitWide4(const std::vector<TmpNode>& T, int32_t root, const std::vector<int32_t>& leafCode, const std::vector<int32_t>& boxId, BVH& out)
{
	struct Item { int32_t tmp; int32_t slot; uint32_t need; };   // a BVH2 inner node that becomes wide node `slot`
	std::vector<Item> work;
	out.nodes4.reserve(T.size() / 3 + 1);
	out.nodes4.emplace_back();
	work.push_back({ root, 0, 0u });
	uint32_t needMax = 0;
	double sah4 = 0.0; const double rootArea4 = std::max((double)T[root].box.halfArea(), 1e-30);
	while (!work.empty()) {
		const Item it = work.back(); work.pop_back();
		sah4 += (double)T[it.tmp].box.halfArea() / rootArea4;
		int32_t kids[4]; const int nk = OpenLargestFirst(T, it.tmp, kids, 4);
		DNode4 nd; memset(&nd, 0, sizeof(nd));
		const uint32_t need = it.need + (uint32_t)(nk - 1);   // entries this node can leave on the stack while one child is followed
		if (need > needMax) needMax = need;
		for (int k = 0; k < 4; ++k) {
			if (k >= nk) {
				nd.lo[0][k] = nd.lo[1][k] = nd.lo[2][k] = FLT_MAX; nd.hi[0][k] = nd.hi[1][k] = nd.hi[2][k] = -FLT_MAX;
				nd.child[k] = DNODE_EMPTY;
				continue;
			}
			const TmpNode& c = T[kids[k]];
			nd.lo[0][k] = c.box.mn.x; nd.lo[1][k] = c.box.mn.y; nd.lo[2][k] = c.box.mn.z;
			nd.hi[0][k] = c.box.mx.x; nd.hi[1][k] = c.box.mx.y; nd.hi[2][k] = c.box.mx.z;
			if (c.left < 0) nd.child[k] = leafCode[kids[k]];
			else {
				const int32_t slot = (int32_t)out.nodes4.size();
				out.nodes4.emplace_back();
				nd.child[k] = slot;
				work.push_back({ kids[k], slot, need });
			}
		}
		out.nodes4[it.slot] = nd;
		out.boxOf4.resize(4 * out.nodes4.size(), -1);
		for (int k = 0; k < nk; ++k) out.boxOf4[4 * (size_t)it.slot + (size_t)k] = boxId[kids[k]];
	}
	out.stackNeed4 = needMax; out.sahNodes4 = (float)sah4;
}

// ---- the leaf list: a scene that 4 * RL_LEAFLIST_RECORDS leaves of <= 8 triangles can hold is walked without a tree ----
// Every ray tests every leaf's box once (4 records of 4 boxes, in lockstep across a wave: no stack, no divergence), then visits the
// leaves it touched nearest first.  In a tree this small a wave's rays take different turns at every node, and the wave pays for
// the union of their walks (Cornell frame: 10 node steps per wave and bounce for 3.5 per ray).  The leaves are a cut through the
// SAH tree: starting from the root, the sub-tree with the largest area x triangle count is opened until the list is full or only the tree's own leaves are left.
// Up to 4.5 triangles per leaf on average: beyond, the leaves of the cut grow towards 8 triangles and the tree wins again (tools/gpu_leaflist.py,
// leaf list / BVH4 walk, first version: 36 triangles 0.86, 72: 0.92, 84: 0.88, 96: 0.89, 108: 0.90, 120 (8-triangle leaves): 1.05; final version: 0.79, 0.80, 0.79,
// 0.77, 0.78 -- the limit is also what the kernel's LDS layout holds, rl_device.h RL_LEAFLIST_MAXTRIS).
// Reads T and the leaf references of a scene of at most RL_LEAFLIST_MAXTRIS triangles, whose slots are in depth-first order (every sub-tree's triangles are
// one range of slots); writes out.leafList and out.boxOfLeafList, or leaves them empty where no cut fits.
void EmitLeafList(const std::vector<TmpNode>& T, int32_t root, const std::vector<int32_t>& leafCode, const std::vector<int32_t>& boxId, BVH& out)
{
	std::vector<uint32_t> triFirst(T.size(), 0), triCount(T.size(), 0);
	for (size_t t = T.size(); t-- > 0;) {   // children follow their parent in T (pre-order): a reverse sweep sees them first
		if (T[t].left < 0) { triFirst[t] = ((uint32_t)~leafCode[t]) >> LEAF_FIRST_SHIFT; triCount[t] = T[t].count; }
		else { triFirst[t] = triFirst[T[t].left]; triCount[t] = triCount[T[t].left] + triCount[T[t].right]; }
	}
	std::vector<int32_t> cut; cut.push_back(root);
	for (;;) {
		int best = -1; double bestCost = -1.0; bool bestOver = false;
		for (size_t k = 0; k < cut.size(); ++k) {
			const int32_t t = cut[k];
			if (T[t].left < 0) continue;
			const bool over = triCount[t] > 8;   // too large for one leaf: goes first
			const double cost = ((double)T[t].box.halfArea() + 1e-30) * triCount[t];
			if (best < 0 || (over && !bestOver) || (over == bestOver && cost > bestCost)) { bestCost = cost; best = (int)k; bestOver = over; }
		}
		if (best < 0 || (cut.size() >= kLeafListMax && !bestOver)) break;
		if (cut.size() >= kLeafListMax) { cut.clear(); break; }   // does not fit
		const int32_t open = cut[(size_t)best];
		cut[(size_t)best] = T[open].left; cut.push_back(T[open].right);
	}
	bool fits = !cut.empty();
	for (int32_t t : cut) if (triCount[t] > 8) fits = false;
	if (!fits) return;
	out.leafList.assign((cut.size() + 3) / 4, DNode4());
	out.boxOfLeafList.assign(4 * out.leafList.size(), -1);
	for (DNode4& nd : out.leafList) {
		memset(&nd, 0, sizeof(nd));
		// an unused slot is the box [+inf, -inf]: whatever the ray, one of its axes enters it at +inf (rl_dev_walk.h TraverseLeafList has no other test for it)
		for (int k = 0; k < 4; ++k) { nd.lo[0][k] = nd.lo[1][k] = nd.lo[2][k] = INFINITY; nd.hi[0][k] = nd.hi[1][k] = nd.hi[2][k] = -INFINITY; nd.child[k] = DNODE_EMPTY; }
	}
	for (size_t at = 0; at < cut.size(); ++at) {
		const int32_t t = cut[at];
		DNode4& nd = out.leafList[at / 4]; const int k = (int)(at % 4);
		nd.lo[0][k] = T[t].box.mn.x; nd.lo[1][k] = T[t].box.mn.y; nd.lo[2][k] = T[t].box.mn.z;
		nd.hi[0][k] = T[t].box.mx.x; nd.hi[1][k] = T[t].box.mx.y; nd.hi[2][k] = T[t].box.mx.z;
		nd.child[k] = leafRef(triFirst[t], PRIM_TRIANGLE, triCount[t]);
		out.boxOfLeafList[at] = boxId[t];
	}
}

} // namespace

// Leaf references keep the first primitive slot in 25 bits (DNode, rl_device.h): more primitives than that cannot be addressed.
bool BVHCapacityOk(size_t numPrimitives) { return numPrimitives < ((size_t)1 << 25); }

void BuildBVH(const std::vector<PrimRef>& prims, BVH& out, const BVHBuildOptions& opt)
{
	// (sahNodes4 and sahNodes8 are written only with their trees: a scene rebuilt without them keeps the figures of its last build with them)
	out.nodes.clear(); out.nodes4.clear(); out.nodes4q.clear(); out.nodes8.clear(); out.depth8 = 0; out.leafList.clear(); out.boxOf4.clear(); out.boxOf8.clear(); out.boxOfLeafList.clear(); out.stackNeed4 = 0; out.triOrder.clear(); out.depth = 0; out.sahCost = 0.0f;
	const uint32_t n = (uint32_t)prims.size();
	if (n == 0) {
		Box empty; empty.reset();
		DNode root; memset(&root, 0, sizeof(root));
		storeBox(root.lmin, root.lmax, empty); storeBox(root.rmin, root.rmax, empty);
		root.left = root.right = DNODE_EMPTY;
		out.nodes.push_back(root);
		return;
	}
	Shared B;
	std::vector<TmpNode> T;
	const int32_t root = BuildBinary(prims, B, T);

	// Triangle-only scenes of at least 8 triangles get the wide trees; the 8-wide one decides the order of the triangle slots (the leaf children of one of its
	// nodes hold consecutive slots), every other format refers to the same slots through its leaf references.
	bool trianglesOnly = true;
	for (uint32_t i = 0; i < n && trianglesOnly; ++i) if (prims[i].kind != PRIM_TRIANGLE) trianglesOnly = false;
	const bool wideTrees = n >= 8 && trianglesOnly && T[root].left >= 0;
	// (not for the scenes small enough for the leaf list: its leaves are sub-trees of this tree, whose triangles must stay one range of slots -- the depth-first order)
	const bool wide8 = wideTrees && n > RL_LEAFLIST_MAXTRIS;
	Wide8 W8;
	if (wide8) {
		// leaves split for the 8-wide plan (SplitLeaves) where that tree is the one the scene's rays will walk
		if (!opt.wideGreedy && opt.splitLeaves8 && ExpectedSteps4(T, root) >= opt.minSteps8) SplitLeaves(T, B);
		CollapseWide8(T, root, W8, opt.wideGreedy, opt.triCost8);
	}
	const std::vector<int32_t> leafCode = AssignLeafSlots(T, B, prims, wide8 ? &W8.leafOrder : nullptr, out.triOrder);
	const std::vector<int32_t> boxId = EmitBinary(T, root, leafCode, out);
	if (!wideTrees) return;
	if (wide8) EmitWide8(T, W8, leafCode, boxId, out);
	EmitWide4(T, root, leafCode, boxId, out);
	QuantizeWide(out);
	if (n <= RL_LEAFLIST_MAXTRIS) EmitLeafList(T, root, leafCode, boxId, out);
}

// The boxes of bvh.nodes have been refitted (RaylibAMD_SceneMoveTriangles: read back from the device): the wide formats from them by the rule the device
// applied (rl_grid.h), and the binary tree's SAH cost, its terms summed in the order EmitBinary sums them -- node, left sub-tree, right sub-tree.
void RefitWideFromBinary(BVH& bvh)
{
	const DNode* nodes = bvh.nodes.data();
	for (size_t i = 0; i < bvh.nodes4.size(); ++i) { RefitNode4(nodes, &bvh.boxOf4[4 * i], bvh.nodes4[i]); bvh.nodes4q[i] = QuantizeNode4(bvh.nodes4[i]); }
	for (size_t i = 0; i < bvh.nodes8.size(); ++i) RefitNode8(nodes, &bvh.boxOf8[8 * i], bvh.nodes8[i]);
	for (size_t i = 0; i < bvh.leafList.size(); ++i) RefitNode4(nodes, &bvh.boxOfLeafList[4 * i], bvh.leafList[i]);
	if (bvh.nodes.empty() || bvh.nodes[0].right == DNODE_EMPTY) return;   // no primitive, or the single-leaf tree: no cost
	auto boxOf = [&](int32_t id) { Box b; float mn[3], mx[3]; BoxOfId(nodes, id, mn, mx); b.mn = F3(mn[0], mn[1], mn[2]); b.mx = F3(mx[0], mx[1], mx[2]); return b; };
	Box rootBox = boxOf(0); rootBox.grow(boxOf(1));
	const float rootArea = std::max(rootBox.halfArea(), 1e-30f);
	double sah = kCostTraverse * rootBox.halfArea() / rootArea;
	std::vector<int32_t> st; st.push_back(1); st.push_back(0);   // box ids, the left one on top
	while (!st.empty()) {
		const int32_t id = st.back(); st.pop_back();
		const int32_t ref = (id & 1) ? nodes[id >> 1].right : nodes[id >> 1].left;
		if (ref == DNODE_EMPTY) continue;
		if (ref < 0) { sah += kCostTri * ((((uint32_t)~ref) & LEAF_COUNT_MASK) + 1u) * boxOf(id).halfArea() / rootArea; continue; }   // (an analytic primitive's leaf: count 1)
		sah += kCostTraverse * boxOf(id).halfArea() / rootArea;
		st.push_back(2 * ref + 1); st.push_back(2 * ref);
	}
	bvh.sahCost = (float)sah;
}

namespace {

inline bool inside(const f3& p, const f3& mn, const f3& mx) { return p.x >= mn.x && p.y >= mn.y && p.z >= mn.z && p.x <= mx.x && p.y <= mx.y && p.z <= mx.z; }
inline uint32_t leafKind(int32_t ref) { return ((uint32_t)~ref >> LEAF_KIND_SHIFT) & LEAF_KIND_MASK; }
// the triangle leaf `ref`: every slot in range, every triangle met for the first time (seen), all three vertices inside the box [mn, mx]
bool LeafTrianglesInside(const BVH& bvh, const std::vector<HostTriangle>& tris, int32_t ref, const f3& mn, const f3& mx, std::vector<uint8_t>& seen)
{
	const uint32_t code = (uint32_t)~ref, first = code >> LEAF_FIRST_SHIFT, count = (code & LEAF_COUNT_MASK) + 1;
	for (uint32_t k = 0; k < count; ++k) {
		if (first + k >= bvh.triOrder.size()) return false;
		const uint32_t ti = bvh.triOrder[first + k];
		if (ti >= tris.size() || seen[ti]) return false;
		seen[ti] = 1;
		const HostTriangle& t = tris[ti];
		if (!inside(t.v0, mn, mx) || !inside(t.v1, mn, mx) || !inside(t.v2, mn, mx)) return false;
	}
	return true;
}

// The grid nodes' box arithmetic as the device does it (rl_dev_pool.h NodeStep4 / NodeStep8), operation by operation in float.  Per axis a ray meets plane q
// of a node's grid at q * A + B, with A = step * inv and B = (origin - o) * inv; E bounds what rounding can have moved that distance by, so entry distances
// are taken E early and exit distances E late.  Bn = B - E is what the 4-wide grid walk adds to q * A for the entry distance; the 8-wide step keeps the
// NEGATED entry distance and adds nB = E - B to q * -A -- computed as the device computes it, not as -Bn (a zero's sign reaches the step's sign test).
constexpr float kGridErrA = 1.21593475e-4f;   // 255 * 2^-21: the rounding of q * A, q <= 255
constexpr float kGridErrB = 4.76837158e-7f;   // 2^-21: the rounding of B
struct GridFactors { float A[3], Bn[3], nB[3], Bf[3]; };
inline GridFactors MakeGridFactors(const float step[3], const float origin[3], const float o[3], const float inv[3])
{
	GridFactors F;
	for (int a = 0; a < 3; ++a) {
		F.A[a] = step[a] * inv[a];
		const float B = (origin[a] - o[a]) * inv[a];
		const float E = fabsf(F.A[a] * kGridErrA) + fabsf(B * kGridErrB);
		F.Bn[a] = B - E; F.nB[a] = E - B; F.Bf[a] = B + E;
	}
	return F;
}
inline float clampInv(float x) { return std::isinf(x) ? copysignf(1e30f, x) : x; }   // the grid walks' reciprocal of a direction component that is zero

// One 8-wide node against one ray (NodeStep8): the steps are the powers of two whose exponents the node holds, one fma per 8-bit plane, the negated entry
// distance (least of ntMin and the planes'), the exit distance (least of tmx and the planes'), and a child is hit where fma(exit, widen, -entry) is not
// negative.  neg[a]: the ray runs down axis a (it enters at the upper plane).  Returns the mask of hit children, by slot.
uint32_t Step8Host(const DNode8& nd, const float o[3], const float inv[3], const bool neg[3], float ntMin, float tmx)
{
	float step[3];
	for (int a = 0; a < 3; ++a) { const uint32_t sb = ((nd.meta >> (8 * a)) & 255u) << 23; memcpy(&step[a], &sb, 4); }
	const GridFactors F = MakeGridFactors(step, nd.origin, o, inv);
	auto plane = [](const uint32_t q[2], int c) { return (float)((q[c >> 2] >> (8 * (c & 3))) & 255u); };
	uint32_t hit = 0;
	for (int ch = 0; ch < 8; ++ch) {
		float ntn = ntMin, tf = tmx;
		for (int a = 0; a < 3; ++a) {
			const float qn = plane(neg[a] ? nd.qhi[a] : nd.qlo[a], ch), qf = plane(neg[a] ? nd.qlo[a] : nd.qhi[a], ch);
			ntn = std::min(ntn, fmaf(qn, -F.A[a], F.nB[a])); tf = std::min(tf, fmaf(qf, F.A[a], F.Bf[a]));
		}
		if (!std::signbit(fmaf(tf, RL_BOX_WIDEN, ntn))) hit |= 1u << ch;
	}
	return hit;
}
// the hit inner children of a node as the next group's bits 24 ... 31: in visiting order, slot XOR octant
inline uint32_t InnerInVisitOrder(uint32_t hitInner, uint32_t oct) { uint32_t p = 0; for (uint32_t b = 0; b < 8u; ++b) if ((hitInner >> b) & 1u) p |= 1u << (b ^ oct); return p; }
// leaf child ch of an 8-wide node: the number of its triangles, and in `first` their first slot
inline uint32_t Leaf8(const DNode8& nd, uint32_t ch, uint32_t& first)
{
	first = nd.triBase + (uint32_t)__builtin_popcount(nd.leafMask & ((1u << (4 * ch)) - 1u));
	return (uint32_t)__builtin_popcount((nd.leafMask >> (4 * ch)) & 15u);
}

} // namespace

bool ValidateBVH(const BVH& bvh, const std::vector<HostTriangle>& tris)
{
	if (bvh.nodes.empty()) return false;
	std::vector<uint8_t> seen(tris.size(), 0);
	struct Item { int32_t ref; f3 mn, mx; };
	std::vector<Item> st;
	const DNode& r = bvh.nodes[0];
	st.push_back({ r.left, F3(r.lmin[0], r.lmin[1], r.lmin[2]), F3(r.lmax[0], r.lmax[1], r.lmax[2]) });
	st.push_back({ r.right, F3(r.rmin[0], r.rmin[1], r.rmin[2]), F3(r.rmax[0], r.rmax[1], r.rmax[2]) });
	while (!st.empty()) {
		Item it = st.back(); st.pop_back();
		if (it.ref == DNODE_EMPTY) continue;
		if (it.ref < 0) {
			if (leafKind(it.ref) != PRIM_TRIANGLE) continue;   // analytic primitive: nothing to check against triangles
			if (!LeafTrianglesInside(bvh, tris, it.ref, it.mn, it.mx, seen)) return false;
			continue;
		}
		if ((size_t)it.ref >= bvh.nodes.size()) return false;
		const DNode& n = bvh.nodes[it.ref];
		f3 lmn = F3(n.lmin[0], n.lmin[1], n.lmin[2]), lmx = F3(n.lmax[0], n.lmax[1], n.lmax[2]);
		f3 rmn = F3(n.rmin[0], n.rmin[1], n.rmin[2]), rmx = F3(n.rmax[0], n.rmax[1], n.rmax[2]);
		if (n.left != DNODE_EMPTY && (!inside(lmn, it.mn, it.mx) || !inside(lmx, it.mn, it.mx))) return false;
		if (n.right != DNODE_EMPTY && (!inside(rmn, it.mn, it.mx) || !inside(rmx, it.mn, it.mx))) return false;
		st.push_back({ n.left, lmn, lmx });
		st.push_back({ n.right, rmn, rmx });
	}
	for (uint8_t s : seen) if (!s) return false;
	return true;
}

// The wide tree must hold every triangle exactly once, inside the box its parent records for it, every child box inside
// its parent's, and never need more stack than stackNeed4 says.
bool ValidateBVH4(const BVH& bvh, const std::vector<HostTriangle>& tris)
{
	if (bvh.nodes4.empty()) return false;
	std::vector<uint8_t> seen(tris.size(), 0);
	struct Item { int32_t ref; f3 mn, mx; uint32_t need; bool haveBox; };
	std::vector<Item> st;
	st.push_back({ 0, F3(0, 0, 0), F3(0, 0, 0), 0u, false });
	while (!st.empty()) {
		const Item it = st.back(); st.pop_back();
		if (it.ref < 0) {
			if (leafKind(it.ref) != PRIM_TRIANGLE || !LeafTrianglesInside(bvh, tris, it.ref, it.mn, it.mx, seen)) return false;   // (no analytic primitive in a wide tree)
			continue;
		}
		if ((size_t)it.ref >= bvh.nodes4.size()) return false;
		const DNode4& n = bvh.nodes4[it.ref];
		{   // the grid node: same children, every grid box around its float box, 255 steps at most
			if (bvh.nodes4q.size() != bvh.nodes4.size()) return false;
			const DNode4Q& q = bvh.nodes4q[it.ref];
			for (int k = 0; k < 4; ++k) {
				if (q.child[k] != n.child[k]) return false;
				if (n.child[k] == DNODE_EMPTY) continue;
				for (int a = 0; a < 3; ++a) {
					const double step = (double)(a == 0 ? q.stepX : (a == 1 ? q.stepY : q.stepZ));
					{ int e2 = 0; if (!(step > 0.0) || frexp(step, &e2) != 0.5) return false; }   // a power of two
					const double lo = (double)q.origin[a] + (double)((q.qlo[a] >> (8 * k)) & 255u) * step, hi = (double)q.origin[a] + (double)((q.qhi[a] >> (8 * k)) & 255u) * step;
					if (!(lo <= (double)n.lo[a][k] && hi >= (double)n.hi[a][k])) return false;
				}
			}
		}
		int nk = 0;
		for (int k = 0; k < 4; ++k) if (n.child[k] != DNODE_EMPTY) ++nk;
		if (nk < 2 && !(it.ref == 0 && nk >= 1)) return false;
		const uint32_t need = it.need + (uint32_t)(nk - 1);
		if (need > bvh.stackNeed4) return false;
		for (int k = 0; k < 4; ++k) {
			if (n.child[k] == DNODE_EMPTY) continue;
			const f3 mn = F3(n.lo[0][k], n.lo[1][k], n.lo[2][k]), mx = F3(n.hi[0][k], n.hi[1][k], n.hi[2][k]);
			if (it.haveBox && (!inside(mn, it.mn, it.mx) || !inside(mx, it.mn, it.mx))) return false;
			st.push_back({ n.child[k], mn, mx, need, true });
		}
	}
	for (uint8_t v : seen) if (!v) return false;
	// the leaf list, if the scene has one: every triangle exactly once, inside its leaf's box; unused slots are the box [+inf, -inf]
	if (!bvh.leafList.empty()) {
		if (bvh.leafList.size() > RL_LEAFLIST_RECORDS) return false;
		std::fill(seen.begin(), seen.end(), 0);
		for (const DNode4& n : bvh.leafList) for (int k = 0; k < 4; ++k) {
			if (n.child[k] == DNODE_EMPTY) {
				for (int a = 0; a < 3; ++a) if (!(n.lo[a][k] == INFINITY && n.hi[a][k] == -INFINITY)) return false;
				continue;
			}
			if (n.child[k] >= 0) return false;
			const f3 mn = F3(n.lo[0][k], n.lo[1][k], n.lo[2][k]), mx = F3(n.hi[0][k], n.hi[1][k], n.hi[2][k]);
			if (leafKind(n.child[k]) != PRIM_TRIANGLE || !LeafTrianglesInside(bvh, tris, n.child[k], mn, mx, seen)) return false;
		}
		for (uint8_t v : seen) if (!v) return false;
	}
	return true;
}

// The 8-wide tree must hold every triangle slot exactly once, and every child's grid box must contain every triangle below it.
bool ValidateBVH8(const BVH& bvh, const std::vector<HostTriangle>& tris)
{
	if (bvh.nodes8.empty()) return true;
	std::vector<uint8_t> seen(bvh.triOrder.size(), 0);
	struct Frame { uint32_t node; int child; double lo[3], hi[3]; double clo[3], chi[3]; };   // lo / hi: bounds of what has been seen below this node so far; clo / chi: ... below the child being walked
	// iterative post-order: for every node, the bounds of the triangles below each child are checked against that child's grid box
	std::vector<Frame> st;
	auto gridBox = [&](const DNode8& n, int c, double* lo, double* hi) {
		for (int a = 0; a < 3; ++a) {
			const double step = ldexp(1.0, (int)((n.meta >> (8 * a)) & 255u) - 127);
			lo[a] = (double)n.origin[a] + (double)((n.qlo[a][c >> 2] >> (8 * (c & 3))) & 255u) * step;
			hi[a] = (double)n.origin[a] + (double)((n.qhi[a][c >> 2] >> (8 * (c & 3))) & 255u) * step;
		}
	};
	Frame f0; f0.node = 0; f0.child = -1; for (int a = 0; a < 3; ++a) { f0.lo[a] = 1e300; f0.hi[a] = -1e300; }
	st.push_back(f0);
	uint32_t depth = 0;
	while (!st.empty()) {
		Frame& F = st.back();
		depth = std::max<uint32_t>(depth, (uint32_t)st.size());
		if (F.node >= bvh.nodes8.size()) return false;
		const DNode8& n = bvh.nodes8[F.node];
		const uint32_t imask = n.meta >> 24;
		if (++F.child >= 8) {
			// done: hand this node's bounds to the parent's current child
			const Frame done = F; st.pop_back();
			if (!st.empty()) {
				Frame& P = st.back();
				const DNode8& pn = bvh.nodes8[P.node];
				double glo[3], ghi[3]; gridBox(pn, P.child, glo, ghi);
				for (int a = 0; a < 3; ++a) {
					if (!(glo[a] <= done.lo[a] && ghi[a] >= done.hi[a])) return false;
					P.lo[a] = std::min(P.lo[a], done.lo[a]); P.hi[a] = std::max(P.hi[a], done.hi[a]);
				}
			}
			continue;
		}
		const int c = F.child;
		const uint32_t nib = (n.leafMask >> (4 * c)) & 15u;
		if (imask & (1u << c)) {
			if (nib) return false;
			Frame ch; ch.node = n.childBase + (uint32_t)__builtin_popcount(imask & ((1u << c) - 1u)); ch.child = -1;
			for (int a = 0; a < 3; ++a) { ch.lo[a] = 1e300; ch.hi[a] = -1e300; }
			st.push_back(ch);
			continue;
		}
		if (!nib) {   // unused: the inverted box
			for (int a = 0; a < 3; ++a) if (((n.qlo[a][c >> 2] >> (8 * (c & 3))) & 255u) != 255u || ((n.qhi[a][c >> 2] >> (8 * (c & 3))) & 255u) != 0u) return false;
			continue;
		}
		if (nib != 1u && nib != 3u && nib != 7u && nib != 15u) return false;
		uint32_t first; const uint32_t count = Leaf8(n, (uint32_t)c, first);
		double glo[3], ghi[3]; gridBox(n, c, glo, ghi);
		for (uint32_t k = 0; k < count; ++k) {
			if (first + k >= bvh.triOrder.size() || seen[first + k]) return false;
			seen[first + k] = 1;
			const uint32_t ti = bvh.triOrder[first + k];
			if (ti >= tris.size()) return false;
			const HostTriangle& t = tris[ti];
			const f3 vs[3] = { t.v0, t.v1, t.v2 };
			for (const f3& v : vs) {
				const double p[3] = { v.x, v.y, v.z };
				for (int a = 0; a < 3; ++a) {
					if (!(glo[a] <= p[a] && ghi[a] >= p[a])) return false;
					F.lo[a] = std::min(F.lo[a], p[a]); F.hi[a] = std::max(F.hi[a], p[a]);
				}
			}
		}
	}
	for (uint8_t v : seen) if (!v) return false;
	return depth <= bvh.depth8;
}

// The 8-wide walk of rl_dev_pool.h (NodeStep8 / LeafStep8) on the host, operation by operation in float -- A = step * inv and B = (corner - o) * inv per axis, the
// rounding bound E = (|B| + 255 |A|) 2^-21, one fma per 8-bit plane, the NEGATED entry distance, the sign of fma(exit, widen, -entry), groups of hit children in
// visiting order, the stack of groups -- with the exit distance fixed at tMax[i] and every triangle of every leaf child reached tested by a tolerant
// double-precision test: outT[i] = the least distance among them (FLT_MAX: none).  What the box arithmetic must never do is skip the leaf that holds the closest
// hit; tests compare outT with the oracle's closest hit on the same rays without a GPU (tests/test_host_logic.py).  outSteps (optional): node steps taken.
bool Walk8Host(const BVH& bvh, const std::vector<HostTriangle>& tris, const float* rays, int n, float tMin, const float* tMax, float* outT, uint32_t* outSteps)
{
	if (bvh.nodes8.empty()) return false;
	for (int r = 0; r < n; ++r) {
		const float* ray = rays + 6 * (size_t)r;
		const float o[3] = { ray[0], ray[1], ray[2] }, d[3] = { ray[3], ray[4], ray[5] };
		float inv[3]; bool neg[3]; uint32_t oct = 0;
		for (int a = 0; a < 3; ++a) { inv[a] = clampInv(1.0f / d[a]); neg[a] = inv[a] < 0.0f; if (!neg[a]) oct |= 1u << a; }
		const float ntMin = -tMin, tmx = std::min(tMax[r], FLT_MAX);
		std::vector<std::pair<uint32_t, uint32_t>> stack;
		uint32_t gx = 0, gy = (1u << (24 + oct)) | 1u, steps = 0;
		double best = (double)FLT_MAX;
		for (;;) {
			if ((gy >> 24) == 0u) { if (stack.empty()) break; gx = stack.back().first; gy = stack.back().second; stack.pop_back(); continue; }
			const uint32_t pos = 31u - (uint32_t)__builtin_clz(gy);
			gy &= ~(1u << pos);
			const uint32_t slot = (pos - 24u) ^ oct;
			const uint32_t node = gx + (uint32_t)__builtin_popcount(gy & 0xffu & ((1u << slot) - 1u));
			if ((gy >> 24) != 0u) stack.push_back({ gx, gy });   // (every group is kept -- a walk past 64 of them is refused --, where WalkStackHost drops the pushes its capacity cannot hold)
			if (node >= bvh.nodes8.size() || stack.size() > 64) return false;
			const DNode8& nd = bvh.nodes8[node];
			++steps;
			const uint32_t imask = nd.meta >> 24, hit = Step8Host(nd, o, inv, neg, ntMin, tmx);   // (the exit distance stays tMax[r]: no hit shortens this walk)
			for (uint32_t ch = 0; ch < 8u; ++ch) {
				if (!((hit & ~imask) >> ch & 1u)) continue;
				uint32_t first; const uint32_t count = Leaf8(nd, ch, first);
				for (uint32_t k = 0; k < count; ++k) {
					if (first + k >= bvh.triOrder.size()) return false;
					const HostTriangle& t = tris[bvh.triOrder[first + k]];
					// tolerant double-precision test (edges and vertices count as inside by 1e-6): a superset of what the reference's float test accepts
					const double e1[3] = { (double)t.v1.x - t.v0.x, (double)t.v1.y - t.v0.y, (double)t.v1.z - t.v0.z }, e2[3] = { (double)t.v2.x - t.v0.x, (double)t.v2.y - t.v0.y, (double)t.v2.z - t.v0.z };
					const double dd[3] = { d[0], d[1], d[2] };
					const double pv[3] = { dd[1] * e2[2] - dd[2] * e2[1], dd[2] * e2[0] - dd[0] * e2[2], dd[0] * e2[1] - dd[1] * e2[0] };
					const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
					if (det == 0.0) continue;
					const double tv[3] = { (double)o[0] - t.v0.x, (double)o[1] - t.v0.y, (double)o[2] - t.v0.z };
					const double u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) / det;
					const double qv[3] = { tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0] };
					const double v = (dd[0] * qv[0] + dd[1] * qv[1] + dd[2] * qv[2]) / det;
					const double tt = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) / det;
					if (u >= -1e-6 && v >= -1e-6 && u + v <= 1.0 + 1e-6 && tt >= (double)tMin * 0.999 && tt < best) best = tt;
				}
			}
			gx = nd.childBase; gy = (InnerInVisitOrder(hit & imask, oct) << 24) | imask;
		}
		outT[r] = best >= (double)FLT_MAX ? FLT_MAX : (float)best;
		if (outSteps) outSteps[r] = steps;
	}
	return true;
}

// The stack discipline of the device walks on the host, with the stack's capacity as an argument: Traverse (tree 2: rl_dev_walk.h, NodeStep of rl_dev_pool.h is the
// same step), Traverse4 on the float boxes (tree 3: RL_WIDE_STEP_F) and on the grid nodes (tree 4: RL_WIDE_STEP_Q; NodeStep4 is the same step) with the 5-comparator sort and far-to-near pushes, and the walk of groups on
// the 8-wide tree (tree 8: NodeStep8 / Push8; capacity in groups) -- the box arithmetic in float, operation by operation, the exit distance shrinking with the
// best hit as on the device, and the device's guard: a push at sp == capacity is DROPPED, silently.  The triangle test is the reference's (geom/triangle.cc:18-58,
// the host's f3 arithmetic is the device record's) with the ray queries' candidate rule (OwnBoxPassBox under RL_OWN_BOX_WIDEN_TMIN): TriangleM1Host, rl_oracle.h; spheres and cubes (tree 2) as
// SphereHit / CubeHit at ray time 0; no cut-out test.  outT[i]: the closest accepted hit over [tMin, FLT_MAX] (INFINITY: none); outHighWater[i]: the largest sp
// the ray reached, counting only pushes that were stored.  What a test proves with it: at the instance's capacity every ray gets the brute-force answer and some
// ray fills the stack to the builder's reported need; at one entry less some ray loses its hit (tests/test_stack_edges_host.py).
bool WalkStackHost(const BVH& bvh, const std::vector<HostTriangle>& tris, const std::vector<HostSphere>& spheres, const std::vector<HostCube>& cubes, int tree,
                   const float* rays, int n, float tMin, int capacity, float* outT, uint32_t* outHighWater)
{
	if (capacity < 0 || (tree != 2 && tree != 3 && tree != 4 && tree != 8)) return false;
	if (tree == 2 ? bvh.nodes.empty() : tree == 3 ? bvh.nodes4.empty() : tree == 4 ? bvh.nodes4q.empty() : bvh.nodes8.empty()) return false;
	const float widen = RL_BOX_WIDEN;
	for (int r = 0; r < n; ++r) {
		const float* ray = rays + 6 * (size_t)r;
		const f3 o = F3(ray[0], ray[1], ray[2]), d = F3(ray[3], ray[4], ray[5]);
		const float oa[3] = { o.x, o.y, o.z };
		const float inv[3] = { 1.0f / d.x, 1.0f / d.y, 1.0f / d.z };                         // exact: the binary tree's boxes and the candidate rule
		const float invc[3] = { clampInv(inv[0]), clampInv(inv[1]), clampInv(inv[2]) };      // the grid trees' boxes
		float best = INFINITY;
		// one triangle slot, as the leaf code of every walk tests it
		auto triangle = [&](uint32_t slot) -> bool {
			if (slot >= bvh.triOrder.size() || bvh.triOrder[slot] >= tris.size()) return false;
			float t, pa, pb;
			if (TriangleM1Host(tris[bvh.triOrder[slot]], o, d, tMin, t, pa, pb) && t < best) best = t;
			return true;
		};
		uint32_t high = 0;
		if (tree == 2 || tree == 3 || tree == 4) {
			std::vector<int32_t> stk((size_t)capacity + 1);
			int sp = 0;
			auto push = [&](int32_t v) { if (sp < capacity) { stk[(size_t)sp] = v; ++sp; high = std::max(high, (uint32_t)sp); } };
			int32_t cur = 0;
			const int32_t DONE = 0x7fffffff;
			for (;;) {
				while (cur >= 0 && cur != DONE) {
					const float tmx = fminf(best, FLT_MAX);
					// the float boxes (trees 2 and 3): the exact reciprocals
					auto slab = [&](const float* mn, const float* mx, float& tNear) {
						float tn = tMin, tf = tmx;
						for (int a = 0; a < 3; ++a) {
							const bool neg = inv[a] < 0.0f;
							tn = fmaxf(tn, ((neg ? mx[a] : mn[a]) - oa[a]) * inv[a]); tf = fminf(tf, ((neg ? mn[a] : mx[a]) - oa[a]) * inv[a]);
						}
						tNear = tn;
						return !(tf * widen < tn);
					};
					if (tree == 2) {
						if ((size_t)cur >= bvh.nodes.size()) return false;
						const DNode& nd = bvh.nodes[(size_t)cur];
						float tl, tr;
						const bool hl = slab(nd.lmin, nd.lmax, tl) && nd.left != DNODE_EMPTY, hr = slab(nd.rmin, nd.rmax, tr) && nd.right != DNODE_EMPTY;
						if (hl && hr) { const bool leftFirst = tl <= tr; push(leftFirst ? nd.right : nd.left); cur = leftFirst ? nd.left : nd.right; }
						else if (hl) cur = nd.left;
						else if (hr) cur = nd.right;
						else if (sp == 0) cur = DONE;
						else cur = stk[(size_t)--sp];
					} else {
						float t[4]; int32_t c[4];
						if (tree == 3) {   // RL_WIDE_STEP_F: the float boxes, the exact reciprocals
							if ((size_t)cur >= bvh.nodes4.size()) return false;
							const DNode4& nd = bvh.nodes4[(size_t)cur];
							for (int k = 0; k < 4; ++k) {
								const float mn[3] = { nd.lo[0][k], nd.lo[1][k], nd.lo[2][k] }, mx[3] = { nd.hi[0][k], nd.hi[1][k], nd.hi[2][k] };
								float tn;
								const bool hitBox = slab(mn, mx, tn);
								c[k] = nd.child[k];
								t[k] = (!hitBox || c[k] == DNODE_EMPTY) ? INFINITY : tn;
							}
						} else {
							if ((size_t)cur >= bvh.nodes4q.size()) return false;
							const DNode4Q& nd = bvh.nodes4q[(size_t)cur];
							const float step[3] = { nd.stepX, nd.stepY, nd.stepZ };
							const GridFactors F = MakeGridFactors(step, nd.origin, oa, invc);
							for (int k = 0; k < 4; ++k) {
								float tn = tMin, tf = tmx;
								for (int a = 0; a < 3; ++a) {
									const bool neg = invc[a] < 0.0f;
									const uint32_t qn = ((neg ? nd.qhi[a] : nd.qlo[a]) >> (8 * k)) & 0xffu, qf = ((neg ? nd.qlo[a] : nd.qhi[a]) >> (8 * k)) & 0xffu;
									tn = fmaxf(tn, fmaf((float)qn, F.A[a], F.Bn[a])); tf = fminf(tf, fmaf((float)qf, F.A[a], F.Bf[a]));
								}
								c[k] = nd.child[k];
								t[k] = (tf * widen < tn || c[k] == DNODE_EMPTY) ? INFINITY : tn;
							}
						}
						auto cswap = [&](int i, int j) { if (t[j] < t[i]) { std::swap(t[i], t[j]); std::swap(c[i], c[j]); } };
						cswap(0, 1); cswap(2, 3); cswap(0, 2); cswap(1, 3); cswap(1, 2);
						if (!(t[0] < INFINITY)) { if (sp == 0) cur = DONE; else cur = stk[(size_t)--sp]; continue; }
						if (t[3] < INFINITY) push(c[3]);
						if (t[2] < INFINITY) push(c[2]);
						if (t[1] < INFINITY) push(c[1]);
						cur = c[0];
					}
				}
				if (cur == DONE) break;
				const uint32_t code = (uint32_t)~cur, first = code >> LEAF_FIRST_SHIFT, count = (code & LEAF_COUNT_MASK) + 1u, kind = (code >> LEAF_KIND_SHIFT) & LEAF_KIND_MASK;
				if (kind == PRIM_TRIANGLE) {
					for (uint32_t i = 0; i < count; ++i) if (!triangle(first + i)) return false;
				} else if (kind == PRIM_SPHERE) {
					if (first >= spheres.size()) return false;
					const HostSphere& s = spheres[first];
					const f3 oc = o - s.center;
					const float a = dot(d, d), b = dot(oc, d), c = dot(oc, oc) - s.radius * s.radius;
					if (b * b - a * c > 0.0f) {
						float temp = (-b - sqrtf(b * b - a * c)) / a;
						if (!(tMin < temp && temp < FLT_MAX)) temp = (-b + sqrtf(b * b - a * c)) / a;
						if (tMin < temp && temp < FLT_MAX && temp < best) best = temp;
					}
				} else {
					if (first >= cubes.size()) return false;
					const HostCube& q = cubes[first];
					const float mna[3] = { q.minBounds.x, q.minBounds.y, q.minBounds.z }, mxa[3] = { q.maxBounds.x, q.maxBounds.y, q.maxBounds.z }, da[3] = { d.x, d.y, d.z };
					float t7 = 0.0f, t8 = 0.0f;
					for (int a = 0; a < 3; ++a) {
						const float t1 = (mna[a] - oa[a]) / da[a], t2 = (mxa[a] - oa[a]) / da[a];
						const float lo = t2 < t1 ? t2 : t1, hi = t1 < t2 ? t2 : t1;
						t7 = a == 0 ? lo : (t7 < lo ? lo : t7); t8 = a == 0 ? hi : (hi < t8 ? hi : t8);
					}
					if (!(t8 < 0 || t7 > t8) && tMin <= t7 && t7 <= FLT_MAX && t7 < best) best = t7;
				}
				if (sp == 0) break;
				cur = stk[(size_t)--sp];
			}
		} else {
			bool neg[3]; uint32_t oct = 0;
			for (int a = 0; a < 3; ++a) { neg[a] = invc[a] < 0.0f; if (!neg[a]) oct |= 1u << a; }
			const float ntMin = -tMin;
			std::vector<std::pair<uint32_t, uint32_t>> stack;
			uint32_t gx = 0, gy = (1u << (24 + oct)) | 1u;
			for (;;) {
				if ((gy >> 24) == 0u) { if (stack.empty()) break; gx = stack.back().first; gy = stack.back().second; stack.pop_back(); continue; }
				const uint32_t pos = 31u - (uint32_t)__builtin_clz(gy);
				gy &= ~(1u << pos);
				const uint32_t slot = (pos - 24u) ^ oct;
				const uint32_t node = gx + (uint32_t)__builtin_popcount(gy & 0xffu & ((1u << slot) - 1u));
				if ((gy >> 24) != 0u && stack.size() < (size_t)capacity) { stack.push_back({ gx, gy }); high = std::max(high, (uint32_t)stack.size()); }   // Push8: sp < GMAX
				if (node >= bvh.nodes8.size()) return false;
				const DNode8& nd = bvh.nodes8[node];
				const uint32_t imask = nd.meta >> 24, hit = Step8Host(nd, oa, invc, neg, ntMin, fminf(best, FLT_MAX));   // (the exit distance shrinks with the best hit)
				// the triangles of the hit leaf children, before any inner child is entered (Next8)
				for (uint32_t ch = 0; ch < 8u; ++ch) {
					if (!((hit & ~imask) >> ch & 1u)) continue;
					uint32_t first; const uint32_t count = Leaf8(nd, ch, first);
					for (uint32_t k = 0; k < count; ++k) if (!triangle(first + k)) return false;
				}
				gx = nd.childBase; gy = (InnerInVisitOrder(hit & imask, oct) << 24) | imask;
			}
		}
		outT[r] = best;
		if (outHighWater) outHighWater[r] = high;
	}
	return true;
}

} // namespace rl
