// Kernel bodies of a move of the scene's triangles (include/raylib_amd.h RaylibAMD_SceneMoveTriangles); included by rl_refit.hip.
//   k_move_count    once per scene: how many records carry a divisor outside [2^-62, 2^125]
//   k_move_scan     a value of the call that is not finite raises the status block's flag
//   k_move_records  per moved triangle: its DTriIsect again, and its DTriShade's normals when the call gives normals
//   k_refit_level   per binary node of one level, deepest level first: both child boxes -- a triangle leaf's from its triangles' vertices, an inner child's from
//                   that node's two boxes, written by the launch before; a sphere's, a cube's and an empty child's stay
//   k_refit_wide4, k_refit_wide8   per wide record: its children's boxes from the binary tree's (rl_grid.h), the grid re-derived
// One launch per level and stage: what a thread reads of another thread's was written by an earlier launch on the same stream.  No thread waits for another.

// the divisor of a record's barycentric divisions, as the host forms it (rl_scene.cc FlattenScene), and whether it is one that clears fastBary
__device__ __forceinline__ bool BadDenom(float uv, float uu, float vv, float& denom)
{
	const float uvuv = uv * uv, uuvv = uu * vv;
	denom = uvuv - uuvv;
	const float mag = fabsf(denom);
	if (denom == 0.0f || denom != denom) return false;
	return !(mag >= 0x1p-62f && mag <= 0x1p125f);
}

__global__ void __launch_bounds__(RL_BLOCK)
k_move_count(const DTriIsect* __restrict__ isect, uint32_t numTris, uint32_t* __restrict__ status)
{
	const uint32_t k = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (k >= numTris) return;
	float denom;
	if (BadDenom(isect[k].uv, isect[k].uu, isect[k].vv, denom)) atomicAdd(&status[RL_MOVE_BAD_DENOM], 1u);
}

__global__ void __launch_bounds__(RL_BLOCK)
k_move_scan(const float* __restrict__ positions, const float* __restrict__ normals, uint32_t floats, uint32_t* __restrict__ status)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= floats) return;
	const float p = positions[i], n = normals ? normals[i] : 0.0f;
	if (!(p - p == 0.0f) || !(n - n == 0.0f)) status[RL_MOVE_NONFINITE] = 1u;   // (x - x is 0 for every finite x, NaN for inf and NaN)
}

// The record of rl_scene.cc FlattenScene, operation by operation: V3's arithmetic is the host f3's, rtm::sqrt_ and rtm::rcp1_ are sqrtf and 1.0f / x bit for bit
// (rl_math.h), and the unit is built without FMA contraction.
__global__ void __launch_bounds__(RL_BLOCK)
k_move_records(DTriIsect* __restrict__ isect, DTriShade* __restrict__ shade, const int32_t* __restrict__ slotOf, uint32_t first, uint32_t count, uint32_t numTris,
               const float* __restrict__ positions, const float* __restrict__ normals, uint32_t* __restrict__ status)
{
	const uint32_t k = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (k >= count || first + k >= numTris || status[RL_MOVE_NONFINITE] != 0u) return;
	const uint32_t slot = (uint32_t)slotOf[first + k];
	if (slot >= numTris) return;
	const float* p = positions + (size_t)k * 9;
	const V3 v0 = ld3(p), v1 = ld3(p + 3), v2 = ld3(p + 6);
	const V3 nrm = normalize(cross(v1 - v0, v2 - v0));
	const V3 u = v1 - v0, v = v2 - v0;
	const float uv = dot(u, v), uu = dot(u, u), vv = dot(v, v);
	float denomOld, denom;
	const bool badOld = BadDenom(isect[slot].uv, isect[slot].uu, isect[slot].vv, denomOld), bad = BadDenom(uv, uu, vv, denom);
	DTriIsect I;
	I.v0[0] = v0.x; I.v0[1] = v0.y; I.v0[2] = v0.z;
	I.n[0] = nrm.x; I.n[1] = nrm.y; I.n[2] = nrm.z;
	I.v1[0] = v1.x; I.v1[1] = v1.y; I.v1[2] = v1.z;
	I.v2[0] = v2.x; I.v2[1] = v2.y; I.v2[2] = v2.z;
	I.uv = uv; I.uu = uu; I.vv = vv;
	I.rden = (denom == 0.0f || denom != denom || bad) ? __builtin_nanf("") : rtm::rcp1_(denom);
	isect[slot] = I;
	if (bad != badOld) atomicAdd(&status[RL_MOVE_BAD_DENOM], bad ? 1u : 0xffffffffu);
	if (normals) {
		const float* n = normals + (size_t)k * 9;
		float* dst = shade[slot].n0;   // n0, n1, n2: the record's first nine floats
#pragma unroll
		for (int i = 0; i < 9; ++i) dst[i] = n[i];
	}
}

// min and max as the host selects them (rl_host.h fmin3 / fmax3, std::min / std::max: the second operand only where it is strictly less / greater), so that zeros of
// either sign come out as in the builder's boxes
__device__ __forceinline__ float SelMin(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float SelMax(float a, float b) { return a < b ? b : a; }
// a triangle's own box, fmin3(fmin3(v0, v1), v2) as rl_scene.cc BuildAccel forms it, into its leaf's box, as the builder grows a node's box over its primitives in slot order
__device__ __forceinline__ void GrowBox(float mn[3], float mx[3], const DTriIsect& t)
{
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		mn[a] = SelMin(mn[a], SelMin(SelMin(t.v0[a], t.v1[a]), t.v2[a]));
		mx[a] = SelMax(mx[a], SelMax(SelMax(t.v0[a], t.v1[a]), t.v2[a]));
	}
}
// the box of child `ref` of a binary node into mn / mx; false: the child keeps the box it has
__device__ __forceinline__ bool ChildBox(const DNode* nodes, const DTriIsect* __restrict__ isect, int32_t ref, uint32_t numNodes, uint32_t numTris, float mn[3], float mx[3])
{
	if (ref == DNODE_EMPTY) return false;
	mn[0] = mn[1] = mn[2] = RL_BOX_MAX; mx[0] = mx[1] = mx[2] = -RL_BOX_MAX;
	if (ref >= 0) {
		if ((uint32_t)ref >= numNodes) return false;
		const DNode& c = nodes[ref];   // (an empty child's box is the inverted one: the union ignores it)
#pragma unroll
		for (int a = 0; a < 3; ++a) { mn[a] = SelMin(c.lmin[a], c.rmin[a]); mx[a] = SelMax(c.lmax[a], c.rmax[a]); }   // (the builder grows an inner node's box over its primitives, not over its children: with zeros of both signs on a face the two may differ in that zero's sign)
		return true;
	}
	const uint32_t code = (uint32_t)~ref, leafFirst = code >> LEAF_FIRST_SHIFT, leafCount = (code & LEAF_COUNT_MASK) + 1u;
	if (((code >> LEAF_KIND_SHIFT) & LEAF_KIND_MASK) != 0u || leafFirst + leafCount > numTris) return false;   // a sphere or a cube: the box the build gave it
	for (uint32_t k = 0; k < leafCount; ++k) {
		GrowBox(mn, mx, isect[leafFirst + k]);
	}
	return true;
}
__global__ void __launch_bounds__(RL_BLOCK)
k_refit_level(DNode* nodes, const DTriIsect* __restrict__ isect, const uint32_t* __restrict__ levelNodes, uint32_t count, uint32_t numNodes, uint32_t numTris)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= count) return;
	const uint32_t node = levelNodes[i];
	if (node >= numNodes) return;
	float mn[3], mx[3];
	if (ChildBox(nodes, isect, nodes[node].left, numNodes, numTris, mn, mx)) {
#pragma unroll
		for (int a = 0; a < 3; ++a) { nodes[node].lmin[a] = mn[a]; nodes[node].lmax[a] = mx[a]; }
	}
	if (ChildBox(nodes, isect, nodes[node].right, numNodes, numTris, mn, mx)) {
#pragma unroll
		for (int a = 0; a < 3; ++a) { nodes[node].rmin[a] = mn[a]; nodes[node].rmax[a] = mx[a]; }
	}
}

__device__ __forceinline__ bool BoxIdsOk(const int32_t* ids, int n, uint32_t numNodes)
{
	bool ok = true;
	for (int k = 0; k < n; ++k) if (ids[k] >= 0 && (uint32_t)(ids[k] >> 1) >= numNodes) ok = false;
	return ok;
}
// nodes4f (may be null): the float-box records, or a leaf list's; nodes4q (may be null): the grid records of the same nodes
__global__ void __launch_bounds__(RL_BLOCK)
k_refit_wide4(const DNode* __restrict__ nodes, uint32_t numNodes, const int32_t* __restrict__ boxOf, DNode4* __restrict__ nodes4f, DNode4Q* __restrict__ nodes4q, uint32_t count)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= count) return;
	int32_t ids[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) ids[k] = boxOf[4 * (size_t)i + k];
	if (!BoxIdsOk(ids, 4, numNodes)) return;
	DNode4 nd;
	if (nodes4f) nd = nodes4f[i];
	else {
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			nd.child[k] = nodes4q[i].child[k]; nd.pad[k] = 0u;
			for (int a = 0; a < 3; ++a) { nd.lo[a][k] = RL_BOX_MAX; nd.hi[a][k] = -RL_BOX_MAX; }
		}
	}
	RefitNode4(nodes, ids, nd);
	if (nodes4f) nodes4f[i] = nd;
	if (nodes4q) nodes4q[i] = QuantizeNode4(nd);
}

__global__ void __launch_bounds__(RL_BLOCK)
k_refit_wide8(const DNode* __restrict__ nodes, uint32_t numNodes, const int32_t* __restrict__ boxOf, DNode8* __restrict__ nodes8, uint32_t count)
{
	const uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (i >= count) return;
	int32_t ids[8];
#pragma unroll
	for (int k = 0; k < 8; ++k) ids[k] = boxOf[8 * (size_t)i + k];
	if (!BoxIdsOk(ids, 8, numNodes)) return;
	DNode8 nd = nodes8[i];
	RefitNode8(nodes, ids, nd);
	nodes8[i] = nd;
}
