// The host oracles (rl_oracle.h): brute force over every triangle in export order, one loop per family.
#include "rl_oracle.h"
#include "rl_progressive.h"
#include "rl_nearest.h"
#include "rl_sweep.h"
#include "rl_sdf.h"
#include "rl_overlap.h"
#include "rl_contact.h"
#include "rl_box.h"
#include "rl_motion.h"
#include "rl_temporal.h"
#include "rl_variance.h"
#include "raylib_amd_rng.h"

#include <string.h>
#include <algorithm>
#include <cmath>
#include <new>

namespace rl {

namespace {

// Statement M1 with the cut-out test on the ray's [tMin, tMax], tMin already raised to 0: TriangleM1Host, the upper end, and for a triangle whose material is a
// microfacet one with an albedo map the test of rl_dev_scene.h AlphaTestCandidateNI / TexFetch on that map (the device's converted copy is this powf of each texel).
bool HostRayAccepts(const Scene& s, const HostTriangle& T, const f3& o, const f3& d, float tMin, float tMax, float& t, float& pa, float& pb)
{
	if (!(TriangleM1Host(T, o, d, tMin, t, pa, pb) && t <= tMax)) return false;
	if (T.material >= 0 && (size_t)T.material < s.materials.size()) {
		const HostMaterial& M = s.materials[(size_t)T.material];
		if (M.type == MAT_MICROFACET && M.tex[0] >= 0 && (size_t)M.tex[0] < s.textures.size()) {
			const Image& im = *s.textures[(size_t)M.tex[0]];
			float U = (1 - pa - pb) * T.s0 + pa * T.s1 + pb * T.s2;
			float V = (1 - pa - pb) * T.t0 + pa * T.t1 + pb * T.t2;
			U = fmodf(U, 1.0f); if (U < 0.0f) U += 1.0f;
			V = fmodf(V, 1.0f); if (V < 0.0f) V += 1.0f; V = 1.0f - V;
			if (std::isnan(U) || std::isinf(U)) U = 0.0f;
			if (std::isnan(V) || std::isinf(V)) V = 0.0f;
			const int x = (int)((float)(uint32_t)(im.width - 1) * U), y = (int)((float)(uint32_t)(im.height - 1) * V);
			const float alpha = powf(im.rgba[4 * ((size_t)y * im.width + (size_t)x) + 3], 2.2f);
			if (!(alpha >= 0.5f)) return false;
		}
	}
	return true;
}

// Statements N1 to N4 (rl_nearest.h, the kernel's own source) for one point over every triangle in export order.  ANY: the first triangle within maxDist;
// CLOSEST: the nearest one; ALL: every one within maxDist, appended to `all` in ascending index.  The tie rule of all of them is stated here: k ascends and a
// found triangle is replaced only by a strictly smaller D, so an equal D keeps the lower index.  A triangle whose own-box distance B already exceeds the bound
// (maxDist^2, or CLOSEST's best so far) is skipped before its E is taken, which changes nothing: D >= B (N3).  The hit's prim is -1 when there is none.
enum NearestWant { NEAREST_ANY, NEAREST_CLOSEST, NEAREST_ALL };
RaylibAMDNearestHit NearestOverTriangles(const Scene& s, const float pos[3], float maxDist, NearestWant want, std::vector<RaylibAMDNearestHit>* all = nullptr)
{
	RaylibAMDNearestHit best = { 0.0f, -1, 0.0f, 0.0f };
	if (!NearestTakesPart(pos[0], pos[1], pos[2], maxDist)) return best;
	const float R2 = maxDist * maxDist;
	for (size_t k = 0; k < s.triangles.size(); ++k) {
		const HostTriangle& t = s.triangles[k];
		const bool found = best.prim >= 0;
		const float B = NearestOwnBoxDist2(pos, &t.v0.x, &t.v1.x, &t.v2.x);
		if (B > (found ? best.dist2 : R2)) continue;
		float b1, b2;
		const float D = NearestTriangleD(NearestTriangleE(pos, &t.v0.x, &t.v1.x, &t.v2.x, b1, b2), B);
		if (!(D <= R2) || (found && !(D < best.dist2))) continue;
		const RaylibAMDNearestHit hit = { D, (int32_t)k, b1, b2 };
		if (want == NEAREST_ALL) { all->push_back(hit); continue; }
		best = hit;
		if (want == NEAREST_ANY) break;
	}
	return best;
}

// Statements O1 to O5 (rl_overlap.h, the kernel's own source) for one query triangle over every triangle in export order: visit(k, triangle) for each accepted
// one, k ascending, until it returns false.
template <typename Visit>
void ForEachOverlap(const Scene& s, const RaylibAMDOverlapQuery& Q, bool skipShared, Visit visit)
{
	if (!OverlapTakesPart(Q.v0, Q.v1, Q.v2)) return;
	float lo[3], hi[3];
	OverlapOwnBox(Q.v0, Q.v1, Q.v2, lo, hi);
	for (size_t k = 0; k < s.triangles.size(); ++k) {
		const HostTriangle& t = s.triangles[k];
		if (OverlapAccepts(Q.v0, Q.v1, Q.v2, lo, hi, &t.v0.x, &t.v1.x, &t.v2.x, skipShared) && !visit(k, t)) return;
	}
}

// the temporal oracle's reads: arrays of any alignment
struct HostTaps {
	const float* colour; const RaylibAMDHitT* hit; const float* length; const float* moments;
	bool Has() const { return colour != nullptr; }
	void Moments(size_t q, float m[2]) const { memcpy(m, moments + 2 * q, 2 * sizeof(float)); }
	TemporalTap Read(size_t q) const
	{
		TemporalTap t; RaylibAMDHitT h;
		memcpy(&h, hit + q, sizeof(h));
		memcpy(&t.r, colour + 4 * q, 3 * sizeof(float));
		t.t = h.t; t.prim = h.prim; memcpy(&t.length, length + q, sizeof(float));
		return t;
	}
};

} // namespace

// Statements M1 to M5: every triangle slot in turn with HostRayAccepts on the ray's own [QueryTMin(tMin), tMax]; the accepted ones sorted by (t, slot).
void TraceRaysAllHost(const Scene& s, const RaylibAMDRay* rays, int32_t n, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount)
{
	const std::vector<uint32_t>& order = s.bvh.triOrder;
	struct Key { float t; uint32_t slot; float b1, b2; };
	std::vector<Key> keys;
	for (int32_t i = 0; i < n; ++i) {
		const RaylibAMDRay& Q = rays[i];
		const f3 o = F3(Q.org[0], Q.org[1], Q.org[2]), d = F3(Q.dir[0], Q.dir[1], Q.dir[2]);
		const float tMin = Q.tMin < 0.0f ? 0.0f : Q.tMin, tMax = Q.tMax;   // (a NaN bound fails every comparison of HostRayAccepts)
		keys.clear();
		for (uint32_t slot = 0; slot < (uint32_t)order.size(); ++slot) {
			if (order[slot] >= s.triangles.size()) continue;
			float t, pa, pb;
			if (HostRayAccepts(s, s.triangles[order[slot]], o, d, tMin, tMax, t, pa, pb)) keys.push_back({ t, slot, pa, pb });
		}
		std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.t < b.t || (a.t == b.t && a.slot < b.slot); });
		RaylibAMDHitT* row = outHits + (size_t)i * (size_t)maxHits;
		for (int32_t k = 0; k < maxHits; ++k) {
			if ((size_t)k < keys.size()) { row[k].t = keys[(size_t)k].t; row[k].prim = (int32_t)order[keys[(size_t)k].slot]; row[k].b1 = keys[(size_t)k].b1; row[k].b2 = keys[(size_t)k].b2; }
			else { row[k].t = 0.0f; row[k].prim = -1; row[k].b1 = 0.0f; row[k].b2 = 0.0f; }
		}
		if (outCount) outCount[i] = (uint32_t)keys.size();
	}
}

void NearestPointsHost(const Scene& s, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out)
{
	const bool within = kind == RAYLIB_AMD_NEAREST_WITHIN;
	for (int32_t i = 0; i < n; ++i) {
		const RaylibAMDNearestHit best = NearestOverTriangles(s, points[i].pos, points[i].maxDist, within ? NEAREST_ANY : NEAREST_CLOSEST);
		if (within) ((uint32_t*)out)[i] = best.prim >= 0 ? 1u : 0u;
		else ((RaylibAMDNearestHit*)out)[i] = best;
	}
}

// Statements K1 to K3 on N1 to N4: the set within maxDist sorted by (D, k)
void NearestPointsAllHost(const Scene& s, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount)
{
	std::vector<RaylibAMDNearestHit> set;
	for (int32_t i = 0; i < n; ++i) {
		set.clear();
		NearestOverTriangles(s, points[i].pos, points[i].maxDist, NEAREST_ALL, &set);
		const size_t listed = std::min(set.size(), (size_t)maxHits);
		std::partial_sort(set.begin(), set.begin() + (ptrdiff_t)listed, set.end(),
		                  [](const RaylibAMDNearestHit& a, const RaylibAMDNearestHit& b) { return a.dist2 < b.dist2 || (a.dist2 == b.dist2 && a.prim < b.prim); });
		RaylibAMDNearestHit* row = outHits + (size_t)i * (size_t)maxHits;
		for (size_t k = 0; k < (size_t)maxHits; ++k) row[k] = k < listed ? set[k] : RaylibAMDNearestHit{ 0.0f, -1, 0.0f, 0.0f };
		if (outCount) outCount[i] = (uint32_t)set.size();
	}
}

// Statements W1 to W6 (rl_sweep.h, the kernel's own source) over every triangle in export order
void SweepSpheresHost(const Scene& s, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out)
{
	for (int32_t i = 0; i < n; ++i) {
		const RaylibAMDSweepQuery& Q = q[i];
		RaylibAMDSweepHit best; memset(&best, 0, sizeof(best)); best.prim = -1;
		SweepMove M;
		if (SweepTakesPart(Q.origin, Q.delta, Q.radius, M)) {
			for (size_t k = 0; k < s.triangles.size(); ++k) {
				const HostTriangle& tr = s.triangles[k];
				float t, p[3]; int feature;
				if (!SweepTriangle(M, &tr.v0.x, &tr.v1.x, &tr.v2.x, t, feature, p)) continue;
				const float T = SweepTriangleT(t, SweepOwnBoxTime(M, &tr.v0.x, &tr.v1.x, &tr.v2.x));
				if (!(T <= 1.0f) || (best.prim >= 0 && !(T < best.t))) continue;   // (ascending k: an equal T keeps the lower index)
				best.t = T; best.prim = (int32_t)k; best.feature = feature; best.point[0] = p[0]; best.point[1] = p[1]; best.point[2] = p[2];
				if (kind == RAYLIB_AMD_SWEEP_ANY) break;
			}
		}
		if (kind == RAYLIB_AMD_SWEEP_ANY) ((uint32_t*)out)[i] = best.prim >= 0 ? 1u : 0u;
		else ((RaylibAMDSweepHit*)out)[i] = best;
	}
}

void OverlapTrianglesHost(const Scene& s, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount)
{
	const bool list = kind == RAYLIB_AMD_OVERLAP_LIST, skipShared = (flags & RAYLIB_AMD_OVERLAP_SKIP_SHARED) != 0u;
	for (int32_t i = 0; i < n; ++i) {
		int32_t* row = list ? (int32_t*)out + (size_t)i * (size_t)maxHits : nullptr;
		uint32_t count = 0;
		ForEachOverlap(s, q[i], skipShared, [&](size_t k, const HostTriangle&) {
			if (list && count < (uint32_t)maxHits) row[count] = (int32_t)k;
			++count;
			return list;   // (ANY stops at the first)
		});
		if (!list) ((uint32_t*)out)[i] = count ? 1u : 0u;
		else {
			for (uint32_t e = count; e < (uint32_t)maxHits; ++e) row[e] = -1;
			if (outCount) outCount[i] = count;
		}
	}
}

// LIST's rows, then statements C1 to C6 (rl_contact.h, the kernel's own source) for every listed pair
void OverlapContactsHost(const Scene& s, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex, RaylibAMDContact* outContact, uint32_t* outCount)
{
	const bool skipShared = (flags & RAYLIB_AMD_OVERLAP_SKIP_SHARED) != 0u;
	for (int32_t i = 0; i < n; ++i) {
		const RaylibAMDOverlapQuery& Q = q[i];
		int32_t* row = outIndex + (size_t)i * (size_t)maxHits;
		RaylibAMDContact* rec = outContact + (size_t)i * (size_t)maxHits;
		uint32_t count = 0;
		ForEachOverlap(s, Q, skipShared, [&](size_t k, const HostTriangle& t) {
			if (count < (uint32_t)maxHits) {
				row[count] = (int32_t)k;
				const ContactRecord R = ContactOfPair(Q.v0, Q.v1, Q.v2, &t.v0.x, &t.v1.x, &t.v2.x);
				memcpy(&rec[count], &R, sizeof(R));
			}
			++count;
			return true;
		});
		for (uint32_t e = count; e < (uint32_t)maxHits; ++e) { row[e] = -1; memset(&rec[e], 0, sizeof(rec[e])); }
		if (outCount) outCount[i] = count;
	}
}

// Statements B1 to B5 (rl_box.h, the kernel's own source) for every query box over every triangle in export order
void OverlapBoxesHost(const Scene& s, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount)
{
	const bool list = kind == RAYLIB_AMD_BOX_LIST, mark = kind == RAYLIB_AMD_BOX_MARK;
	if (mark && out) memset(out, 0, (s.triangles.size() + 31u) / 32u * sizeof(uint32_t));
	for (int32_t i = 0; i < n; ++i) {
		BoxQ Q;
		for (int a = 0; a < 3; ++a) {
			Q.c[a] = q[i].center[a]; Q.h[a] = q[i].axis[a].half;
			for (int k = 0; k < 3; ++k) Q.a[a][k] = q[i].axis[a].dir[k];
		}
		int32_t* row = list ? (int32_t*)out + (size_t)i * (size_t)maxHits : nullptr;
		uint32_t count = 0;
		if (BoxTakesPart(Q)) {
			BoxEnclosing(Q);
			for (size_t k = 0; k < s.triangles.size(); ++k) {
				const HostTriangle& t = s.triangles[k];
				if (!BoxAccepts(Q, &t.v0.x, &t.v1.x, &t.v2.x)) continue;
				if (list && count < (uint32_t)maxHits) row[count] = (int32_t)k;
				if (mark) ((uint32_t*)out)[k >> 5] |= 1u << (k & 31u);
				++count;
				if (!list && !mark) break;   // (ANY stops at the first)
			}
		}
		if (list) {
			for (uint32_t e = count; e < (uint32_t)maxHits; ++e) row[e] = -1;
			if (outCount) outCount[i] = count;
		} else if (!mark) ((uint32_t*)out)[i] = count ? 1u : 0u;
	}
}

// V3 and V4 per sign axis and row: statement M1 (HostRayAccepts) on every triangle, then for every voxel of the row the crossings ahead of its centre counted
// one by one (no prefix trick: that is the device's).  V2 per voxel: the nearest triangle of its centre (NearestOverTriangles).  V5 at the store.
void BakeDistanceFieldHost(const Scene& s, const RaylibAMDDistanceFieldParams& G, float* outDist, int32_t* outPrim)
{
	const uint32_t n[3] = { (uint32_t)G.dims[0], (uint32_t)G.dims[1], (uint32_t)G.dims[2] };
	const size_t voxels = (size_t)n[0] * n[1] * n[2];
	// how many of the asked axes call a voxel inside
	std::vector<uint8_t> votes(G.sign == RAYLIB_AMD_SDF_UNSIGNED ? 0 : voxels, 0);
	const int asked = G.sign == RAYLIB_AMD_SDF_UNSIGNED ? 0 : G.sign == RAYLIB_AMD_SDF_SIGN_MAJORITY ? 3 : 1;
	std::vector<float> ts;
	for (int a = 0; a < 3 && asked; ++a) {
		if (asked == 1 && a != G.sign - RAYLIB_AMD_SDF_SIGN_X) continue;
		const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;   // the other two axes, the lower one first
		for (uint32_t ic = 0; ic < n[c]; ++ic) for (uint32_t ib = 0; ib < n[b]; ++ib) {
			float org[3]; org[a] = G.origin[a]; org[b] = SdfCentre(G.origin[b], G.spacing[b], ib); org[c] = SdfCentre(G.origin[c], G.spacing[c], ic);
			const f3 o = F3(org[0], org[1], org[2]), d = F3(a == 0 ? 1.0f : 0.0f, a == 1 ? 1.0f : 0.0f, a == 2 ? 1.0f : 0.0f);
			ts.clear();
			for (const HostTriangle& T : s.triangles) {
				float t, pa, pb;
				if (HostRayAccepts(s, T, o, d, 0.0f, FLT_MAX, t, pa, pb)) ts.push_back(t);
			}
			if (ts.empty()) continue;
			for (uint32_t i = 0; i < n[a]; ++i) {
				const float ti = SdfT(G.spacing[a], i);
				size_t ahead = 0;
				for (float t : ts) if (t > ti) ++ahead;
				if (!(ahead & 1u)) continue;
				uint32_t v[3]; v[a] = i; v[b] = ib; v[c] = ic;
				++votes[((size_t)v[2] * n[1] + v[1]) * n[0] + v[0]];
			}
		}
	}
	for (uint32_t k = 0; k < n[2]; ++k) for (uint32_t j = 0; j < n[1]; ++j) for (uint32_t i = 0; i < n[0]; ++i) {
		const float pos[3] = { SdfCentre(G.origin[0], G.spacing[0], i), SdfCentre(G.origin[1], G.spacing[1], j), SdfCentre(G.origin[2], G.spacing[2], k) };
		const RaylibAMDNearestHit best = NearestOverTriangles(s, pos, G.maxDist, NEAREST_CLOSEST);
		const size_t at = ((size_t)k * n[1] + j) * n[0] + i;
		float m = best.prim >= 0 ? __builtin_sqrtf(best.dist2) : G.maxDist;
		if (asked && 2 * (int)votes[at] > asked) m = -m;
		outDist[at] = m;
		if (outPrim) outPrim[at] = best.prim;
	}
}

// Statements T2 to T4 (rl_motion.h, the kernel's own source) per pixel
void MotionHost(uint32_t width, uint32_t height, const DCamera& pc, int32_t first, int32_t count, const float* prevPositions, const float* rays, const RaylibAMDHitT* hit,
                RaylibAMDMotion* outMotion)
{
	for (size_t p = 0; p < (size_t)width * height; ++p) {
		const float* r = rays + 7 * p;
		RaylibAMDHitT h; memcpy(&h, hit + p, sizeof(h));
		const bool isHit = h.prim >= 0;
		float P[3] = { r[3], r[4], r[5] };
		if (isHit) {
			const int64_t k = (int64_t)h.prim - first;
			if (h.prim < RAYLIB_AMD_PRIM_SPHERE && k >= 0 && k < count) MotionTrianglePoint(prevPositions + 9 * (size_t)k, h.b1, h.b2, P);
			else MotionRayPoint(r, r + 3, h.t, P);
		}
		float o[3];
		RaylibAMDMotion m;
		m.status = MotionProject(pc.origin, pc.top_left, pc.horizontal, pc.vertical, (float)width, (float)height, isHit, P, o);
		m.prevX = o[0]; m.prevY = o[1]; m.prevT = o[2];
		memcpy(outMotion + p, &m, sizeof(m));
	}
}

// Statement T7 (rl_temporal.h, the kernel's own source) per pixel; MOMENTS: with statement S1 beside it
template <bool MOMENTS>
static void TemporalPixelsHost(const TemporalCall& C)
{
	const HostTaps taps = { C.history.colour, C.history.hit, C.history.length, C.history.moments };
	for (size_t p = 0; p < (size_t)C.width * C.height; ++p) {
		RaylibAMDHitT h; RaylibAMDMotion m; float c[3], o[4], len, mom[2];
		memcpy(&h, C.hit + p, sizeof(h)); memcpy(&m, C.motion + p, sizeof(m)); memcpy(c, C.colour + 4 * p, sizeof(c));
		TemporalPixelM<MOMENTS>(C.width, C.height, c, h.prim, m.prevX, m.prevY, m.prevT, m.status, C.params->depthTolerance, C.params->maxLength, taps, o, len, mom);
		o[3] = 1.0f;
		memcpy(C.outColour + 4 * p, o, sizeof(o)); memcpy(C.outLength + p, &len, sizeof(len));
		if (MOMENTS) memcpy(C.outMoments + 2 * p, mom, sizeof(mom));
	}
}
void TemporalAccumulateHost(const TemporalCall& C)
{
	if (C.moments) TemporalPixelsHost<true>(C);
	else TemporalPixelsHost<false>(C);
}

// Statements S3 to S6 (rl_variance.h, the kernels' own source): the packed records the device makes, then the same per-pixel functions in the same order of
// launches.  The caller's arrays may have any alignment and outColour may be any of them but `colour`: everything is read before anything is written.
bool FilterVarianceHost(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams& P, const RaylibAMDVarianceFilterPlanes& planes, float* outColour, float* outVariance)
{
	const int W = (int)width, H = (int)height;
	const size_t n = (size_t)width * height;
	const VfConst c = MakeVfConst(P.sigmaLuminance, P.sigmaNormal, P.sigmaPlane, P.historyLength);
	std::vector<VfGuide> guides;
	std::vector<VfValue> a, b;
	std::vector<float> moments, length;
	try { guides.resize(n); a.resize(n); b.resize(n); moments.resize(2 * n); length.resize(n); }
	catch (const std::bad_alloc&) { return false; }   // (the ABI logs it)
	memcpy(moments.data(), planes.moments, 2 * n * sizeof(float)); memcpy(length.data(), planes.length, n * sizeof(float));
	for (size_t p = 0; p < n; ++p) {
		RaylibAMDHitT h; float s[11], col[3];
		memcpy(&h, planes.hit + p, sizeof(h)); memcpy(s, (const char*)planes.surface + 44 * p, sizeof(s)); memcpy(col, planes.colour + 4 * p, sizeof(col));
		guides[p] = VfPackGuide(h.prim, s + 2, s + 5);
		a[p].r = VfFin(col[0]); a[p].g = VfFin(col[1]); a[p].b = VfFin(col[2]); a[p].var = 0.0f;
	}
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x) {
			const size_t p = (size_t)y * width + (size_t)x;
			if (guides[p].prim != -1) a[p].var = VfInitialVariance(guides.data(), moments.data(), length.data(), W, H, x, y, c);
		}
	for (int i = 0; i < P.iterations; ++i) {
		for (int y = 0; y < H; ++y)
			for (int x = 0; x < W; ++x) {
				const size_t p = (size_t)y * width + (size_t)x;
				b[p] = guides[p].prim == -1 ? a[p] : VfFilterPixel(a.data(), guides.data(), W, H, x, y, 1 << i, c);
			}
		a.swap(b);
	}
	for (size_t p = 0; p < n; ++p) {
		const float o[4] = { a[p].r, a[p].g, a[p].b, 1.0f };
		memcpy(outColour + 4 * p, o, sizeof(o));
		if (outVariance) memcpy(outVariance + p, &a[p].var, sizeof(float));
	}
	return true;
}

// statements A1 to A3 on the caller's keys: the oracle of k_gather_adaptive_resolve's moments and decision (rl_progressive.h, built without FMA)
void GatherAdaptiveDecideHost(const RaylibAMDGatherAdaptiveParams& adaptive, uint32_t cap, const float* keys, int64_t count, uint32_t* outSamples)
{
	for (int64_t i = 0; i < count; ++i) {
		const float* key = keys + (size_t)i * cap * 3;
		float s1 = 0.0f, s2 = 0.0f;
		uint32_t n = 0;
		for (;;) {
			const uint32_t now = (uint32_t)std::min<uint64_t>(cap, (uint64_t)n + adaptive.passSamples);
			for (; n < now; ++n) {
				const float lum = key[3 * (size_t)n] * 0.2126f + key[3 * (size_t)n + 1] * 0.7152f + key[3 * (size_t)n + 2] * 0.0722f;
				const float y = lum / (1.0f + lum);
				s1 += y; s2 += y * y;
			}
			if (n == cap || ProgressiveCellStops(ProgressivePixelError(s1, s2, n), n, adaptive.threshold, adaptive.minSamples)) break;
		}
		outSamples[i] = n;
	}
}

// statement 1 of the gather's contract with the host's libm: rl_dev_core.h RandomInUnitSphere and normalize, rl_dev_shade.h's Lambertian flip
void GatherDirectionsHost(const RaylibAMDGatherParams& params, const RaylibAMDGatherPoint* points, int32_t n, uint64_t seed, uint32_t sample, float* outDirs)
{
	for (int32_t i = 0; i < n; ++i) {
		RaylibRngStream g = raylib_rng_begin(seed, points[i].stream, params.sampleFirst + sample);
		for (uint32_t k = 0; k < params.skipDraws; ++k) (void)raylib_rng_next_u32(&g);
		const float u1 = raylib_rng_next_float(&g);
		const float u2 = raylib_rng_next_float(&g);
		const float z = 1.0f - 2.0f * u1;
		const float r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
		const float phi = 2.0f * 3.141592f * u2;
		float w[3] = { r * cosf(phi), r * sinf(phi), z };
		const float* N = points[i].normal;
		if (params.kind == RAYLIB_AMD_GATHER_IRRADIANCE && (double)(w[0] * N[0] + w[1] * N[1] + w[2] * N[2]) < 0.0) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; }
		const float k = 1.0f / sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
		outDirs[3 * (size_t)i + 0] = w[0] * k; outDirs[3 * (size_t)i + 1] = w[1] * k; outDirs[3 * (size_t)i + 2] = w[2] * k;
	}
}

} // namespace rl
