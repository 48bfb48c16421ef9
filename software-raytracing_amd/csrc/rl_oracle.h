// The host oracles (rl_oracle.cc): every query family's brute-force loop over the scene's triangles, in the arithmetic the kernels compile from the same
// headers (rl_nearest.h, rl_sweep.h, rl_overlap.h, rl_contact.h, rl_box.h, rl_sdf.h, rl_motion.h, rl_temporal.h, rl_variance.h, rl_progressive.h).  They are test instruments: the
// tests hold the kernels to them byte for byte.  Plain C++ on a scene whose host copies are current: no handle, no log, no refusal and no device -- the ABI
// (rl_abi.cc: the family's ...ArgsValid, then RunOnHost) has checked the arguments and read back what a move left stale before it calls one of these.
#pragma once

#include "rl_host.h"
#include "rl_slack.h"

#include <float.h>
#include <utility>

namespace rl {

// Statement M1 on one ray and one triangle, the one host text of the device's triangle test under the ray queries' candidate rule (rl_dev_walk.h OwnBoxPassBox
// under RL_OWN_BOX_WIDEN_TMIN): the plane's t in [tMin, FLT_MAX] (a NaN t fails here), the barycentrics, the triangle's own box with the widened tMin clause, the
// slack.  d's reciprocals are the exact ones.  True: accepted, with its t and barycentrics; the caller adds its own upper end (t <= tMax, t < the best so far)
// and, where the family has one, the cut-out test.  Inline: rl_bvh.cc's walks use it in programs built from that unit alone.
inline bool TriangleM1Host(const HostTriangle& T, const f3& o, const f3& d, float tMin, float& tOut, float& paOut, float& pbOut)
{
	const float oa[3] = { o.x, o.y, o.z }, inv[3] = { 1.0f / d.x, 1.0f / d.y, 1.0f / d.z };
	const f3 nrm = normalize(cross(T.v1 - T.v0, T.v2 - T.v0));
	const float t = dot((T.v0 - o), nrm) / dot(d, nrm);
	if (!(t >= tMin && t <= FLT_MAX)) return false;
	const f3 p = o + t * d;
	const f3 u = T.v1 - T.v0, v = T.v2 - T.v0, w = p - T.v0;
	const float uv = dot(u, v), wv = dot(w, v), uu = dot(u, u), vv = dot(v, v), wu = dot(w, u);
	const float denom = uv * uv - uu * vv;
	const float pa = (uv * wv - vv * wu) / denom, pb = (uv * wu - uu * wv) / denom;
	if (!(0.0f <= pa && 0.0f <= pb && pa + pb <= 1.0f)) return false;
	const f3 mn = fmin3(fmin3(T.v0, T.v1), T.v2), mx = fmax3(fmax3(T.v0, T.v1), T.v2);
	const float mna[3] = { mn.x, mn.y, mn.z }, mxa[3] = { mx.x, mx.y, mx.z };
	float lo = -INFINITY, hi = FLT_MAX; bool ok = true;
	for (int a = 0; a < 3; ++a) {
		float t0 = (mna[a] - oa[a]) * inv[a], t1 = (mxa[a] - oa[a]) * inv[a];
		if (inv[a] < 0.0f) std::swap(t0, t1);
		lo = fmaxf(lo, t0); hi = fminf(hi, t1);
		if (hi < lo) ok = false;
	}
	if (!(ok && !(hi * RL_BOX_WIDEN < tMin) && t * RL_CANDIDATE_SLACK >= fmaxf(lo, tMin))) return false;
	tOut = t; paOut = pa; pbOut = pb;
	return true;
}

// One function per RaylibAMD_*Host entry of include/raylib_amd.h, with that entry's arrays; what the entry's refusals promise holds.
void TraceRaysAllHost(const Scene& s, const RaylibAMDRay* rays, int32_t n, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount);
void NearestPointsHost(const Scene& s, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out);
void NearestPointsAllHost(const Scene& s, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount);
void SweepSpheresHost(const Scene& s, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out);
void OverlapTrianglesHost(const Scene& s, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount);
void OverlapContactsHost(const Scene& s, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex, RaylibAMDContact* outContact, uint32_t* outCount);
// MARK: out is the call's mask of (triangles + 31) / 32 words, written whole
void OverlapBoxesHost(const Scene& s, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount);
// G: the caller's grid with maxDist's -0.0 read as +0.0
void BakeDistanceFieldHost(const Scene& s, const RaylibAMDDistanceFieldParams& G, float* outDist, int32_t* outPrim);
// prevCamera: the previous frame's camera (the current one when the caller names none); first, count, prevPositions: the parameters'
void MotionHost(uint32_t width, uint32_t height, const DCamera& prevCamera, int32_t first, int32_t count, const float* prevPositions, const float* rays, const RaylibAMDHitT* hit,
                RaylibAMDMotion* outMotion);
// both accumulations' entries: call.moments says which
void TemporalAccumulateHost(const TemporalCall& call);
// P: the caller's parameters or the defaults; planes: all five given.  False: no memory for the packed planes (nothing written)
bool FilterVarianceHost(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams& P, const RaylibAMDVarianceFilterPlanes& planes, float* outColour, float* outVariance);
void GatherAdaptiveDecideHost(const RaylibAMDGatherAdaptiveParams& adaptive, uint32_t cap, const float* keys, int64_t count, uint32_t* outSamples);
void GatherDirectionsHost(const RaylibAMDGatherParams& params, const RaylibAMDGatherPoint* points, int32_t n, uint64_t seed, uint32_t sample, float* outDirs);

} // namespace rl
