// Scene / camera host logic: what the reference does in geom/scene.cc,
// render/camera.h and raylib.cc between Raylib_CreateScene and Raylib_FinalizeScene,
// re-stated for a flat device scene.
#include "rl_host.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <limits>
#include <thread>
#include <stdlib.h>
#include <string.h>

namespace rl {

// reference render/camera.h:55-78
void Camera::UpdateInternal()
{
	lensRadius = aperture * 0.5f;
	timePeriod = endTime - beginTime;
	w = normalize(origin - lookAt);
	f3 up = F3(0.0f, 1.0f, 0.0f);
	if (dot(w, up) >= 0.9f) up = F3(1.0f, 0.0f, 0.0f);
	u = normalize(cross(up, w));
	v = cross(w, u);
	const float pi_f = (float)3.1415926535897932385;
	float theta = fovY_degrees * pi_f / 180.0f;
	float hh = tanf(theta / 2.0f);
	float hw = aspectWH * hh;
	top_left = origin - (hw * focalDistance * u) - (hh * focalDistance * v) - (focalDistance * w);
	horizontal = 2.0f * hw * focalDistance * u;
	vertical = 2.0f * hh * focalDistance * v;
}

DCamera Camera::ToDevice() const
{
	DCamera d; memset(&d, 0, sizeof(d));
	d.origin[0] = origin.x; d.origin[1] = origin.y; d.origin[2] = origin.z; d.lensRadius = lensRadius;
	d.top_left[0] = top_left.x; d.top_left[1] = top_left.y; d.top_left[2] = top_left.z; d.beginTime = beginTime;
	d.horizontal[0] = horizontal.x; d.horizontal[1] = horizontal.y; d.horizontal[2] = horizontal.z; d.timePeriod = timePeriod;
	d.vertical[0] = vertical.x; d.vertical[1] = vertical.y; d.vertical[2] = vertical.z;
	d.u[0] = u.x; d.u[1] = u.y; d.u[2] = u.z;
	d.v[0] = v.x; d.v[1] = v.y; d.v[2] = v.z;
	return d;
}

// reference geom/scene.cc:6-10
Scene::Scene()
{
	sunIlluminance = F3(0.0f, 0.0f, 0.0f);
	sunDirection = normalize(F3(0.0f, -1.0f, -0.5f));
}

Scene::~Scene()
{
	if (device) DeviceReleaseScene(device);
}

// reference geom/scene.cc:23-31 builds the top BVH over the elements added so far and
// ignores later additions.  Here: concatenate the borrowed models' triangles, offset
// their material / texture indices, build the flat BVH, mark alpha-tested leaves.
void Scene::Finalize()
{
	if (finalized) return;
	finalized = true;
	triangles.clear(); materials.clear(); textures.clear();
	int32_t shapeBase = 0;
	for (OBJModel* m : models) {
		const int32_t matBase = (int32_t)materials.size();
		const int32_t texBase = (int32_t)textures.size();
		for (const std::shared_ptr<Image>& im : m->images) textures.push_back(im);
		for (HostMaterial hm : m->materials) {
			for (int k = 0; k < 5; ++k) if (hm.tex[k] >= 0) hm.tex[k] += texBase;
			materials.push_back(hm);
		}
		for (HostTriangle t : m->triangles) {
			t.material += matBase;
			t.shape += shapeBase;
			triangles.push_back(t);
		}
		shapeBase += m->numShapes;
	}
	// elements added with Raylib_AddSceneElement: spheres, cubes, loose triangles; each brings its material
	spheres.clear(); cubes.clear();
	for (SceneElement* e : elements) {
		const int32_t mat = (int32_t)materials.size();
		HostMaterial hm = e->material->m;
		for (int k = 0; k < 5; ++k) hm.tex[k] = -1;
		materials.push_back(hm);
		if (e->kind == PRIM_SPHERE) { HostSphere s; s.center = e->center; s.radius = e->radius; s.material = mat; spheres.push_back(s); }
		else if (e->kind == PRIM_CUBE) { HostCube c; c.minBounds = e->minBounds; c.maxBounds = e->maxBounds; c.timeStartMove = e->timeStartMove; c.velocity = e->velocity; c.material = mat; cubes.push_back(c); }
		else { HostTriangle t = e->tri; t.material = mat; t.shape = shapeBase++; triangles.push_back(t); }
	}
	hasMovingCubes = false;
	for (const HostCube& c : cubes) if (c.velocity.x != 0.0f || c.velocity.y != 0.0f || c.velocity.z != 0.0f) hasMovingCubes = true;
	if (!BuildAccel(0.0f, 0.0f)) {
		// the reference would run out of memory long before (152-byte triangles + a heap node each); here the limit is the leaf
		// reference's 25-bit slot number.  The scene stays un-finalized: Raylib_Render refuses it with a log line.
		triangles.clear(); triangles.shrink_to_fit(); spheres.clear(); cubes.clear();
		finalized = false;
	}
}

// The flat BVH.  [t0, t1] is the shutter interval the boxes of moving cubes must cover.
// The reference always builds with t0 = t1 = 0 (geom/scene.cc:28) and tests a primitive's own box never, only its
// parent's union box -- so whether it still finds a cube that has moved out of its t = 0 box depends on which sibling
// its random build happened to pair it with.  Here a cube's box covers its whole motion over the camera's shutter
// (Cube::BoundingBox(t0, t1), geom/cube.cc:45-52), i.e. the cube is found wherever it really is.
bool Scene::BuildAccel(float t0, float t1)
{
	accelT0 = t0; accelT1 = t1;
	if (!BVHCapacityOk(triangles.size() + spheres.size() + cubes.size())) {
		Log("Raylib_FinalizeScene: %zu primitives exceed the %u this library's BVH can address; the scene was NOT finalized",
		    triangles.size() + spheres.size() + cubes.size(), (1u << 25) - 1u);
		return false;
	}
	std::vector<PrimRef> prims;
	prims.reserve(triangles.size() + spheres.size() + cubes.size());
	for (size_t i = 0; i < triangles.size(); ++i) {
		const HostTriangle& t = triangles[i];
		PrimRef p; p.mn = fmin3(fmin3(t.v0, t.v1), t.v2); p.mx = fmax3(fmax3(t.v0, t.v1), t.v2); p.kind = PRIM_TRIANGLE; p.index = (uint32_t)i;
		prims.push_back(p);
	}
	for (size_t i = 0; i < spheres.size(); ++i) {   // reference geom/sphere.cc:47-52
		const f3 R = F3(spheres[i].radius, spheres[i].radius, spheres[i].radius);
		PrimRef p; p.mn = spheres[i].center - R; p.mx = spheres[i].center + R; p.kind = PRIM_SPHERE; p.index = (uint32_t)i;
		prims.push_back(p);
	}
	for (size_t i = 0; i < cubes.size(); ++i) {
		const float d0 = t0 - cubes[i].timeStartMove, d1 = t1 - cubes[i].timeStartMove;
		const f3 m0 = cubes[i].velocity * (d0 > 0.0f ? d0 : 0.0f), m1 = cubes[i].velocity * (d1 > 0.0f ? d1 : 0.0f);
		PrimRef p;
		p.mn = fmin3(cubes[i].minBounds + m0, cubes[i].minBounds + m1);
		p.mx = fmax3(cubes[i].maxBounds + m0, cubes[i].maxBounds + m1);
		p.kind = PRIM_CUBE; p.index = (uint32_t)i;
		prims.push_back(p);
	}
	const auto tBuild = std::chrono::steady_clock::now();
	BVHBuildOptions bopt;
	{ const char* e = getenv("RAYLIB_WIDE_GREEDY"); bopt.wideGreedy = e && atoi(e) != 0; }   // read here, once per scene: rl_host.h BVHBuildOptions
	if (const char* e = getenv("RAYLIB_W8_SPLIT")) bopt.splitLeaves8 = atoi(e) != 0;
	if (const char* e = getenv("RAYLIB_W8_TRI_COST")) bopt.triCost8 = (float)atof(e);
	BuildBVH(prims, bvh, bopt);
	const double buildSec = std::chrono::duration<double>(std::chrono::steady_clock::now() - tBuild).count();
	// leaves that contain a triangle whose material has an albedo texture run the
	// cut-out test inside traversal (reference geom/triangle.cc:54, material.cc:397-404)
	std::vector<uint8_t> alpha(triangles.size(), 0);
	bool any = false;
	for (size_t i = 0; i < triangles.size(); ++i) {
		const HostMaterial& hm = materials[triangles[i].material];
		if (hm.type == MAT_MICROFACET && hm.tex[0] >= 0) { alpha[i] = 1; any = true; }
	}
	if (any) {
		auto patch = [&](int32_t& ref) {
			if (ref >= 0 || ref == DNODE_EMPTY) return;
			uint32_t code = (uint32_t)~ref, first = code >> LEAF_FIRST_SHIFT, count = (code & LEAF_COUNT_MASK) + 1;
			if (((code >> LEAF_KIND_SHIFT) & LEAF_KIND_MASK) != PRIM_TRIANGLE) return;
			for (uint32_t k = 0; k < count; ++k) if (alpha[bvh.triOrder[first + k]]) { code |= LEAF_ALPHA_BIT; break; }
			ref = ~(int32_t)code;
		};
		for (DNode& n : bvh.nodes) { patch(n.left); patch(n.right); }
		for (DNode4& n : bvh.nodes4) for (int k = 0; k < 4; ++k) patch(n.child[k]);
		for (DNode4Q& n : bvh.nodes4q) for (int k = 0; k < 4; ++k) patch(n.child[k]);
		for (DNode4& n : bvh.leafList) for (int k = 0; k < 4; ++k) patch(n.child[k]);
		for (DNode8& n : bvh.nodes8) {   // the 8-wide node names its leaf children's triangles through triBase + leafMask; the flag is a bit per child
			n.alphaMask = 0;
			for (int c = 0; c < 8; ++c) {
				const uint32_t nib = (n.leafMask >> (4 * c)) & 15u;
				if (!nib) continue;
				const uint32_t first = n.triBase + (uint32_t)__builtin_popcount(n.leafMask & ((1u << (4 * c)) - 1u)), count = (uint32_t)__builtin_popcount(nib);
				for (uint32_t k = 0; k < count; ++k) if (alpha[bvh.triOrder[first + k]]) { n.alphaMask |= 1u << c; break; }
			}
		}
	}
	Log("Scene finalized: %u triangles, %u BVH nodes, depth %u, SAH cost %.2f (BVH build %.2f s)",
	    (unsigned)triangles.size(), (unsigned)bvh.nodes.size(), bvh.depth, bvh.sahCost, buildSec);
	if (!bvh.nodes4.empty()) Log("\twide tree: %u BVH4 nodes, worst-case traversal stack %u entries", (unsigned)bvh.nodes4.size(), bvh.stackNeed4);
	if (!bvh.nodes8.empty()) Log("\t8-wide tree: %u nodes, %u levels; expected node steps of a random ray %.1f (4-wide tree: %.1f)", (unsigned)bvh.nodes8.size(), bvh.depth8, bvh.sahNodes8, bvh.sahNodes4);
	if (!bvh.leafList.empty()) {
		unsigned leaves = 0;
		for (const DNode4& nd : bvh.leafList) for (int k = 0; k < 4; ++k) if (nd.child[k] != DNODE_EMPTY) ++leaves;
		Log("\tleaf list: %u leaves in %u records (k_trace walks it instead of the tree)", leaves, (unsigned)bvh.leafList.size());
	}
	return true;
}

bool ScenePlain(const Scene& sc)
{
	for (const HostMaterial& m : sc.materials) for (int k = 0; k < 5; ++k) if (m.tex[k] >= 0) return false;
	for (const DNode4& n : sc.bvh.leafList) for (int k = 0; k < 4; ++k) {
		const int32_t ref = n.child[k];
		if (ref < 0 && ref != DNODE_EMPTY && (((uint32_t)~ref) & 8u) != 0u) return false;
	}
	return true;
}

// The scene half of the choice of k_trace's lazy-reflectance instance: a plain scene of triangles whose materials are all microfacet or mirrors (a material no
// triangle uses -- the OBJ loader's fallback -- does not count), with finite emission and with roughness, albedo and metallic inside the closed intervals for which
// a vertex that passes the kernel's guard has a finite reflectance (rl_dev_shade.h LazyVertexSafe: roughness 0 is outside -- GeometryBeckmann's
// a = rcp1_(-0) -- and every compare fails on NaN).  A mirror's reflectance is its albedo.
bool SceneLazyRefl(const Scene& sc)
{
	if (!ScenePlain(sc) || sc.triangles.empty() || !sc.spheres.empty() || !sc.cubes.empty()) return false;
	std::vector<char> used(sc.materials.size(), 0);
	for (const HostTriangle& t : sc.triangles) {
		if (t.material < 0 || (size_t)t.material >= sc.materials.size()) return false;
		used[(size_t)t.material] = 1;
	}
	for (size_t i = 0; i < sc.materials.size(); ++i) {
		if (!used[i]) continue;
		const HostMaterial& m = sc.materials[i];
		if (m.type == MAT_MIRROR) {
			for (int k = 0; k < 3; ++k) if (!(std::fabs(m.albedo[k]) <= RL_LAZY_COLOR_MAX)) return false;
			continue;
		}
		if (m.type != MAT_MICROFACET) return false;
		if (!(m.roughness >= RL_LAZY_ROUGHNESS_MIN && m.roughness <= RL_LAZY_ROUGHNESS_MAX) || !(std::fabs(m.metallic) <= RL_LAZY_COLOR_MAX)) return false;
		for (int k = 0; k < 3; ++k) if (!(std::fabs(m.albedo[k]) <= RL_LAZY_COLOR_MAX) || !std::isfinite(m.emissive[k])) return false;
	}
	return true;
}

// Image2D::PostProcess on the host (reference render/image.cc:44-103): max-luminance
// scan, extended Reinhard on luminance, clamp to white, gamma 1/2.2.
void PostProcessHost(Image& img)
{
	img.SyncHost();
	const size_t len = (size_t)img.width * img.height;
	float maxWhiteLuminance = 1.0f;
	for (size_t i = 0; i < len; ++i) {
		const float* p = &img.rgba[4 * i];
		float L = dot(F3(p[0], p[1], p[2]), F3(0.2126f, 0.7152f, 0.0722f));
		if (maxWhiteLuminance < L) maxWhiteLuminance = L;
	}
	Log("Max white luminance: %f", maxWhiteLuminance);
	for (size_t i = 0; i < len; ++i) {
		float* p = &img.rgba[4 * i];
		f3 rgb = F3(p[0], p[1], p[2]);
		float luminanceOld = dot(rgb, F3(0.2126f, 0.7152f, 0.0722f));
		if (luminanceOld <= 0.0001f) rgb = F3(0.0f, 0.0f, 0.0f);
		else {
			float numerator = luminanceOld * (1.0f + (luminanceOld / (maxWhiteLuminance * maxWhiteLuminance)));
			float luminanceNew = numerator / (1.0f + luminanceOld);
			rgb = rgb * (luminanceNew / luminanceOld);
		}
		rgb = fmin3(F3(1.0f, 1.0f, 1.0f), rgb);
		const float K = 1.0f / 2.2f;
		p[0] = powf(rgb.x, K); p[1] = powf(rgb.y, K); p[2] = powf(rgb.z, K);
	}
}

// Flatten the host scene into device records (leaf order): plain host code, no device involved (rl_rt_scene.hip UploadScene copies the result to every device in use).
FlatScene FlattenScene(const Scene& sc)
{
	FlatScene F;
	const size_t n = sc.triangles.size();
	F.isect.resize(n);
	std::vector<DTriIsect>& isect = F.isect;
	std::atomic<int> fastBary(1);
	if (const char* e = getenv("RAYLIB_FAST_BARY")) fastBary.store(atoi(e) != 0 ? 1 : 0);   // 0: the divisions, whatever the scene (parity tests compare the two)
	F.shade.resize(n);
	std::vector<DTriShade>& shade = F.shade;
	auto flatten = [&](size_t k0, size_t k1) { for (size_t k = k0; k < k1; ++k) {
		const HostTriangle& t = sc.triangles[sc.bvh.triOrder[k]];
		DTriIsect& I = isect[k];
		const f3 nrm = normalize(cross(t.v1 - t.v0, t.v2 - t.v0));   // geom/triangle.h:34-38
		const f3 u = t.v1 - t.v0, v = t.v2 - t.v0;                   // geom/triangle.cc:30-31
		const float uv = dot(u, v), uu = dot(u, u), vv = dot(v, v);  // :34-38
		const float uvuv = uv * uv, uuvv = uu * vv;                  // :39-40
		I.v0[0] = t.v0.x; I.v0[1] = t.v0.y; I.v0[2] = t.v0.z;
		I.n[0] = nrm.x; I.n[1] = nrm.y; I.n[2] = nrm.z;
		I.v1[0] = t.v1.x; I.v1[1] = t.v1.y; I.v1[2] = t.v1.z;
		I.v2[0] = t.v2.x; I.v2[1] = t.v2.y; I.v2[2] = t.v2.z;
		I.uv = uv; I.uu = uu; I.vv = vv;
		{   // the reciprocal of denom = uvuv - uuvv for the short barycentric divisions (rl_dev_walk.h Barycentric, which states the conditions)
			const float denom = uvuv - uuvv, mag = fabsf(denom);
			if (denom == 0.0f || denom != denom) I.rden = std::numeric_limits<float>::quiet_NaN();
			else if (mag >= 0x1p-62f && mag <= 0x1p125f) I.rden = 1.0f / denom;
			else { I.rden = std::numeric_limits<float>::quiet_NaN(); fastBary.store(0, std::memory_order_relaxed); }
		}
		DTriShade& Sh = shade[k];
		Sh.n0[0] = t.n0.x; Sh.n0[1] = t.n0.y; Sh.n0[2] = t.n0.z;
		Sh.n1[0] = t.n1.x; Sh.n1[1] = t.n1.y; Sh.n1[2] = t.n1.z;
		Sh.n2[0] = t.n2.x; Sh.n2[1] = t.n2.y; Sh.n2[2] = t.n2.z;
		Sh.s0 = t.s0; Sh.t0 = t.t0; Sh.s1 = t.s1; Sh.t1 = t.t1; Sh.s2 = t.s2; Sh.t2 = t.t2;
		Sh.material = t.material;
	} };
	{   // per-triangle records are independent: all host threads for large scenes (10 M triangles: 0.6 s on one thread)
		unsigned threads = n >= (1u << 17) ? std::min(32u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
		if (const char* e = getenv("RAYLIB_BUILD_THREADS")) { int v = atoi(e); if (v > 0 && n >= (1u << 17)) threads = (unsigned)std::min(v, 32); }
		std::vector<std::thread> pool;
		const size_t per = (n + threads - 1) / threads;
		for (unsigned t = 1; t < threads; ++t) { const size_t k0 = std::min(n, t * per), k1 = std::min(n, (t + 1) * per); if (k0 < k1) pool.emplace_back(flatten, k0, k1); }
		flatten(0, std::min(n, per));
		for (std::thread& th : pool) th.join();
	}
	F.fastBary = fastBary.load();
	std::vector<DMaterial>& mats = F.materials;
	mats.resize(sc.materials.size());
	for (size_t i = 0; i < mats.size(); ++i) {
		const HostMaterial& h = sc.materials[i];
		DMaterial& m = mats[i]; memset(&m, 0, sizeof(m));
		m.type = h.type;
		memcpy(m.albedo, h.albedo, 12); m.roughness = h.roughness; m.metallic = h.metallic;
		memcpy(m.emissive, h.emissive, 12); m.ior = h.ior; memcpy(m.transmission, h.transmission, 12);
		m.fuzziness = h.fuzziness; memcpy(m.tex, h.tex, 20);
	}
	std::vector<DTexture>& texs = F.textures;
	texs.resize(sc.textures.size());
	std::vector<float>& pool = F.texels;
	for (size_t i = 0; i < texs.size(); ++i) {
		const Image& im = *sc.textures[i];
		texs[i].offset = (uint32_t)(pool.size() / 4); texs[i].width = (int32_t)im.width; texs[i].height = (int32_t)im.height; texs[i].pad = 0;
		// (a rendered image used as a texture has been fetched from the device by the caller: rl_rt_scene.hip UploadScene)
		pool.insert(pool.end(), im.rgba.begin(), im.rgba.end());
	}
	// Albedo maps are read through Texture2D::Sample(bSRGB = true): nearest texel, then pow(texel, 2.2) on all four channels
	// (reference render/texture.cc:44-50, material.cc:383,400) -- four powf per shading event and per alpha-tested candidate.
	// The power of a texel does not depend on the ray: every texture some material uses as albedo gets a converted copy here
	// (host powf = the reference's own function, the one csrc/rl_glibc_math.h restates), and the material points at the copy.
	{
		std::vector<int32_t> converted(texs.size(), -1);
		for (DMaterial& m : mats) {
			if (m.type != MAT_MICROFACET || m.tex[0] < 0 || (size_t)m.tex[0] >= converted.size()) continue;
			const size_t src = (size_t)m.tex[0];
			if (converted[src] < 0) {
				DTexture t = texs[src];
				const size_t count = (size_t)t.width * t.height * 4, from = (size_t)t.offset * 4;
				t.offset = (uint32_t)(pool.size() / 4);
				pool.resize(pool.size() + count);
				float* dst = pool.data() + (size_t)t.offset * 4; const float* in = pool.data() + from;
				unsigned threads = count >= (1u << 20) ? std::min(32u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
				std::vector<std::thread> workers;
				const size_t per = (count + threads - 1) / threads;
				auto run = [dst, in](size_t a, size_t b) { for (size_t i = a; i < b; ++i) dst[i] = powf(in[i], 2.2f); };
				for (unsigned w = 1; w < threads; ++w) { const size_t a = std::min(count, w * per), b = std::min(count, (w + 1) * per); if (a < b) workers.emplace_back(run, a, b); }
				run(0, std::min(count, per));
				for (std::thread& th : workers) th.join();
				converted[src] = (int32_t)texs.size();
				texs.push_back(t);
			}
			m.tex[0] = converted[src];
		}
	}
	// The cut-out test of a candidate (geom/triangle.cc:54 -> MicrofacetMaterial::AlphaTest) needs one texel of the triangle's material's albedo map: as a table per
	// triangle slot the texture is known from the triangle alone, and the test's chain of dependent loads inside the walk is triangle -> texture -> texel instead
	// of triangle -> material -> texture -> texel (round 5).
	std::vector<int32_t>& alphaTex = F.alphaTex;
	{
		bool any = false;
		for (const DMaterial& m : mats) if (m.type == MAT_MICROFACET && m.tex[0] >= 0) any = true;
		if (any) {
			alphaTex.resize(n);
			for (size_t k = 0; k < n; ++k) {
				const int32_t mi = shade[k].material;
				alphaTex[k] = (mi >= 0 && (size_t)mi < mats.size() && mats[(size_t)mi].type == MAT_MICROFACET && mats[(size_t)mi].tex[0] >= 0) ? mats[(size_t)mi].tex[0] : -1;
			}
		}
	}
	std::vector<DSphere>& dsph = F.spheres;
	dsph.resize(sc.spheres.size());
	for (size_t i = 0; i < dsph.size(); ++i) {
		memset(&dsph[i], 0, sizeof(DSphere));
		dsph[i].center[0] = sc.spheres[i].center.x; dsph[i].center[1] = sc.spheres[i].center.y; dsph[i].center[2] = sc.spheres[i].center.z;
		dsph[i].radius = sc.spheres[i].radius; dsph[i].material = sc.spheres[i].material;
	}
	std::vector<DCube>& dcub = F.cubes;
	dcub.resize(sc.cubes.size());
	for (size_t i = 0; i < dcub.size(); ++i) {
		memset(&dcub[i], 0, sizeof(DCube));
		const HostCube& h = sc.cubes[i];
		dcub[i].minBounds[0] = h.minBounds.x; dcub[i].minBounds[1] = h.minBounds.y; dcub[i].minBounds[2] = h.minBounds.z; dcub[i].timeStartMove = h.timeStartMove;
		dcub[i].maxBounds[0] = h.maxBounds.x; dcub[i].maxBounds[1] = h.maxBounds.y; dcub[i].maxBounds[2] = h.maxBounds.z; dcub[i].material = h.material;
		dcub[i].velocity[0] = h.velocity.x; dcub[i].velocity[1] = h.velocity.y; dcub[i].velocity[2] = h.velocity.z;
	}
	{   // Rotator(yaw = 90).rotate rows, reference geom/transform.cc:47-65 (host libm, as the reference)
		const float pi_f = (float)3.1415926535897932385;
		const float ry = 90.0f * pi_f / 180.0f, rp = 0.0f * pi_f / 180.0f, rr = 0.0f * pi_f / 180.0f;
		const float ch = cosf(ry), sh = sinf(ry), cp = cosf(rp), sp = sinf(rp), cb = cosf(rr), sb = sinf(rr);
		F.skyRot.m0[0] = ch * cb + sh * sp * sb; F.skyRot.m0[1] = sb * cp; F.skyRot.m0[2] = -sh * cb + ch * sp * sb;
		F.skyRot.m1[0] = -ch * sb + sh * sp * cb; F.skyRot.m1[1] = cb * cp; F.skyRot.m1[2] = sb * sh + ch * sp * cb;
		F.skyRot.m2[0] = sh * cp; F.skyRot.m2[1] = -sp; F.skyRot.m2[2] = ch * cp;
	}
	return F;
}

} // namespace rl
