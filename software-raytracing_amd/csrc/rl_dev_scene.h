// Device library, part 2 of 6: the scene's records in registers and in LDS -- textures, materials, the LDS layouts, triangle and shading records,
// the cut-out test of a candidate.
#pragma once

#include "rl_dev_core.h"

namespace rl {

// ---------------------------------------------------------------------------
// Texture2D::Sample (reference render/texture.cc:30-53, render/image.h:79-83)
// Out of line (textured scenes only) and fed plain pointers, so that no caller-side struct has its
// address taken (that would push it to scratch).
__device__ __noinline__ float4 TexFetch(const DTexture* textures, const float* texels, int tex, bool srgb, float u, float v)
{
	const DTexture T = textures[tex];
	u = rtm::fmod1_(u); if (u < 0.0f) u += 1.0f;
	v = rtm::fmod1_(v); if (v < 0.0f) v += 1.0f; v = 1.0f - v;
	if (isnan(u) || isinf(u)) u = 0.0f;
	if (isnan(v) || isinf(v)) v = 0.0f;
	int x = (int)((float)(uint32_t)(T.width - 1) * u);
	int y = (int)((float)(uint32_t)(T.height - 1) * v);
	float4 px = ((const float4*)texels)[T.offset + (uint32_t)(y * T.width + x)];
	if (srgb) { px.x = rtm::pow_(px.x, 2.2f); px.y = rtm::pow_(px.y, 2.2f); px.z = rtm::pow_(px.z, 2.2f); px.w = rtm::pow_(px.w, 2.2f); }
	return px;
}
// The texture descriptors (first texel, width, height) of a scene with at most RL_LDS_TEXTURES textures are copied to LDS at the top of the pool kernel
// (RL_TEX_PROLOGUE): a fetch is then descriptor (LDS) -> texel instead of two dependent trips through the vector memory pipeline.  TexFetch takes a generic
// pointer and loads through it with a flat instruction, which serves either address space.  RL_LDS_TEXTURE_TABLE is a translation unit's setting, made before
// its includes, and only the pool schedule's unit (rl_render_pool.hip) sets it: k_trace renders the
// scenes of a few hundred triangles, where a texel fetch is rare, and the Cornell frame was 0.6 % slower with the table in its kernel (12.36 against 12.28 ms).
#ifndef RL_LDS_TEXTURE_TABLE
#define RL_LDS_TEXTURE_TABLE 0
#endif
#if RL_LDS_TEXTURE_TABLE
__shared__ DTexture rl_lds_tex[RL_LDS_TEXTURES];
#define RL_TEX_PROLOGUE(S_) { if ((S_).numTextures <= RL_LDS_TEXTURES) for (int i_ = (int)threadIdx.x; i_ < (S_).numTextures; i_ += (int)blockDim.x) rl_lds_tex[i_] = (S_).textures[i_]; }
__device__ __forceinline__ const DTexture* TexTable(const DSceneView& S) { return (S.numTextures <= RL_LDS_TEXTURES) ? (const DTexture*)rl_lds_tex : S.textures; }
#else
#define RL_TEX_PROLOGUE(S_)
__device__ __forceinline__ const DTexture* TexTable(const DSceneView& S) { return S.textures; }
#endif
__device__ __forceinline__ float4 TexSample(const DSceneView& S, int tex, bool srgb, float u, float v, Counters& c)
{
	c.texels++;
	return TexFetch(TexTable(S), S.texels, tex, srgb, u, v);
}

struct Mat {   // DMaterial in registers
	int type;
	V3 albedo; float roughness, metallic; V3 emissive; float ior; V3 transmission; float fuzz;
	int tex0, tex1, tex2, tex3, tex4;
};
__device__ __forceinline__ Mat LoadMat(const DSceneView& S, int i)
{
	const float4* p = (const float4*)(S.materials + i);
	float4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
	Mat m;
	m.type = __float_as_int(a.x); m.albedo = v3(a.y, a.z, a.w);
	m.roughness = b.x; m.metallic = b.y; m.emissive = v3(b.z, b.w, c.x);
	m.ior = c.y; m.transmission = v3(c.z, c.w, d.x); m.fuzz = d.y;
	m.tex0 = __float_as_int(d.z); m.tex1 = __float_as_int(d.w);
	m.tex2 = __float_as_int(e.x); m.tex3 = __float_as_int(e.y); m.tex4 = __float_as_int(e.z);
	return m;
}

// ---------------------------------------------------------------------------
// A scene small enough lives in LDS for the duration of a k_trace workgroup (<= 32 wide nodes, <= 128 triangles, <= 32 materials:
// the Cornell class): the BVH2 root, the float-box wide nodes, both triangle record arrays and the material table, 23 KB at fixed
// offsets (float4 units) so that every access is a ds_read_b128 with an immediate offset.  Every dependent fetch of a bounce --
// three to six node steps, the triangle records, the shading record, the material -- then costs an LDS round trip instead of a trip
// through the vector memory pipeline (TA / L1 / L2), which sixteen waves per CU keep busy with 64-address gathers.
#define RL_LDS_ROOT   0
#define RL_LDS_NODES  4
#ifndef RL_LDS_NSTRIDE
#define RL_LDS_NSTRIDE 8   /* float4 per node record (8 = packed) */
#define RL_LDS_TSTRIDE 4   /* float4 per triangle record, both arrays */
#endif
#define RL_LDS_ISECT  (RL_LDS_NODES + RL_LDS_MAXNODES * RL_LDS_NSTRIDE)
#define RL_LDS_SHADE  (RL_LDS_ISECT + RL_LDS_MAXTRIS * RL_LDS_TSTRIDE)
#define RL_LDS_MATS   (RL_LDS_SHADE + RL_LDS_MAXTRIS * RL_LDS_TSTRIDE)
#define RL_LDS_TOTAL  (RL_LDS_MATS + RL_LDS_MAXMATS * 5)
// The leaf-list kernel (LDS == 2) has its own layout: six records of leaf boxes instead of a tree, at most 108 triangles, and an intersection
// record of SIX float4 that holds what the triangle test would otherwise recompute per test -- the edges u = v1 - v0, v = v2 - v0 (triangle.cc:30-31)
// and the triangle's own box (the candidate rule's) -- computed once per workgroup when the scene is copied in, with the same operations.
template <int LDS> struct LdsAt {
	static constexpr int NODES = RL_LDS_NODES;
	static constexpr int MAXNODES = LDS == 2 ? RL_LEAFLIST_RECORDS : RL_LDS_MAXNODES;
	static constexpr int TRI = LDS == 2 ? 6 : RL_LDS_TSTRIDE;                 // float4 per intersection record
	static constexpr int MAXTRIS = LDS == 2 ? RL_LEAFLIST_MAXTRIS : RL_LDS_MAXTRIS;
	static constexpr int ISECT = NODES + MAXNODES * RL_LDS_NSTRIDE;
	static constexpr int SHADE = ISECT + MAXTRIS * TRI;
	static constexpr int MATS = SHADE + MAXTRIS * RL_LDS_TSTRIDE;
	static constexpr int TOTAL = MATS + RL_LDS_MAXMATS * 5;
};

// PLAIN (k_trace's instance for scenes without a texture slot, rl_plan.cc): the record in LDS is the first four float4 of the
// material (RL_LDS_MSTRIDE), and every texture slot is the constant -1 -- what each slot of such a scene holds, or another negative number, which every
// reader takes the same way (tex >= 0 is "textured") -- so that the texture branches of the shading code fold away with their calls.
#define RL_LDS_MSTRIDE(plain) ((plain) ? 4 : 5)
template <bool PLAIN = false>
__device__ __forceinline__ Mat MatFrom(const float4* p)
{
	float4 a = p[0], b = p[1], c = p[2], d = p[3], e = PLAIN ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : p[4];
	Mat m;
	m.type = __float_as_int(a.x); m.albedo = v3(a.y, a.z, a.w);
	m.roughness = b.x; m.metallic = b.y; m.emissive = v3(b.z, b.w, c.x);
	m.ior = c.y; m.transmission = v3(c.z, c.w, d.x); m.fuzz = d.y;
	m.tex0 = __float_as_int(d.z); m.tex1 = __float_as_int(d.w);
	m.tex2 = __float_as_int(e.x); m.tex3 = __float_as_int(e.y); m.tex4 = __float_as_int(e.z);
	if (PLAIN) m.tex0 = m.tex1 = m.tex2 = m.tex3 = m.tex4 = -1;
	return m;
}

// ---------------------------------------------------------------------------
// Closest hit on the flat BVH2.
struct HitRec { float t, a, b; int tri; };   // tri: triangle slot, or (kind << 28) | index for sphere (1) / cube (2, with the face in a)

struct Tri { V3 v0, n, v1, v2, u, v; float uv, uu, vv, denom, rden; };
__device__ __forceinline__ Tri TriFrom(const float4* p)
{
	float4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
	Tri t;
	t.v0 = v3(q0.x, q0.y, q0.z); t.n = v3(q0.w, q1.x, q1.y);
	t.v1 = v3(q1.z, q1.w, q2.x); t.v2 = v3(q2.y, q2.z, q2.w);
	t.u = t.v1 - t.v0; t.v = t.v2 - t.v0;   // geom/triangle.cc:30-31
	t.uv = q3.x; t.uu = q3.y; t.vv = q3.z; t.rden = q3.w;
	t.denom = t.uv * t.uv - t.uu * t.vv;    // geom/triangle.cc:39-41, the host's own three operations (rl_scene.cc FlattenScene): the record's slot holds 1 / denom
	return t;
}
__device__ __forceinline__ Tri LoadTri(const DSceneView& S, int i) { return TriFrom((const float4*)(S.isect + i)); }

struct Shade { V3 n0, n1, n2; float s0, t0, s1, t1, s2, t2; int material; };
__device__ __forceinline__ Shade ShadeFrom(const float4* p)
{
	float4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
	Shade s;
	s.n0 = v3(q0.x, q0.y, q0.z); s.n1 = v3(q0.w, q1.x, q1.y); s.n2 = v3(q1.z, q1.w, q2.x);
	s.s0 = q2.y; s.t0 = q2.z; s.s1 = q2.w; s.t1 = q3.x; s.s2 = q3.y; s.t2 = q3.z;
	s.material = __float_as_int(q3.w);
	return s;
}
__device__ __forceinline__ Shade LoadShade(const DSceneView& S, int i) { return ShadeFrom((const float4*)(S.shade + i)); }

// MicrofacetMaterial::AlphaTest for a candidate (reference render/material.cc:397-404 via geom/triangle.cc:48-54).
// Returns bit 0 = passes, bit 1 = a texel was fetched.  Out of line: only leaves flagged as textured reach it.  (RL_ALPHA_TEST_ATTR: a unit whose kernels are to
// keep no call frame -- rl_sdf.hip -- takes it inline; the statements are the same.)
#ifndef RL_ALPHA_TEST_ATTR
#define RL_ALPHA_TEST_ATTR __noinline__
#endif
__device__ RL_ALPHA_TEST_ATTR int AlphaTestCandidateNI(const DTriShade* shade, const int32_t* alphaTex, const DMaterial* materials, const DTexture* textures,
                                                 const float* texels, int tri, float a, float b)
{
	const float4* p = (const float4*)(shade + tri);
	// the texture comes from the per-triangle table (rl_scene.cc FlattenScene), fetched beside the triangle's UVs: one dependent load fewer than through the material
	int tex = alphaTex ? alphaTex[tri] : 0;
	const float4 q2 = p[2], q3 = p[3];
	const float s0 = q2.y, t0 = q2.z, s1 = q2.w, t1 = q3.x, s2 = q3.y, t2 = q3.z;
	if (!alphaTex) {
		const DMaterial* M = materials + __float_as_int(q3.w);
		tex = (M->type == MAT_MICROFACET) ? M->tex[0] : -1;
	}
	if (tex < 0) return 1;
	float U = (1 - a - b) * s0 + a * s1 + b * s2;
	float V = (1 - a - b) * t0 + a * t1 + b * t2;
	float4 px = TexFetch(textures, texels, tex, false, U, V);   // the pow(2.2) copy made at upload
	return (px.w >= 0.5f ? 1 : 0) | 2;
}
__device__ __forceinline__ bool AlphaTestCandidate(const DSceneView& S, int tri, float a, float b, Counters& c)
{
	const int r = AlphaTestCandidateNI(S.shade, S.alphaTex, S.materials, TexTable(S), S.texels, tri, a, b);
	c.shaded++;
	if (r & 2) c.texels++;
	return (r & 1) != 0;
}

} // namespace rl
