/*
 * TEST INFRASTRUCTURE -- C API of the CPU oracle (oracle/oracle.cc).
 * Same entry points as oracle/ref_glue.cc (prefix oracle_ instead of ref_) so
 * that tests can run one set of inputs through both and compare bit for bit.
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may use it.
 */
#ifndef ORACLE_H
#define ORACLE_H

#include "flat_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OracleCounters {
	uint64_t rays;          /* closest-hit / occlusion queries (reference renderer.cc:129,194,70,79) */
	uint64_t nodesVisited;  /* BVHNode::Hit calls whose box test ran (reference bvh.cc:82-84) */
	uint64_t trisTested;    /* Triangle::Hit calls (reference triangle.cc:18) */
	uint64_t cameraSamples;
	uint64_t closestHitTies; /* BVH nodes where both subtrees returned a hit at exactly the same t (answer depends on the tree shape) */
	uint64_t hitsOutsideOwnBox; /* triangle hits accepted although the ray fails the box test of the triangle's own AABB (reachability depends on the tree) */
} OracleCounters;

/* One ray's answer from oracle_interval_hits.  prims: RaylibAMD_SceneExportTriangles indices (the flat order of FlatSceneDesc), or
 * RAYLIB_AMD_PRIM_SPHERE|k (0x10000000) / RAYLIB_AMD_PRIM_CUBE|k (0x20000000); -1 where unused. */
typedef struct OracleIntervalHit {
	float   t;               /* the least accepted t; +inf when nothing is accepted */
	int32_t count;           /* primitives accepted at exactly that t */
	int32_t prims[8];        /* the first eight of them */
	int32_t nearerRejected;  /* triangles TriangleHit accepts at a smaller t but the device's candidate rule rejects (information only) */
} OracleIntervalHit;

/* buildSeed != 0: the reference's BVH construction (random axis per node, drawn from the stream keyed by buildSeed);
 * buildSeed == 0: a median-split tree built in n log n -- for multi-million-triangle scenes' windows (see BuildBVHFast). */
void*   oracle_scene_create(const FlatSceneDesc* desc, uint64_t buildSeed);
void    oracle_scene_destroy(void* scene);
void    oracle_render(void* scene, const FlatCamera* cam, const FlatSettings* st, uint64_t seed,
                      int32_t numThreads, float* outRGBA, float* outSamples);
void    oracle_render_region(void* scene, const FlatCamera* cam, const FlatSettings* st, uint64_t seed,
                             int32_t numThreads, int32_t x0, int32_t y0, int32_t rw, int32_t rh,
                             float* outRGBA, float* outSamples);
void    oracle_get_counters(void* scene, OracleCounters* out);   /* counters of the last oracle_render */
void    oracle_closest_hit(void* scene, const float* rays, int32_t n, float tMin, FlatHit* out);
/* Oracle-only: every primitive against each ray's own [tMin, tMax], no tree and no box culling.  rays8: n x (org, tMin, dir, tMax).
 * A triangle counts when TriangleHit accepts it and the device's candidate rule passes; a sphere by SphereHit; a cube by CubeHit at rayTime. */
void    oracle_interval_hits(void* scene, const float* rays8, int32_t n, float rayTime, int32_t threads, OracleIntervalHit* out);
void    oracle_aabb_hit(const float* boxes, const float* rays, int32_t n, float tMin, float tMax, int32_t* out);
void    oracle_triangle_hit(const FlatTriangle* tris, const float* rays, int32_t n, float tMin, float tMax, FlatHit* out);
void    oracle_onb(const float* normals, const float* vecs, int32_t n, float* outLocal, float* outWorld);
void    oracle_camera_rays(const FlatCamera* cam, const float* uv, int32_t n, uint64_t seed, float* out);
void    oracle_scatter(void* scene, int32_t material, const float* in, int32_t n, uint64_t seed, float* out);
void    oracle_texture_sample(const FlatTexture* t, int32_t bSRGB, const float* uv, int32_t n, float* out);
void    oracle_bvh_stats(void* scene, int64_t* outNodes, int32_t* outDepth);
/* MTL -> material mapping (reference loader/obj_loader.cc:354-397).  Inputs are the
 * tinyobjloader material_t fields the reference reads. */
void    oracle_material_from_mtl(const float Kd[3], const float Ks[3], const float Ke[3], const float Tf[3],
                                 float Ns, float Ni, int32_t illum, float Pr, float Pm,
                                 int32_t hasMapKd, FlatMaterial* out);
/* Image2D::PostProcess (reference render/image.cc:44-103), in place on n RGBA pixels. */
void    oracle_postprocess(float* rgba, int64_t numPixels);
/* Test-scene utility: OBJ text of a triangle list in the format of raylib_amd/scenes.py, written by `threads` host threads. */
int32_t oracle_write_obj(const char* path, const char* mtlName, int64_t numTris, const float* tri, const float* uv, const float* normal,
                         const int32_t* owner, const char* const* objectNames, const char* const* objectMaterials, int32_t threads);

#ifdef __cplusplus
}
#endif
#endif
