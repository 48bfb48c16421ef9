// Host-side object model of the MI355X raylib (everything behind the C-ABI that is
// not a kernel): OBJ models, images, cameras, scenes, and the flattening step
// that turns them into the device layout of rl_device.h.
#pragma once

#include "raylib_types.h"
#include "raylib_amd.h"
#include "rl_device.h"

#include <math.h>
#include <stdint.h>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace rl {

// ---------------------------------------------------------------------------
// float3 with the arithmetic conventions the reference's results depend on
// (reference core/vec3.h): normalize multiplies by 1/length, dot sums left to
// right, cross negates the middle term.  Host code is compiled with
// -ffp-contract=off so that these produce the same bits as the reference build.
struct f3 { float x, y, z; };
inline f3 F3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
inline f3 operator+(f3 a, f3 b) { return F3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline f3 operator-(f3 a, f3 b) { return F3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline f3 operator*(f3 a, f3 b) { return F3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline f3 operator*(f3 a, float t) { return F3(a.x * t, a.y * t, a.z * t); }
inline f3 operator*(float t, f3 a) { return F3(a.x * t, a.y * t, a.z * t); }
inline f3 operator-(f3 a) { return F3(-a.x, -a.y, -a.z); }
inline float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline f3 cross(f3 a, f3 b) { return F3(a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x); }
inline float length(f3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
inline f3 normalize(f3 a) { float k = 1.0f / length(a); return F3(a.x * k, a.y * k, a.z * k); }
// std::min / std::max selection order (reference core/vec3.h:151-162): min(a,b) = (b < a) ? b : a
inline f3 fmin3(f3 a, f3 b) { return F3(b.x < a.x ? b.x : a.x, b.y < a.y ? b.y : a.y, b.z < a.z ? b.z : a.z); }
inline f3 fmax3(f3 a, f3 b) { return F3(a.x < b.x ? b.x : a.x, a.y < b.y ? b.y : a.y, a.z < b.z ? b.z : a.z); }

// ---------------------------------------------------------------------------
// 26-word triangle / 19-word material records: the host-side truth, identical in
// layout to what RaylibAMD_SceneExport* hand out.
struct HostTriangle {
	f3 v0, v1, v2;
	f3 n0, n1, n2;
	float s0, t0, s1, t1, s2, t2;
	int32_t material;
	int32_t shape;
};
static_assert(sizeof(HostTriangle) == 104, "HostTriangle layout");

enum MaterialType { MAT_LAMBERTIAN = 0, MAT_MIRROR = 1, MAT_DIELECTRIC = 2, MAT_MICROFACET = 3, MAT_METAL = 4, MAT_DIFFUSE_LIGHT = 5 };

struct HostMaterial {
	int32_t type;
	float albedo[3];
	float roughness, metallic;
	float emissive[3];
	float ior;
	float transmission[3];
	float fuzziness;
	int32_t tex[5];   // albedo, normal, roughness, metallic, emissive; -1 = none
};
static_assert(sizeof(HostMaterial) == 76, "HostMaterial layout");

uint64_t NextImageVersion();   // rl_image_io.cc: 1, 2, 3, ... over all images of the process
struct Image {
	uint32_t width = 0, height = 0;
	std::vector<float> rgba;          // 4 floats per pixel, row 0 = top
	// device-resident copy (float4 per pixel): written by Raylib_Render, consumed by Raylib_PostProcess
	void* devPixels = nullptr;
	size_t devBytes = 0;
	bool devValid = false;
	// Raylib_Render / Raylib_PostProcess leave the result on the device and mark the host pixels stale; whoever reads `rgba`
	// on the host calls SyncHost() first (one read-back when the pixels are asked for, none per render)
	bool hostStale = false;
	// bumped whenever the pixels change (reallocation, a render into the image, PostProcess): a scene that uses the image as its
	// sky panorama re-reads it at the next render, as the reference does through the handle (renderer.cc:159-176)
	// The value is unique in the PROCESS, not per image (NextImageVersion): a new image that malloc puts at a destroyed image's address
	// can never look like that image to a cache keyed on (pointer, version) -- the device copy of the sky, rl_rt_scene.hip SyncSky.
	uint64_t version = NextImageVersion();
	void Touch() { version = NextImageVersion(); }
	void SyncHost() const;
	Image() = default;
	Image(const Image& o) : width(o.width), height(o.height) { o.SyncHost(); rgba = o.rgba; }
	Image& operator=(const Image& o) { o.SyncHost(); width = o.width; height = o.height; rgba = o.rgba; devValid = false; hostStale = false; Touch(); return *this; }
	~Image();
	void Reallocate(uint32_t w, uint32_t h, float r, float g, float b, float a);
};

struct OBJModel {
	std::vector<HostTriangle> triangles;
	std::vector<HostMaterial> materials;           // MTL order, then the fallback Lambertian(0.5)
	std::vector<std::string> materialNames;
	std::vector<std::shared_ptr<Image>> images;    // textures referenced by materials[].tex
	int32_t numShapes = 0;
	bool finalized = false;
};

struct Camera {
	// settable state (reference render/camera.h:80-93)
	f3 origin = F3(0, 0, 0), lookAt = F3(0, 0, -1);
	float fovY_degrees = 60.0f, aspectWH = 16.0f / 9.0f;
	float aperture = 0.0f, focalDistance = 1.0f;
	float beginTime = 0.0f, endTime = 0.0f;
	// derived (reference render/camera.h:55-78)
	float lensRadius, timePeriod;
	f3 top_left, horizontal, vertical, u, v, w;
	void UpdateInternal();
	DCamera ToDevice() const;
};

struct BVH {
	std::vector<DNode> nodes;
	std::vector<DNode4> nodes4;       // the same tree collapsed to <= 4 children per node (empty for small scenes / analytic primitives)
	std::vector<DNode4Q> nodes4q;     // nodes4 on the 8-bit grid (same indices, same children): what the kernels walk by default
	uint32_t stackNeed4 = 0;          // worst-case traversal-stack entries of nodes4 (sum of children - 1 along the deepest path)
	std::vector<DNode8> nodes8;       // the 8-wide tree (DNode8, rl_device.h); its leaves are the BVH2's leaves, and the order of the triangle slots is ITS order (a node's leaf children hold consecutive slots)
	uint32_t depth8 = 0;              // levels of nodes8: a traversal's stack holds at most one entry (the rest of a node's hit children) per level
	float sahNodes4 = 0.0f, sahNodes8 = 0.0f;   // sum over the wide tree's nodes of (node's surface area / root's): the expected node steps of a random ray through either tree
	std::vector<DNode4> leafList;     // scenes of <= 4 * RL_LEAFLIST_RECORDS leaves: every leaf's box, four to a record, no inner nodes (k_trace's flat walk; empty otherwise)
	std::vector<uint32_t> triOrder;   // leaf order -> index into the flat triangle array
	// per child of every nodes4 (4), nodes8 (8) and leafList (4) record: the box of `nodes` it was emitted from, 2 * node + (0 left, 1 right); -1: unused
	// (rl_grid.h BoxOfId).  What a refit re-derives the wide formats from after the scene's triangles have moved.
	std::vector<int32_t> boxOf4, boxOf8, boxOfLeafList;
	uint32_t depth = 0;
	float sahCost = 0.0f;
};
// Binned-SAH BVH2 over primitive bounds.  A leaf holds <= 4 triangles or one analytic primitive.
enum PrimKind { PRIM_TRIANGLE = 0, PRIM_SPHERE = 1, PRIM_CUBE = 2 };
struct PrimRef { f3 mn, mx; uint8_t kind; uint32_t index; };
// wideGreedy: collapse the 8-wide tree by opening the largest child first instead of the plan that minimises the summed node area (an A/B switch: the scene reads
// RAYLIB_WIDE_GREEDY once, when it is finalized).  The 8-wide collapse decides the ORDER OF THE TRIANGLE SLOTS, and with it which of two surfaces at exactly the
// same distance wins (the lower slot: DESIGN.md section 4) -- frames of the two settings may differ in such tie pixels.
// splitLeaves8: give every leaf of a scene whose rays are expected to take >= minSteps8 node steps on the 4-wide tree (the scenes that walk the 8-wide tree by
// default) a split of its triangles for the 8-wide plan to open in otherwise empty slots (rl_bvh.cc SplitLeaves); triCost8: what an expected triangle test
// weighs against an expected node step in that plan.
// (Round 5, measured: triangle tests per ray 2.26 -> 1.96 ... 2.03 on the 298 k room whatever triCost8 between 0.25 and 2, no frame gets shorter -- the triangle steps
//  are a twelfth of the walk --, and the binary and 4-wide trees, emitted from the same nodes, gain a level or two: off unless RAYLIB_W8_SPLIT=1 asks for it.)
struct BVHBuildOptions { bool wideGreedy = false; bool splitLeaves8 = false; float triCost8 = 0.5f; float minSteps8 = RL_BVH8_MIN_STEPS; };
void BuildBVH(const std::vector<PrimRef>& prims, BVH& out, const BVHBuildOptions& opt = BVHBuildOptions());
bool BVHCapacityOk(size_t numPrimitives);   // a leaf reference addresses 2^25 primitive slots
void RefitWideFromBinary(BVH& bvh);         // nodes' boxes were refitted: nodes4, nodes4q, nodes8 and leafList from them, and sahCost
bool ValidateBVH(const BVH& bvh, const std::vector<HostTriangle>& tris);
bool ValidateBVH4(const BVH& bvh, const std::vector<HostTriangle>& tris);
bool ValidateBVH8(const BVH& bvh, const std::vector<HostTriangle>& tris);   // true also when the scene has no 8-wide tree
// the megakernel's 8-wide walk restated on the host (box arithmetic, visiting order, groups): least distance among the triangles of the leaf children it reaches
bool Walk8Host(const BVH& bvh, const std::vector<HostTriangle>& tris, const float* rays, int n, float tMin, const float* tMax, float* outT, uint32_t* outSteps);

// Scene elements created through include/raylib_amd.h (the reference's procedural scenes `new` C++ objects in the
// application instead: src/main.cc:913-984).  A material is owned by the library and shared by reference.
struct MaterialObj { HostMaterial m; };
struct SceneElement {
	PrimKind kind;
	MaterialObj* material;
	// sphere (reference geom/sphere.h:22-25)
	f3 center; float radius;
	// cube (reference geom/cube.h:36-41)
	f3 minBounds, maxBounds; float timeStartMove; f3 velocity;
	// loose triangle (reference geom/triangle.h)
	HostTriangle tri;
};
struct HostSphere { f3 center; float radius; int32_t material; };
struct HostCube { f3 minBounds, maxBounds; float timeStartMove; f3 velocity; int32_t material; };
// the stack discipline of the binary, 4-wide float-box, 4-wide grid and 8-wide walks restated on the host with the capacity as an argument (rl_bvh.cc): closest t and the stack's high-water mark per ray
bool WalkStackHost(const BVH& bvh, const std::vector<HostTriangle>& tris, const std::vector<HostSphere>& spheres, const std::vector<HostCube>& cubes, int tree,
                   const float* rays, int n, float tMin, int capacity, float* outT, uint32_t* outHighWater);

struct DeviceScene;   // rl_rt.h

struct Scene {
	std::vector<OBJModel*> models;    // borrowed (reference raylib.cc:264-268)
	std::vector<SceneElement*> elements;   // borrowed (reference raylib.cc:258-262)
	std::vector<HostSphere> spheres;  // flattened at Finalize
	std::vector<HostCube> cubes;
	Image* sky = nullptr;             // borrowed (reference raylib.cc:270-273)
	f3 sunIlluminance = F3(0, 0, 0);
	f3 sunDirection;
	bool finalized = false;

	// flattened at Raylib_FinalizeScene
	std::vector<HostTriangle> triangles;
	std::vector<HostMaterial> materials;
	std::vector<std::shared_ptr<Image>> textures;
	BVH bvh;
	DeviceScene* device = nullptr;    // uploaded lazily at first render

	bool hasMovingCubes = false;
	float accelT0 = 0.0f, accelT1 = 0.0f;   // shutter interval the BVH boxes cover

	// RaylibAMD_SceneMoveTriangles: the device's copy is ahead of `triangles` (after the device entry) / of bvh's boxes but the root's (after either entry) until
	// DeviceSyncMovedScene reads them back; whoever reads them on the host calls it first
	bool hostTrisStale = false, hostTreesStale = false;

	Scene();
	~Scene();
	void Finalize();
	bool BuildAccel(float t0, float t1);   // false: the scene exceeds the BVH's addressing (logged); nothing was built
};
// true when no material has a texture slot (>= 0) and no leaf of the leaf list carries the cut-out bit: the leaf-list kernel's
// plain instance may render the scene (rl_plan.cc adds the per-render conditions)
bool ScenePlain(const Scene& sc);
// ... and k_trace's lazy-reflectance instance: plain, every material microfacet with parameters inside the instance's intervals (rl_scene.cc)
bool SceneLazyRefl(const Scene& sc);

// The scene as the devices hold it (rl_device.h), in leaf order (rl_scene.cc FlattenScene): triangle records -- rden is 1 / denom for the short barycentric
// divisions, NaN where denom is 0 or NaN or outside [2^-62, 2^125], and the last case clears fastBary for the whole scene (RAYLIB_FAST_BARY=0 clears it whatever
// the scene) --, materials, textures with a pow(texel, 2.2) copy of every map a microfacet material uses as albedo (the material points at the copy), the texel
// pool, per triangle slot the texture its cut-out test reads (alphaTex; empty: no material has a map), spheres, cubes, and the sky panorama's rotation.
struct FlatScene {
	std::vector<DTriIsect> isect; std::vector<DTriShade> shade; std::vector<int32_t> alphaTex;
	std::vector<DMaterial> materials; std::vector<DTexture> textures; std::vector<float> texels;
	std::vector<DSphere> spheres; std::vector<DCube> cubes;
	int32_t fastBary = 1;
	SkyRot skyRot;
};
FlatScene FlattenScene(const Scene& sc);   // every texture's host pixels are current (Image::hostStale is not looked at)

// loaders (rl_obj_loader.cc, rl_image_io.cc)
bool LoadOBJ(const char* path, OBJModel& out);
void TransformOBJ(OBJModel& m, float tx, float ty, float tz, float yaw, float pitch, float roll, float sx, float sy, float sz);
Image* LoadImageFile(const char* path);
bool WriteImageFile(const Image& img, const char* path, uint32_t fileType);
void PostProcessHost(Image& img);   // rl_scene.cc; Raylib_PostProcess (rl_abi.cc) uses it only when the image never lived on a device

// logging (rl_log.cc)
void Log(const char* fmt, ...);
void LogStart();
void LogFlush();
void LogStop();

// device side (the host runtime: rl_rt.h, rl_rt_*.hip)
struct RenderRequest {
	RendererSettings settings;
	DCamera camera;
	uint64_t seed;
	uint32_t cellFirst, cellStride;
	bool cellMajor = false; // the rank's cells back to back even when it owns every cell (one rank going through the gather path)
	int slot = 0;           // frame slot (0 / 1) of the rank's events and counter buffers: a multi-rank frame in flight while the next is enqueued
	void* outDevice;        // may be null
	bool callerOwnsOut = false; // outDevice is memory of the CALLER (RaylibAMD_RenderDevice), not an image of the library: the call returns with the frame complete in it
	float* outHostRGBA;     // may be null; receives what outDevice would (row-major image or the rank's cells)
};
bool DeviceAvailable();
int DeviceNumRanks();                          // logical ranks (RAYLIB_NUM_GPUS) the library drives from this process; 0 without a device
float ParseDecimalFloat(const char* token);   // csrc/rl_obj_loader.cc: the OBJ parser's number reader (= strtof, with exact fast paths)
// Decoders refuse images beyond this many pixels (16384 x 16384), and images whose claimed size the file cannot plausibly hold:
// a corrupt header must not turn into a multi-gigabyte allocation.
constexpr uint64_t kMaxImagePixels = 1ull << 28;
inline bool PlausibleImageSize(uint64_t w, uint64_t h, uint64_t fileBytes, uint64_t maxPixelsPerByte)
{
	return w > 0 && h > 0 && w <= 65535 && h <= 65535 && w * h <= kMaxImagePixels && w * h <= (fileBytes + 64) * maxPixelsPerByte;
}
// csrc/rl_jpeg.cc: top-down RGBA8
bool DecodeJPEG(const std::vector<uint8_t>& data, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba);
bool DecodeTGA(const std::vector<uint8_t>& data, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba);
bool EncodeJPEG(uint32_t w, uint32_t h, const uint8_t* rgbTopDown, std::vector<uint8_t>& out);   // baseline, quality 75, 4:2:0
bool DeviceRender(Scene& scene, const RenderRequest& req, RaylibAMDStats& stats);
// RaylibAMD_RenderViews: `count` views (cameras[v]) of req.settings / req.seed into outDevice (view-major, count * W * H float4; nullptr: the library's
// own buffer) and, when imagePixels is given, each view's frame copied into imagePixels[v] (W * H float4 on rank 0's device).  Synchronous.
bool DeviceRenderViews(Scene& scene, const RenderRequest& req, const DCamera* cameras, uint32_t count, void* outDevice, void* const* imagePixels, RaylibAMDStats& stats);
int32_t DeviceLastTraceLazy();    // 1: ... and of that, the lazy-reflectance instance (k_trace_lazy or its hit-queue form)
int32_t DeviceLastHitQueue();     // 1: ... and of that, its hit-queue form (k_trace_lazy_hitq)
int32_t DeviceLastLitMask();      // 1: ... and that launch kept a lit-sample mask (rl_lit_mask.h: k_resolve_lit behind it)
int32_t DeviceLastTracePlain();   // 1: the last path-traced render's megakernel was the leaf-list kernel's plain instance (rl_plan.cc)
bool DeviceDrain(RaylibAMDStats* outLastStats);   // waits for multi-rank frames in flight; true + stats when that completed the last render call's numbers
void DeviceOwnStats();                            // the caller reports a synchronous call's own numbers: a frame still in flight, or completed inside that call, is no longer the last call
bool DeviceClosestHit(Scene& scene, const float* rays, int32_t n, float tMin, void* outHits);
// RaylibAMD_TraceRays (hostMem: rays / out / outPrim in host memory) and RaylibAMD_TraceRaysDevice (device pointers; stream null: the library's stream,
// synchronous; else enqueued on that hipStream_t).  stats: filled by a synchronous call.  kind is valid, n >= 0, the scene finalized: the ABI checked.
bool DeviceTraceRays(Scene& scene, int32_t kind, const void* rays, int32_t n, float rayTime, void* out, int32_t* outPrim, bool hostMem, void* stream,
                     RaylibAMDStats& stats);
// RaylibAMD_RenderGBuffer (hostMem: the planes are host memory) and RaylibAMD_RenderGBufferDevice, as DeviceTraceRays: the planes asked for (non-null) of the
// settings' frame, from the camera's sample-0 rays under `seed`.  The frame has 1 .. 2^31 - 1 pixels, a plane is asked for, rayTMin is finite, the scene
// finalized and its boxes built for the camera's shutter interval: the ABI checked.
bool DeviceRenderGBuffer(Scene& scene, const RendererSettings& settings, const DCamera& camera, uint64_t seed, const RaylibAMDGBufferPlanes& planes, bool hostMem, void* stream,
                         RaylibAMDStats& stats);
// RaylibAMD_RenderMotion (hostMem: the planes and the previous positions are host memory) and RaylibAMD_RenderMotionDevice, as DeviceRenderGBuffer: the hit
// and the motion plane, whichever was asked for, with the previous camera and the previous positions of triangles [first, first + count).  What
// DeviceRenderGBuffer expects of the ABI, and: a plane is asked for, the range lies in the scene's triangles, positions are given when count > 0.
bool DeviceRenderMotion(Scene& scene, const RendererSettings& settings, const DCamera& camera, const DCamera& prevCamera, uint64_t seed, int32_t first, int32_t count,
                        const float* prevPositions, const RaylibAMDMotionPlanes& planes, bool hostMem, void* stream, RaylibAMDStats& stats);
// An accumulation call as its entry got it, RaylibAMD_TemporalAccumulate's (moments false: history.moments and outMoments are null and not looked at) or
// RaylibAMD_TemporalAccumulateMoments's.  hasHistory false: the first frame, `history` is all null.
struct TemporalCall {
	uint32_t width, height; const RaylibAMDTemporalParams* params;
	const float* colour; const RaylibAMDHitT* hit; const RaylibAMDMotion* motion;
	bool hasHistory; RaylibAMDTemporalMomentsFrame history;
	float *outColour, *outLength, *outMoments;
	bool moments;
};
// RaylibAMD_TemporalAccumulate[Moments] (hostMem) and ...Device on rank 0's device, behind frames in flight (stream: as DeviceTraceRays).  The history's planes
// are all given, the frame has 1 .. 2^31 - 1 pixels, the parameters are in range, no output is a history plane: the ABI checked.
bool DeviceTemporalAccumulate(const TemporalCall& call, bool hostMem, void* stream, RaylibAMDStats& stats);
// RaylibAMD_FilterVariance (hostMem) and RaylibAMD_FilterVarianceDevice, under the same rules.  params: the caller's or the defaults, checked.
bool DeviceFilterVariance(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams& params, const RaylibAMDVarianceFilterPlanes& planes, float* outColour,
                          float* outVariance, bool hostMem, void* stream, RaylibAMDStats& stats);
// RaylibAMD_TraceRaysAll (hostMem) and RaylibAMD_TraceRaysAllDevice, as DeviceTraceRays: outHits holds n rows of maxHits records, outCount (may be null) n words.
// The scene holds triangles only, 1 <= maxHits <= RAYLIB_AMD_MAX_HITS and n * maxHits fits an int32_t: the ABI checked.
bool DeviceTraceRaysAll(Scene& scene, const void* rays, int32_t n, int32_t maxHits, void* outHits, uint32_t* outCount, bool hostMem, void* stream, RaylibAMDStats& stats);
// RaylibAMD_NearestPoints (hostMem) and RaylibAMD_NearestPointsDevice, as DeviceTraceRays; the scene holds triangles only: the ABI checked.
bool DeviceNearestPoints(Scene& scene, int32_t kind, const void* points, int32_t n, void* out, bool hostMem, void* stream, RaylibAMDStats& stats);
// RaylibAMD_NearestPointsAll (hostMem) and RaylibAMD_NearestPointsAllDevice, as DeviceTraceRaysAll: outHits holds n rows of maxHits records, outCount (may be
// null) n words.  The scene holds triangles only, 1 <= maxHits <= RAYLIB_AMD_MAX_NEAREST and n * maxHits fits an int32_t: the ABI checked.
bool DeviceNearestPointsAll(Scene& scene, const void* points, int32_t n, int32_t maxHits, void* outHits, uint32_t* outCount, bool hostMem, void* stream, RaylibAMDStats& stats);
// RaylibAMD_SweepSpheres (hostMem) and RaylibAMD_SweepSpheresDevice, as DeviceNearestPoints: 32-byte queries, a word (ANY) or a 32-byte record (CLOSEST) out.
bool DeviceSweepSpheres(Scene& scene, int32_t kind, const void* queries, int32_t n, void* out, bool hostMem, void* stream, RaylibAMDStats& stats);
// RaylibAMD_BakeDistanceField (hostMem) and RaylibAMD_BakeDistanceFieldDevice, as DeviceNearestPoints: outDist and outPrim (may be null) hold a word per voxel.
// grid is valid (statement V7) with maxDist >= +0, the scene holds triangles only: the ABI checked.
bool DeviceBakeDistanceField(Scene& scene, const RaylibAMDDistanceFieldParams& grid, float* outDist, int32_t* outPrim, bool hostMem, void* stream, RaylibAMDStats& stats);
// RaylibAMD_OverlapTriangles (hostMem) and RaylibAMD_OverlapTrianglesDevice, as DeviceNearestPoints; kind, flags and (for LIST) maxHits are valid, outCount is
// null for ANY, n * maxHits fits 2^31 - 1: the ABI checked.
// contacts: RaylibAMD_OverlapContacts (Device) -- kind is LIST and outContact takes n * maxHits 32-byte records (non-null when n > 0).
bool DeviceOverlapTriangles(Scene& scene, int32_t kind, uint32_t flags, const void* queries, int32_t n, int32_t maxHits, void* out, uint32_t* outCount, bool hostMem, void* stream,
                            RaylibAMDStats& stats, void* outContact = nullptr, bool contacts = false);
// RaylibAMD_OverlapBoxes (hostMem) and RaylibAMD_OverlapBoxesDevice, as DeviceOverlapTriangles; kind and (for LIST) maxHits are valid, outCount is null for ANY
// and MARK, n * maxHits fits 2^31 - 1: the ABI checked.  MARK: out is the call's mask, (triangles + 31) / 32 words, written whole even when n is 0.
bool DeviceOverlapBoxes(Scene& scene, int32_t kind, const void* queries, int32_t n, int32_t maxHits, void* out, uint32_t* outCount, bool hostMem, void* stream, RaylibAMDStats& stats);
// RaylibAMD_TraceRadiance (hostMem) and RaylibAMD_TraceRadianceDevice, as DeviceTraceRays; prm is valid (timeMin <= timeMax cover every ray's time and the
// scene's boxes), seed is the library's: the ABI checked.
// The path stack's budget: the grid is cut until its stack (32 bytes per bounce and resident lane) fits, and a maxPathLength at which one workgroup of 256
// lanes does not fit is refused (RL_RADIANCE_STACK_BUDGET / (32 * 256)).
constexpr uint64_t RL_RADIANCE_STACK_BUDGET = 256ull << 20;
constexpr int32_t RL_RADIANCE_MAX_PATH = 32768;
bool DeviceTraceRadiance(Scene& scene, const RaylibAMDRadianceParams& prm, uint64_t seed, const void* rays, int32_t n, float* out, bool hostMem, void* stream,
                         RaylibAMDStats& stats);
// RaylibAMD_Gather (hostMem) and RaylibAMD_GatherDevice: kind is RAYLIB_AMD_GATHER_*, prm holds the gather's parameters as a radiance call's and is valid, as above.
// The sample buffer of a launch is held to RL_GATHER_SAMPLE_BUDGET (RAYLIB_GATHER_BATCH: so many slots instead, at most RL_GATHER_MAX_SLOTS); a call of more
// (point, sample) pairs runs as several launches.  A synchronous call times up to RL_GATHER_TIMED trace launches apart from their resolves.
constexpr uint64_t RL_GATHER_SAMPLE_BUDGET = 256ull << 20;
constexpr uint64_t RL_GATHER_MAX_SLOTS = 1ull << 28;
constexpr uint64_t RL_GATHER_TIMED = 4096;
// With A, RaylibAMD_GatherAdaptive (hostMem) and RaylibAMD_GatherAdaptiveDevice: the gather in passes with per-point stopping (statements A1 to A5); prm.sampleCount
// is the cap, A is valid and gives at most RL_GATHER_ADAPTIVE_MAX_PASSES passes.  outSamples (with A only) may be null; memory as out's.  With a stream the call waits
// for it once per pass.
constexpr uint32_t RL_GATHER_ADAPTIVE_MAX_PASSES = 4096;
bool DeviceGather(Scene& scene, int32_t kind, const RaylibAMDRadianceParams& prm, uint64_t seed, const void* points, int32_t n, float* out, bool hostMem, void* stream,
                  RaylibAMDStats& stats, const RaylibAMDGatherAdaptiveParams* A = nullptr, uint32_t* outSamples = nullptr);
// RaylibAMD_GatherCompactTest: the compaction behind a pass on uploaded copies, launched as a pass launches it; the ABI checked the arguments (live strictly
// ascending below numPoints).  false without a device or memory; outputs are written only on success.
bool DeviceGatherCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const RaylibAMDGatherPoint* points, uint32_t numPoints,
                             uint32_t* outLive, RaylibAMDGatherPoint* outPoints, uint32_t* outCount);
// Lightmaps (include/raylib_amd.h RaylibAMD_BakeLightmap).  The ABI checked the arguments: the atlas' size, the dilation, the time, triFirst / triCount a non-empty
// range of the scene's triangles, capacity >= 0, prm the gather's parameters as a radiance call's with timeMin = timeMax = the time.
// LightmapPointsHost (rl_lightmap_host.cc): the oracle of the raster stages; -1 without memory.
int64_t LightmapPointsHost(const Scene& scene, const RaylibAMDLightmapParams& P, int32_t triFirst, int32_t triCount, const float* uv,
                           RaylibAMDGatherPoint* outPoints, uint32_t* outTexel, int64_t capacity);
// DeviceLightmapPoints: the raster stages on rank 0's device (rl_lightmap.hip's kernels), uv and the outputs in host memory; the count, or -1.
int64_t DeviceLightmapPoints(Scene& scene, const RaylibAMDLightmapParams& P, int32_t triFirst, int32_t triCount, const float* uv,
                             RaylibAMDGatherPoint* outPoints, uint32_t* outTexel, int64_t capacity);
// DeviceBakeLightmap: raster, gather, scatter, dilation.  who: the entry's name in the log.  hostMem: uv / out / outCoverage in host memory (stream is null), else
// device pointers; stream as DeviceGather's.
// filter (may be null; checked by the ABI): statement F between the gather and the scatter.  in (with a filter only; memory as out's, may be out): the covered
// texels take their values from that atlas instead of a gather (RaylibAMD_FilterLightmap).
// adaptive (may be null; checked by the ABI; without filter and in): statement 7 is the adaptive DeviceGather's passes, and outSamples (may be null; memory as out's)
// receives the atlas of the texels' sample counts.
bool DeviceBakeLightmap(const char* who, Scene& scene, const RaylibAMDLightmapParams& P, int32_t triFirst, int32_t triCount, const RaylibAMDRadianceParams& prm, uint64_t seed,
                        const float* uv, float* out, uint8_t* outCoverage, bool hostMem, void* stream, RaylibAMDStats& stats,
                        const RaylibAMDLightmapFilterParams* filter = nullptr, const float* in = nullptr,
                        const RaylibAMDGatherAdaptiveParams* adaptive = nullptr, uint32_t* outSamples = nullptr);
// Statement F's constants (F4), computed once on the host for both paths, and the statement on the host (rl_lightmap_filter.hip): the oracle of k_lm_filter.
// The ABI checked the arguments but the texel array; false: that array is not strictly ascending inside the atlas, or no memory (nothing written).
struct LmFilterInv { float invC[8], invN, invP[8]; };
LmFilterInv MakeLmFilterInv(const RaylibAMDLightmapFilterParams& F);
bool FilterLightmapHost(int32_t width, int32_t height, int32_t kind, const RaylibAMDLightmapFilterParams& F, const RaylibAMDGatherPoint* points, const uint32_t* texel,
                        int64_t count, const float* values, float* outValues);
bool DevicePostProcess(Image& img);          // Image2D::PostProcess on the device; false when no device
bool DeviceDumpRGB(Image& img, float* outRGB);   // a device-resident frame packed to RGB on the device and copied to caller memory through pinned staging; false: not applicable
bool DeviceReadback(Image& img);            // device copy -> img.rgba (the caller checked hostStale)
void* DeviceImagePixels(Image& img);          // (re)allocates img.devPixels for width*height float4; nullptr when no device
void DeviceFreePixels(void* p);
// cells outside the scene's silhouette (rl_cull.cc)
struct CullScene { double boundsMin[3] = { 0, 0, 0 }, boundsMax[3] = { 0, 0, 0 }; bool boundsValid = false, prims = false, hasSky = false, hasSun = false; float sunDirection[3] = { 0, 0, 0 }, sunIlluminance[3] = { 0, 0, 0 }; };
struct CullResult { std::vector<uint32_t> active; std::vector<unsigned char> empty; uint64_t emptyPixels = 0; float L[3] = { 0, 0, 0 }; uint32_t raysPerSample = 1; };
bool CullCells(const CullScene& DS, const DCamera& cam, int32_t maxPathLength, float rayTMin, uint32_t W, uint32_t H,
               uint32_t cellsX, uint32_t cellFirst, uint32_t stride, uint32_t numLocalCells, CullResult& out);
bool DeviceEvalMath(int fn, const float* x, const float* y, int n, float* out);
bool DeviceVerifyLazyRefl(uint32_t n, uint64_t seed, uint64_t out[3]);   // k_verify_lazy_refl: events, guard passed with a non-finite refl or sp, guard failed
bool DeviceVerifyLazyPdf(uint32_t n, uint64_t seed, uint64_t out[3]);    // k_verify_lazy_pdf: events, quick with a pdf that is not positive and finite or a record that folds to other bits, not quick
bool DeviceVerifySamplerRanged(int mode, uint64_t out[6]);   // k_verify_sampler_ranged: mismatches, the smallest mismatching bit pattern, mode 1's largest differing positive pattern below the branch and its mismatches outside the interval, the bits of C_MIN and of the branch's threshold
bool DeviceVerifyNormalizeRanged(int mode, uint64_t out[4]);   // k_verify_normalize_ranged: mismatches, the smallest mismatching input, mode 0's smallest differing pattern outside the domain, mode 0's count of those or mode 2's vectors on the guard-free side
bool DeviceVerifyExactMath(int which, uint64_t* outMismatches, uint64_t* outFirst);   // 0: rtm::rcp1_ vs 1.0f / x, 1: rtm::sqrt_ vs sqrtf, 2: rtm::div_by_ vs a / b, 3: Barycentric short vs divisions, 4: acosf_t / tanf_t short vs IEEE divisions; all 2^32 inputs
bool DeviceEvalHook(int kind, Scene* sc, const DCamera* cam, int a, int b, const float* in, int n, uint64_t seed, float* out);
void DeviceReleaseScene(DeviceScene* dev);
// RaylibAMD_SceneMoveTriangles (hostMem) / RaylibAMD_SceneMoveTrianglesDevice (rl_rt_move.hip); the ABI checked the scene, the range and a host call's values.
bool DeviceMoveTriangles(Scene& scene, int32_t first, int32_t count, const float* positions, const float* normals, bool hostMem, void* stream);
// the host copies of a moved scene (triangles, trees) current again: one read-back where they are stale, nothing otherwise
bool DeviceSyncMovedScene(Scene& scene);
// RaylibAMD_SceneCheckTrees: rl_bvh.cc's checks on what the device holds; *outFailedTree: 0, or 2 / 4 / 8 for the first tree that failed
bool DeviceCheckTrees(Scene& scene, uint32_t* outFailedTree);
// RaylibAMD_SceneCompareTrees: the wide formats every device's copy holds against RefitWideFromBinary of that copy's own binary nodes, and its records against
// rank 0's; *outDiffMask: 1 float-4, 2 grid-4, 4 leaf list, 8 8-wide, 16 records.  false with the mask untouched when the check could not run.
bool DeviceCompareTrees(Scene& scene, uint32_t* outDiffMask);

// Progressive rendering (include/raylib_amd.h RaylibAMD_BeginProgressive; rl_rt_render.hip).  Begin: nullptr without a device or memory.  Step: the number of
// live cells after the pass (0: finished), -1 when refused or failed -- `rendered` tells whether a pass ran (and `stats` is its numbers).
struct ProgressiveSession;
ProgressiveSession* DeviceProgressiveBegin(Scene& sc, const RenderRequest& req, float threshold, uint32_t minSamples);
int32_t DeviceProgressiveStep(ProgressiveSession& S, uint32_t samples, void* outDevice, RaylibAMDStats& stats, bool& rendered);
bool DeviceProgressiveExport(ProgressiveSession& S, uint32_t* cellSamples, uint8_t* cellStopped, float* sumY, float* sumY2);
void DeviceProgressiveEnd(ProgressiveSession* S);
// RaylibAMD_ProgressiveCompactTest: k_progressive_compact on uploaded copies of the lists, launched as a pass launches it; the ABI checked the arguments
// (numLive <= numCells = the frame's cells, every entry of live < numCells).  false without a device or memory; outputs are written only on success.
bool DeviceProgressiveCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const uint8_t* emptyOrNull, uint32_t numCells,
                                  uint32_t width, uint32_t height, uint32_t* outLive, uint32_t* outTrace, uint32_t outCounts[4]);

// denoiser (rl_denoise.hip): the a-trous filter on the device and its host restatement; params checked by the caller (rl_abi.cc RaylibAMD_Denoise / RaylibAMD_DenoiseHost)
void DenoiseHost(uint32_t width, uint32_t height, const float* color, bool hdr, const float* albedo, const float* normal,
                 const RaylibAMDDenoiseParams& params, float* out);
// main, albedo and normal are uploaded first when their pixels live only on the host; out (which may be any of them) is reallocated
// to main's size and left on the device (devValid, hostStale).  The caller has waited for frames in flight (DeviceDrain).
bool DeviceDenoise(Image& main, bool hdr, Image* albedo, Image* normal, Image& out, const RaylibAMDDenoiseParams& params);

} // namespace rl
