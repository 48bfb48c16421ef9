// The C-ABI of the MI355X raylib: the 33 entry points of include/raylib.h (one per
// reference function, reference raylib/raylib.cc:25-331) plus the additional exports
// of include/raylib_amd.h.  Handles are raw pointers kept in mutex-guarded registries,
// as in the reference (raylib.cc:18-21, core/concurrent_vector.h:8-49).
#include "raylib.h"
#include "raylib_amd.h"
#include "rl_host.h"
#include "rl_oracle.h"
#include "rl_plan.h"
#include "rl_progressive.h"   // RaylibAMD_ProgressiveDecideHost's rule
#include "rl_lightmap.h"
#include "rl_sdf.h"           // SdfCentre: a refusal of the distance field's grid
#include "rl_contact.h"       // ContactRecord and the contact kinds: the static_asserts on the ABI's record

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

using namespace rl;

namespace {

template <typename T>
struct Registry {
	std::mutex mu;
	std::vector<T*> items;
	void add(T* p) { std::lock_guard<std::mutex> lk(mu); items.push_back(p); }
	bool eraseFirst(T* p) {
		std::lock_guard<std::mutex> lk(mu);
		auto it = std::find(items.begin(), items.end(), p);
		if (it == items.end()) return false;
		items.erase(it);
		return true;
	}
	bool contains(T* p) { std::lock_guard<std::mutex> lk(mu); return std::find(items.begin(), items.end(), p) != items.end(); }
};
Registry<OBJModel> g_objModels;
Registry<Camera>   g_cameras;
Registry<Image>    g_images;
Registry<Scene>    g_scenes;
Registry<MaterialObj>  g_materials;
Registry<SceneElement> g_elements;

std::mutex g_stateMu;
uint64_t g_seed = 1;
bool g_seedSet = false;
RaylibAMDStats g_lastStats;
int g_denoiser = -1;   // RaylibAMD_EnableDenoiser; -1: not set yet, RAYLIB_DENOISER decides at first use

bool DenoiserEnabled()
{
	std::lock_guard<std::mutex> lk(g_stateMu);
	if (g_denoiser < 0) { const char* e = getenv("RAYLIB_DENOISER"); g_denoiser = (e && e[0] == '1' && e[1] == 0) ? 1 : 0; }
	return g_denoiser == 1;
}

// Chosen with the Cornell quality test (tests/test_gpu_denoise.py; DESIGN.md, "Denoiser").
const RaylibAMDDenoiseParams kDenoiseDefaults = { 5, 2.0f, 0.3f, 0.05f };
bool DenoiseParamsValid(const RaylibAMDDenoiseParams& P)
{
	auto ok = [](float s) { return s >= 1e-3f && s <= 1e3f; };   // (also false for NaN): 1 / s^2 and 4^7 / s^2 stay finite and nonzero
	return P.iterations >= 1 && P.iterations <= 8 && ok(P.sigmaColor) && ok(P.sigmaNormal) && ok(P.sigmaAlbedo);
}

uint64_t CurrentSeed()
{
	std::lock_guard<std::mutex> lk(g_stateMu);
	if (!g_seedSet) {
		if (const char* e = getenv("RAYLIB_SEED")) g_seed = strtoull(e, nullptr, 10);
		g_seedSet = true;
	}
	return g_seed;
}

// The scene's device copy goes (the next call uploads the host's scene again): had its triangles moved on the device, the host's copies are brought up to date
// first (RaylibAMD_SceneMoveTriangles)
void ReleaseDeviceCopy(Scene* s)
{
	if (!s->device) return;
	if (!DeviceSyncMovedScene(*s)) Log("the scene's moved triangles could not be read back: its next upload is of the triangles the host holds");
	DeviceReleaseScene(s->device); s->device = nullptr;
}

// Moving cubes: their boxes must cover the motion over THIS camera's shutter interval (a render, and a G-buffer of the camera's rays)
bool PrepareShutter(const char* who, Scene* scene, const Camera* camera)
{
	if (scene->hasMovingCubes && (scene->accelT0 != camera->beginTime || scene->accelT1 != camera->endTime)) {
		ReleaseDeviceCopy(scene);
		if (!scene->BuildAccel(camera->beginTime, camera->endTime)) { Log("%s: the acceleration structure could not be rebuilt for this camera's shutter interval", who); return false; }
	}
	return true;
}

// What every render checks and prepares before it reaches the device (Raylib_Render and RaylibAMD_BeginProgressive; `who` names the caller in the log).
bool PrepareRender(const char* who, const RendererSettings* settings, Scene* scene, Camera* camera)
{
	if (!settings || !scene || !camera) { Log("%s: null argument", who); return false; }
	if (!scene->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return false; }
	if (settings->renderMode >= RAYLIB_RENDERMODE_MAX) { Log("%s: invalid render mode %u", who, settings->renderMode); return false; }
	if (!PrepareShutter(who, scene, camera)) return false;
	if (scene->sky && !g_images.contains(scene->sky)) {
		// the reference would read freed memory here; a destroyed panorama is treated as none
		Log("%s: the scene's sky panorama was destroyed; rendering without it", who);
		scene->sky = nullptr;
	}
	return true;
}

bool RenderInternal(const RendererSettings* settings, Scene* scene, Camera* camera,
                    uint32_t cellFirst, uint32_t cellStride, void* outDevice, float* outHost, bool callerOwnsOut = false)
{
	if (!PrepareRender("Raylib_Render", settings, scene, camera)) return false;
	RenderRequest req;
	req.settings = *settings;
	req.camera = camera->ToDevice();
	req.seed = CurrentSeed();
	req.cellFirst = cellFirst; req.cellStride = cellStride;
	req.outDevice = outDevice; req.outHostRGBA = outHost;
	req.callerOwnsOut = callerOwnsOut;
	RaylibAMDStats stats; memset(&stats, 0, sizeof(stats));
	bool ok = DeviceRender(*scene, req, stats);
	{ std::lock_guard<std::mutex> lk(g_stateMu); g_lastStats = stats; }
	return ok;
}

// The numbers of a synchronous query, radiance call, gather or bake become RaylibAMD_GetLastStats': those calls do not wait for a multi-rank frame in flight,
// whose numbers, completed later, must not replace them (rl_rt_render.hip FinishInflight).  A call on a caller's stream reports nothing and does not come here.
void ReportOwnStats(const RaylibAMDStats& stats)
{
	DeviceOwnStats();
	std::lock_guard<std::mutex> lk(g_stateMu);
	g_lastStats = stats;
}

// ---- what the query entries share ----
// An accepted call's way to the device: `call` runs the Device* function on the zeroed stats block; a synchronous call's numbers are the last call's
template <typename Call>
int32_t RunOnDevice(void* stream, Call call)
{
	if (!DeviceAvailable()) return 0;
	RaylibAMDStats stats; memset(&stats, 0, sizeof(stats));
	if (!call(stats)) return 0;
	if (!stream) ReportOwnStats(stats);
	return 1;
}
// An accepted call's way to its host oracle (rl_oracle.h): the host's copies made current -- the triangles and trees a move left stale, a texture's pixels that
// live on the device -- then `call`, which runs the oracle on the scene
template <typename Call>
int32_t RunOnHost(Scene* s, Call call)
{
	if (!DeviceSyncMovedScene(*s)) return 0;
	for (const std::shared_ptr<Image>& t : s->textures) t->SyncHost();
	call();
	return 1;
}
// The refusals of the queries on triangles (`family`: what the log calls them), for device entries and oracles alike: the arguments, a finalized scene of
// triangles only whose tree fits the walk's stack, and, for a call that writes rows (`rows`), maxHits within the family's capacity and n * maxHits in 2^31 - 1.
struct QueryRows { int32_t maxHits, cap; const char *inputs, *items, *unit; };   // the last three: the log's words, "%d <inputs> x %d <items> exceed 2^31 - 1 <unit>"
bool TriangleQueryArgsValid(const char* who, const char* family, const Scene* s, const void* in, int32_t n, const void* out, const QueryRows* rows = nullptr)
{
	if (!s || n < 0 || (n > 0 && (!in || !out))) { Log("%s: null argument", who); return false; }
	if (rows) {
		if (rows->maxHits < 1 || rows->maxHits > rows->cap) { Log("%s: maxHits %d is outside 1..%d", who, rows->maxHits, rows->cap); return false; }
		if ((int64_t)n * rows->maxHits > 0x7fffffffll) { Log("%s: %d %s x %d %s exceed 2^31 - 1 %s", who, n, rows->inputs, rows->maxHits, rows->items, rows->unit); return false; }
	}
	if (!s->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return false; }
	if (!s->spheres.empty() || !s->cubes.empty()) { Log("%s: the scene holds spheres or cubes; %s are defined on triangles", who, family); return false; }
	if (s->bvh.depth > 64) { Log("%s: BVH depth %u exceeds the traversal stack (64)", who, s->bvh.depth); return false; }
	return true;
}
// A planner's answer as the ABI reports it: -1 with `out` zeroed when the tree is too deep, else 1.  prims, early: what the entry reports of them (0: not the family's)
int32_t ExportPlan(const QueryPlan& p, int32_t prims, int32_t early, RaylibAMDQueryPlan* out)
{
	memset(out, 0, sizeof(*out));
	if (!p.ok) return -1;
	out->tree = p.tree; out->treeWidth = p.treeWidth; out->nodeBytes = p.nodeBytes; out->stack = p.stack; out->prims = prims; out->early = early;
	return 1;
}

// A progressive session as the ABI hands it out: the device session and the handles it was begun with.
struct Progressive {
	Scene* scene;
	Image* out;
	uint32_t width, height;
	ProgressiveSession* dev;
};
Registry<Progressive> g_progressive;

bool ProgressiveParamsValid(const RaylibAMDProgressiveParams& P)
{
	return P.threshold >= 0.0f && P.threshold <= 3.40282347e+38f && P.minSamples >= 2;   // (false for NaN)
}

// The checks RaylibAMD_RenderViews / RenderViewsDevice / PlanViews make before anything is touched (include/raylib_amd.h); images may be null (the device form)
bool ViewsArgsValid(const char* who, const RendererSettings* settings, Scene* scene, const CameraHandle* cameras, int32_t count, const ImageHandle* images)
{
	if (!settings || !scene || !cameras) { Log("%s: null argument", who); return false; }
	if (count < 1 || count > RAYLIB_AMD_MAX_VIEWS) { Log("%s: %d views (1..%d)", who, count, RAYLIB_AMD_MAX_VIEWS); return false; }
	if (!g_scenes.contains(scene)) { Log("%s: unknown scene", who); return false; }
	for (int32_t v = 0; v < count; ++v) {
		Camera* c = (Camera*)cameras[v];
		if (!c || !g_cameras.contains(c)) { Log("%s: camera %d is 0 or unknown", who, v); return false; }
		if (images) {
			Image* img = (Image*)images[v];
			if (!img || !g_images.contains(img)) { Log("%s: image %d is 0 or unknown", who, v); return false; }
			for (int32_t w = 0; w < v; ++w) if (images[w] == images[v]) { Log("%s: image %d appears twice", who, v); return false; }
		}
	}
	if (!scene->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return false; }
	if (settings->renderMode >= RAYLIB_RENDERMODE_MAX) { Log("%s: invalid render mode %u", who, settings->renderMode); return false; }
	if ((uint64_t)settings->viewportWidth * settings->viewportHeight == 0) { Log("%s: empty viewport", who); return false; }
	const uint64_t cells = (uint64_t)((settings->viewportWidth + 7) / 8) * ((settings->viewportHeight + 7) / 8);
	if (cells * (uint64_t)count * 64u > 0xF0000000ull) { Log("%s: job count overflow", who); return false; }
	if (scene->hasMovingCubes) {
		const Camera* c0 = (const Camera*)cameras[0];
		for (int32_t v = 1; v < count; ++v) {
			const Camera* c = (const Camera*)cameras[v];
			if (c->beginTime != c0->beginTime || c->endTime != c0->endTime) { Log("%s: the scene has moving cubes and the cameras' shutter intervals differ", who); return false; }
		}
	}
	return true;
}

bool RenderViewsInternal(const char* who, const RendererSettings* settings, Scene* s, const CameraHandle* cameras, int32_t count, void* outDevice, void* const* imagePixels)
{
	if (!PrepareRender(who, settings, s, (Camera*)cameras[0])) return false;
	RenderRequest req;
	req.settings = *settings;
	req.camera = ((Camera*)cameras[0])->ToDevice();
	req.seed = CurrentSeed();
	req.cellFirst = 0; req.cellStride = 1;
	req.outDevice = nullptr; req.outHostRGBA = nullptr;
	std::vector<DCamera> cams((size_t)count);
	for (int32_t v = 0; v < count; ++v) cams[(size_t)v] = ((Camera*)cameras[v])->ToDevice();
	RaylibAMDStats stats; memset(&stats, 0, sizeof(stats));
	const bool ok = DeviceRenderViews(*s, req, cams.data(), (uint32_t)count, outDevice, imagePixels, stats);
	{ std::lock_guard<std::mutex> lk(g_stateMu); g_lastStats = stats; }
	return ok;
}

} // namespace

extern "C" {

// ---------------------------------------------------------------------------
// reference raylib.cc:25-51
int32_t Raylib_Initialize(void)
{
	{ const char* q = getenv("RAYLIB_QUIET"); if (!(q && q[0] == '1')) printf("Initialize raylib\n"); }   // raylib.cc:27 prints this unconditionally
	LogStart();
	if (!DeviceAvailable()) {
		fprintf(stderr, "Raylib_Initialize: no usable HIP device (gfx950) -- this library has no CPU render path\n");
		return 0;
	}
	Log("Initialize obj loader");
	return 1;
}

int32_t Raylib_Terminate(void)
{
	{ const char* q = getenv("RAYLIB_QUIET"); if (!(q && q[0] == '1')) printf("Terminate raylib\n"); }
	Log("Destroy obj loader");
	LogStop();
	return 0;   // the reference returns 0 here despite its header comment (raylib.cc:50)
}

// ---------------------------------------------------------------------------
// reference raylib.cc:56-113
OBJModelHandle Raylib_LoadOBJModel(const char* objPath)
{
	OBJModel* m = new OBJModel;
	if (LoadOBJ(objPath, *m)) { g_objModels.add(m); return (OBJModelHandle)m; }
	delete m;
	return 0;
}

void Raylib_TransformOBJModel(OBJModelHandle h, float tx, float ty, float tz, float yaw, float pitch, float roll, float sx, float sy, float sz)
{
	if (!h) return;
	TransformOBJ(*(OBJModel*)h, tx, ty, tz, yaw, pitch, roll, sx, sy, sz);
}

void Raylib_FinalizeOBJModel(OBJModelHandle h)
{
	if (!h) return;
	((OBJModel*)h)->finalized = true;   // locks geometry (reference geom/static_mesh.cc:80-95); the BVH is built per scene
}

int32_t Raylib_UnloadOBJModel(OBJModelHandle h)
{
	OBJModel* m = (OBJModel*)h;
	if (g_objModels.eraseFirst(m)) { delete m; return 1; }
	return 0;
}

ImageHandle Raylib_LoadImage(const char* filepath)
{
	Image* img = LoadImageFile(filepath);
	if (!img) return 0;   // the reference registers a null image here (raylib.cc:108-113); returning NULL as its header documents
	g_images.add(img);
	return (ImageHandle)img;
}

// ---------------------------------------------------------------------------
// reference raylib.cc:118-179
CameraHandle Raylib_CreateCamera(void)
{
	Camera* c = new Camera;   // the reference leaves a default camera uninitialised (camera.h:14-21); this one is valid
	c->UpdateInternal();
	g_cameras.add(c);
	return (CameraHandle)c;
}
void Raylib_CameraSetPosition(CameraHandle h, float x, float y, float z) { Camera* c = (Camera*)h; if (!c) return; c->origin = F3(x, y, z); c->UpdateInternal(); }
void Raylib_CameraSetLookAt(CameraHandle h, float x, float y, float z) { Camera* c = (Camera*)h; if (!c) return; c->lookAt = F3(x, y, z); c->UpdateInternal(); }
void Raylib_CameraSetPerspective(CameraHandle h, float fovY, float aspect) { Camera* c = (Camera*)h; if (!c) return; c->fovY_degrees = fovY; c->aspectWH = aspect; c->UpdateInternal(); }
void Raylib_CameraSetLens(CameraHandle h, float aperture, float focal) { Camera* c = (Camera*)h; if (!c) return; c->aperture = aperture; c->focalDistance = focal; c->UpdateInternal(); }
void Raylib_CameraSetMotion(CameraHandle h, float t0, float t1) { Camera* c = (Camera*)h; if (!c) return; c->beginTime = t0; c->endTime = t1; c->UpdateInternal(); }
void Raylib_CameraCopy(CameraHandle src, CameraHandle dst) { if (!src || !dst) return; *(Camera*)dst = *(Camera*)src; }
int32_t Raylib_DestroyCamera(CameraHandle h)
{
	Camera* c = (Camera*)h;
	if (g_cameras.eraseFirst(c)) { delete c; return 1; }
	return 0;
}

// ---------------------------------------------------------------------------
// reference raylib.cc:181-203
ImageHandle Raylib_CreateImage(uint32_t width, uint32_t height)
{
	Image* img = new Image;
	img->Reallocate(width, height, 0.0f, 0.0f, 0.0f, 0.0f);   // Image2D(w, h, 0x0): ARGB 0 -> all channels 0
	g_images.add(img);
	return (ImageHandle)img;
}

void Raylib_DumpImageData(ImageHandle h, float* outDest)
{
	Image* img = (Image*)h;
	if (!img || !outDest) return;
	// a frame that lives on the device (Raylib_Render / Raylib_PostProcess left it there): packed to RGB there, 25 MB instead of 33 over the bus, through pinned staging
	if (img->hostStale && img->devValid && DeviceDumpRGB(*img, outDest)) return;
	img->SyncHost();   // the one read-back of a rendered / post-processed frame
	const size_t n = (size_t)img->width * img->height;
	for (size_t k = 0; k < n; ++k) {   // reference render/image.cc:121-135: packed RGB, row-major
		outDest[3 * k + 0] = img->rgba[4 * k + 0];
		outDest[3 * k + 1] = img->rgba[4 * k + 1];
		outDest[3 * k + 2] = img->rgba[4 * k + 2];
	}
}

int32_t Raylib_DestroyImage(ImageHandle h)
{
	Image* img = (Image*)h;
	if (g_images.eraseFirst(img)) { delete img; return 1; }
	return 0;
}

// ---------------------------------------------------------------------------
// reference raylib.cc:205-283
SceneHandle Raylib_CreateScene(void)
{
	Scene* s = new Scene;
	g_scenes.add(s);
	return (SceneHandle)s;
}

void Raylib_AddSceneElement(SceneHandle sh, SceneElementHandle eh)
{
	// The reference casts the handle to its C++ `Hitable*` (raylib.cc:258-262): a C++-ABI contract (vtables, class
	// layouts), not a C one.  Elements made by RaylibAMD_CreateSphere / Cube / Triangle are accepted; see INTEGRATION.md.
	Scene* s = (Scene*)sh; SceneElement* e = (SceneElement*)eh;
	if (!s || !e) return;
	if (!g_elements.contains(e)) {
		Log("Raylib_AddSceneElement: not an element created by this library (foreign C++ Hitable objects are not supported)");
		return;
	}
	if (!s->finalized) s->elements.push_back(e);   // reference geom/scene.cc:15-21: ignored after Finalize
}

void Raylib_AddOBJModelToScene(SceneHandle sh, OBJModelHandle oh)
{
	Scene* s = (Scene*)sh; OBJModel* m = (OBJModel*)oh;
	if (!s || !m) return;
	if (!s->finalized) s->models.push_back(m);   // reference geom/scene.cc:15-21: ignored after Finalize
}

void Raylib_SetSkyPanorama(SceneHandle sh, ImageHandle ih)
{
	Scene* s = (Scene*)sh;
	if (!s) return;
	// reference geom/scene.h keeps the handle and renderer.cc:159-176 reads the image through it at every miss: the panorama can be
	// set or replaced after Raylib_FinalizeScene and its pixels are those of render time.  Triangles and BVH are not touched.
	s->sky = (Image*)ih;
}
void Raylib_SetSunIlluminance(SceneHandle sh, float r, float g, float b)
{
	Scene* s = (Scene*)sh;
	if (!s) return;
	s->sunIlluminance = F3(r, g, b);
	ReleaseDeviceCopy(s);
}
void Raylib_SetSunDirection(SceneHandle sh, float x, float y, float z)
{
	Scene* s = (Scene*)sh;
	if (!s) return;
	s->sunDirection = normalize(F3(x, y, z));   // reference geom/scene.h:20
	ReleaseDeviceCopy(s);
}
void Raylib_FinalizeScene(SceneHandle sh)
{
	Scene* s = (Scene*)sh;
	if (!s) return;
	s->Finalize();
}
int32_t Raylib_DestroyScene(SceneHandle sh)
{
	Scene* s = (Scene*)sh;
	if (g_scenes.eraseFirst(s)) { delete s; return 1; }
	return 0;
}

// ---------------------------------------------------------------------------
// reference raylib.cc:231-239 -> render/renderer.cc:273-356
void Raylib_Render(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, ImageHandle outMainImage)
{
	Image* img = (Image*)outMainImage;
	if (!settings || !img) { Log("Raylib_Render: null argument"); return; }
	if (settings->viewportWidth != img->width || settings->viewportHeight != img->height)
		img->Reallocate(settings->viewportWidth, settings->viewportHeight, 0.0f, 0.0f, 0.0f, 1.0f);   // renderer.cc:292-296
	if ((size_t)img->width * img->height == 0) return;
	// The frame stays on the device: Raylib_PostProcess works on it there, and the host pixels are fetched when somebody asks for them
	// (Raylib_DumpImageData, Raylib_WriteImageToDisk, ...).  A render that is REFUSED (scene not finalized, invalid mode, no device)
	// must leave the image as it was -- including a previous frame that still lives only on the device (hostStale): the image's state
	// changes only on success.  (Every refusal happens before anything is enqueued; DeviceImagePixels keeps a buffer that is large enough.)
	void* dev = DeviceImagePixels(*img);
	if (!RenderInternal(settings, (Scene*)scene, (Camera*)camera, 0, 1, dev, dev ? nullptr : img->rgba.data()))
		fprintf(stderr, "Raylib_Render: FAILED (no HIP device or invalid arguments); the image was not written\n");
	else { img->devValid = (dev != nullptr); img->hostStale = (dev != nullptr); img->Touch(); }
}

int32_t Raylib_Denoise(ImageHandle mainImage, int32_t bHDR, ImageHandle albedo, ImageHandle normal, ImageHandle out)
{
	// reference render/renderer.cc:358-370 returns false when OIDN is not integrated (every non-Windows build); here the same unless the
	// denoiser switch is on (RaylibAMD_EnableDenoiser, RAYLIB_DENOISER=1), and then the a-trous filter of csrc/rl_denoise.hip with its defaults
	if (!DenoiserEnabled()) return 0;
	return RaylibAMD_Denoise(mainImage, bHDR, albedo, normal, out, nullptr);
}

void Raylib_PostProcess(ImageHandle h)
{
	Image* img = (Image*)h;
	if (!img) return;
	if (!DevicePostProcess(*img)) {
		Log("Raylib_PostProcess: no HIP device, running on the host");
		PostProcessHost(*img);
		img->Touch();
	}
}

int32_t Raylib_IsDenoiserSupported(void) { return DenoiserEnabled() ? RaylibAMD_DeviceAvailable() : 0; }

// ---------------------------------------------------------------------------
// reference raylib.cc:298-331
const char* Raylib_GetRenderModeString(uint32_t auxMode)
{
	static const char* names[] = { "Default", "Albedo", "SurfaceNormal", "MicrosurfaceNormal", "Texcoord", "Emission", "Reflectance" };
	return auxMode < RAYLIB_RENDERMODE_MAX ? names[auxMode] : nullptr;
}

int32_t Raylib_WriteImageToDisk(ImageHandle h, const char* filepath, uint32_t fileType)
{
	if (h == 0 || filepath == nullptr || fileType >= RAYLIB_IMAGEFILETYPE_MAX) return 0;
	return WriteImageFile(*(Image*)h, filepath, fileType) ? 1 : 0;
}

void Raylib_FlushLogThread(void) { LogFlush(); }

// ===========================================================================
// include/raylib_amd.h
// ===========================================================================
void RaylibAMD_SetSeed(uint64_t seed) { std::lock_guard<std::mutex> lk(g_stateMu); g_seed = seed; g_seedSet = true; }
uint64_t RaylibAMD_GetSeed(void) { return CurrentSeed(); }
void RaylibAMD_GetLastStats(RaylibAMDStats* out)
{
	if (!out) return;
	// a whole-frame render over several ranks returns with the frame in flight (rl_rt_render.hip RenderMulti): its counters and times arrive now
	RaylibAMDStats late;
	const bool have = DeviceDrain(&late);
	std::lock_guard<std::mutex> lk(g_stateMu);
	if (have) g_lastStats = late;
	*out = g_lastStats;
}
int32_t RaylibAMD_DeviceAvailable(void) { return DeviceAvailable() ? 1 : 0; }
#ifndef RL_BUILD_ID
#define RL_BUILD_ID "unknown"
#endif
const char* RaylibAMD_BuildId(void) { return RL_BUILD_ID; }

void RaylibAMD_EnableDenoiser(int32_t enable) { std::lock_guard<std::mutex> lk(g_stateMu); g_denoiser = enable ? 1 : 0; }

int32_t RaylibAMD_Denoise(ImageHandle mainImage, int32_t bHDR, ImageHandle albedo, ImageHandle normal, ImageHandle out, const RaylibAMDDenoiseParams* params)
{
	Image* m = (Image*)mainImage; Image* a = (Image*)albedo; Image* n = (Image*)normal; Image* o = (Image*)out;
	const RaylibAMDDenoiseParams& P = params ? *params : kDenoiseDefaults;
	if (!m || !o) { Log("RaylibAMD_Denoise: null main or output image"); return 0; }
	for (Image* g : { a, n })
		if (g && (g->width != m->width || g->height != m->height)) { Log("RaylibAMD_Denoise: a guide's size differs from the main image's"); return 0; }
	if (!DenoiseParamsValid(P)) { Log("RaylibAMD_Denoise: parameters out of range"); return 0; }
	if (!DeviceAvailable()) return 0;
	// a whole-frame render over several ranks returns with the frame in flight: wait for it, and keep its numbers for RaylibAMD_GetLastStats
	RaylibAMDStats late;
	if (DeviceDrain(&late)) { std::lock_guard<std::mutex> lk(g_stateMu); g_lastStats = late; }
	return DeviceDenoise(*m, bHDR != 0, a, n, *o, P) ? 1 : 0;
}

int32_t RaylibAMD_DenoiseHost(uint32_t width, uint32_t height, const float* colorRGBA, int32_t bHDR, const float* albedoRGBA, const float* normalRGBA,
                              const RaylibAMDDenoiseParams* params, float* outRGBA)
{
	const RaylibAMDDenoiseParams& P = params ? *params : kDenoiseDefaults;
	if (!colorRGBA || !outRGBA || !DenoiseParamsValid(P)) return 0;
	DenoiseHost(width, height, colorRGBA, bHDR != 0, albedoRGBA, normalRGBA, P, outRGBA);
	return 1;
}

RaylibAMDProgressiveHandle RaylibAMD_BeginProgressive(const RendererSettings* settings, SceneHandle scene, CameraHandle camera,
                                                      ImageHandle out, const RaylibAMDProgressiveParams* params)
{
	Scene* s = (Scene*)scene; Camera* c = (Camera*)camera; Image* img = (Image*)out;
	if (!settings || !s || !c || !img) { Log("RaylibAMD_BeginProgressive: null argument"); return 0; }
	if (settings->renderMode != RAYLIB_RENDERMODE_Default) { Log("RaylibAMD_BeginProgressive: render mode %u is not the path-traced one", settings->renderMode); return 0; }
	if (params && !ProgressiveParamsValid(*params)) { Log("RaylibAMD_BeginProgressive: parameters out of range"); return 0; }
	if ((uint64_t)settings->viewportWidth * settings->viewportHeight == 0) { Log("RaylibAMD_BeginProgressive: empty viewport"); return 0; }
	if (!s->finalized) { Log("RaylibAMD_BeginProgressive: scene was not finalized (Raylib_FinalizeScene)"); return 0; }
	if (!DeviceAvailable()) return 0;
	if (!PrepareRender("RaylibAMD_BeginProgressive", settings, s, c)) return 0;
	if (settings->viewportWidth != img->width || settings->viewportHeight != img->height)
		img->Reallocate(settings->viewportWidth, settings->viewportHeight, 0.0f, 0.0f, 0.0f, 1.0f);   // as Raylib_Render
	if (!DeviceImagePixels(*img)) return 0;
	RenderRequest req;
	req.settings = *settings;
	req.camera = c->ToDevice();
	req.seed = CurrentSeed();
	req.cellFirst = 0; req.cellStride = 1;
	req.outDevice = nullptr; req.outHostRGBA = nullptr;
	ProgressiveSession* d = DeviceProgressiveBegin(*s, req, params ? params->threshold : 0.0f, params ? params->minSamples : 2u);
	if (!d) return 0;
	Progressive* p = new Progressive{ s, img, settings->viewportWidth, settings->viewportHeight, d };
	g_progressive.add(p);
	return (RaylibAMDProgressiveHandle)p;
}

int32_t RaylibAMD_ProgressiveStep(RaylibAMDProgressiveHandle h, uint32_t samples)
{
	Progressive* p = (Progressive*)h;
	if (!p || !g_progressive.contains(p)) { Log("RaylibAMD_ProgressiveStep: unknown session"); return -1; }
	if (samples == 0) { Log("RaylibAMD_ProgressiveStep: no samples asked for"); return -1; }
	if (!g_scenes.contains(p->scene)) { Log("RaylibAMD_ProgressiveStep: the session's scene was destroyed"); return -1; }
	if (!g_images.contains(p->out)) { Log("RaylibAMD_ProgressiveStep: the session's image was destroyed"); return -1; }
	if (p->out->width != p->width || p->out->height != p->height) { Log("RaylibAMD_ProgressiveStep: the session's image was resized; it is unchanged"); return -1; }
	if (p->scene->sky && !g_images.contains(p->scene->sky)) { Log("RaylibAMD_ProgressiveStep: the scene's sky panorama was destroyed; the image is unchanged"); return -1; }
	void* dev = DeviceImagePixels(*p->out);
	if (!dev) return -1;
	RaylibAMDStats stats; memset(&stats, 0, sizeof(stats));
	bool rendered = false;
	const int32_t r = DeviceProgressiveStep(*p->dev, samples, dev, stats, rendered);
	if (rendered) {
		p->out->devValid = true; p->out->hostStale = true; p->out->Touch();
		std::lock_guard<std::mutex> lk(g_stateMu);
		g_lastStats = stats;
	}
	return r;
}

int32_t RaylibAMD_ProgressiveExport(RaylibAMDProgressiveHandle h, uint32_t* cellSamples, uint8_t* cellStopped, float* sumY, float* sumY2)
{
	Progressive* p = (Progressive*)h;
	if (!p || !g_progressive.contains(p)) return 0;
	return DeviceProgressiveExport(*p->dev, cellSamples, cellStopped, sumY, sumY2) ? 1 : 0;
}

int32_t RaylibAMD_EndProgressive(RaylibAMDProgressiveHandle h)
{
	Progressive* p = (Progressive*)h;
	if (!p || !g_progressive.eraseFirst(p)) return 0;
	DeviceProgressiveEnd(p->dev);
	delete p;
	return 1;
}

int32_t RaylibAMD_ProgressiveDecideHost(uint32_t width, uint32_t height, const uint32_t* cellSamples, const float* sumY,
                                        const float* sumY2, const RaylibAMDProgressiveParams* params, uint8_t* outStop)
{
	if (!cellSamples || !sumY || !sumY2 || !outStop) return 0;
	if (params && !ProgressiveParamsValid(*params)) return 0;
	const float threshold = params ? params->threshold : 0.0f;
	const uint32_t minSamples = params ? params->minSamples : 2u;
	const uint32_t cellsX = (width + 7) / 8, cellsY = (height + 7) / 8;
	for (uint32_t cy = 0; cy < cellsY; ++cy)
		for (uint32_t cx = 0; cx < cellsX; ++cx) {
			const uint32_t n = cellSamples[(size_t)cy * cellsX + cx];
			float e = 0.0f;
			for (uint32_t y = cy * 8; y < std::min(height, cy * 8 + 8); ++y)
				for (uint32_t x = cx * 8; x < std::min(width, cx * 8 + 8); ++x) {
					const float v = ProgressivePixelError(sumY[(size_t)y * width + x], sumY2[(size_t)y * width + x], n);
					e = e < v ? v : e;
				}
			outStop[(size_t)cy * cellsX + cx] = ProgressiveCellStops(e, n, threshold, minSamples) ? 1 : 0;
		}
	return 1;
}

int32_t RaylibAMD_ProgressiveCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const uint8_t* emptyOrNull, uint32_t numCells,
                                         uint32_t width, uint32_t height, uint32_t* outLive, uint32_t* outTrace, uint32_t outCounts[4])
{
	if (!live || !stopped || !outLive || !outTrace || !outCounts) return 0;
	if (width == 0 || height == 0 || (uint64_t)((width + 7ull) / 8) * ((height + 7ull) / 8) != numCells || numLive > numCells) return 0;
	for (uint32_t i = 0; i < numLive; ++i) if (live[i] >= numCells) return 0;   // (the kernel indexes stopped and empty by the entries)
	return DeviceProgressiveCompactTest(live, numLive, stopped, emptyOrNull, numCells, width, height, outLive, outTrace, outCounts) ? 1 : 0;
}

int32_t RaylibAMD_RenderViews(const RendererSettings* settings, SceneHandle scene, const CameraHandle* cameras, int32_t count, const ImageHandle* outImages)
{
	static const char* who = "RaylibAMD_RenderViews";
	Scene* s = (Scene*)scene;
	if (!outImages) { Log("%s: null argument", who); return 0; }
	if (!ViewsArgsValid(who, settings, s, cameras, count, outImages)) return 0;
	if (!DeviceAvailable()) return 0;
	// Every refusal is behind us: the images take the viewport's size and device storage (as Raylib_Render), and the batch's frames are copied there
	std::vector<void*> dev((size_t)count);
	for (int32_t v = 0; v < count; ++v) {
		Image* img = (Image*)outImages[v];
		if (settings->viewportWidth != img->width || settings->viewportHeight != img->height)
			img->Reallocate(settings->viewportWidth, settings->viewportHeight, 0.0f, 0.0f, 0.0f, 1.0f);
		dev[(size_t)v] = DeviceImagePixels(*img);
		if (!dev[(size_t)v]) { Log("%s: no device storage for image %d", who, v); return 0; }
	}
	if (!RenderViewsInternal(who, settings, s, cameras, count, nullptr, dev.data())) return 0;
	for (int32_t v = 0; v < count; ++v) { Image* img = (Image*)outImages[v]; img->devValid = true; img->hostStale = true; img->Touch(); }
	return 1;
}

int32_t RaylibAMD_RenderViewsDevice(const RendererSettings* settings, SceneHandle scene, const CameraHandle* cameras, int32_t count, void* outDevice)
{
	static const char* who = "RaylibAMD_RenderViewsDevice";
	Scene* s = (Scene*)scene;
	if (!ViewsArgsValid(who, settings, s, cameras, count, nullptr)) return 0;
	if (!DeviceAvailable()) return 0;
	return RenderViewsInternal(who, settings, s, cameras, count, outDevice, nullptr) ? 1 : 0;
}

uint32_t RaylibAMD_NumCells(uint32_t w, uint32_t h) { return ((w + 7) / 8) * ((h + 7) / 8); }
uint64_t RaylibAMD_CellBufferFloats(uint32_t w, uint32_t h, uint32_t cellFirst, uint32_t cellStride)
{
	if (cellStride <= 1 && cellFirst == 0) return (uint64_t)w * h * 4;
	const uint32_t n = RaylibAMD_NumCells(w, h);
	const uint32_t local = cellFirst < n ? (n - cellFirst + cellStride - 1) / cellStride : 0;
	return (uint64_t)local * 64 * 4;
}

int32_t RaylibAMD_RenderDevice(const RendererSettings* settings, SceneHandle scene, CameraHandle camera,
                               uint32_t cellFirst, uint32_t cellStride, void* outDevice)
{
	if (!settings || settings->viewportWidth == 0 || settings->viewportHeight == 0) return 0;
	// (a buffer of the caller's: nothing of the library's protects it while a frame is in flight, so this entry is synchronous on every path -- rl_rt_render.hip RenderMulti)
	return RenderInternal(settings, (Scene*)scene, (Camera*)camera, cellFirst, cellStride ? cellStride : 1, outDevice, nullptr, outDevice != nullptr) ? 1 : 0;
}

int32_t RaylibAMD_RenderCellsHost(const RendererSettings* settings, SceneHandle scene, CameraHandle camera,
                                  uint32_t cellFirst, uint32_t cellStride, float* outHost)
{
	if (!settings || settings->viewportWidth == 0 || settings->viewportHeight == 0 || !outHost) return 0;
	return RenderInternal(settings, (Scene*)scene, (Camera*)camera, cellFirst, cellStride ? cellStride : 1, nullptr, outHost) ? 1 : 0;
}

MaterialHandle RaylibAMD_CreateMaterial(int32_t type, const float albedo[3], float roughness, float metallic,
                                        const float emissive[3], float ior, const float transmission[3], float fuzziness)
{
	if (type < 0 || type > MAT_DIFFUSE_LIGHT) return 0;
	MaterialObj* M = new MaterialObj; memset(&M->m, 0, sizeof(M->m));
	HostMaterial& m = M->m;
	m.type = type;
	for (int i = 0; i < 5; ++i) m.tex[i] = -1;
	auto clamp01 = [](float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); };
	for (int i = 0; i < 3; ++i) {
		m.albedo[i] = albedo ? albedo[i] : 0.0f;
		m.emissive[i] = emissive ? emissive[i] : 0.0f;
		m.transmission[i] = transmission ? transmission[i] : 1.0f;
	}
	m.roughness = roughness; m.metallic = metallic; m.ior = ior; m.fuzziness = fuzziness;
	// constructor-side clamps of the reference (render/material.h:79-82,107,236-238)
	if (type == MAT_LAMBERTIAN) for (int i = 0; i < 3; ++i) m.albedo[i] = clamp01(m.albedo[i]);
	if (type == MAT_METAL) m.fuzziness = clamp01(m.fuzziness);
	if (type == MAT_MICROFACET) { for (int i = 0; i < 3; ++i) m.albedo[i] = clamp01(m.albedo[i]); m.roughness = clamp01(m.roughness); m.metallic = clamp01(m.metallic); }
	g_materials.add(M);
	return (MaterialHandle)M;
}
int32_t RaylibAMD_DestroyMaterial(MaterialHandle h)
{
	MaterialObj* M = (MaterialObj*)h;
	if (g_materials.eraseFirst(M)) { delete M; return 1; }
	return 0;
}
static SceneElement* NewElement(PrimKind kind, MaterialHandle mh)
{
	MaterialObj* M = (MaterialObj*)mh;
	if (!M || !g_materials.contains(M)) return nullptr;
	SceneElement* e = new SceneElement; memset(e, 0, sizeof(*e));
	e->kind = kind; e->material = M;
	g_elements.add(e);
	return e;
}
SceneElementHandle RaylibAMD_CreateSphere(float cx, float cy, float cz, float radius, MaterialHandle material)
{
	SceneElement* e = NewElement(PRIM_SPHERE, material);
	if (!e) return 0;
	e->center = F3(cx, cy, cz); e->radius = radius;
	return (SceneElementHandle)e;
}
SceneElementHandle RaylibAMD_CreateCube(const float mn[3], const float mx[3], float timeStartMove, const float velocity[3], MaterialHandle material)
{
	if (!mn || !mx) return 0;
	SceneElement* e = NewElement(PRIM_CUBE, material);
	if (!e) return 0;
	e->minBounds = F3(mn[0], mn[1], mn[2]); e->maxBounds = F3(mx[0], mx[1], mx[2]); e->timeStartMove = timeStartMove;
	e->velocity = velocity ? F3(velocity[0], velocity[1], velocity[2]) : F3(0, 0, 0);
	return (SceneElementHandle)e;
}
SceneElementHandle RaylibAMD_CreateTriangle(const float v0[3], const float v1[3], const float v2[3],
                                            const float n0[3], const float n1[3], const float n2[3], const float uv[6], MaterialHandle material)
{
	if (!v0 || !v1 || !v2 || !n0 || !n1 || !n2) return 0;
	SceneElement* e = NewElement(PRIM_TRIANGLE, material);
	if (!e) return 0;
	HostTriangle& t = e->tri;
	t.v0 = F3(v0[0], v0[1], v0[2]); t.v1 = F3(v1[0], v1[1], v1[2]); t.v2 = F3(v2[0], v2[1], v2[2]);
	t.n0 = F3(n0[0], n0[1], n0[2]); t.n1 = F3(n1[0], n1[1], n1[2]); t.n2 = F3(n2[0], n2[1], n2[2]);
	if (uv) { t.s0 = uv[0]; t.t0 = uv[1]; t.s1 = uv[2]; t.t1 = uv[3]; t.s2 = uv[4]; t.t2 = uv[5]; }
	return (SceneElementHandle)e;
}
int32_t RaylibAMD_DestroySceneElement(SceneElementHandle h)
{
	SceneElement* e = (SceneElement*)h;
	if (g_elements.eraseFirst(e)) { delete e; return 1; }
	return 0;
}

int32_t RaylibAMD_EvalScatter(SceneHandle sh, int32_t material, const float* records, int32_t n, uint64_t seed, float* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !records || !out || material < 0 || material >= (int32_t)s->materials.size()) return 0;
	return DeviceEvalHook(0, s, nullptr, material, 0, records, n, seed, out) ? 1 : 0;
}
int32_t RaylibAMD_EvalCameraRays(CameraHandle ch, const float* uv, int32_t n, uint64_t seed, float* out)
{
	Camera* c = (Camera*)ch;
	if (!c || !uv || !out) return 0;
	const DCamera d = c->ToDevice();
	return DeviceEvalHook(1, nullptr, &d, 0, 0, uv, n, seed, out) ? 1 : 0;
}
int32_t RaylibAMD_CullCells(CameraHandle ch, const float* bounds, const float* sunIlluminance, const float* sunDirection, int32_t width, int32_t height,
                            uint8_t* outEmpty, float* outConstant)
{
	Camera* c = (Camera*)ch;
	if (!c || !bounds || width <= 0 || height <= 0) return -1;
	CullScene cs;
	for (int k = 0; k < 3; ++k) { cs.boundsMin[k] = bounds[k]; cs.boundsMax[k] = bounds[3 + k]; }
	cs.boundsValid = true;
	if (sunIlluminance && sunDirection) {
		for (int k = 0; k < 3; ++k) { cs.sunIlluminance[k] = sunIlluminance[k]; cs.sunDirection[k] = sunDirection[k]; }
		cs.hasSun = !(sunIlluminance[0] == 0.0f && sunIlluminance[1] == 0.0f && sunIlluminance[2] == 0.0f);
	}
	const uint32_t W = (uint32_t)width, H = (uint32_t)height, cellsX = (W + 7) / 8, cellsY = (H + 7) / 8;
	CullResult r;
	if (!CullCells(cs, c->ToDevice(), 1, 0.0f, W, H, cellsX, 0, 1, cellsX * cellsY, r)) {
		if (outEmpty) memset(outEmpty, 0, (size_t)cellsX * cellsY);
		return r.empty.empty() ? -1 : 0;   // not eligible, or eligible with nothing to drop
	}
	if (outEmpty) memcpy(outEmpty, r.empty.data(), (size_t)cellsX * cellsY);
	if (outConstant) { outConstant[0] = r.L[0]; outConstant[1] = r.L[1]; outConstant[2] = r.L[2]; }
	return (int32_t)(cellsX * cellsY - (uint32_t)r.active.size());
}
int32_t RaylibAMD_EvalTexture(SceneHandle sh, int32_t texture, int32_t bSRGB, const float* uv, int32_t n, float* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !uv || !out || texture < 0 || texture >= (int32_t)s->textures.size()) return 0;
	return DeviceEvalHook(2, s, nullptr, texture, bSRGB, uv, n, 0, out) ? 1 : 0;
}

int32_t RaylibAMD_EvalDeviceMath(int32_t fn, const float* x, const float* y, int32_t n, float* out)
{
	if (!x || !out) return 0;
	return DeviceEvalMath(fn, x, y, n, out) ? 1 : 0;
}

int32_t RaylibAMD_VerifyExactMath(int32_t which, uint64_t* outMismatches, uint64_t* outFirstBits)
{
	if (which < 0 || which > 4) return 0;
	return DeviceVerifyExactMath(which, outMismatches, outFirstBits) ? 1 : 0;
}

// outInterval: lo, hi and the compiled RL_SAMPLER_C_MIN as bit patterns (the agreeing interval begins one pattern above the largest differing one and ends one below the branch's threshold)
int32_t RaylibAMD_VerifySamplerRanged(int32_t mode, uint64_t* outMismatches, uint64_t* outFirstBits, uint32_t* outInterval, uint64_t* outOutside)
{
	if (mode < 0 || mode > 3) return 0;
	uint64_t out[6] = { 0, 0, 0, 0, 0, 0 };
	if (!DeviceVerifySamplerRanged(mode, out)) return 0;
	if (outMismatches) *outMismatches = out[0];
	if (outFirstBits) *outFirstBits = out[1];
	if (outInterval) { outInterval[0] = (uint32_t)out[2] + 1u; outInterval[1] = (uint32_t)out[5] - 1u; outInterval[2] = (uint32_t)out[4]; }
	if (outOutside) *outOutside = out[3];
	return 1;
}

int32_t RaylibAMD_VerifyNormalizeRanged(int32_t mode, uint64_t* outMismatches, uint64_t* outFirst, uint64_t* outFirstOutside, uint64_t* outCount)
{
	if (mode < 0 || mode > 2) return 0;
	uint64_t out[4] = { 0, 0, 0, 0 };
	if (!DeviceVerifyNormalizeRanged(mode, out)) return 0;
	if (outMismatches) *outMismatches = out[0];
	if (outFirst) *outFirst = out[1];
	if (outFirstOutside) *outFirstOutside = out[2];
	if (outCount) *outCount = out[3];
	return 1;
}

int32_t RaylibAMD_VerifyLazyRefl(uint32_t n, uint64_t seed, uint64_t* outEvents, uint64_t* outUnsafe, uint64_t* outGuardFailed)
{
	uint64_t out[3] = { 0, 0, 0 };
	if (!DeviceVerifyLazyRefl(n, seed, out)) return 0;
	if (outEvents) *outEvents = out[0];
	if (outUnsafe) *outUnsafe = out[1];
	if (outGuardFailed) *outGuardFailed = out[2];
	return 1;
}

int32_t RaylibAMD_VerifyLazyPdf(uint32_t n, uint64_t seed, uint64_t* outEvents, uint64_t* outWrong, uint64_t* outRefused)
{
	uint64_t out[3] = { 0, 0, 0 };
	if (!DeviceVerifyLazyPdf(n, seed, out)) return 0;
	if (outEvents) *outEvents = out[0];
	if (outWrong) *outWrong = out[1];
	if (outRefused) *outRefused = out[2];
	return 1;
}

int32_t RaylibAMD_ClosestHit(SceneHandle sh, const float* rays, int32_t n, float tMin, void* outHits)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !rays || !outHits) return 0;
	return DeviceClosestHit(*s, rays, n, tMin, outHits) ? 1 : 0;
}

// RaylibAMD_TraceRays / RaylibAMD_TraceRaysDevice: the refusals of include/raylib_amd.h (ray queries take spheres and cubes too), then the device
static int32_t TraceRaysInternal(const char* who, SceneHandle sh, int32_t kind, const RaylibAMDRay* rays, int32_t n, float rayTime, void* out, int32_t* outPrim,
                                 bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (!s || n < 0 || (n > 0 && (!rays || !out))) { Log("%s: null argument", who); return 0; }
	if (!s->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return 0; }
	if (kind < RAYLIB_AMD_QUERY_ANY || kind > RAYLIB_AMD_QUERY_SURFACE) { Log("%s: unknown query kind %d", who, kind); return 0; }
	if (!std::isfinite(rayTime)) { Log("%s: ray time %g is not finite", who, rayTime); return 0; }
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) {
		if (s->hasMovingCubes && !(rayTime >= s->accelT0 && rayTime <= s->accelT1)) {
			// moving cubes: their boxes must cover the motion up to this ray time (as a render rebuilds them for its camera's shutter interval)
			const float t0 = std::min(s->accelT0, rayTime), t1 = std::max(s->accelT1, rayTime);
			ReleaseDeviceCopy(s);
			if (!s->BuildAccel(t0, t1)) { Log("%s: the acceleration structure could not be rebuilt for ray time %g", who, rayTime); return false; }
		}
		return DeviceTraceRays(*s, kind, rays, n, rayTime, out, outPrim, hostMem, stream, stats);
	});
}
int32_t RaylibAMD_TraceRays(SceneHandle sh, int32_t kind, const RaylibAMDRay* rays, int32_t n, float rayTime, void* out, int32_t* outPrim)
{
	return TraceRaysInternal("RaylibAMD_TraceRays", sh, kind, rays, n, rayTime, out, outPrim, true, nullptr);
}
int32_t RaylibAMD_TraceRaysDevice(SceneHandle sh, int32_t kind, const RaylibAMDRay* rays, int32_t n, float rayTime, void* out, int32_t* outPrim, void* stream)
{
	return TraceRaysInternal("RaylibAMD_TraceRaysDevice", sh, kind, rays, n, rayTime, out, outPrim, false, stream);
}
int32_t RaylibAMD_PlanRayQuery(SceneHandle sh, int32_t kind, RaylibAMDQueryPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out || kind < RAYLIB_AMD_QUERY_ANY || kind > RAYLIB_AMD_QUERY_SURFACE) return 0;
	const QueryPlan p = PlanQuery(*s, kind, ReadRenderKnobs());
	return ExportPlan(p, p.prims, p.early, out);
}

// RaylibAMD_RenderGBuffer / RaylibAMD_RenderGBufferDevice / RaylibAMD_RenderGuides / RaylibAMD_PlanGBuffer (statements G1 to G6): the refusals every entry
// shares (G6; samplesPerPixel, maxPathLength and renderMode are not read), then, as a render, the scene's boxes for the camera's shutter interval, then the device
static bool GBufferArgsValid(const char* who, const RendererSettings* settings, const Scene* s, const Camera* c)
{
	if (!settings || !s || !c) { Log("%s: null argument", who); return false; }
	const uint64_t pixels = (uint64_t)settings->viewportWidth * settings->viewportHeight;
	if (pixels == 0 || pixels > 0x7fffffffull) { Log("%s: a frame of %u x %u pixels (1 .. 2^31 - 1)", who, settings->viewportWidth, settings->viewportHeight); return false; }
	if (!std::isfinite(settings->rayTMin)) { Log("%s: rayTMin %g is not finite", who, settings->rayTMin); return false; }
	if (!s->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return false; }
	if (s->bvh.depth > 64) { Log("%s: BVH depth %u exceeds the traversal stack (64)", who, s->bvh.depth); return false; }
	return true;
}
static int32_t RenderGBufferInternal(const char* who, const RendererSettings* settings, SceneHandle sh, CameraHandle ch, const RaylibAMDGBufferPlanes* planes, bool hostMem,
                                     void* stream)
{
	Scene* s = (Scene*)sh; Camera* c = (Camera*)ch;
	if (!planes) { Log("%s: null argument", who); return 0; }
	if (!GBufferArgsValid(who, settings, s, c)) return 0;
	if (!planes->hit && !planes->surface && !planes->albedo && !planes->surfaceNormal && !planes->microNormal && !planes->texcoord && !planes->emission) {
		Log("%s: no plane asked for", who); return 0;
	}
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) {
		if (!PrepareShutter(who, s, c)) return false;
		return DeviceRenderGBuffer(*s, *settings, c->ToDevice(), CurrentSeed(), *planes, hostMem, stream, stats);
	});
}
int32_t RaylibAMD_RenderGBuffer(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, const RaylibAMDGBufferPlanes* hostPlanes)
{
	return RenderGBufferInternal("RaylibAMD_RenderGBuffer", settings, scene, camera, hostPlanes, true, nullptr);
}
int32_t RaylibAMD_RenderGBufferDevice(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, const RaylibAMDGBufferPlanes* devicePlanes, void* stream)
{
	return RenderGBufferInternal("RaylibAMD_RenderGBufferDevice", settings, scene, camera, devicePlanes, false, stream);
}
int32_t RaylibAMD_RenderGuides(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, ImageHandle albedo, ImageHandle microNormal)
{
	static const char* who = "RaylibAMD_RenderGuides";
	Image* imgs[2] = { (Image*)albedo, (Image*)microNormal };
	if (!imgs[0] && !imgs[1]) { Log("%s: no image given", who); return 0; }
	if (imgs[0] == imgs[1]) { Log("%s: the same image given twice", who); return 0; }
	for (Image* img : imgs) if (img && !g_images.contains(img)) { Log("%s: unknown image", who); return 0; }
	if (!GBufferArgsValid(who, settings, (Scene*)scene, (Camera*)camera)) return 0;   // (before an image is touched)
	if (!DeviceAvailable()) return 0;
	// a whole-frame render over several ranks may still be writing one of these images: wait for it, and keep its numbers for RaylibAMD_GetLastStats
	RaylibAMDStats late;
	if (DeviceDrain(&late)) { std::lock_guard<std::mutex> lk(g_stateMu); g_lastStats = late; }
	void* dev[2] = { nullptr, nullptr };
	for (int k = 0; k < 2; ++k) {
		Image* img = imgs[k];
		if (!img) continue;
		if (settings->viewportWidth != img->width || settings->viewportHeight != img->height)
			img->Reallocate(settings->viewportWidth, settings->viewportHeight, 0.0f, 0.0f, 0.0f, 1.0f);   // as Raylib_Render
		dev[k] = DeviceImagePixels(*img);
		if (!dev[k]) { Log("%s: no device storage for an image", who); return 0; }
	}
	RaylibAMDGBufferPlanes planes; memset(&planes, 0, sizeof(planes));
	planes.albedo = (float*)dev[0]; planes.microNormal = (float*)dev[1];
	if (!RenderGBufferInternal(who, settings, scene, camera, &planes, false, nullptr)) return 0;
	for (Image* img : imgs) if (img) { img->devValid = true; img->hostStale = true; img->Touch(); }
	return 1;
}
int32_t RaylibAMD_PlanGBuffer(SceneHandle sh, RaylibAMDQueryPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out) return 0;
	const QueryPlan p = PlanGBuffer(*s, ReadRenderKnobs());
	return ExportPlan(p, p.prims, 0, out);
}

// RaylibAMD_RenderMotion / RaylibAMD_RenderMotionDevice / RaylibAMD_MotionHost / RaylibAMD_PlanMotion (statements T1 to T6): what the params add to the
// G-buffer's refusals -- the range, the positions (a host call's are scanned) and the previous camera, which is `camera` when the params name none
static bool MotionParamsValid(const char* who, const Scene* s, const RaylibAMDMotionParams* p, bool hostMem)
{
	if (!p) { Log("%s: null argument", who); return false; }
	if (p->first < 0 || p->count < 0 || (int64_t)p->first + (int64_t)p->count > (int64_t)s->triangles.size()) {
		Log("%s: triangles [%d, %d + %d) are not the scene's", who, p->first, p->first, p->count); return false;
	}
	if (p->count > 0 && !p->prevPositions) { Log("%s: null previous positions", who); return false; }
	if (hostMem) for (size_t i = 0; i < (size_t)p->count * 9; ++i) if (!std::isfinite(p->prevPositions[i])) { Log("%s: a previous position is not finite", who); return false; }
	if (p->prevCamera && !g_cameras.contains((Camera*)p->prevCamera)) { Log("%s: unknown previous camera", who); return false; }
	return true;
}
static int32_t RenderMotionInternal(const char* who, const RendererSettings* settings, SceneHandle sh, CameraHandle ch, const RaylibAMDMotionParams* params,
                                    const RaylibAMDMotionPlanes* planes, bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh; Camera* c = (Camera*)ch;
	if (!planes) { Log("%s: null argument", who); return 0; }
	if (!GBufferArgsValid(who, settings, s, c)) return 0;
	if (!planes->hit && !planes->motion) { Log("%s: no plane asked for", who); return 0; }
	if (!MotionParamsValid(who, s, params, hostMem)) return 0;
	const Camera* pc = params->prevCamera ? (const Camera*)params->prevCamera : c;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) {
		if (!PrepareShutter(who, s, c)) return false;
		return DeviceRenderMotion(*s, *settings, c->ToDevice(), pc->ToDevice(), CurrentSeed(), params->first, params->count, params->prevPositions, *planes, hostMem, stream, stats);
	});
}
int32_t RaylibAMD_RenderMotion(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, const RaylibAMDMotionParams* params, const RaylibAMDMotionPlanes* hostPlanes)
{
	return RenderMotionInternal("RaylibAMD_RenderMotion", settings, scene, camera, params, hostPlanes, true, nullptr);
}
int32_t RaylibAMD_RenderMotionDevice(const RendererSettings* settings, SceneHandle scene, CameraHandle camera, const RaylibAMDMotionParams* params,
                                     const RaylibAMDMotionPlanes* devicePlanes, void* stream)
{
	return RenderMotionInternal("RaylibAMD_RenderMotionDevice", settings, scene, camera, params, devicePlanes, false, stream);
}
int32_t RaylibAMD_MotionHost(uint32_t width, uint32_t height, SceneHandle sh, CameraHandle ch, const RaylibAMDMotionParams* params, const float* rays, const RaylibAMDHitT* hit,
                             RaylibAMDMotion* outMotion)
{
	static const char* who = "RaylibAMD_MotionHost";
	Scene* s = (Scene*)sh; Camera* c = (Camera*)ch;
	if (!s || !c || !rays || !hit || !outMotion) { Log("%s: null argument", who); return 0; }
	const uint64_t pixels = (uint64_t)width * height;
	if (pixels == 0 || pixels > 0x7fffffffull) { Log("%s: a frame of %u x %u pixels (1 .. 2^31 - 1)", who, width, height); return 0; }
	if (!s->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return 0; }
	if (!MotionParamsValid(who, s, params, true)) return 0;
	MotionHost(width, height, (params->prevCamera ? (const Camera*)params->prevCamera : c)->ToDevice(), params->first, params->count, params->prevPositions, rays, hit, outMotion);
	return 1;
}
int32_t RaylibAMD_PlanMotion(SceneHandle scene, RaylibAMDQueryPlan* out) { return RaylibAMD_PlanGBuffer(scene, out); }

// RaylibAMD_TemporalAccumulate / ...Device / ...Host (statements T7 and T8) and RaylibAMD_TemporalAccumulateMoments / ...Device / ...Host (statements S1 and
// S2): one description of the call (rl_host.h TemporalCall), which every entry fills from its arguments, and the refusals all six share -- the moments' own
// null pointers first, then T8's list; an output that is one of the history's planes: outColour or outLength in place in the plain call, any of the three
// outputs and any of the four planes in the moments call
static RaylibAMDTemporalMomentsFrame History3(const RaylibAMDTemporalFrame* h)
{
	return h ? RaylibAMDTemporalMomentsFrame{ h->colour, h->hit, h->length, nullptr } : RaylibAMDTemporalMomentsFrame{};
}
static RaylibAMDTemporalMomentsFrame History4(const RaylibAMDTemporalMomentsFrame* h) { return h ? *h : RaylibAMDTemporalMomentsFrame{}; }
static bool TemporalArgsValid(const char* who, const TemporalCall& C)
{
	const RaylibAMDTemporalMomentsFrame& h = C.history;
	if (C.moments && (!C.outMoments || (C.hasHistory && !h.moments))) { Log("%s: null argument", who); return false; }
	if (!C.params || !C.colour || !C.hit || !C.motion || !C.outColour || !C.outLength || (C.hasHistory && (!h.colour || !h.hit || !h.length))) {
		Log("%s: null argument", who); return false;
	}
	const uint64_t pixels = (uint64_t)C.width * C.height;
	if (pixels == 0 || pixels > 0x7fffffffull) { Log("%s: a frame of %u x %u pixels (1 .. 2^31 - 1)", who, C.width, C.height); return false; }
	if (!std::isfinite(C.params->depthTolerance) || C.params->depthTolerance < 0.0f) { Log("%s: depthTolerance %g is not a finite number >= 0", who, C.params->depthTolerance); return false; }
	if (!std::isfinite(C.params->maxLength) || C.params->maxLength < 1.0f) { Log("%s: maxLength %g is not a finite number >= 1", who, C.params->maxLength); return false; }
	bool inPlace = C.hasHistory && (C.outColour == h.colour || C.outLength == h.length);
	if (C.hasHistory && C.moments)
		for (const void* o : { (const void*)C.outColour, (const void*)C.outLength, (const void*)C.outMoments })
			for (const void* p : { (const void*)h.colour, (const void*)h.hit, (const void*)h.length, (const void*)h.moments }) inPlace |= o == p;
	if (inPlace) { Log("%s: an output plane is one of the history's: the taps read neighbours, in place is a race", who); return false; }
	return true;
}
static int32_t TemporalInternal(const char* who, const TemporalCall& C, bool hostMem, void* stream)
{
	if (!TemporalArgsValid(who, C)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceTemporalAccumulate(C, hostMem, stream, stats); });
}
static int32_t TemporalHostInternal(const char* who, const TemporalCall& C)
{
	if (!TemporalArgsValid(who, C)) return 0;
	TemporalAccumulateHost(C);
	return 1;
}
int32_t RaylibAMD_TemporalAccumulate(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
                                     const RaylibAMDMotion* motion, const RaylibAMDTemporalFrame* history, float* outColour, float* outLength)
{
	return TemporalInternal("RaylibAMD_TemporalAccumulate",
	                        { width, height, params, colour, hit, motion, history != nullptr, History3(history), outColour, outLength, nullptr, false }, true, nullptr);
}
int32_t RaylibAMD_TemporalAccumulateDevice(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
                                           const RaylibAMDMotion* motion, const RaylibAMDTemporalFrame* history, float* outColour, float* outLength, void* stream)
{
	return TemporalInternal("RaylibAMD_TemporalAccumulateDevice",
	                        { width, height, params, colour, hit, motion, history != nullptr, History3(history), outColour, outLength, nullptr, false }, false, stream);
}
int32_t RaylibAMD_TemporalAccumulateHost(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
                                         const RaylibAMDMotion* motion, const RaylibAMDTemporalFrame* history, float* outColour, float* outLength)
{
	return TemporalHostInternal("RaylibAMD_TemporalAccumulateHost",
	                        { width, height, params, colour, hit, motion, history != nullptr, History3(history), outColour, outLength, nullptr, false });
}
int32_t RaylibAMD_TemporalAccumulateMoments(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
                                            const RaylibAMDMotion* motion, const RaylibAMDTemporalMomentsFrame* history, float* outColour, float* outLength, float* outMoments)
{
	return TemporalInternal("RaylibAMD_TemporalAccumulateMoments",
	                        { width, height, params, colour, hit, motion, history != nullptr, History4(history), outColour, outLength, outMoments, true }, true, nullptr);
}
int32_t RaylibAMD_TemporalAccumulateMomentsDevice(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
                                                  const RaylibAMDMotion* motion, const RaylibAMDTemporalMomentsFrame* history, float* outColour, float* outLength, float* outMoments,
                                                  void* stream)
{
	return TemporalInternal("RaylibAMD_TemporalAccumulateMomentsDevice",
	                        { width, height, params, colour, hit, motion, history != nullptr, History4(history), outColour, outLength, outMoments, true }, false, stream);
}
int32_t RaylibAMD_TemporalAccumulateMomentsHost(uint32_t width, uint32_t height, const RaylibAMDTemporalParams* params, const float* colour, const RaylibAMDHitT* hit,
                                                const RaylibAMDMotion* motion, const RaylibAMDTemporalMomentsFrame* history, float* outColour, float* outLength, float* outMoments)
{
	return TemporalHostInternal("RaylibAMD_TemporalAccumulateMomentsHost",
	                        { width, height, params, colour, hit, motion, history != nullptr, History4(history), outColour, outLength, outMoments, true });
}

// RaylibAMD_FilterVariance / ...Device / ...Host (statements S3 to S7): the refusals every entry shares; `use` receives the caller's parameters or the defaults
static bool FilterVarianceArgsValid(const char* who, uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams* params, const RaylibAMDVarianceFilterPlanes* planes,
                                    const float* outColour, RaylibAMDVarianceFilterParams& use)
{
	if (!planes || !planes->colour || !planes->moments || !planes->length || !planes->hit || !planes->surface || !outColour) { Log("%s: null argument", who); return false; }
	const uint64_t pixels = (uint64_t)width * height;
	if (pixels == 0 || pixels > 0x7fffffffull) { Log("%s: a frame of %u x %u pixels (1 .. 2^31 - 1)", who, width, height); return false; }
	use = params ? *params : RaylibAMDVarianceFilterParams{ 5, 4.0f, 0.35f, 0.1f, 4.0f };
	if (use.iterations < 1 || use.iterations > 6) { Log("%s: %d iterations (1 .. 6)", who, use.iterations); return false; }
	const float sigma[3] = { use.sigmaLuminance, use.sigmaNormal, use.sigmaPlane };
	for (float v : sigma) if (!std::isfinite(v) || v < 1e-3f || v > 1e3f) { Log("%s: a sigma of %g is not in [1e-3, 1e3]", who, v); return false; }
	if (!std::isfinite(use.historyLength) || use.historyLength < 1.0f) { Log("%s: historyLength %g is not a finite number >= 1", who, use.historyLength); return false; }
	if (outColour == planes->colour) { Log("%s: outColour is the colour plane: the taps read neighbours", who); return false; }
	return true;
}
static int32_t FilterVarianceInternal(const char* who, uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams* params, const RaylibAMDVarianceFilterPlanes* planes,
                                      float* outColour, float* outVariance, bool hostMem, void* stream)
{
	RaylibAMDVarianceFilterParams use;
	if (!FilterVarianceArgsValid(who, width, height, params, planes, outColour, use)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceFilterVariance(width, height, use, *planes, outColour, outVariance, hostMem, stream, stats); });
}
int32_t RaylibAMD_FilterVariance(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams* params, const RaylibAMDVarianceFilterPlanes* planes, float* outColour,
                                 float* outVariance)
{
	return FilterVarianceInternal("RaylibAMD_FilterVariance", width, height, params, planes, outColour, outVariance, true, nullptr);
}
int32_t RaylibAMD_FilterVarianceDevice(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams* params, const RaylibAMDVarianceFilterPlanes* planes, float* outColour,
                                       float* outVariance, void* stream)
{
	return FilterVarianceInternal("RaylibAMD_FilterVarianceDevice", width, height, params, planes, outColour, outVariance, false, stream);
}
int32_t RaylibAMD_FilterVarianceHost(uint32_t width, uint32_t height, const RaylibAMDVarianceFilterParams* params, const RaylibAMDVarianceFilterPlanes* planes, float* outColour,
                                     float* outVariance)
{
	RaylibAMDVarianceFilterParams use;
	if (!FilterVarianceArgsValid("RaylibAMD_FilterVarianceHost", width, height, params, planes, outColour, use)) return 0;
	if (!FilterVarianceHost(width, height, use, *planes, outColour, outVariance)) { Log("RaylibAMD_FilterVarianceHost: no memory for a frame of %u x %u pixels", width, height); return 0; }
	return 1;
}

// RaylibAMD_TraceRaysAll / RaylibAMD_TraceRaysAllDevice / RaylibAMD_TraceRaysAllHost / RaylibAMD_PlanRayQueryAll (statements M1 to M5): the refusals every entry shares
static bool TraceRaysAllArgsValid(const char* who, const Scene* s, const void* rays, int32_t n, float rayTime, int32_t maxHits, const void* outHits)
{
	const QueryRows rows = { maxHits, RAYLIB_AMD_MAX_HITS, "rays", "hits", "records" };
	if (!TriangleQueryArgsValid(who, "multi-hit queries", s, rays, n, outHits, &rows)) return false;
	if (!std::isfinite(rayTime)) { Log("%s: ray time %g is not finite", who, rayTime); return false; }
	return true;
}
static int32_t TraceRaysAllInternal(const char* who, SceneHandle sh, const RaylibAMDRay* rays, int32_t n, float rayTime, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount,
                                    bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (!TraceRaysAllArgsValid(who, s, rays, n, rayTime, maxHits, outHits)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceTraceRaysAll(*s, rays, n, maxHits, outHits, outCount, hostMem, stream, stats); });
}
int32_t RaylibAMD_TraceRaysAll(SceneHandle sh, const RaylibAMDRay* rays, int32_t n, float rayTime, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount)
{
	return TraceRaysAllInternal("RaylibAMD_TraceRaysAll", sh, rays, n, rayTime, maxHits, outHits, outCount, true, nullptr);
}
int32_t RaylibAMD_TraceRaysAllDevice(SceneHandle sh, const RaylibAMDRay* rays, int32_t n, float rayTime, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount, void* stream)
{
	return TraceRaysAllInternal("RaylibAMD_TraceRaysAllDevice", sh, rays, n, rayTime, maxHits, outHits, outCount, false, stream);
}
int32_t RaylibAMD_TraceRaysAllHost(SceneHandle sh, const RaylibAMDRay* rays, int32_t n, float rayTime, int32_t maxHits, RaylibAMDHitT* outHits, uint32_t* outCount)
{
	Scene* s = (Scene*)sh;
	if (!TraceRaysAllArgsValid("RaylibAMD_TraceRaysAllHost", s, rays, n, rayTime, maxHits, outHits)) return 0;
	return RunOnHost(s, [&] { TraceRaysAllHost(*s, rays, n, maxHits, outHits, outCount); });
}
int32_t RaylibAMD_PlanRayQueryAll(SceneHandle sh, int32_t maxHits, int32_t wantCount, RaylibAMDQueryPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out || maxHits < 1 || maxHits > RAYLIB_AMD_MAX_HITS || !s->spheres.empty() || !s->cubes.empty()) return 0;
	(void)wantCount;   // (the count changes the kernel's instance and what it may prune, not the tree)
	return ExportPlan(PlanQueryAll(*s, ReadRenderKnobs()), 0, 0, out);
}

// RaylibAMD_NearestPoints / RaylibAMD_NearestPointsDevice / RaylibAMD_NearestPointsHost / RaylibAMD_PlanNearest: the refusals every entry shares
static bool NearestArgsValid(const char* who, const Scene* s, int32_t kind, const void* points, int32_t n, const void* out)
{
	if (kind != RAYLIB_AMD_NEAREST_WITHIN && kind != RAYLIB_AMD_NEAREST_CLOSEST) { Log("%s: unknown nearest kind %d", who, kind); return false; }
	return TriangleQueryArgsValid(who, "nearest-point queries", s, points, n, out);
}
static int32_t NearestPointsInternal(const char* who, SceneHandle sh, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out, bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (!NearestArgsValid(who, s, kind, points, n, out)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceNearestPoints(*s, kind, points, n, out, hostMem, stream, stats); });
}
int32_t RaylibAMD_NearestPoints(SceneHandle sh, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out)
{
	return NearestPointsInternal("RaylibAMD_NearestPoints", sh, kind, points, n, out, true, nullptr);
}
int32_t RaylibAMD_NearestPointsDevice(SceneHandle sh, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out, void* stream)
{
	return NearestPointsInternal("RaylibAMD_NearestPointsDevice", sh, kind, points, n, out, false, stream);
}
int32_t RaylibAMD_NearestPointsHost(SceneHandle sh, int32_t kind, const RaylibAMDNearestQuery* points, int32_t n, void* out)
{
	Scene* s = (Scene*)sh;
	if (!NearestArgsValid("RaylibAMD_NearestPointsHost", s, kind, points, n, out)) return 0;
	return RunOnHost(s, [&] { NearestPointsHost(*s, kind, points, n, out); });
}
int32_t RaylibAMD_PlanNearest(SceneHandle sh, int32_t kind, RaylibAMDQueryPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out || (kind != RAYLIB_AMD_NEAREST_WITHIN && kind != RAYLIB_AMD_NEAREST_CLOSEST) || !s->spheres.empty() || !s->cubes.empty()) return 0;
	const QueryPlan p = PlanNearest(*s, kind, ReadRenderKnobs());
	return ExportPlan(p, 0, p.early, out);
}

// RaylibAMD_SweepSpheres / RaylibAMD_SweepSpheresDevice / RaylibAMD_SweepSpheresHost / RaylibAMD_PlanSweep (statements W1 to W7): the refusals every entry shares
static bool SweepArgsValid(const char* who, const Scene* s, int32_t kind, const void* q, int32_t n, const void* out)
{
	if (kind != RAYLIB_AMD_SWEEP_ANY && kind != RAYLIB_AMD_SWEEP_CLOSEST) { Log("%s: unknown sweep kind %d", who, kind); return false; }
	return TriangleQueryArgsValid(who, "swept-sphere queries", s, q, n, out);
}
static int32_t SweepSpheresInternal(const char* who, SceneHandle sh, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out, bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (!SweepArgsValid(who, s, kind, q, n, out)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceSweepSpheres(*s, kind, q, n, out, hostMem, stream, stats); });
}
int32_t RaylibAMD_SweepSpheres(SceneHandle sh, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out)
{
	return SweepSpheresInternal("RaylibAMD_SweepSpheres", sh, kind, q, n, out, true, nullptr);
}
int32_t RaylibAMD_SweepSpheresDevice(SceneHandle sh, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out, void* stream)
{
	return SweepSpheresInternal("RaylibAMD_SweepSpheresDevice", sh, kind, q, n, out, false, stream);
}
int32_t RaylibAMD_SweepSpheresHost(SceneHandle sh, int32_t kind, const RaylibAMDSweepQuery* q, int32_t n, void* out)
{
	Scene* s = (Scene*)sh;
	if (!SweepArgsValid("RaylibAMD_SweepSpheresHost", s, kind, q, n, out)) return 0;
	return RunOnHost(s, [&] { SweepSpheresHost(*s, kind, q, n, out); });
}
int32_t RaylibAMD_PlanSweep(SceneHandle sh, int32_t kind, RaylibAMDQueryPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out || (kind != RAYLIB_AMD_SWEEP_ANY && kind != RAYLIB_AMD_SWEEP_CLOSEST) || !s->spheres.empty() || !s->cubes.empty()) return 0;
	const QueryPlan p = PlanSweep(*s, kind, ReadRenderKnobs());
	return ExportPlan(p, 0, p.early, out);
}

// RaylibAMD_NearestPointsAll / RaylibAMD_NearestPointsAllDevice / RaylibAMD_NearestPointsAllHost / RaylibAMD_PlanNearestAll (statements K1 to K5): the refusals every entry shares
static bool NearestAllArgsValid(const char* who, const Scene* s, const void* points, int32_t n, int32_t maxHits, const void* outHits)
{
	const QueryRows rows = { maxHits, RAYLIB_AMD_MAX_NEAREST, "points", "records", "records" };
	return TriangleQueryArgsValid(who, "nearest-point queries", s, points, n, outHits, &rows);
}
static int32_t NearestPointsAllInternal(const char* who, SceneHandle sh, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount,
                                        bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (!NearestAllArgsValid(who, s, points, n, maxHits, outHits)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceNearestPointsAll(*s, points, n, maxHits, outHits, outCount, hostMem, stream, stats); });
}
int32_t RaylibAMD_NearestPointsAll(SceneHandle sh, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount)
{
	return NearestPointsAllInternal("RaylibAMD_NearestPointsAll", sh, points, n, maxHits, outHits, outCount, true, nullptr);
}
int32_t RaylibAMD_NearestPointsAllDevice(SceneHandle sh, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount, void* stream)
{
	return NearestPointsAllInternal("RaylibAMD_NearestPointsAllDevice", sh, points, n, maxHits, outHits, outCount, false, stream);
}
int32_t RaylibAMD_NearestPointsAllHost(SceneHandle sh, const RaylibAMDNearestQuery* points, int32_t n, int32_t maxHits, RaylibAMDNearestHit* outHits, uint32_t* outCount)
{
	Scene* s = (Scene*)sh;
	if (!NearestAllArgsValid("RaylibAMD_NearestPointsAllHost", s, points, n, maxHits, outHits)) return 0;
	return RunOnHost(s, [&] { NearestPointsAllHost(*s, points, n, maxHits, outHits, outCount); });
}
int32_t RaylibAMD_PlanNearestAll(SceneHandle sh, int32_t maxHits, int32_t wantCount, RaylibAMDQueryPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out || maxHits < 1 || maxHits > RAYLIB_AMD_MAX_NEAREST || !s->spheres.empty() || !s->cubes.empty()) return 0;
	(void)wantCount;   // (the count changes the kernel's instance and what it may prune, not the tree)
	return ExportPlan(PlanNearestAll(*s, ReadRenderKnobs()), 0, 0, out);
}

// RaylibAMD_OverlapTriangles / RaylibAMD_OverlapTrianglesDevice / RaylibAMD_OverlapTrianglesHost (statements O1 to O6): the refusals every entry shares
static bool OverlapArgsValid(const char* who, const Scene* s, int32_t kind, uint32_t flags, const void* q, int32_t n, int32_t maxHits, const void* out, const uint32_t* outCount)
{
	if (kind != RAYLIB_AMD_OVERLAP_ANY && kind != RAYLIB_AMD_OVERLAP_LIST) { Log("%s: unknown overlap kind %d", who, kind); return false; }
	if ((flags & ~RAYLIB_AMD_OVERLAP_SKIP_SHARED) != 0u) { Log("%s: unknown flag bits 0x%x", who, flags); return false; }
	const bool list = kind == RAYLIB_AMD_OVERLAP_LIST;
	if (!list && outCount) { Log("%s: outCount belongs to RAYLIB_AMD_OVERLAP_LIST", who); return false; }
	const QueryRows rows = { maxHits, RAYLIB_AMD_MAX_OVERLAPS, "queries", "indices", "words" };
	return TriangleQueryArgsValid(who, "overlap queries", s, q, n, out, list ? &rows : nullptr);
}
static int32_t OverlapTrianglesInternal(const char* who, SceneHandle sh, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount,
                                        bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (!OverlapArgsValid(who, s, kind, flags, q, n, maxHits, out, outCount)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceOverlapTriangles(*s, kind, flags, q, n, maxHits, out, outCount, hostMem, stream, stats); });
}
int32_t RaylibAMD_OverlapTriangles(SceneHandle sh, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount)
{
	return OverlapTrianglesInternal("RaylibAMD_OverlapTriangles", sh, kind, flags, q, n, maxHits, out, outCount, true, nullptr);
}
int32_t RaylibAMD_OverlapTrianglesDevice(SceneHandle sh, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount, void* stream)
{
	return OverlapTrianglesInternal("RaylibAMD_OverlapTrianglesDevice", sh, kind, flags, q, n, maxHits, out, outCount, false, stream);
}
int32_t RaylibAMD_OverlapTrianglesHost(SceneHandle sh, int32_t kind, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount)
{
	Scene* s = (Scene*)sh;
	if (!OverlapArgsValid("RaylibAMD_OverlapTrianglesHost", s, kind, flags, q, n, maxHits, out, outCount)) return 0;
	return RunOnHost(s, [&] { OverlapTrianglesHost(*s, kind, flags, q, n, maxHits, out, outCount); });
}
int32_t RaylibAMD_PlanOverlap(SceneHandle sh, int32_t kind, RaylibAMDQueryPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out || (kind != RAYLIB_AMD_OVERLAP_ANY && kind != RAYLIB_AMD_OVERLAP_LIST) || !s->spheres.empty() || !s->cubes.empty()) return 0;
	const QueryPlan p = PlanOverlap(*s, kind, ReadRenderKnobs());
	return ExportPlan(p, 0, p.early, out);
}

// RaylibAMD_OverlapContacts / ...Device / ...Host (statements C1 to C6): LIST's refusals, and the records' own
static_assert(sizeof(RaylibAMDContact) == 32 && sizeof(ContactRecord) == 32, "contact records");
static_assert(RAYLIB_AMD_CONTACT_NONE == RL_CONTACT_NONE && RAYLIB_AMD_CONTACT_SEGMENT == RL_CONTACT_SEGMENT && RAYLIB_AMD_CONTACT_GAP == RL_CONTACT_GAP &&
              RAYLIB_AMD_CONTACT_NO_CROSSING == RL_CONTACT_NO_CROSSING, "contact kinds");
static bool ContactArgsValid(const char* who, const Scene* s, uint32_t flags, const void* q, int32_t n, int32_t maxHits, const void* outIndex, const void* outContact, const uint32_t* outCount)
{
	if (n > 0 && !outContact) { Log("%s: null argument", who); return false; }
	return OverlapArgsValid(who, s, RAYLIB_AMD_OVERLAP_LIST, flags, q, n, maxHits, outIndex, outCount);
}
static int32_t OverlapContactsInternal(const char* who, SceneHandle sh, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex,
                                       RaylibAMDContact* outContact, uint32_t* outCount, bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (!ContactArgsValid(who, s, flags, q, n, maxHits, outIndex, outContact, outCount)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) {
		return DeviceOverlapTriangles(*s, RAYLIB_AMD_OVERLAP_LIST, flags, q, n, maxHits, outIndex, outCount, hostMem, stream, stats, outContact, true);
	});
}
int32_t RaylibAMD_OverlapContacts(SceneHandle sh, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex, RaylibAMDContact* outContact,
                                  uint32_t* outCount)
{
	return OverlapContactsInternal("RaylibAMD_OverlapContacts", sh, flags, q, n, maxHits, outIndex, outContact, outCount, true, nullptr);
}
int32_t RaylibAMD_OverlapContactsDevice(SceneHandle sh, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex, RaylibAMDContact* outContact,
                                        uint32_t* outCount, void* stream)
{
	return OverlapContactsInternal("RaylibAMD_OverlapContactsDevice", sh, flags, q, n, maxHits, outIndex, outContact, outCount, false, stream);
}
int32_t RaylibAMD_OverlapContactsHost(SceneHandle sh, uint32_t flags, const RaylibAMDOverlapQuery* q, int32_t n, int32_t maxHits, int32_t* outIndex, RaylibAMDContact* outContact,
                                      uint32_t* outCount)
{
	Scene* s = (Scene*)sh;
	if (!ContactArgsValid("RaylibAMD_OverlapContactsHost", s, flags, q, n, maxHits, outIndex, outContact, outCount)) return 0;
	return RunOnHost(s, [&] { OverlapContactsHost(*s, flags, q, n, maxHits, outIndex, outContact, outCount); });
}
int32_t RaylibAMD_PlanOverlapContacts(SceneHandle sh, RaylibAMDQueryPlan* out) { return RaylibAMD_PlanOverlap(sh, RAYLIB_AMD_OVERLAP_LIST, out); }

// RaylibAMD_OverlapBoxes / RaylibAMD_OverlapBoxesDevice / RaylibAMD_OverlapBoxesHost / RaylibAMD_PlanOverlapBoxes (statements B1 to B6): the refusals every entry shares
static_assert(sizeof(RaylibAMDBoxQuery) == 64, "box records");
static bool BoxKindValid(int32_t kind) { return kind == RAYLIB_AMD_BOX_ANY || kind == RAYLIB_AMD_BOX_LIST || kind == RAYLIB_AMD_BOX_MARK; }
static bool OverlapBoxesArgsValid(const char* who, const Scene* s, int32_t kind, const void* q, int32_t n, int32_t maxHits, const void* out, const uint32_t* outCount)
{
	if (!BoxKindValid(kind)) { Log("%s: unknown box kind %d", who, kind); return false; }
	const bool list = kind == RAYLIB_AMD_BOX_LIST;
	if (!list && outCount) { Log("%s: outCount belongs to RAYLIB_AMD_BOX_LIST", who); return false; }
	const QueryRows rows = { maxHits, RAYLIB_AMD_MAX_OVERLAPS, "queries", "indices", "words" };
	return TriangleQueryArgsValid(who, "box queries", s, q, n, out, list ? &rows : nullptr);
}
static int32_t OverlapBoxesInternal(const char* who, SceneHandle sh, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount, bool hostMem,
                                    void* stream)
{
	Scene* s = (Scene*)sh;
	if (!OverlapBoxesArgsValid(who, s, kind, q, n, maxHits, out, outCount)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceOverlapBoxes(*s, kind, q, n, maxHits, out, outCount, hostMem, stream, stats); });
}
int32_t RaylibAMD_OverlapBoxes(SceneHandle sh, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount)
{
	return OverlapBoxesInternal("RaylibAMD_OverlapBoxes", sh, kind, q, n, maxHits, out, outCount, true, nullptr);
}
int32_t RaylibAMD_OverlapBoxesDevice(SceneHandle sh, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount, void* stream)
{
	return OverlapBoxesInternal("RaylibAMD_OverlapBoxesDevice", sh, kind, q, n, maxHits, out, outCount, false, stream);
}
int32_t RaylibAMD_OverlapBoxesHost(SceneHandle sh, int32_t kind, const RaylibAMDBoxQuery* q, int32_t n, int32_t maxHits, void* out, uint32_t* outCount)
{
	Scene* s = (Scene*)sh;
	if (!OverlapBoxesArgsValid("RaylibAMD_OverlapBoxesHost", s, kind, q, n, maxHits, out, outCount)) return 0;
	return RunOnHost(s, [&] { OverlapBoxesHost(*s, kind, q, n, maxHits, out, outCount); });
}
int32_t RaylibAMD_PlanOverlapBoxes(SceneHandle sh, int32_t kind, RaylibAMDQueryPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out || !BoxKindValid(kind) || !s->spheres.empty() || !s->cubes.empty()) return 0;
	const QueryPlan p = PlanOverlapBoxes(*s, kind, ReadRenderKnobs());
	return ExportPlan(p, 0, p.early, out);
}

// RaylibAMD_BakeDistanceField / RaylibAMD_BakeDistanceFieldDevice / RaylibAMD_BakeDistanceFieldHost / RaylibAMD_PlanDistanceField (statements V1 to V7): the
// refusals every entry shares; `grid` is the caller's parameters with maxDist's -0.0 read as +0.0
static bool DistanceFieldArgsValid(const char* who, const Scene* s, const RaylibAMDDistanceFieldParams* p, const void* outDist, bool needOut, RaylibAMDDistanceFieldParams& grid)
{
	if (!s || !p || (needOut && !outDist)) { Log("%s: null argument", who); return false; }
	int64_t voxels = 1;
	for (int a = 0; a < 3; ++a) {
		if (p->dims[a] < 1) { Log("%s: dims[%d] = %d is below 1", who, a, p->dims[a]); return false; }
		voxels *= p->dims[a];
		if (voxels > 0x7fffffffll) { Log("%s: %d x %d x %d voxels exceed 2^31 - 1", who, p->dims[0], p->dims[1], p->dims[2]); return false; }
		if (!std::isfinite(p->spacing[a]) || !(p->spacing[a] > 0.0f)) { Log("%s: spacing[%d] = %g is not a finite positive size", who, a, p->spacing[a]); return false; }
		if (!std::isfinite(p->origin[a])) { Log("%s: origin[%d] = %g is not finite", who, a, p->origin[a]); return false; }
		if (!std::isfinite(SdfCentre(p->origin[a], p->spacing[a], (uint32_t)(p->dims[a] - 1)))) { Log("%s: the last voxel centre of axis %d is not finite", who, a); return false; }
	}
	if (!(p->maxDist >= 0.0f)) { Log("%s: maxDist %g is negative or NaN", who, p->maxDist); return false; }
	if (p->sign < RAYLIB_AMD_SDF_UNSIGNED || p->sign > RAYLIB_AMD_SDF_SIGN_MAJORITY) { Log("%s: unknown sign mode %d", who, p->sign); return false; }
	if (!s->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return false; }
	if (!s->spheres.empty() || !s->cubes.empty()) { Log("%s: the scene holds spheres or cubes; distance fields are defined on triangles", who); return false; }
	if (s->bvh.depth > 64) { Log("%s: BVH depth %u exceeds the traversal stack (64)", who, s->bvh.depth); return false; }
	grid = *p;
	if (grid.maxDist == 0.0f) grid.maxDist = 0.0f;   // -0.0 is 0
	return true;
}
static int32_t BakeDistanceFieldInternal(const char* who, SceneHandle sh, const RaylibAMDDistanceFieldParams* params, float* outDist, int32_t* outPrim, bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	RaylibAMDDistanceFieldParams grid;
	if (!DistanceFieldArgsValid(who, s, params, outDist, true, grid)) return 0;
	return RunOnDevice(stream, [&](RaylibAMDStats& stats) { return DeviceBakeDistanceField(*s, grid, outDist, outPrim, hostMem, stream, stats); });
}
int32_t RaylibAMD_BakeDistanceField(SceneHandle sh, const RaylibAMDDistanceFieldParams* params, float* outDist, int32_t* outPrim)
{
	return BakeDistanceFieldInternal("RaylibAMD_BakeDistanceField", sh, params, outDist, outPrim, true, nullptr);
}
int32_t RaylibAMD_BakeDistanceFieldDevice(SceneHandle sh, const RaylibAMDDistanceFieldParams* params, float* outDist, int32_t* outPrim, void* stream)
{
	return BakeDistanceFieldInternal("RaylibAMD_BakeDistanceFieldDevice", sh, params, outDist, outPrim, false, stream);
}
int32_t RaylibAMD_BakeDistanceFieldHost(SceneHandle sh, const RaylibAMDDistanceFieldParams* params, float* outDist, int32_t* outPrim)
{
	Scene* s = (Scene*)sh;
	RaylibAMDDistanceFieldParams G;
	if (!DistanceFieldArgsValid("RaylibAMD_BakeDistanceFieldHost", s, params, outDist, true, G)) return 0;
	return RunOnHost(s, [&] { BakeDistanceFieldHost(*s, G, outDist, outPrim); });
}
int32_t RaylibAMD_PlanDistanceField(SceneHandle sh, const RaylibAMDDistanceFieldParams* params, RaylibAMDQueryPlan* outNearest, RaylibAMDQueryPlan* outRows)
{
	Scene* s = (Scene*)sh;
	RaylibAMDDistanceFieldParams grid;
	if (!s || !s->finalized || !params || !s->spheres.empty() || !s->cubes.empty()) return 0;
	if (s->bvh.depth > 64) return -1;
	if (!DistanceFieldArgsValid("RaylibAMD_PlanDistanceField", s, params, nullptr, false, grid)) return 0;
	const DistanceFieldPlan p = PlanDistanceField(*s, ReadRenderKnobs());
	if (!p.nearest.ok || !p.rows.ok) return -1;
	if (outNearest) ExportPlan(p.nearest, 0, 0, outNearest);
	if (outRows) ExportPlan(p.rows, 0, 0, outRows);
	return 1;
}

// RaylibAMD_TraceRadiance / RaylibAMD_TraceRadianceDevice / RaylibAMD_PlanRadiance: what of RaylibAMDRadianceParams needs no device and no rays
static bool RadianceParamsValid(const char* who, const Scene* s, const RaylibAMDRadianceParams* p)
{
	if (!s || !p) { Log("%s: null argument", who); return false; }
	if (!s->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return false; }
	if (p->maxPathLength < 0) { Log("%s: maxPathLength %d is negative", who, p->maxPathLength); return false; }
	if (p->maxPathLength > RL_RADIANCE_MAX_PATH) { Log("%s: maxPathLength %d exceeds %d", who, p->maxPathLength, RL_RADIANCE_MAX_PATH); return false; }
	if (p->sampleCount == 0) { Log("%s: sampleCount is 0", who); return false; }
	if (p->skipDraws > 64) { Log("%s: skipDraws %u exceeds 64", who, p->skipDraws); return false; }
	if (!std::isfinite(p->rayTMin) || p->rayTMin < 0.0f) { Log("%s: rayTMin %g is negative or not finite", who, p->rayTMin); return false; }
	return true;
}
// What a radiance call and a gather do between their own refusals and the device.  First the time interval: the host entry scans the records' times (word 3 of
// each 32-byte record; `what` names a record in the log), the device entry is given it.  prm.timeMin / timeMax are set.
static bool PathTimesValid(const char* who, const char* what, RaylibAMDRadianceParams& prm, const void* records, int32_t n, bool hostMem)
{
	if (hostMem) {
		// the host entry scans the times itself (timeMin / timeMax are the device entry's)
		const float* rec = (const float*)records;
		prm.timeMin = prm.timeMax = n > 0 ? rec[3] : 0.0f;
		for (int32_t i = 0; i < n; ++i) {
			const float t = rec[(size_t)i * 8 + 3];
			if (!std::isfinite(t)) { Log("%s: %s %d has a time that is not finite", who, what, i); return false; }
			prm.timeMin = std::min(prm.timeMin, t); prm.timeMax = std::max(prm.timeMax, t);
		}
	} else if (!std::isfinite(prm.timeMin) || !std::isfinite(prm.timeMax) || prm.timeMin > prm.timeMax) {
		Log("%s: the time interval [%g, %g] is empty or not finite", who, prm.timeMin, prm.timeMax);
		return false;
	}
	return true;
}
// ... then, with a device: the boxes of moving cubes for that interval, and a sky panorama that was destroyed
static bool PreparePathScene(const char* who, Scene* s, const RaylibAMDRadianceParams& prm, int32_t n)
{
	if (n > 0 && s->hasMovingCubes && !(prm.timeMin >= s->accelT0 && prm.timeMax <= s->accelT1)) {
		// moving cubes: their boxes must cover the motion at every ray's time (as RaylibAMD_TraceRays rebuilds them for its rayTime)
		const float t0 = std::min(s->accelT0, prm.timeMin), t1 = std::max(s->accelT1, prm.timeMax);
		ReleaseDeviceCopy(s);
		if (!s->BuildAccel(t0, t1)) { Log("%s: the acceleration structure could not be rebuilt for the times [%g, %g]", who, prm.timeMin, prm.timeMax); return false; }
	}
	if (s->sky && !g_images.contains(s->sky)) {
		Log("%s: the scene's sky panorama was destroyed; tracing without it", who);   // as a render (PrepareRender)
		s->sky = nullptr;
	}
	return true;
}
static_assert(offsetof(RaylibAMDPathRay, time) == 12 && offsetof(RaylibAMDGatherPoint, time) == 12 && sizeof(RaylibAMDPathRay) == 32 && sizeof(RaylibAMDGatherPoint) == 32, "a record's time");
static int32_t TraceRadianceInternal(const char* who, SceneHandle sh, const RaylibAMDRadianceParams* params, const RaylibAMDPathRay* rays, int32_t n, float* out,
                                     bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (n < 0 || (n > 0 && (!rays || !out))) { Log("%s: null argument", who); return 0; }
	if (!RadianceParamsValid(who, s, params)) return 0;
	RaylibAMDRadianceParams prm = *params;
	if (!PathTimesValid(who, "ray", prm, rays, n, hostMem)) return 0;
	if (!DeviceAvailable()) return 0;
	if (!PreparePathScene(who, s, prm, n)) return 0;
	RaylibAMDStats stats; memset(&stats, 0, sizeof(stats));
	if (!DeviceTraceRadiance(*s, prm, CurrentSeed(), rays, n, out, hostMem, stream, stats)) return 0;
	if (!stream) ReportOwnStats(stats);
	return 1;
}
int32_t RaylibAMD_TraceRadiance(SceneHandle sh, const RaylibAMDRadianceParams* params, const RaylibAMDPathRay* rays, int32_t n, float* outRGBA)
{
	return TraceRadianceInternal("RaylibAMD_TraceRadiance", sh, params, rays, n, outRGBA, true, nullptr);
}
int32_t RaylibAMD_TraceRadianceDevice(SceneHandle sh, const RaylibAMDRadianceParams* params, const RaylibAMDPathRay* rays, int32_t n, float* outRGBA, void* stream)
{
	return TraceRadianceInternal("RaylibAMD_TraceRadianceDevice", sh, params, rays, n, outRGBA, false, stream);
}
int32_t RaylibAMD_PlanRadiance(SceneHandle sh, const RaylibAMDRadianceParams* params, RaylibAMDQueryPlan* out)
{
	if (!out || !RadianceParamsValid("RaylibAMD_PlanRadiance", (Scene*)sh, params)) return 0;
	const QueryPlan p = PlanRadiance(*(Scene*)sh, ReadRenderKnobs());
	return ExportPlan(p, p.prims, 0, out);
}

// RaylibAMD_Gather / RaylibAMD_GatherDevice / RaylibAMD_GatherDirectionsHost: a gather's own refusals; the rest are a radiance call's
static bool GatherKindValid(const char* who, const RaylibAMDGatherParams* p)
{
	if (p->kind != RAYLIB_AMD_GATHER_IRRADIANCE && p->kind != RAYLIB_AMD_GATHER_SH9) { Log("%s: unknown gather kind %d", who, p->kind); return false; }
	if (p->skipDraws > 62) { Log("%s: skipDraws %u exceeds 62", who, p->skipDraws); return false; }
	return true;
}
// a gather's parameters as a radiance call's
static RaylibAMDRadianceParams RadianceParamsOf(const RaylibAMDGatherParams& g)
{
	RaylibAMDRadianceParams prm;
	prm.maxPathLength = g.maxPathLength; prm.rayTMin = g.rayTMin; prm.sampleFirst = g.sampleFirst; prm.sampleCount = g.sampleCount;
	prm.skipDraws = g.skipDraws; prm.timeMin = g.timeMin; prm.timeMax = g.timeMax;
	return prm;
}
// RaylibAMD_GatherAdaptive / ...Device / ...DecideHost / RaylibAMD_BakeLightmapAdaptive*: the refusals of the adaptive parameters under the cap `cap`
static bool GatherAdaptiveValid(const char* who, const RaylibAMDGatherAdaptiveParams* a, uint32_t cap)
{
	if (!a) { Log("%s: null adaptive parameters", who); return false; }
	if (!(a->threshold >= 0.0f && a->threshold <= 3.40282347e+38f)) { Log("%s: the threshold %g is negative or not finite", who, a->threshold); return false; }
	if (a->minSamples < 2) { Log("%s: minSamples %u is below 2", who, a->minSamples); return false; }
	if (a->passSamples == 0) { Log("%s: passSamples is 0", who); return false; }
	if (((uint64_t)cap + a->passSamples - 1) / a->passSamples > RL_GATHER_ADAPTIVE_MAX_PASSES) {
		Log("%s: %u samples in passes of %u are more than %u passes", who, cap, a->passSamples, RL_GATHER_ADAPTIVE_MAX_PASSES);
		return false;
	}
	return true;
}
// the four gather entries; adaptive: what an adaptive entry was given (its parameters, which may not be null, and outSamples), null for a plain entry
struct GatherAdaptiveArgs { const RaylibAMDGatherAdaptiveParams* params; uint32_t* outSamples; };
static int32_t GatherInternal(const char* who, SceneHandle sh, const RaylibAMDGatherParams* params, const RaylibAMDGatherPoint* points, int32_t n, float* out,
                              bool hostMem, void* stream, const GatherAdaptiveArgs* adaptive)
{
	Scene* s = (Scene*)sh;
	if (n < 0 || (n > 0 && (!points || !out))) { Log("%s: null argument", who); return 0; }
	if (!s || !params) { Log("%s: null argument", who); return 0; }
	RaylibAMDRadianceParams prm = RadianceParamsOf(*params);
	if (!RadianceParamsValid(who, s, &prm) || !GatherKindValid(who, params)) return 0;
	if (adaptive && !GatherAdaptiveValid(who, adaptive->params, params->sampleCount)) return 0;
	if (!PathTimesValid(who, "point", prm, points, n, hostMem)) return 0;
	if (!DeviceAvailable()) return n == 0 ? 1 : 0;   // (no points: nothing to gather, with or without a device)
	if (!PreparePathScene(who, s, prm, n)) return 0;
	RaylibAMDStats stats; memset(&stats, 0, sizeof(stats));
	if (!DeviceGather(*s, params->kind, prm, CurrentSeed(), points, n, out, hostMem, stream, stats, adaptive ? adaptive->params : nullptr, adaptive ? adaptive->outSamples : nullptr)) return 0;
	if (!stream) ReportOwnStats(stats);
	return 1;
}
int32_t RaylibAMD_Gather(SceneHandle sh, const RaylibAMDGatherParams* params, const RaylibAMDGatherPoint* points, int32_t n, float* out)
{
	return GatherInternal("RaylibAMD_Gather", sh, params, points, n, out, true, nullptr, nullptr);
}
int32_t RaylibAMD_GatherDevice(SceneHandle sh, const RaylibAMDGatherParams* params, const RaylibAMDGatherPoint* points, int32_t n, float* out, void* stream)
{
	return GatherInternal("RaylibAMD_GatherDevice", sh, params, points, n, out, false, stream, nullptr);
}
int32_t RaylibAMD_GatherAdaptive(SceneHandle sh, const RaylibAMDGatherParams* params, const RaylibAMDGatherAdaptiveParams* adaptive, const RaylibAMDGatherPoint* points,
                                 int32_t n, float* out, uint32_t* outSamples)
{
	const GatherAdaptiveArgs a = { adaptive, outSamples };
	return GatherInternal("RaylibAMD_GatherAdaptive", sh, params, points, n, out, true, nullptr, &a);
}
int32_t RaylibAMD_GatherAdaptiveDevice(SceneHandle sh, const RaylibAMDGatherParams* params, const RaylibAMDGatherAdaptiveParams* adaptive, const RaylibAMDGatherPoint* points,
                                       int32_t n, float* out, uint32_t* outSamples, void* stream)
{
	const GatherAdaptiveArgs a = { adaptive, outSamples };
	return GatherInternal("RaylibAMD_GatherAdaptiveDevice", sh, params, points, n, out, false, stream, &a);
}
// statements A1 to A3 on the caller's keys (rl_oracle.cc): the oracle of k_gather_adaptive_resolve's moments and decision
int32_t RaylibAMD_GatherAdaptiveDecideHost(const RaylibAMDGatherAdaptiveParams* adaptive, uint32_t cap, const float* keys, int64_t count, uint32_t* outSamples)
{
	const char* who = "RaylibAMD_GatherAdaptiveDecideHost";
	if (count < 0 || (count > 0 && (!keys || !outSamples))) { Log("%s: null argument, or a negative count", who); return 0; }
	if (cap == 0) { Log("%s: the cap is 0", who); return 0; }
	if (!GatherAdaptiveValid(who, adaptive, cap)) return 0;
	GatherAdaptiveDecideHost(*adaptive, cap, keys, count, outSamples);
	return 1;
}
int32_t RaylibAMD_GatherCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const RaylibAMDGatherPoint* points, uint32_t numPoints,
                                    uint32_t* outLive, RaylibAMDGatherPoint* outPoints, uint32_t* outCount)
{
	if (!live || !stopped || !points || !outLive || !outPoints || !outCount) return 0;
	if (numLive > numPoints) return 0;
	for (uint32_t i = 0; i < numLive; ++i) if (live[i] >= numPoints || (i > 0 && live[i] <= live[i - 1])) return 0;   // (the kernels index stopped by the entries)
	return DeviceGatherCompactTest(live, numLive, stopped, points, numPoints, outLive, outPoints, outCount) ? 1 : 0;
}
int32_t RaylibAMD_PlanGatherCut(const RaylibAMDGatherParams* params, int32_t n, uint64_t launchIndex, RaylibAMDGatherCut* out)
{
	const char* who = "RaylibAMD_PlanGatherCut";
	if (!params || !out || n <= 0 || params->sampleCount == 0) { Log("%s: null argument, or nothing to cut", who); return 0; }
	if (!GatherKindValid(who, params)) return 0;
	const GatherCut c = PlanGatherCut((uint32_t)n, params->sampleCount, params->kind == RAYLIB_AMD_GATHER_SH9, ReadRenderKnobs());
	if (launchIndex >= c.launches) { Log("%s: launch %llu of %llu", who, (unsigned long long)launchIndex, (unsigned long long)c.launches); return 0; }
	const GatherLaunch L = GatherLaunchAt(c, (uint32_t)n, params->sampleCount, launchIndex);
	out->pointsPerLaunch = c.pointsPer; out->samplesPerLaunch = c.samplesPer; out->pointRanges = c.pointRanges; out->sampleRanges = c.sampleRanges; out->launches = c.launches;
	out->pointFirst = L.pointFirst; out->numPoints = L.numPoints; out->sampleBase = L.sampleBase; out->numSamples = L.numSamples; out->first = L.first; out->last = L.last;
	return 1;
}
// statement 1 of the header's contract with the host's libm (rl_oracle.cc)
int32_t RaylibAMD_GatherDirectionsHost(const RaylibAMDGatherParams* params, const RaylibAMDGatherPoint* points, int32_t n, uint64_t seed, uint32_t sample, float* outDirs)
{
	const char* who = "RaylibAMD_GatherDirectionsHost";
	if (!params || n < 0 || (n > 0 && (!points || !outDirs))) { Log("%s: null argument", who); return 0; }
	if (!GatherKindValid(who, params)) return 0;
	GatherDirectionsHost(*params, points, n, seed, sample, outDirs);
	return 1;
}

// RaylibAMD_LightmapPoints / RaylibAMD_LightmapPointsHost / RaylibAMD_BakeLightmap / RaylibAMD_BakeLightmapDevice: what the four refuse alike.  Sets the triangle
// range (triCount -1 resolved) and the gather's parameters as a radiance call's, with both ends of the time interval at the lightmap's time.
static bool LightmapArgsValid(const char* who, const Scene* s, const RaylibAMDLightmapParams* p, int32_t& triFirst, int32_t& triCount, RaylibAMDRadianceParams& prm)
{
	if (!s || !p) { Log("%s: null argument", who); return false; }
	if (!s->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return false; }
	if (p->width < 1 || p->width > RL_LM_MAX_SIZE || p->height < 1 || p->height > RL_LM_MAX_SIZE) { Log("%s: the atlas %d x %d is outside 1 .. %d", who, p->width, p->height, RL_LM_MAX_SIZE); return false; }
	if (p->dilate < 0 || p->dilate > RL_LM_MAX_DILATE) { Log("%s: dilate %d is outside 0 .. %d", who, p->dilate, RL_LM_MAX_DILATE); return false; }
	const int64_t numTris = (int64_t)s->triangles.size();
	triFirst = p->triFirst;
	triCount = p->triCount == -1 ? (int32_t)std::max<int64_t>(0, numTris - (int64_t)p->triFirst) : p->triCount;
	if (triFirst < 0 || triCount <= 0 || (int64_t)triFirst + (int64_t)triCount > numTris) {
		Log("%s: triangles %d .. %d + %d are not a non-empty range of the scene's %lld", who, p->triFirst, p->triFirst, p->triCount, (long long)numTris);
		return false;
	}
	if (!std::isfinite(p->time)) { Log("%s: the time is not finite", who); return false; }
	prm = RadianceParamsOf(p->gather);
	prm.timeMin = prm.timeMax = p->time;
	return RadianceParamsValid(who, s, &prm) && GatherKindValid(who, &p->gather);
}
static int64_t LightmapPointsInternal(const char* who, SceneHandle sh, const RaylibAMDLightmapParams* params, const float* uv, RaylibAMDGatherPoint* outPoints, uint32_t* outTexel,
                                      int64_t capacity, bool device)
{
	Scene* s = (Scene*)sh;
	int32_t triFirst = 0, triCount = 0; RaylibAMDRadianceParams prm;
	if (!LightmapArgsValid(who, s, params, triFirst, triCount, prm)) return -1;
	if (capacity < 0 || (capacity > 0 && !outPoints)) { Log("%s: a negative capacity, or no room for the points", who); return -1; }
	if (!device) return DeviceSyncMovedScene(*s) ? LightmapPointsHost(*s, *params, triFirst, triCount, uv, outPoints, outTexel, capacity) : -1;
	if (!DeviceAvailable()) return -1;
	return DeviceLightmapPoints(*s, *params, triFirst, triCount, uv, outPoints, outTexel, capacity);
}
int64_t RaylibAMD_LightmapPoints(SceneHandle sh, const RaylibAMDLightmapParams* params, const float* uv, RaylibAMDGatherPoint* outPoints, uint32_t* outTexel, int64_t capacity)
{
	return LightmapPointsInternal("RaylibAMD_LightmapPoints", sh, params, uv, outPoints, outTexel, capacity, true);
}
int64_t RaylibAMD_LightmapPointsHost(SceneHandle sh, const RaylibAMDLightmapParams* params, const float* uv, RaylibAMDGatherPoint* outPoints, uint32_t* outTexel, int64_t capacity)
{
	return LightmapPointsInternal("RaylibAMD_LightmapPointsHost", sh, params, uv, outPoints, outTexel, capacity, false);
}
// RaylibAMD_BakeLightmapFiltered* / RaylibAMD_FilterLightmap*: the filter's own refusals
static bool LightmapFilterValid(const char* who, const RaylibAMDLightmapFilterParams* f)
{
	if (!f) { Log("%s: null filter", who); return false; }
	if (f->iterations < 1 || f->iterations > 8) { Log("%s: %d filter iterations are outside 1 .. 8", who, f->iterations); return false; }
	for (const float sigma : { f->sigmaColor, f->sigmaNormal, f->sigmaPosition })
		if (!(std::isfinite(sigma) && sigma >= 1e-3f && sigma <= 1e3f)) { Log("%s: a filter sigma (%g) is not finite or outside [1e-3, 1e3]", who, sigma); return false; }
	return true;
}
// What a bake entry takes beside the atlas' arguments: a filter, the filter's input atlas, adaptive parameters (takes*: the entry has the argument, and a null
// pointer is refused), with the pointers it was given
struct BakeEntry {
	bool takesFilter, takesIn, takesAdaptive;
	const RaylibAMDLightmapFilterParams* filter; const float* in; const RaylibAMDGatherAdaptiveParams* adaptive; uint32_t* outSamples;
	static BakeEntry Plain() { return { false, false, false, nullptr, nullptr, nullptr, nullptr }; }
	static BakeEntry Filtered(const RaylibAMDLightmapFilterParams* filter) { return { true, false, false, filter, nullptr, nullptr, nullptr }; }
	static BakeEntry FilterOf(const RaylibAMDLightmapFilterParams* filter, const float* in) { return { true, true, false, filter, in, nullptr, nullptr }; }
	static BakeEntry Adaptive(const RaylibAMDGatherAdaptiveParams* adaptive, uint32_t* outSamples) { return { false, false, true, nullptr, nullptr, adaptive, outSamples }; }
};
static int32_t BakeLightmapInternal(const char* who, SceneHandle sh, const RaylibAMDLightmapParams* params, const float* uv, float* out, uint8_t* outCoverage, bool hostMem, void* stream,
                                    const BakeEntry& e)
{
	Scene* s = (Scene*)sh;
	int32_t triFirst = 0, triCount = 0; RaylibAMDRadianceParams prm;
	if (!out || (e.takesIn && !e.in)) { Log("%s: null argument", who); return 0; }
	if (!LightmapArgsValid(who, s, params, triFirst, triCount, prm)) return 0;
	if (e.takesFilter && !LightmapFilterValid(who, e.filter)) return 0;
	if (e.takesAdaptive && !GatherAdaptiveValid(who, e.adaptive, prm.sampleCount)) return 0;
	if (!DeviceAvailable()) return 0;
	if (!PreparePathScene(who, s, prm, 1)) return 0;
	RaylibAMDStats stats; memset(&stats, 0, sizeof(stats));
	if (!DeviceBakeLightmap(who, *s, *params, triFirst, triCount, prm, CurrentSeed(), uv, out, outCoverage, hostMem, stream, stats, e.filter, e.in, e.adaptive, e.outSamples)) return 0;
	if (!stream) ReportOwnStats(stats);
	return 1;
}
int32_t RaylibAMD_BakeLightmap(SceneHandle sh, const RaylibAMDLightmapParams* params, const float* uv, float* out, uint8_t* outCoverage)
{
	return BakeLightmapInternal("RaylibAMD_BakeLightmap", sh, params, uv, out, outCoverage, true, nullptr, BakeEntry::Plain());
}
int32_t RaylibAMD_BakeLightmapDevice(SceneHandle sh, const RaylibAMDLightmapParams* params, const float* uv, float* out, uint8_t* outCoverage, void* stream)
{
	return BakeLightmapInternal("RaylibAMD_BakeLightmapDevice", sh, params, uv, out, outCoverage, false, stream, BakeEntry::Plain());
}
int32_t RaylibAMD_BakeLightmapAdaptive(SceneHandle sh, const RaylibAMDLightmapParams* params, const RaylibAMDGatherAdaptiveParams* adaptive, const float* uv, float* out,
                                       uint8_t* outCoverage, uint32_t* outSamples)
{
	return BakeLightmapInternal("RaylibAMD_BakeLightmapAdaptive", sh, params, uv, out, outCoverage, true, nullptr, BakeEntry::Adaptive(adaptive, outSamples));
}
int32_t RaylibAMD_BakeLightmapAdaptiveDevice(SceneHandle sh, const RaylibAMDLightmapParams* params, const RaylibAMDGatherAdaptiveParams* adaptive, const float* uv, float* out,
                                             uint8_t* outCoverage, uint32_t* outSamples, void* stream)
{
	return BakeLightmapInternal("RaylibAMD_BakeLightmapAdaptiveDevice", sh, params, uv, out, outCoverage, false, stream, BakeEntry::Adaptive(adaptive, outSamples));
}
int32_t RaylibAMD_BakeLightmapFiltered(SceneHandle sh, const RaylibAMDLightmapParams* params, const RaylibAMDLightmapFilterParams* filter, const float* uv, float* out, uint8_t* outCoverage)
{
	return BakeLightmapInternal("RaylibAMD_BakeLightmapFiltered", sh, params, uv, out, outCoverage, true, nullptr, BakeEntry::Filtered(filter));
}
int32_t RaylibAMD_BakeLightmapFilteredDevice(SceneHandle sh, const RaylibAMDLightmapParams* params, const RaylibAMDLightmapFilterParams* filter, const float* uv, float* out,
                                             uint8_t* outCoverage, void* stream)
{
	return BakeLightmapInternal("RaylibAMD_BakeLightmapFilteredDevice", sh, params, uv, out, outCoverage, false, stream, BakeEntry::Filtered(filter));
}
int32_t RaylibAMD_FilterLightmap(SceneHandle sh, const RaylibAMDLightmapParams* params, const RaylibAMDLightmapFilterParams* filter, const float* uv, const float* in, float* out,
                                 uint8_t* outCoverage)
{
	return BakeLightmapInternal("RaylibAMD_FilterLightmap", sh, params, uv, out, outCoverage, true, nullptr, BakeEntry::FilterOf(filter, in));
}
int32_t RaylibAMD_FilterLightmapDevice(SceneHandle sh, const RaylibAMDLightmapParams* params, const RaylibAMDLightmapFilterParams* filter, const float* uv, const float* in, float* out,
                                       uint8_t* outCoverage, void* stream)
{
	return BakeLightmapInternal("RaylibAMD_FilterLightmapDevice", sh, params, uv, out, outCoverage, false, stream, BakeEntry::FilterOf(filter, in));
}
int32_t RaylibAMD_FilterLightmapHost(int32_t width, int32_t height, int32_t kind, const RaylibAMDLightmapFilterParams* filter, const RaylibAMDGatherPoint* points, const uint32_t* texel,
                                     int64_t count, const float* values, float* outValues)
{
	const char* who = "RaylibAMD_FilterLightmapHost";
	if (count < 0 || (count > 0 && (!points || !texel || !values || !outValues))) { Log("%s: null argument, or a negative count", who); return 0; }
	if (kind != RAYLIB_AMD_GATHER_IRRADIANCE && kind != RAYLIB_AMD_GATHER_SH9) { Log("%s: unknown gather kind %d", who, kind); return 0; }
	if (!LightmapFilterValid(who, filter)) return 0;
	if (width < 1 || width > RL_LM_MAX_SIZE || height < 1 || height > RL_LM_MAX_SIZE) { Log("%s: the atlas %d x %d is outside 1 .. %d", who, width, height, RL_LM_MAX_SIZE); return 0; }
	if (count > (int64_t)width * (int64_t)height) { Log("%s: %lld points are more than the atlas' texels", who, (long long)count); return 0; }
	return FilterLightmapHost(width, height, kind, *filter, points, texel, count, values, outValues) ? 1 : 0;
}

int32_t RaylibAMD_SceneNumTriangles(SceneHandle sh) { Scene* s = (Scene*)sh; return s ? (int32_t)s->triangles.size() : 0; }
int32_t RaylibAMD_SceneNumMaterials(SceneHandle sh) { Scene* s = (Scene*)sh; return s ? (int32_t)s->materials.size() : 0; }
int32_t RaylibAMD_SceneNumTextures(SceneHandle sh) { Scene* s = (Scene*)sh; return s ? (int32_t)s->textures.size() : 0; }
void RaylibAMD_SceneExportTriangles(SceneHandle sh, void* out) { Scene* s = (Scene*)sh; if (s && out && !s->triangles.empty() && DeviceSyncMovedScene(*s)) memcpy(out, s->triangles.data(), s->triangles.size() * sizeof(HostTriangle)); }
void RaylibAMD_SceneExportMaterials(SceneHandle sh, void* out) { Scene* s = (Scene*)sh; if (s && out && !s->materials.empty()) memcpy(out, s->materials.data(), s->materials.size() * sizeof(HostMaterial)); }
void RaylibAMD_SceneTextureSize(SceneHandle sh, int32_t i, int32_t* w, int32_t* h)
{
	Scene* s = (Scene*)sh;
	if (!s || i < 0 || i >= (int32_t)s->textures.size()) { if (w) *w = 0; if (h) *h = 0; return; }
	if (w) *w = (int32_t)s->textures[i]->width;
	if (h) *h = (int32_t)s->textures[i]->height;
}
int32_t RaylibAMD_SceneExportTriOrder(SceneHandle sh, uint32_t* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !out) return 0;
	std::copy(s->bvh.triOrder.begin(), s->bvh.triOrder.end(), out);
	return 1;
}
void RaylibAMD_SceneExportTexture(SceneHandle sh, int32_t i, float* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !out || i < 0 || i >= (int32_t)s->textures.size()) return;
	s->textures[i]->SyncHost();
	memcpy(out, s->textures[i]->rgba.data(), s->textures[i]->rgba.size() * sizeof(float));
}
void RaylibAMD_SceneGetSun(SceneHandle sh, float ill[3], float dir[3])
{
	Scene* s = (Scene*)sh;
	if (!s) return;
	ill[0] = s->sunIlluminance.x; ill[1] = s->sunIlluminance.y; ill[2] = s->sunIlluminance.z;
	dir[0] = s->sunDirection.x; dir[1] = s->sunDirection.y; dir[2] = s->sunDirection.z;
}
int32_t RaylibAMD_SceneBVHInfo(SceneHandle sh, uint32_t* nodes, uint32_t* depth, float* sah)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !DeviceSyncMovedScene(*s)) return 0;
	if (nodes) *nodes = (uint32_t)s->bvh.nodes.size();
	if (depth) *depth = s->bvh.depth;
	if (sah) *sah = s->bvh.sahCost;
	return ValidateBVH(s->bvh, s->triangles) ? 1 : 0;
}
int32_t RaylibAMD_SceneBVH4Info(SceneHandle sh, uint32_t* nodes4, uint32_t* stackNeed)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || s->bvh.nodes4.empty() || !DeviceSyncMovedScene(*s)) return 0;
	if (nodes4) *nodes4 = (uint32_t)s->bvh.nodes4.size();
	if (stackNeed) *stackNeed = s->bvh.stackNeed4;
	return (ValidateBVH4(s->bvh, s->triangles) && ValidateBVH8(s->bvh, s->triangles)) ? 1 : -1;   // (the 8-wide tree, where the scene has one, is part of the check)
}
int32_t RaylibAMD_SceneBVH8Info(SceneHandle sh, uint32_t* nodes8, uint32_t* levels, float* steps4, float* steps8)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || s->bvh.nodes8.empty() || !DeviceSyncMovedScene(*s)) return 0;
	if (nodes8) *nodes8 = (uint32_t)s->bvh.nodes8.size();
	if (levels) *levels = s->bvh.depth8;
	if (steps4) *steps4 = s->bvh.sahNodes4;
	if (steps8) *steps8 = s->bvh.sahNodes8;
	return ValidateBVH8(s->bvh, s->triangles) ? 1 : -1;
}
int32_t RaylibAMD_SceneWalk8Host(SceneHandle sh, const float* rays, int32_t count, float tMin, const float* tMax, float* outT, uint32_t* outSteps)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || s->bvh.nodes8.empty() || !rays || !tMax || !outT || count < 0 || !DeviceSyncMovedScene(*s)) return 0;
	return Walk8Host(s->bvh, s->triangles, rays, count, tMin, tMax, outT, outSteps) ? 1 : -1;
}
int32_t RaylibAMD_SceneWalkStackHost(SceneHandle sh, int32_t tree, const float* rays, int32_t count, float tMin, int32_t capacity, float* outT, uint32_t* outHighWater)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !rays || !outT || count < 0 || capacity < 0 || (tree != 2 && tree != 3 && tree != 4 && tree != 8)) return 0;
	if (tree == 2 ? s->bvh.nodes.empty() : tree == 3 ? s->bvh.nodes4.empty() : tree == 4 ? s->bvh.nodes4q.empty() : s->bvh.nodes8.empty()) return 0;
	if (!DeviceSyncMovedScene(*s)) return 0;
	return WalkStackHost(s->bvh, s->triangles, s->spheres, s->cubes, tree, rays, count, tMin, capacity, outT, outHighWater) ? 1 : -1;
}
int32_t RaylibAMD_SceneLeafListInfo(SceneHandle sh, uint32_t* maxPerLeaf)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized) return 0;
	int32_t leaves = 0; uint32_t most = 0;
	for (const DNode4& n : s->bvh.leafList) for (int k = 0; k < 4; ++k) if (n.child[k] != DNODE_EMPTY) { ++leaves; most = std::max(most, (((uint32_t)~n.child[k]) & LEAF_COUNT_MASK) + 1u); }
	if (maxPerLeaf) *maxPerLeaf = most;
	return leaves;
}
int32_t RaylibAMD_ScenePlain(SceneHandle sh)
{
	Scene* s = (Scene*)sh;
	return (s && s->finalized && ScenePlain(*s)) ? 1 : 0;
}
int32_t RaylibAMD_LastTracePlain(void) { return DeviceLastTracePlain(); }
int32_t RaylibAMD_SceneLazyRefl(SceneHandle sh)
{
	Scene* s = (Scene*)sh;
	return (s && s->finalized && SceneLazyRefl(*s)) ? 1 : 0;
}
int32_t RaylibAMD_LastTraceLazy(void) { return DeviceLastTraceLazy(); }
int32_t RaylibAMD_LastHitQueue(void) { return DeviceLastHitQueue(); }
int32_t RaylibAMD_LastLitMask(void) { return DeviceLastLitMask(); }
int32_t RaylibAMD_PlanRender(SceneHandle sh, const RendererSettings* settings, int32_t hasSky, int32_t numCUs, int32_t workgroupsPerCU, RaylibAMDRenderPlan* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !settings || !out || numCUs < 1) return 0;
	memset(out, 0, sizeof(*out));
	const RenderKnobs knobs = ReadRenderKnobs();
	const TracePlan t = PlanTrace(*s, *settings, hasSky != 0, knobs);
	if (!t.ok) return -1;
	out->pathTrace = t.pathTrace; out->stack = t.stack; out->prims = t.prims; out->poolK = t.poolK; out->tree = t.tree; out->lstack = t.lstack; out->lds = t.lds; out->plain = t.plain; out->lazy = t.lazy ? 1 : 0; out->hitQueue = t.hitQueue ? 1 : 0;
	out->pathsPerWave = t.pathsPerWave; out->treeWidth = t.treeWidth; out->nodeBytes = t.nodeBytes;
	out->keepNodes4 = t.keepNodes4; out->keepNodes4f = t.keepNodes4f; out->eagerTree = t.eagerTree;
	const uint32_t cells = ((settings->viewportWidth + 7) / 8) * ((settings->viewportHeight + 7) / 8);
	const uint32_t spp = (uint32_t)(settings->samplesPerPixel > 1 ? settings->samplesPerPixel : 1);
	const LaunchPlan L = PlanLaunch(cells, cells, spp, 0, numCUs, workgroupsPerCU, t, knobs);
	out->batch = L.batch; out->sampleCount = L.sampleCount; out->blocks = L.blocks; out->stackStride = L.stackStride; out->jobChunk = L.jobChunk;
	out->heads = L.heads; out->jobsPerHead = L.jobsPerHead; out->guideShift = L.guideShift; out->jobs = L.jobs;
	return 1;
}
int32_t RaylibAMD_PlanViews(SceneHandle sh, const RendererSettings* settings, const CameraHandle* cameras, int32_t count, int32_t hasSky,
                           int32_t numCUs, int32_t workgroupsPerCU, RaylibAMDRenderPlan* out, uint8_t* outCellEmpty)
{
	Scene* s = (Scene*)sh;
	if (!out || numCUs < 1 || !ViewsArgsValid("RaylibAMD_PlanViews", settings, s, cameras, count, nullptr)) return 0;
	memset(out, 0, sizeof(*out));
	const RenderKnobs knobs = ReadRenderKnobs();
	const TracePlan t = PlanTrace(*s, *settings, hasSky != 0, knobs);
	if (!t.ok) return -1;
	out->pathTrace = t.pathTrace; out->stack = t.stack; out->prims = t.prims; out->poolK = t.poolK; out->tree = t.tree; out->lstack = t.lstack; out->lds = t.lds; out->plain = t.plain; out->lazy = 0;   // (the views twin of a lazy plan is the plain instance's)
	out->pathsPerWave = t.pathsPerWave; out->treeWidth = t.treeWidth; out->nodeBytes = t.nodeBytes;
	out->keepNodes4 = t.keepNodes4; out->keepNodes4f = t.keepNodes4f; out->eagerTree = t.eagerTree;
	std::vector<DCamera> cams((size_t)count);
	for (int32_t v = 0; v < count; ++v) cams[(size_t)v] = ((Camera*)cameras[v])->ToDevice();
	if (!DeviceSyncMovedScene(*s)) return 0;   // (the cull's bounds: the root's boxes)
	const ViewsPlan V = PlanViews(SceneCullScene(*s, hasSky != 0), *settings, cams.data(), (uint32_t)count, t, numCUs, workgroupsPerCU, knobs);
	if (!V.ok) return 0;
	if (outCellEmpty) memcpy(outCellEmpty, V.empty.data(), V.empty.size());
	const LaunchPlan& L = V.launch;
	out->batch = L.batch; out->sampleCount = L.sampleCount; out->blocks = L.blocks; out->stackStride = L.stackStride; out->jobChunk = L.jobChunk;
	out->heads = L.heads; out->jobsPerHead = L.jobsPerHead; out->guideShift = L.guideShift; out->jobs = L.jobs;
	return 1;
}
uint64_t RaylibAMD_SceneBVHHash(SceneHandle sh)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !DeviceSyncMovedScene(*s)) return 0;
	uint64_t h = 1469598103934665603ull;   // FNV-1a over the node records and the leaf order
	auto feed = [&h](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
	feed(s->bvh.nodes.data(), s->bvh.nodes.size() * sizeof(DNode));
	feed(s->bvh.triOrder.data(), s->bvh.triOrder.size() * sizeof(uint32_t));
	feed(s->bvh.nodes4.data(), s->bvh.nodes4.size() * sizeof(DNode4));
	feed(s->bvh.nodes4q.data(), s->bvh.nodes4q.size() * sizeof(DNode4Q));
	feed(s->bvh.leafList.data(), s->bvh.leafList.size() * sizeof(DNode4));
	feed(s->bvh.nodes8.data(), s->bvh.nodes8.size() * sizeof(DNode8));
	return h;
}
// ---- a finalized scene's triangles moved (include/raylib_amd.h; rl_rt_move.hip) ----
static int32_t MoveTrianglesInternal(const char* who, SceneHandle sh, int32_t first, int32_t count, const float* positions, const float* normals, bool hostMem, void* stream)
{
	Scene* s = (Scene*)sh;
	if (!s || !g_scenes.contains(s)) { Log("%s: unknown scene", who); return 0; }
	if (!s->finalized) { Log("%s: scene was not finalized (Raylib_FinalizeScene)", who); return 0; }
	if (first < 0 || count < 0 || (int64_t)first + (int64_t)count > (int64_t)s->triangles.size()) { Log("%s: triangles [%d, %d + %d) are not the scene's", who, first, first, count); return 0; }
	if (count == 0) return 1;
	if (!positions) { Log("%s: null positions", who); return 0; }
	{
		std::lock_guard<std::mutex> lk(g_progressive.mu);
		for (const Progressive* p : g_progressive.items) if (p->scene == s) { Log("%s: a progressive session is open on the scene", who); return 0; }
	}
	if (hostMem) {
		for (size_t i = 0; i < (size_t)count * 9; ++i) if (!std::isfinite(positions[i]) || (normals && !std::isfinite(normals[i]))) { Log("%s: a position or normal is not finite", who); return 0; }
	}
	return DeviceMoveTriangles(*s, first, count, positions, normals, hostMem, stream) ? 1 : 0;
}
int32_t RaylibAMD_SceneMoveTriangles(SceneHandle sh, int32_t first, int32_t count, const float* positions, const float* normals)
{
	return MoveTrianglesInternal("RaylibAMD_SceneMoveTriangles", sh, first, count, positions, normals, true, nullptr);
}
int32_t RaylibAMD_SceneMoveTrianglesDevice(SceneHandle sh, int32_t first, int32_t count, const float* positions, const float* normals, void* stream)
{
	return MoveTrianglesInternal("RaylibAMD_SceneMoveTrianglesDevice", sh, first, count, positions, normals, false, stream);
}
int32_t RaylibAMD_SceneRebuild(SceneHandle sh)
{
	Scene* s = (Scene*)sh;
	if (!s || !g_scenes.contains(s) || !s->finalized) { Log("RaylibAMD_SceneRebuild: unknown scene, or not finalized"); return 0; }
	ReleaseDeviceCopy(s);   // (a progressive session notices the new upload and ends: rl_rt_render.hip)
	return s->BuildAccel(s->accelT0, s->accelT1) ? 1 : 0;
}
int32_t RaylibAMD_SceneCheckTrees(SceneHandle sh, uint32_t* outFailedTree)
{
	Scene* s = (Scene*)sh;
	if (outFailedTree) *outFailedTree = 0;
	if (!s || !g_scenes.contains(s) || !s->finalized) return 0;
	return DeviceCheckTrees(*s, outFailedTree) ? 1 : 0;
}
int32_t RaylibAMD_SceneCompareTrees(SceneHandle sh, uint32_t* outDiffMask)
{
	Scene* s = (Scene*)sh;
	if (outDiffMask) *outDiffMask = 0;
	if (!s || !g_scenes.contains(s) || !s->finalized) return 0;
	return DeviceCompareTrees(*s, outDiffMask) ? 1 : 0;
}
int32_t RaylibAMD_SceneExportBVHNodes(SceneHandle sh, void* out)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized || !DeviceSyncMovedScene(*s)) return 0;
	if (out) memcpy(out, s->bvh.nodes.data(), s->bvh.nodes.size() * sizeof(DNode));
	return (int32_t)s->bvh.nodes.size();
}
uint64_t RaylibAMD_SceneTopologyHash(SceneHandle sh)
{
	Scene* s = (Scene*)sh;
	if (!s || !s->finalized) return 0;
	uint64_t h = 1469598103934665603ull;   // FNV-1a over what a move keeps: child references, leaf order, the 8-wide nodes' masks and bases -- no box
	auto feed = [&h](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
	for (const DNode& n : s->bvh.nodes) { feed(&n.left, 4); feed(&n.right, 4); }
	feed(s->bvh.triOrder.data(), s->bvh.triOrder.size() * sizeof(uint32_t));
	for (const DNode4& n : s->bvh.nodes4) feed(n.child, 16);
	for (const DNode4& n : s->bvh.leafList) feed(n.child, 16);
	for (const DNode8& n : s->bvh.nodes8) { const uint32_t imask = n.meta >> 24; feed(&imask, 4); feed(&n.childBase, 16); }   // childBase, triBase, leafMask, alphaMask
	return h;
}
void RaylibAMD_CameraExport(CameraHandle h, float out[19])
{
	Camera* c = (Camera*)h;
	if (!c || !out) return;
	const f3* v[6] = { &c->origin, &c->top_left, &c->horizontal, &c->vertical, &c->u, &c->v };
	int k = 0;
	out[k++] = c->origin.x; out[k++] = c->origin.y; out[k++] = c->origin.z; out[k++] = c->lensRadius;
	for (int i = 1; i < 6; ++i) { out[k++] = v[i]->x; out[k++] = v[i]->y; out[k++] = v[i]->z; }
}
ImageHandle RaylibAMD_CreateImageFromData(uint32_t w, uint32_t h, const float* rgba)
{
	if (!rgba) return 0;
	Image* img = new Image;
	img->width = w; img->height = h;
	img->rgba.assign(rgba, rgba + (size_t)w * h * 4);
	g_images.add(img);
	return (ImageHandle)img;
}
void RaylibAMD_DumpImageRGBA(ImageHandle h, float* out)
{
	Image* img = (Image*)h;
	if (!img || !out) return;
	img->SyncHost();
	memcpy(out, img->rgba.data(), img->rgba.size() * sizeof(float));
}
float RaylibAMD_ParseFloat(const char* token) { return token ? ParseDecimalFloat(token) : 0.0f; }
int32_t RaylibAMD_ImageSize(ImageHandle h, uint32_t* w, uint32_t* ht)
{
	Image* img = (Image*)h;
	if (!img) return 0;
	if (w) *w = img->width;
	if (ht) *ht = img->height;
	return 1;
}
int32_t RaylibAMD_OBJModelSetTexture(OBJModelHandle oh, const char* materialName, int32_t slot, ImageHandle ih)
{
	OBJModel* m = (OBJModel*)oh; Image* img = (Image*)ih;
	if (!m || !materialName || slot < 0 || slot > 4 || !img || m->finalized) return 0;
	for (size_t i = 0; i < m->materialNames.size(); ++i) {
		if (m->materialNames[i] == materialName && m->materials[i].type == MAT_MICROFACET) {
			m->images.push_back(std::make_shared<Image>(*img));
			m->materials[i].tex[slot] = (int32_t)m->images.size() - 1;
			return 1;
		}
	}
	return 0;
}

} // extern "C"
