// Host runtime: a flattened scene (rl_scene.cc FlattenScene) on every device in use, its sky and wide trees; and the images, which live on rank 0's
// device -- read-back, the RGB dump, post-processing (rl_rt.h).
#include "rl_rt.h"

namespace rl {

// the wide tree a render is about to walk (TracePlan::tree), on this rank's device: UploadScene puts the default plan's there (TracePlan::eagerTree), the other
// follows the first time a render asks for it.  The copy's pointers are set only once the tree is there.
template <typename T>
static bool UploadOnce(DevBuf<T>& have, const T*& inView, const std::vector<T>& src)
{
	if (have.ptr || src.empty()) return true;
	if (!have.Upload(src.data(), src.size())) { have.Free(); return false; }
	inView = have.ptr;
	return true;
}
bool EnsureWideTree(DeviceSceneCopy* C, Scene& sc, int32_t tree)
{
	// (after a move the host's wide trees are behind the device's binary tree: they are re-derived before one of them is uploaded for the first time)
	if ((tree == TREE_WIDE8 ? !C->nodes8.ptr : tree == TREE_GRID4 ? !C->nodes4.ptr : false) && !SyncMovedLocked(sc)) return false;
	if (tree == TREE_WIDE8) return UploadOnce(C->nodes8, C->view.nodes8, sc.bvh.nodes8);
	if (tree == TREE_GRID4) return UploadOnce(C->nodes4, C->view.nodes4, sc.bvh.nodes4q);
	return true;
}
static void FreeScene(DeviceScene* D)
{
	if (!D) return;
	for (DeviceSceneCopy* C : D->copy) { (void)hipSetDevice(C->device); delete C; }   // (a copy's buffers go with it, on its device)
	delete D;
	if (Rt().ok) (void)hipSetDevice(Rt().devices[0]);
}

// A copy of the flattened scene (device records in leaf order) to every device in use.
bool UploadScene(Scene& sc)
{
	if (sc.device) return SettleMove(sc);
	for (size_t i = 0; i < sc.textures.size(); ++i) {
		Image& im = *sc.textures[i];
		if (!im.hostStale) continue;   // a rendered image used as a texture: fetch it
		if (!ReadbackLocked(im)) Log("UploadScene: texture %zu could not be read back from the device", i);
		im.hostStale = false;
	}
	const FlatScene F = FlattenScene(sc);
	const size_t n = sc.triangles.size();
	DeviceScene* D = new DeviceScene;
	static uint64_t s_serial = 0;
	D->serial = ++s_serial;   // (under the runtime lock)
	D->skyRot = F.skyRot;
	// the float-box wide nodes (and the leaf list) for scenes small enough to stay in the caches (k_trace's class); of the two wide trees the pool schedule can walk, the
	// one the default plan walks goes to the device now, the other follows when a render asks for it (EnsureWideTree: the switches are read per render).  A 10 M-triangle
	// scene keeps 190 MB of nodes per device instead of 290.
	const bool wantFull = !sc.bvh.nodes4.empty() && n < RL_FLOAT_BOX_MAX_TRIS;
	const int32_t eager = EagerTree(sc);
	for (size_t slot = 0; slot < Rt().devices.size(); ++slot) {
		DeviceSceneCopy* C = new DeviceSceneCopy;
		C->device = Rt().devices[slot];
		memset(&C->view, 0, sizeof(C->view));
		D->copy.push_back(C);
		bool ok = hipSetDevice(C->device) == hipSuccess;
		ok = ok && C->nodes.Upload(sc.bvh.nodes.data(), sc.bvh.nodes.size());
		if (ok && eager == TREE_GRID4) ok = C->nodes4.Upload(sc.bvh.nodes4q.data(), sc.bvh.nodes4q.size());
		if (ok && eager == TREE_WIDE8) ok = C->nodes8.Upload(sc.bvh.nodes8.data(), sc.bvh.nodes8.size());
		if (ok && wantFull) ok = C->nodes4f.Upload(sc.bvh.nodes4.data(), sc.bvh.nodes4.size());
		if (ok && wantFull && !sc.bvh.leafList.empty()) ok = C->leafList.Upload(sc.bvh.leafList.data(), sc.bvh.leafList.size());
		ok = ok && C->isect.Upload(F.isect.data(), n) && C->shade.Upload(F.shade.data(), n);
		if (ok && !F.alphaTex.empty()) ok = C->alphaTex.Upload(F.alphaTex.data(), F.alphaTex.size());
		ok = ok && C->materials.Upload(F.materials.data(), F.materials.size()) && C->textures.Upload(F.textures.data(), F.textures.size()) && C->texels.Upload(F.texels.data(), F.texels.size());
		ok = ok && C->spheres.Upload(F.spheres.data(), F.spheres.size()) && C->cubes.Upload(F.cubes.data(), F.cubes.size());
		if (!ok) { Log("UploadScene: device %d could not take the scene", C->device); FreeScene(D); return false; }   // nothing of a failed upload is left behind
		DSceneView& V = C->view;
		V.nodes = C->nodes.ptr; V.nodes4 = C->nodes4.ptr; V.nodes4f = C->nodes4f.ptr; V.nodes8 = C->nodes8.ptr; V.isect = C->isect.ptr; V.shade = C->shade.ptr; V.alphaTex = C->alphaTex.ptr; V.materials = C->materials.ptr;
		V.textures = C->textures.ptr; V.numTextures = (int32_t)F.textures.size(); V.texels = C->texels.ptr; V.spheres = C->spheres.ptr; V.cubes = C->cubes.ptr;
		V.sunIlluminance[0] = sc.sunIlluminance.x; V.sunIlluminance[1] = sc.sunIlluminance.y; V.sunIlluminance[2] = sc.sunIlluminance.z;
		V.sunDirection[0] = sc.sunDirection.x; V.sunDirection[1] = sc.sunDirection.y; V.sunDirection[2] = sc.sunDirection.z;
		V.sky = nullptr; V.skyWidth = V.skyHeight = 0;
		V.hasSun = !(sc.sunIlluminance.x == 0.0f && sc.sunIlluminance.y == 0.0f && sc.sunIlluminance.z == 0.0f);   // renderer.cc:192
		V.numTriangles = (int32_t)n;
		V.numNodes4 = (int32_t)sc.bvh.nodes4.size(); V.numMaterials = (int32_t)F.materials.size();
		V.leafList = C->leafList.ptr; V.numLeafRecords = C->leafList.ptr ? (int32_t)sc.bvh.leafList.size() : 0;
		V.fastBary = F.fastBary;
		V.numNodes8 = (int32_t)sc.bvh.nodes8.size();
	}
	HIP_OK(hipSetDevice(Rt().devices[0]));
	sc.device = D;
	return true;
}

// The sky panorama as it is NOW: the reference reads the image through the handle at every miss (renderer.cc:159-176), so pixels
// written after Raylib_FinalizeScene / Raylib_SetSkyPanorama are seen by the next render.  Only the sky texels move; triangles,
// BVH and textures stay where they are.  A frame that was rendered into the image and never left the device is copied on it.
bool SyncSky(Scene& sc)
{
	DeviceScene* D = sc.device;
	Image* sky = sc.sky;
	for (DeviceSceneCopy* C : D->copy) {
		if (!sky || (size_t)sky->width * sky->height == 0) { C->view.sky = nullptr; C->view.skyWidth = C->view.skyHeight = 0; C->skyImage = nullptr; continue; }
		if (C->skyImage == sky && C->skyVersion == sky->version && C->view.sky) continue;
		const size_t bytes = (size_t)sky->width * sky->height * sizeof(float4);
		(void)DrainLocked();   // a frame in flight reads the texels that are about to be replaced
		HIP_OK(hipSetDevice(C->device));
		if (!C->sky.Grow(bytes)) return false;
		if (sky->hostStale && sky->devValid && sky->devPixels) {
			HIP_OK(hipMemcpyPeer(C->sky.ptr, C->device, sky->devPixels, Rank0().device, bytes));   // images live on rank 0's device
		} else {
			HIP_OK(hipMemcpy(C->sky.ptr, sky->rgba.data(), bytes, hipMemcpyHostToDevice));
		}
		C->skyImage = sky; C->skyVersion = sky->version;
		C->view.sky = (const float*)C->sky.ptr; C->view.skyWidth = (int32_t)sky->width; C->view.skyHeight = (int32_t)sky->height;
	}
	HIP_OK(hipSetDevice(Rt().devices[0]));
	return true;
}

void DeviceReleaseScene(DeviceScene* D)
{
	if (!D) return;
	std::lock_guard<std::mutex> lk(Rt().lock);
	(void)DrainLocked();   // frames in flight read this scene
	FreeScene(D);
}

// Images live on rank 0's device.
void* DeviceImagePixels(Image& img)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return nullptr;
	const size_t need = (size_t)img.width * img.height * sizeof(float4);
	if (need == 0) return nullptr;
	if (img.devPixels && img.devBytes >= need) return img.devPixels;
	(void)DrainLocked();   // a frame in flight may be writing the buffer that is about to be freed
	if (hipSetDevice(Rank0().device) != hipSuccess) return nullptr;
	if (img.devPixels) { (void)hipFree(img.devPixels); img.devPixels = nullptr; img.devBytes = 0; }
	if (hipMalloc(&img.devPixels, need) != hipSuccess) { img.devPixels = nullptr; return nullptr; }
	img.devBytes = need;
	img.devValid = false;
	return img.devPixels;
}

bool DeviceReadback(Image& img)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	return ReadbackLocked(img);
}
bool ReadbackLocked(Image& img)
{
	const size_t n = (size_t)img.width * img.height;
	if (n == 0) return true;
	if (!Rt().ok || !img.devPixels || !img.devValid || img.devBytes < n * sizeof(float4)) return false;
	if (!DrainLocked()) Log("Image read-back: a frame in flight did not complete");
	HIP_OK(hipSetDevice(Rank0().device));
	img.rgba.resize(n * 4);
	HIP_OK(hipMemcpyAsync(img.rgba.data(), img.devPixels, n * sizeof(float4), hipMemcpyDeviceToHost, Rank0().stream));
	HIP_OK(hipStreamSynchronize(Rank0().stream));
	return true;
}


// Raylib_DumpImageData for a frame that lives on the device (reference raylib.h:90-93: the caller's buffer of 3 * 4 * w * h bytes; in the reference the pixels
// are in host memory when Raylib_Render returns, renderer.cc:292-296, so this copy is part of what a front-end sees of a render).  k_pack_rgb packs RGB on
// the device; the packed frame crosses the bus in chunks into PINNED staging memory (a pageable destination makes the runtime stage the copy through its own
// small buffers: 12 GB/s measured in round 3); helper threads copy every chunk on to the caller's memory as soon as its event has fired, so the host copies
// run beside the rest of the transfer.  img.rgba stays stale: another reader fetches its own copy (Image::SyncHost).
struct DumpStage {
	DevBuf<float> packed;     // device: RGB, 12 bytes per pixel
	PinBuf<float> pinned;     // host, page-locked
	hipEvent_t ev[16] = {};
	bool evReady = false;
	std::vector<Worker*> helpers;
};
bool DeviceDumpRGB(Image& img, float* outDest)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	const size_t n = (size_t)img.width * img.height;
	if (n == 0) return true;
	if (!Rt().ok || !img.devPixels || !img.devValid || img.devBytes < n * sizeof(float4)) return false;
	if (const char* e = getenv("RAYLIB_FAST_DUMP")) if (atoi(e) == 0) return false;   // the plain path: read RGBA back, pack on the host
	if (!DrainLocked()) Log("Raylib_DumpImageData: a frame in flight did not complete");
	RankCtx& R = Rank0();
	static DumpStage& D = *new DumpStage;   // (kept for the process, as the runtime: rl_rt.h Runtime)
	HIP_OK(hipSetDevice(R.device));
	const size_t bytes = n * 3 * sizeof(float);
	if (!D.packed.Grow((bytes + 15) & ~(size_t)15) || !D.pinned.Grow(bytes)) return false;
	if (!D.evReady) { for (hipEvent_t& e : D.ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); D.evReady = true; }
	const uint32_t blocks = (uint32_t)(((n + 3) / 4 + RL_BLOCK - 1) / RL_BLOCK);
	hipLaunchKernelGGL(k_pack_rgb, dim3(blocks), dim3(RL_BLOCK), 0, R.stream, (const float4*)img.devPixels, (float4*)D.packed.ptr, D.packed.ptr, n);
	HIP_OK(hipGetLastError());
	// chunks of ~2 MB (at most 16): the first host copy starts after 1/chunks of the transfer, the last one is all that is left when the transfer ends
	const size_t chunks = std::max<size_t>(1, std::min<size_t>(16, bytes / (2u << 20)));
	const size_t per = ((bytes / chunks) + 63) & ~(size_t)63;
	size_t nChunks = 0;
	for (size_t off = 0; off < bytes; off += per, ++nChunks) {
		const size_t len = std::min(per, bytes - off);
		HIP_OK(hipMemcpyAsync((char*)D.pinned.ptr + off, (const char*)D.packed.ptr + off, len, hipMemcpyDeviceToHost, R.stream));
		HIP_OK(hipEventRecord(D.ev[nChunks], R.stream));
	}
	// helper threads: chunk c is copied by helper c % (helpers + 1), the calling thread takes its share too
	const size_t wantHelpers = nChunks > 1 ? std::min<size_t>(3, std::max(1u, std::thread::hardware_concurrency()) - 1) : 0;
	while (D.helpers.size() < wantHelpers) { Worker* w = new Worker; w->Start(R.device); D.helpers.push_back(w); }
	const size_t lanes = wantHelpers + 1;
	auto copyLane = [outDest, per, bytes, nChunks, lanes](size_t lane) -> bool {
		bool ok = true;
		for (size_t c = lane; c < nChunks; c += lanes) {
			if (hipEventSynchronize(D.ev[c]) != hipSuccess) { ok = false; break; }
			const size_t off = c * per;
			memcpy((char*)outDest + off, (const char*)D.pinned.ptr + off, std::min(per, bytes - off));
		}
		return ok;
	};
	for (size_t h = 0; h < wantHelpers; ++h) D.helpers[h]->Post([&copyLane, h]() { return copyLane(h + 1); });
	bool ok = copyLane(0);
	for (size_t h = 0; h < wantHelpers; ++h) ok = D.helpers[h]->Wait() && ok;
	if (!ok) { Log("Raylib_DumpImageData: the device copy failed"); (void)hipStreamSynchronize(R.stream); return false; }
	return true;
}

void DeviceFreePixels(void* p)
{
	if (!p) return;
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (Rt().ok) { (void)DrainLocked(); (void)hipSetDevice(Rank0().device); (void)hipFree(p); }
}

// Image2D::PostProcess (reference render/image.cc:44-103) on the device: k_pp_max finds the white point
// (max is exact in any order), k_pp_map applies extended Reinhard on luminance, the clamp and gamma 1/2.2
// with glibc's exact powf.  Bit-identical to the host statement of the same function.
bool DevicePostProcess(Image& img)
{
	const size_t n = (size_t)img.width * img.height;
	if (n == 0) return true;
	float4* px = (float4*)DeviceImagePixels(img);
	if (!px) return false;
	std::lock_guard<std::mutex> lk(Rt().lock);
	(void)DrainLocked();   // the frame this works on may still be in flight on the gather stream
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (!img.devValid) HIP_OK(hipMemcpyAsync(px, img.rgba.data(), n * sizeof(float4), hipMemcpyHostToDevice, R.stream));   // (never stale here: stale implies devValid)
	unsigned int one; { float f = 1.0f; memcpy(&one, &f, 4); }
	HIP_OK(hipMemcpyAsync(R.jobCounter.ptr, &one, sizeof(one), hipMemcpyHostToDevice, R.stream));
	const uint32_t blocks = (uint32_t)std::min<size_t>((n + RL_BLOCK - 1) / RL_BLOCK, 2048);
	hipLaunchKernelGGL(k_pp_max, dim3(blocks), dim3(RL_BLOCK), 0, R.stream, px, n, R.jobCounter.ptr);
	HIP_OK(hipGetLastError());
	hipLaunchKernelGGL(k_pp_map, dim3((uint32_t)((n + RL_BLOCK - 1) / RL_BLOCK)), dim3(RL_BLOCK), 0, R.stream, px, n, R.jobCounter.ptr);
	HIP_OK(hipGetLastError());
	float white = 1.0f;
	HIP_OK(hipMemcpyAsync(&white, R.jobCounter.ptr, 4, hipMemcpyDeviceToHost, R.stream));
	HIP_OK(hipStreamSynchronize(R.stream));
	img.devValid = true;
	img.hostStale = true;   // read back when the pixels are asked for (Image::SyncHost)
	img.Touch();
	Log("Max white luminance: %f", white);
	return true;
}

} // namespace rl
