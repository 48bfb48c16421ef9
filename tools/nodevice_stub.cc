// Sanitizer harness only (tools/asan_host_check.sh and the stand-alone *_host_check programs of tools/host_check.sh): stands in for the HIP units -- the kernels and the host runtime
// that launches them (csrc/rl_rt_*.hip), every Device* entry of csrc/rl_host.h -- so that the HOST side of the library (ABI, OBJ/MTL loader, BVH builder,
// scene flattening, planner, codecs, registries) can be built with g++ -fsanitize=address,undefined.  Never part of libraylib.so.
#include "rl_host.h"
namespace rl {
bool DeviceAvailable() { return false; }
bool DeviceRender(Scene&, const RenderRequest&, RaylibAMDStats&) { return false; }
bool DeviceRenderViews(Scene&, const RenderRequest&, const DCamera*, uint32_t, void*, void* const*, RaylibAMDStats&) { return false; }
bool DeviceClosestHit(Scene&, const float*, int32_t, float, void*) { return false; }
bool DeviceTraceRays(Scene&, int32_t, const void*, int32_t, float, void*, int32_t*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceRenderGBuffer(Scene&, const RendererSettings&, const DCamera&, uint64_t, const RaylibAMDGBufferPlanes&, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceRenderMotion(Scene&, const RendererSettings&, const DCamera&, const DCamera&, uint64_t, int32_t, int32_t, const float*, const RaylibAMDMotionPlanes&, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceTemporalAccumulate(const TemporalCall&, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceFilterVariance(uint32_t, uint32_t, const RaylibAMDVarianceFilterParams&, const RaylibAMDVarianceFilterPlanes&, float*, float*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceTraceRaysAll(Scene&, const void*, int32_t, int32_t, void*, uint32_t*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceNearestPoints(Scene&, int32_t, const void*, int32_t, void*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceSweepSpheres(Scene&, int32_t, const void*, int32_t, void*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceNearestPointsAll(Scene&, const void*, int32_t, int32_t, void*, uint32_t*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceBakeDistanceField(Scene&, const RaylibAMDDistanceFieldParams&, float*, int32_t*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceOverlapTriangles(Scene&, int32_t, uint32_t, const void*, int32_t, int32_t, void*, uint32_t*, bool, void*, RaylibAMDStats&, void*, bool) { return false; }
bool DeviceOverlapBoxes(Scene&, int32_t, const void*, int32_t, int32_t, void*, uint32_t*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceTraceRadiance(Scene&, const RaylibAMDRadianceParams&, uint64_t, const void*, int32_t, float*, bool, void*, RaylibAMDStats&) { return false; }
bool DeviceGather(Scene&, int32_t, const RaylibAMDRadianceParams&, uint64_t, const void*, int32_t, float*, bool, void*, RaylibAMDStats&, const RaylibAMDGatherAdaptiveParams*,
                  uint32_t*) { return false; }
int64_t DeviceLightmapPoints(Scene&, const RaylibAMDLightmapParams&, int32_t, int32_t, const float*, RaylibAMDGatherPoint*, uint32_t*, int64_t) { return -1; }
bool DeviceBakeLightmap(const char*, Scene&, const RaylibAMDLightmapParams&, int32_t, int32_t, const RaylibAMDRadianceParams&, uint64_t, const float*, float*, uint8_t*, bool, void*, RaylibAMDStats&,
                        const RaylibAMDLightmapFilterParams*, const float*, const RaylibAMDGatherAdaptiveParams*, uint32_t*) { return false; }
bool DeviceGatherCompactTest(const uint32_t*, uint32_t, const uint8_t*, const RaylibAMDGatherPoint*, uint32_t, uint32_t*, RaylibAMDGatherPoint*, uint32_t*) { return false; }
// rl_lightmap_filter.hip is a HIP unit too: its host restatement (RaylibAMD_FilterLightmapHost) is not part of this build
bool FilterLightmapHost(int32_t, int32_t, int32_t, const RaylibAMDLightmapFilterParams&, const RaylibAMDGatherPoint*, const uint32_t*, int64_t, const float*, float*) { return false; }
bool DevicePostProcess(Image&) { return false; }
void* DeviceImagePixels(Image&) { return nullptr; }
bool DeviceReadback(Image&) { return false; }
bool DeviceDumpRGB(Image&, float*) { return false; }
void DeviceFreePixels(void*) {}
bool DeviceEvalMath(int, const float*, const float*, int, float*) { return false; }
bool DeviceEvalHook(int, Scene*, const DCamera*, int, int, const float*, int, uint64_t, float*) { return false; }
void DeviceReleaseScene(DeviceScene*) {}
bool DeviceMoveTriangles(Scene&, int32_t, int32_t, const float*, const float*, bool, void*) { return false; }
bool DeviceSyncMovedScene(Scene&) { return true; }   // (never uploaded: the host's copies are the scene)
bool DeviceCheckTrees(Scene&, uint32_t*) { return false; }
bool DeviceCompareTrees(Scene&, uint32_t*) { return false; }
int DeviceNumRanks() { return 0; }
bool DeviceDrain(RaylibAMDStats*) { return false; }
void DeviceOwnStats() {}
int32_t DeviceLastTracePlain() { return 0; }
int32_t DeviceLastTraceLazy() { return 0; }
int32_t DeviceLastHitQueue() { return 0; }
int32_t DeviceLastLitMask() { return 0; }
bool DeviceVerifyLazyRefl(uint32_t, uint64_t, uint64_t*) { return false; }
bool DeviceVerifyLazyPdf(uint32_t, uint64_t, uint64_t*) { return false; }
bool DeviceVerifyExactMath(int, uint64_t*, uint64_t*) { return false; }
bool DeviceVerifySamplerRanged(int, uint64_t*) { return false; }
bool DeviceVerifyNormalizeRanged(int, uint64_t*) { return false; }
// rl_denoise.hip is a HIP unit too: the device filter fails, and its host restatement (RaylibAMD_DenoiseHost) is not part of this build
bool DeviceDenoise(Image&, bool, Image*, Image*, Image&, const RaylibAMDDenoiseParams&) { return false; }
void DenoiseHost(uint32_t, uint32_t, const float*, bool, const float*, const float*, const RaylibAMDDenoiseParams&, float*) {}
ProgressiveSession* DeviceProgressiveBegin(Scene&, const RenderRequest&, float, uint32_t) { return nullptr; }
int32_t DeviceProgressiveStep(ProgressiveSession&, uint32_t, void*, RaylibAMDStats&, bool& rendered) { rendered = false; return -1; }
bool DeviceProgressiveExport(ProgressiveSession&, uint32_t*, uint8_t*, float*, float*) { return false; }
void DeviceProgressiveEnd(ProgressiveSession*) {}
bool DeviceProgressiveCompactTest(const uint32_t*, uint32_t, const uint8_t*, const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*) { return false; }
}
