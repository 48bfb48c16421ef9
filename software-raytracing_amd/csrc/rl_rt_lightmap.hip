// Host runtime: lightmaps (RaylibAMD_LightmapPoints, RaylibAMD_BakeLightmap, RaylibAMD_BakeLightmapDevice; include/raylib_amd.h) on rank 0's device.
// The raster stages (rl_lightmap.hip: setup, the counts' scan, cover, the flags, their scan, the points) run on the library's stream and are waited for -- the
// host must know the number of points before it can plan the gather --; a bake then enters DeviceGather's body (rl_rt_rays.hip GatherLocked) with the points
// on the device, and puts the scatter, the dilation's passes and the copies into the caller's memory behind it, on the call's stream.  A filtered bake
// (RaylibAMD_BakeLightmapFiltered) puts statement F's iterations (rl_lightmap_filter.hip) between the gather and the scatter, on the points' values in compacted
// form; RaylibAMD_FilterLightmap takes those values from the caller's atlas instead of a gather; RaylibAMD_BakeLightmapAdaptive gathers them in passes with
// per-texel stopping (GatherLocked with the adaptive parameters) and scatters the texels' sample counts into an atlas of their own.  The scratch is the rank's (rl_rt.h RankCtx lm*: the raster's
// records, counts and maps, the points, their texels and values, the filter's second array of values, the two atlases and coverage maps), ordered by the
// radiance calls' event: a call waits for it before its first kernel and records it behind its last.
#include "rl_rt.h"
#include "rl_lightmap.h"

#include <stdlib.h>

namespace rl {

#define RL_LM_COVER_PAIRS (1ull << 30)   /* (triangle, texel) pairs per launch of k_lm_cover: its grid index stays within 32 bits; a call makes at most RL_LM_MAX_PAIRS / this = 64 */
static_assert(sizeof(HostTriangle) == 26 * sizeof(float), "a triangle record is 26 floats");

// the exclusive scan of data[0 .. n) in place, data[n] = the total: reduce, scan, add (rl_kernels.h); sums holds a value per tile and one more
template <typename T>
static bool ScanInPlace(T* data, uint64_t n, DevBuf<unsigned long long>& sums, hipStream_t st)
{
	const uint32_t tiles = (uint32_t)((n + RL_SCAN_TILE - 1) / RL_SCAN_TILE);   // (n <= 2^28 texels or 2^31 triangles: <= 2^20 tiles)
	if (!sums.Grow(((size_t)tiles + 1) * sizeof(unsigned long long))) return false;
	T* s = (T*)sums.ptr;
	hipLaunchKernelGGL(k_lm_scan_reduce<T>, dim3(tiles), dim3(RL_BLOCK), 0, st, (const T*)data, (unsigned long long)n, s);
	HIP_OK(hipGetLastError());
	hipLaunchKernelGGL(k_lm_scan_sums<T>, dim3(1), dim3(RL_SCAN_SUMS_BLOCK), 0, st, s, tiles);
	HIP_OK(hipGetLastError());
	hipLaunchKernelGGL(k_lm_scan_add<T>, dim3(tiles), dim3(RL_BLOCK), 0, st, data, (unsigned long long)n, (const T*)s, tiles);
	HIP_OK(hipGetLastError());
	return true;
}
static uint32_t BlocksFor(uint64_t n) { return (uint32_t)((n + RL_BLOCK - 1) / RL_BLOCK); }

// What the raster stages leave: the number of points, the pairs they tested, and in R.lmPoints / R.lmTexel the first min(count, capacity) records; R.lmRank
// holds the ranks of all texels (the scatter reads them).  The stream is idle when it returns.  timed: R.lmEv[0 .. 2] around the two halves.
struct LmRaster { uint64_t count = 0, pairs = 0; };
static bool Raster(Scene& sc, RankCtx& R, const RaylibAMDLightmapParams& P, int32_t triFirst, int32_t triCount, const float* uv, bool uvOnHost, uint64_t capacity, bool all,
                   bool timed, hipStream_t callerStream, LmRaster& out)
{
	if (!UploadScene(sc)) return false;
	DeviceSceneCopy* Cp = sc.device->copy[(size_t)R.devSlot];
	if ((!Cp->lmTris.ptr || Cp->lmTrisStale) && (!SyncMovedLocked(sc) || !Cp->lmTris.Upload((const float*)sc.triangles.data(), sc.triangles.size() * 26))) { Cp->lmTris.Free(); return false; }
	Cp->lmTrisStale = false;
	const hipStream_t st = R.stream;
	const uint32_t nTri = (uint32_t)triCount, nTex = (uint32_t)P.width * (uint32_t)P.height;   // (<= 2^28)
	if (!R.lmRec.Grow((size_t)nTri * sizeof(DLmTri)) || !R.lmCounts.Grow(((size_t)nTri + 1) * sizeof(unsigned long long)) || !R.lmHost.Grow(2 * sizeof(unsigned long long))) return false;
	if (!R.radEv) HIP_OK(hipEventCreateWithFlags(&R.radEv, hipEventDisableTiming));
	if (timed && !R.lmEv[0]) for (hipEvent_t& e : R.lmEv) HIP_OK(hipEventCreate(&e));
	if (R.radEvUsed) HIP_OK(hipStreamWaitEvent(st, R.radEv, 0));   // a bake enqueued on a caller's stream may still be using the scratch
	if (callerStream && callerStream != st) {
		// the caller's uv may still be in the making on the caller's stream: the raster stages, which read it on the library's stream, go behind whatever is
		// enqueued there now -- as RaylibAMD_GatherDevice's kernels, which run on the caller's stream, are behind it by themselves
		if (!R.lmInEv) HIP_OK(hipEventCreateWithFlags(&R.lmInEv, hipEventDisableTiming));
		HIP_OK(hipEventRecord(R.lmInEv, callerStream));
		HIP_OK(hipStreamWaitEvent(st, R.lmInEv, 0));
	}
	const float* dUv = uv;
	if (uv && uvOnHost) {
		if (!R.lmUv.Grow((size_t)nTri * 6 * sizeof(float))) return false;
		HIP_OK(hipMemcpyAsync(R.lmUv.ptr, uv, (size_t)nTri * 6 * sizeof(float), hipMemcpyHostToDevice, st));
		dUv = R.lmUv.ptr;
	}
	const float* dTris = Cp->lmTris.ptr + (size_t)triFirst * 26;
	if (timed) HIP_OK(hipEventRecord(R.lmEv[0], st));
	hipLaunchKernelGGL(k_lm_setup, dim3(BlocksFor(nTri)), dim3(RL_BLOCK), 0, st, dTris, dUv, nTri, P.width, P.height, R.lmRec.ptr, R.lmCounts.ptr);
	HIP_OK(hipGetLastError());
	if (!ScanInPlace<unsigned long long>(R.lmCounts.ptr, nTri, R.lmSums, st)) return false;
	HIP_OK(hipMemcpyAsync(R.lmHost.ptr, R.lmCounts.ptr + nTri, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	out.pairs = R.lmHost.ptr[0];
	if (out.pairs > RL_LM_MAX_PAIRS) {
		Log("lightmap: %llu (triangle, texel) pairs exceed the %llu a call tests -- many triangles whose boxes span the atlas (INTEGRATION.md section 3g); bake them in ranges",
		    (unsigned long long)out.pairs, (unsigned long long)RL_LM_MAX_PAIRS);
		return false;
	}
	// the maps of the atlas' size only now: a refused call allocates neither
	if (!R.lmOwner.Grow((size_t)nTex * sizeof(uint32_t)) || !R.lmRank.Grow(((size_t)nTex + 1) * sizeof(uint32_t))) return false;
	HIP_OK(hipMemsetAsync(R.lmOwner.ptr, 0xff, (size_t)nTex * sizeof(uint32_t), st));
	for (uint64_t base = 0; base < out.pairs; base += RL_LM_COVER_PAIRS) {
		const uint32_t pairs = (uint32_t)std::min<uint64_t>(RL_LM_COVER_PAIRS, out.pairs - base);
		hipLaunchKernelGGL(k_lm_cover, dim3(BlocksFor(pairs)), dim3(RL_BLOCK), 0, st, (const DLmTri*)R.lmRec.ptr, (const unsigned long long*)R.lmCounts.ptr, nTri,
		                   (unsigned long long)base, pairs, P.width, nTex, R.lmOwner.ptr);
		HIP_OK(hipGetLastError());
	}
	if (timed) HIP_OK(hipEventRecord(R.lmEv[1], st));
	hipLaunchKernelGGL(k_lm_points<false>, dim3(BlocksFor(nTex)), dim3(RL_BLOCK), 0, st, (const DLmTri*)R.lmRec.ptr, dTris, (const uint32_t*)R.lmOwner.ptr, R.lmRank.ptr, P.width, nTex,
	                   P.time, (float4*)nullptr, (uint32_t*)nullptr, 0ull);
	HIP_OK(hipGetLastError());
	if (!ScanInPlace<uint32_t>(R.lmRank.ptr, nTex, R.lmSums, st)) return false;
	HIP_OK(hipMemcpyAsync(R.lmHost.ptr + 1, R.lmRank.ptr + nTex, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	out.count = (uint64_t)*(const uint32_t*)(R.lmHost.ptr + 1);
	const uint64_t keep = all ? out.count : std::min<uint64_t>(out.count, capacity);
	if (keep) {
		if (!R.lmPoints.Grow((size_t)keep * 2 * sizeof(float4)) || !R.lmTexel.Grow((size_t)keep * sizeof(uint32_t))) return false;
		hipLaunchKernelGGL(k_lm_points<true>, dim3(BlocksFor(nTex)), dim3(RL_BLOCK), 0, st, (const DLmTri*)R.lmRec.ptr, dTris, (const uint32_t*)R.lmOwner.ptr, R.lmRank.ptr, P.width, nTex,
		                   P.time, R.lmPoints.ptr, R.lmTexel.ptr, (unsigned long long)keep);
		HIP_OK(hipGetLastError());
	}
	if (timed) HIP_OK(hipEventRecord(R.lmEv[2], st));
	HIP_OK(hipStreamSynchronize(st));
	return true;
}

int64_t DeviceLightmapPoints(Scene& sc, const RaylibAMDLightmapParams& P, int32_t triFirst, int32_t triCount, const float* uv,
                             RaylibAMDGatherPoint* outPoints, uint32_t* outTexel, int64_t capacity)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return -1;
	RankCtx& R = Rank0();
	if (hipSetDevice(R.device) != hipSuccess) return -1;
	LmRaster r;
	if (!Raster(sc, R, P, triFirst, triCount, uv, true, (uint64_t)capacity, false, false, nullptr, r)) return -1;
	const size_t keep = (size_t)std::min<uint64_t>(r.count, (uint64_t)capacity);
	if (keep) {
		if (hipMemcpy(outPoints, R.lmPoints.ptr, keep * sizeof(RaylibAMDGatherPoint), hipMemcpyDeviceToHost) != hipSuccess) return -1;
		if (outTexel && hipMemcpy(outTexel, R.lmTexel.ptr, keep * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
	}
	return (int64_t)r.count;
}

// statement F on the points' values, K iterations between R.lmValues and R.lmFilt (rl_lightmap_filter.hip); `values`: where the last one left them
template <int C>
static bool EnqueueFilter(RankCtx& R, const RaylibAMDLightmapParams& P, const RaylibAMDLightmapFilterParams& F, uint32_t count, hipStream_t st, const float*& values)
{
	const LmFilterInv inv = MakeLmFilterInv(F);
	float* buf[2] = { R.lmValues.ptr, R.lmFilt.ptr };
	int cur = 0;
	for (int32_t i = 0; i < F.iterations && count; ++i, cur ^= 1) {
		hipLaunchKernelGGL(k_lm_filter<C>, dim3(BlocksFor(count)), dim3(RL_BLOCK), 0, st, (const uint32_t*)R.lmRank.ptr, (const uint32_t*)R.lmTexel.ptr, (const float4*)R.lmPoints.ptr,
		                   (const float*)buf[cur], buf[cur ^ 1], count, P.width, P.height, 1 << i, inv.invC[i], inv.invN, inv.invP[i], i == 0 ? 1 : 0);
		HIP_OK(hipGetLastError());
	}
	values = buf[cur];
	return true;
}

template <int C>
static bool EnqueueAtlas(RankCtx& R, const RaylibAMDLightmapParams& P, uint32_t nTex, hipStream_t st, const float* values, int& last)
{
	hipLaunchKernelGGL(k_lm_scatter<C>, dim3(BlocksFor(nTex)), dim3(RL_BLOCK), 0, st, (const uint32_t*)R.lmRank.ptr, values, nTex, R.lmAtlas[0].ptr, R.lmCov[0].ptr);
	HIP_OK(hipGetLastError());
	last = 0;
	for (int32_t k = 1; k <= P.dilate; ++k) {
		hipLaunchKernelGGL(k_lm_dilate<C>, dim3(BlocksFor(nTex)), dim3(RL_BLOCK), 0, st, (const float*)R.lmAtlas[last].ptr, (const uint8_t*)R.lmCov[last].ptr,
		                   R.lmAtlas[last ^ 1].ptr, R.lmCov[last ^ 1].ptr, P.width, P.height, k);
		HIP_OK(hipGetLastError());
		last ^= 1;
	}
	return true;
}

// RaylibAMD_FilterLightmap's statement 7: the covered texels' values from the caller's atlas.  A host atlas goes through R.lmAtlas[0], which the scatter
// overwrites only behind this on the same stream; a device atlas is read where it is, before the call's last copy writes `out` (which may be `in`).
template <int C>
static bool EnqueueTake(RankCtx& R, uint32_t nTex, const float* in, bool hostMem, hipStream_t st)
{
	const float* src = in;
	if (hostMem) {
		HIP_OK(hipMemcpyAsync(R.lmAtlas[0].ptr, in, (size_t)nTex * C * sizeof(float), hipMemcpyHostToDevice, st));
		src = R.lmAtlas[0].ptr;
	}
	hipLaunchKernelGGL(k_lm_take<C>, dim3(BlocksFor(nTex)), dim3(RL_BLOCK), 0, st, (const uint32_t*)R.lmRank.ptr, src, nTex, R.lmValues.ptr);
	HIP_OK(hipGetLastError());
	return true;
}

bool DeviceBakeLightmap(const char* who, Scene& sc, const RaylibAMDLightmapParams& P, int32_t triFirst, int32_t triCount, const RaylibAMDRadianceParams& prm, uint64_t seed,
                        const float* uv, float* out, uint8_t* outCoverage, bool hostMem, void* stream, RaylibAMDStats& stats,
                        const RaylibAMDLightmapFilterParams* filter, const float* in, const RaylibAMDGatherAdaptiveParams* adaptive, uint32_t* outSamples)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	const bool sphere = P.gather.kind == RAYLIB_AMD_GATHER_SH9;
	const uint32_t C = sphere ? 27u : 4u, nTex = (uint32_t)P.width * (uint32_t)P.height;
	if (!hostMem) {
		if (!OnDevice(out, R.device) || (uv && !OnDevice(uv, R.device)) || (outCoverage && !OnDevice(outCoverage, R.device)) || (in && !OnDevice(in, R.device))
		    || (outSamples && !OnDevice(outSamples, R.device))) {
			Log("%s: a pointer is not device memory of device %d", who, R.device);
			return false;
		}
		if (((uintptr_t)out & 3u) != 0 || ((uintptr_t)uv & 3u) != 0 || ((uintptr_t)in & 3u) != 0 || ((uintptr_t)outSamples & 3u) != 0) {
			Log("%s: uv, the input or an output is not 4-byte aligned", who);
			return false;
		}
	}
	const bool sync = !stream;
	const size_t atlasBytes = (size_t)nTex * C * sizeof(float);
	// everything the call allocates, before anything is enqueued (growing frees, and hipFree waits for the device)
	if (!R.lmAtlas[0].Grow(atlasBytes) || !R.lmCov[0].Grow(nTex)) return false;
	if (P.dilate > 0 && (!R.lmAtlas[1].Grow(atlasBytes) || !R.lmCov[1].Grow(nTex))) return false;
	if (adaptive && outSamples && !R.lmSampleAtlas.Grow((size_t)nTex * sizeof(uint32_t))) return false;
	LmRaster r;
	if (!Raster(sc, R, P, triFirst, triCount, uv, hostMem, 0, true, sync, (hipStream_t)stream, r)) return false;
	const size_t valueBytes = std::max<size_t>(1, (size_t)r.count) * C * sizeof(float);
	if (!R.lmValues.Grow(valueBytes) || (filter && !R.lmFilt.Grow(valueBytes))) return false;
	if (adaptive && outSamples && !R.lmSamples.Grow(std::max<size_t>(1, (size_t)r.count) * sizeof(uint32_t))) return false;
	const hipStream_t st = stream ? (hipStream_t)stream : R.stream;
	bool ok = true;
	if (!in) {
		// statement 7: DeviceGather's body on the points, on the call's stream -- with `adaptive` as A1 to A5 --; a synchronous call returns from it with the gather's
		// stats and an idle stream, an adaptive one with the last pass complete
		if (!GatherLocked(sc, R, P.gather.kind, prm, seed, R.lmPoints.ptr, (int32_t)r.count, R.lmValues.ptr, false, stream, t0, stats, adaptive, adaptive && outSamples ? R.lmSamples.ptr : nullptr)) return false;
		if (adaptive && outSamples) {
			// the counts through the ranks into their atlas, undilated: 0 where no point is
			hipLaunchKernelGGL(k_gather_scatter_counts, dim3(BlocksFor(nTex)), dim3(RL_BLOCK), 0, st, (const uint32_t*)R.lmRank.ptr, (const uint32_t*)R.lmSamples.ptr, nTex, R.lmSampleAtlas.ptr);
			HIP_TRY(hipGetLastError());
		}
	} else {
		// ... or the caller's atlas.  (The raster waited for the scratch's event and for its own stream: nothing else holds the scratch now.)
		memset(&stats, 0, sizeof(stats));
		OneRankStats(stats, sc);
		ok = sphere ? EnqueueTake<27>(R, nTex, in, hostMem, st) : EnqueueTake<4>(R, nTex, in, hostMem, st);
	}
	if (ok && sync) HIP_TRY(hipEventRecord(R.lmEv[3], st));
	const float* values = R.lmValues.ptr;
	if (ok && filter) ok = sphere ? EnqueueFilter<27>(R, P, *filter, (uint32_t)r.count, st, values) : EnqueueFilter<4>(R, P, *filter, (uint32_t)r.count, st, values);
	if (ok && sync) HIP_TRY(hipEventRecord(R.lmEv[4], st));
	int last = 0;
	ok = ok && (sphere ? EnqueueAtlas<27>(R, P, nTex, st, values, last) : EnqueueAtlas<4>(R, P, nTex, st, values, last));
	if (ok && sync) HIP_TRY(hipEventRecord(R.lmEv[5], st));
	const hipMemcpyKind kind = hostMem ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
	if (ok) HIP_TRY(hipMemcpyAsync(out, R.lmAtlas[last].ptr, atlasBytes, kind, st));
	if (ok && outCoverage) HIP_TRY(hipMemcpyAsync(outCoverage, R.lmCov[last].ptr, nTex, kind, st));
	if (ok && adaptive && outSamples) HIP_TRY(hipMemcpyAsync(outSamples, R.lmSampleAtlas.ptr, (size_t)nTex * sizeof(uint32_t), kind, st));
	// the event behind whatever was enqueued: the next call on any stream waits for it before it touches the scratch
	const hipError_t evErr = hipEventRecord(R.radEv, st);
	if (evErr == hipSuccess) R.radEvUsed = true;
	else { Log("HIP error %s recording the bake's event", hipGetErrorName(evErr)); (void)hipStreamSynchronize(st); }
	if (!ok || evErr != hipSuccess) return false;
	if (!sync) return true;
	HIP_OK(hipStreamSynchronize(st));
	// setup + scan + cover, points + compaction, gather (or the atlas taken), filter, scatter + dilate
	float ms[5] = { 0, 0, 0, 0, 0 }, whole = 0.0f;
	for (int k = 0; k < 5; ++k) HIP_OK(hipEventElapsedTime(&ms[k], R.lmEv[k], R.lmEv[k + 1]));
	HIP_OK(hipEventElapsedTime(&whole, R.lmEv[0], R.lmEv[5]));
	stats.pixels = r.count;
	stats.kernelMs = whole;
	stats.wallMs = MsSince(t0);
	const char* e = getenv("RAYLIB_LIGHTMAP_LOG");
	if (e && atoi(e) != 0) {
		char filt[64] = "";
		if (filter) snprintf(filt, sizeof(filt), "filter (%d iterations) %.3f ms, ", filter->iterations, ms[3]);
		Log("%s: %d x %d, %d triangles, %llu pairs in %llu launches of one pair per lane, %llu points | setup + scan + cover %.3f ms, points + compaction %.3f ms, "
		    "%s %.3f ms, %sscatter + dilate %.3f ms, whole %.3f ms", who, P.width, P.height, triCount, (unsigned long long)r.pairs,
		    (unsigned long long)((r.pairs + RL_LM_COVER_PAIRS - 1) / RL_LM_COVER_PAIRS), (unsigned long long)r.count, ms[0], ms[1], in ? "atlas taken" : adaptive ? "adaptive gather" : "gather", ms[2], filt, ms[4], whole);
	}
	return true;
}

} // namespace rl
