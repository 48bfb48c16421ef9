// Host runtime: the test hooks -- arrays of the caller's through one kernel on rank 0's stream and back (rl_rt.h).  Their device buffers are locals: whatever
// way a hook leaves, they are freed.
#include "rl_rt.h"

namespace rl {

// `kernel` on rank 0's stream over `blocks` workgroups of `threads`, the launch checked and the stream waited for
template <typename... P, typename... A>
static bool RunOnRank0(void (*kernel)(P...), uint32_t blocks, uint32_t threads, A... args)
{
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, Rank0().stream, args...);
	return hipGetLastError() == hipSuccess && hipStreamSynchronize(Rank0().stream) == hipSuccess;
}
static uint32_t BlocksFor(int n) { return ((uint32_t)n + RL_BLOCK - 1) / RL_BLOCK; }
template <typename T>
static bool Download(T* host, const T* dev, size_t count) { return hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess; }

bool DeviceClosestHit(Scene& sc, const float* rays, int32_t n, float tMin, void* outHits)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (sc.bvh.depth > 64) { Log("RaylibAMD_ClosestHit: BVH depth %u exceeds the traversal stack (64)", sc.bvh.depth); return false; }
	if (!UploadScene(sc)) return false;
	if (n <= 0) return true;
	DevBuf<float> dRays; DevBuf<DHitOut> dOut;
	const DSceneView& view = sc.device->copy[(size_t)R.devSlot]->view;
	bool ok = dRays.Upload(rays, (size_t)n * 6) && dOut.Grow((size_t)n * sizeof(DHitOut));
	ok = ok && RunOnRank0(sc.bvh.depth <= 32 ? k_closest_hit<32, true> : k_closest_hit<64, true>, BlocksFor(n), RL_BLOCK, view, dRays.ptr, n, tMin, dOut.ptr);
	ok = ok && Download((DHitOut*)outHits, dOut.ptr, (size_t)n);
	if (!ok) Log("RaylibAMD_ClosestHit: a HIP call failed");
	return ok;
}

// kind 0: scatter (in 16 / out 16 floats per record, a = material), 1: camera rays (in 2 / out 7), 2: texture (in 2 / out 4, a = texture, b = sRGB)
bool DeviceEvalHook(int kind, Scene* sc, const DCamera* cam, int a, int b, const float* in, int n, uint64_t seed, float* out)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	RankCtx& R = Rank0();
	HIP_OK(hipSetDevice(R.device));
	if (sc && !UploadScene(*sc)) return false;
	if (n <= 0) return true;
	const size_t inW = kind == 0 ? 16 : 2, outW = kind == 0 ? 16 : (kind == 1 ? 7 : 4);
	DevBuf<float> din, dout;
	if (!din.Upload(in, (size_t)n * inW) || !dout.Grow((size_t)n * outW * sizeof(float))) return false;
	bool ok;
	if (kind == 0) ok = RunOnRank0(k_eval_scatter, BlocksFor(n), RL_BLOCK, sc->device->copy[(size_t)R.devSlot]->view, a, din.ptr, n, (unsigned long long)seed, dout.ptr);
	else if (kind == 1) ok = RunOnRank0(k_eval_camera, BlocksFor(n), RL_BLOCK, *cam, din.ptr, n, (unsigned long long)seed, dout.ptr);
	else ok = RunOnRank0(k_eval_texture, BlocksFor(n), RL_BLOCK, sc->device->copy[(size_t)R.devSlot]->view, a, b, din.ptr, n, dout.ptr);
	return ok && Download(out, dout.ptr, (size_t)n * outW);
}

bool DeviceEvalMath(int fn, const float* x, const float* y, int n, float* out)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	if (n <= 0) return true;
	DevBuf<float> dx, dy, dout;
	if (!dx.Upload(x, (size_t)n) || !dout.Grow((size_t)n * sizeof(float)) || (y && !dy.Upload(y, (size_t)n))) return false;
	return RunOnRank0(k_eval_math, BlocksFor(n), RL_BLOCK, fn, dx.ptr, dy.ptr, n, dout.ptr) && Download(out, dout.ptr, (size_t)n);
}

bool DeviceVerifyExactMath(int which, uint64_t* outMismatches, uint64_t* outFirst)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	unsigned long long h[2] = { 0ull, ~0ull };
	DevBuf<unsigned long long> d;
	if (!d.Upload(h, 2)) return false;
	const bool ok = RunOnRank0(k_verify_exact_math, 4096, RL_BLOCK, which, d.ptr) && Download(h, d.ptr, 2);
	if (outMismatches) *outMismatches = h[0];
	if (outFirst) *outFirst = h[1];
	return ok;
}

// the ranged sampler's sweeps (rl_render_lazy.hip): all 2^32 bit patterns in one launch, as DeviceVerifyExactMath's
bool DeviceVerifySamplerRanged(int mode, uint64_t out[6])
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	unsigned long long h[6] = { 0ull, ~0ull, 0ull, 0ull, 0ull, 0ull };
	DevBuf<unsigned long long> d;
	if (!d.Upload(h, 6)) return false;
	const bool ok = RunOnRank0(k_verify_sampler_ranged, 4096, RL_BLOCK, mode, d.ptr) && Download(h, d.ptr, 6);
	for (int k = 0; k < 6; ++k) out[k] = h[k];
	return ok;
}

// the ranged normalisations' sweeps (rl_render_lazy.hip), launched the same way
bool DeviceVerifyNormalizeRanged(int mode, uint64_t out[4])
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	unsigned long long h[4] = { 0ull, ~0ull, ~0ull, 0ull };
	DevBuf<unsigned long long> d;
	if (!d.Upload(h, 4)) return false;
	const bool ok = RunOnRank0(k_verify_normalize_ranged, 4096, RL_BLOCK, mode, d.ptr) && Download(h, d.ptr, 4);
	for (int k = 0; k < 4; ++k) out[k] = h[k];
	return ok;
}

// the two sweeps of the lazy instance's guards: three counts each
static bool VerifyLazySweep(void (*kernel)(uint32_t, unsigned long long, unsigned long long*), uint32_t n, uint64_t seed, uint64_t out[3])
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	unsigned long long h[3] = { 0ull, 0ull, 0ull };
	DevBuf<unsigned long long> d;
	if (!d.Upload(h, 3)) return false;
	const uint32_t blocks = std::max(1u, std::min(1024u, (n + RL_BLOCK - 1) / RL_BLOCK));
	const bool ok = RunOnRank0(kernel, blocks, RL_BLOCK, n, (unsigned long long)seed, d.ptr) && Download(h, d.ptr, 3);
	for (int k = 0; k < 3; ++k) out[k] = h[k];
	return ok;
}
bool DeviceVerifyLazyRefl(uint32_t n, uint64_t seed, uint64_t out[3]) { return VerifyLazySweep(k_verify_lazy_refl, n, seed, out); }
bool DeviceVerifyLazyPdf(uint32_t n, uint64_t seed, uint64_t out[3]) { return VerifyLazySweep(k_verify_lazy_pdf, n, seed, out); }

// The lists of a progressive session after a pass, from arrays of the caller's.  The launch is EnqueueFrame's (one workgroup of RL_COMPACT_BLOCK threads on rank 0's
// stream); the kernel writes live and trace in place, entries at indices <= their own, so numLive entries of each suffice.
bool DeviceProgressiveCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const uint8_t* emptyOrNull, uint32_t numCells,
                                  uint32_t width, uint32_t height, uint32_t* outLive, uint32_t* outTrace, uint32_t outCounts[4])
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	DevBuf<uint32_t> dLive, dTrace, dCounts; DevBuf<uint8_t> dStopped, dEmpty;
	uint32_t counts[4] = { 0, 0, 0, 0 };
	if (!dLive.Upload(live, numLive) || !dTrace.Grow(std::max<size_t>(1, numLive) * sizeof(uint32_t)) || !dCounts.Grow(sizeof(counts))) return false;
	if (!dStopped.Upload(stopped, numCells) || (emptyOrNull && !dEmpty.Upload(emptyOrNull, numCells))) return false;
	bool ok = RunOnRank0(k_progressive_compact, 1, RL_COMPACT_BLOCK, dLive.ptr, dTrace.ptr, (const uint8_t*)dStopped.ptr, (const uint8_t*)dEmpty.ptr, numLive, width, height, (width + 7) / 8, dCounts.ptr);
	ok = ok && Download(counts, dCounts.ptr, 4);
	ok = ok && counts[1] <= counts[0] && counts[0] <= numLive;   // (nothing is copied past the caller's arrays, whatever the kernel says)
	ok = ok && (counts[0] == 0 || Download(outLive, dLive.ptr, counts[0])) && (counts[1] == 0 || Download(outTrace, dTrace.ptr, counts[1]));
	if (ok) memcpy(outCounts, counts, sizeof(counts));
	return ok;
}

// The live set of an adaptive gather after a pass, from arrays of the caller's.  The launches are an adaptive GatherLocked's (EnqueueGatherCompact on rank 0's stream): the
// live points' records go up contiguous, record i beside live[i], as a pass holds them.  The output buffers on the device have numLive entries -- the kernels write
// count <= numLive of them.
bool DeviceGatherCompactTest(const uint32_t* live, uint32_t numLive, const uint8_t* stopped, const RaylibAMDGatherPoint* points, uint32_t numPoints,
                             uint32_t* outLive, RaylibAMDGatherPoint* outPoints, uint32_t* outCount)
{
	std::lock_guard<std::mutex> lk(Rt().lock);
	if (!EnsureRuntime()) return false;
	HIP_OK(hipSetDevice(Rank0().device));
	if (numLive == 0) { *outCount = 0; return true; }
	std::vector<RaylibAMDGatherPoint> rec(numLive);
	for (uint32_t i = 0; i < numLive; ++i) rec[i] = points[live[i]];
	DevBuf<uint32_t> dLive, dOutLive, dTiles; DevBuf<uint8_t> dStopped; DevBuf<float4> dPoints, dOutPoints; PinBuf<uint32_t> count;
	const uint32_t numTiles = (uint32_t)(((uint64_t)numLive + RL_GATHER_COMPACT_TILE - 1) / RL_GATHER_COMPACT_TILE);
	if (!dLive.Upload(live, numLive) || !dStopped.Upload(stopped, numPoints) || !dPoints.Upload((const float4*)rec.data(), (size_t)numLive * 2)) return false;
	if (!dOutLive.Grow((size_t)numLive * sizeof(uint32_t)) || !dOutPoints.Grow((size_t)numLive * 2 * sizeof(float4)) || !dTiles.Grow(((size_t)numTiles + 1) * sizeof(uint32_t))
	    || !count.Grow(sizeof(uint32_t))) return false;
	const hipStream_t st = Rank0().stream;
	bool ok = EnqueueGatherCompact(dLive.ptr, numLive, dStopped.ptr, dPoints.ptr, dOutLive.ptr, dOutPoints.ptr, dTiles.ptr, count.ptr, st);
	ok = (hipStreamSynchronize(st) == hipSuccess) && ok;
	const uint32_t c = ok ? count.ptr[0] : 0u;
	ok = ok && c <= numLive;   // (nothing is copied past the caller's arrays, whatever the kernels say)
	ok = ok && (c == 0 || (Download(outLive, dOutLive.ptr, c) && Download((float4*)outPoints, (const float4*)dOutPoints.ptr, (size_t)c * 2)));
	if (ok) *outCount = c;
	return ok;
}

} // namespace rl
