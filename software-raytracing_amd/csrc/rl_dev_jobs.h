// Device library, part 5 of 6: from a job number to a camera ray and back to a pixel -- the camera, the job decoding (one view and a batch of
// views), the job list sharded over the XCDs, the megakernels' argument reload, and the per-slot sum of the resolve kernels.
#pragma once

#include "rl_dev_shade.h"

namespace rl {

// ---------------------------------------------------------------------------
// Camera::GetCameraRay (reference render/camera.h:44-53)
__device__ __forceinline__ void CameraRay(const DCamera& k, float s, float t, Rng& g, V3& o, V3& d, float& rayTime)
{
	V3 rd;
	if (k.lensRadius == 0.0f) {
		// Pinhole: lensRadius * RandomInUnitDisk() is a vector of zeros.  Only their SIGNS can still matter (a +-0 offset decides
		// the sign of an exactly-zero direction component), and those follow from the signs of cos/sin of the lens angle, which
		// do not need the polynomials.  The two draws are consumed as always (reference core/random.cc:42-50).
		(void)Next(g);
		const float u2 = Next(g);
		const float theta = 2.0f * 3.14159265358979323846f * u2;
		bool sn, cn; rtm::sincos_signs_(theta, &sn, &cn);
		rd = k.lensRadius * v3(cn ? -1.0f : 1.0f, sn ? -1.0f : 1.0f, 0.0f);
	} else {
		rd = k.lensRadius * RandomInUnitDisk(g);
	}
	V3 cu = ld3(k.u), cv = ld3(k.v);
	V3 offset = (cu * rd.x) + (cv * rd.y);
	float captureTime = k.beginTime + k.timePeriod * Next(g);
	rayTime = captureTime;   // ray.t: consumed by the moving Cube primitive (geom/cube.cc:5), inherited by scattered rays
	V3 origin = ld3(k.origin);
	o = origin + offset;
	d = normalize(ld3(k.top_left) + s * ld3(k.horizontal) + (1.0f - t) * ld3(k.vertical) - origin - offset);
}

// GenerateCell's pixel -> [0, 1) coordinates, reference render/renderer.cc:232-239:  u = x / W, v = y / H, each plus (Next() - 0.5) * 2 / W resp. H from the second
// sample on: four divisions by two constants of the launch, 144 issue cycles per camera ray.  With P.invWidth = RN(1 / W) they are rtm::div_by_'s 6 each, and its
// conditions hold without a guard: W, H are integers in [1, 2^32] as floats, the numerators are +0 or integers below 2^32 or multiples of 2^-23 in (-1, 1)
// (Next() is a multiple of 2^-24; x - 0.5 == 0 is +0) -- every quotient is +0 or at least 2^-55 in magnitude.
__device__ __forceinline__ void PixelUV(const DRenderParams& P, uint32_t x, uint32_t y, uint32_t sampleIndex, Rng& g, float& u, float& v)
{
	const float imageWidth = (float)P.width, imageHeight = (float)P.height;
	u = rtm::div_by_((float)x, imageWidth, P.invWidth);
	v = rtm::div_by_((float)y, imageHeight, P.invHeight);
	if (sampleIndex != 0) {
		u += rtm::div_by_((Next(g) - 0.5f) * 2.0f, imageWidth, P.invWidth);
		v += rtm::div_by_((Next(g) - 0.5f) * 2.0f, imageHeight, P.invHeight);
	}
}

__device__ __forceinline__ SampleRGB make_sample(float x, float y, float z) { SampleRGB s; s.x = x; s.y = y; s.z = z; return s; }

// job -> (local cell, sample, pixel in cell) -> image coordinates
struct JobPixel { uint32_t x, y, slot, sample; bool valid; };
__device__ __forceinline__ JobPixel DecodeJob(const DRenderParams& P, uint32_t job)
{
	JobPixel j;
	const uint32_t p = job & 63u;
	const uint32_t rest = job >> 6;
	// n / d with d fixed per launch: q = mulhi(n, floor(2^32 / d)) is at most a few short; correct it
	uint32_t cellLocal = __umulhi(rest, P.magicSamples);
	uint32_t sLocal = rest - cellLocal * P.sampleCount;
	while (sLocal >= P.sampleCount) { sLocal -= P.sampleCount; ++cellLocal; }
#ifdef RL_EXP_STRIPS
	{   // experiment (whole frames whose cell columns divide by the heads only): a head's cells are a vertical STRIP of the frame, walked row by row
		const uint32_t cph = P.jobsPerHead / (P.sampleCount * 64u), hh = cellLocal / cph, ii = cellLocal % cph, sw = P.cellsX / P.numHeads;
		cellLocal = (ii / sw) * P.cellsX + hh * sw + ii % sw;
	}
#endif
	if (P.activeCells) cellLocal = P.activeCells[cellLocal];   // the job list holds the cells that can see the scene only (rl_device.h)
	const uint32_t cell = P.cellFirst + cellLocal * P.cellStride;
	uint32_t cy = __umulhi(cell, P.magicCellsX);
	uint32_t cx = cell - cy * P.cellsX;
	while (cx >= P.cellsX) { cx -= P.cellsX; ++cy; }
	j.x = cx * 8u + (p & 7u); j.y = cy * 8u + (p >> 3);
	j.slot = cellLocal * 64u + p;
	j.sample = sLocal;
	j.valid = (j.x < P.width) && (j.y < P.height);
	return j;
}

// The same for 64 consecutive jobs from a base that is a multiple of 64 (the leaf-list kernel's batches): one cell at one sample, the lane is the pixel.
// Everything but the pixel's coordinates is wave-uniform -- scalar arithmetic and, for the list of cells that can see the scene, a scalar load (the list
// is written before the launch: constant address space) -- where the per-lane form spends ~25 VALU instructions and a vector load whose s_waitcnt
// also waits for the wave's stores in flight.
__device__ __forceinline__ JobPixel DecodeJobBatch(const DRenderParams& P, uint32_t base, uint32_t lane)
{
	JobPixel j;
	const uint32_t rest = (uint32_t)__builtin_amdgcn_readfirstlane((int)base) >> 6;
	uint32_t cellLocal = __umulhi(rest, P.magicSamples);
	uint32_t sLocal = rest - cellLocal * P.sampleCount;
	while (sLocal >= P.sampleCount) { sLocal -= P.sampleCount; ++cellLocal; }
	if (P.activeCells) cellLocal = *(const __attribute__((address_space(4))) uint32_t*)(P.activeCells + cellLocal);
	const uint32_t cell = P.cellFirst + cellLocal * P.cellStride;
	uint32_t cy = __umulhi(cell, P.magicCellsX);
	uint32_t cx = cell - cy * P.cellsX;
	while (cx >= P.cellsX) { cx -= P.cellsX; ++cy; }
	j.x = cx * 8u + (lane & 7u); j.y = cy * 8u + (lane >> 3);
	j.slot = cellLocal * 64u + lane;
	j.sample = sLocal;
	j.valid = (j.x < P.width) && (j.y < P.height);
	return j;
}

// ---- the views twins (DViews): a batch cell is (view, cell of that view's frame) ----
// batch cell -> view (one more multiply-high, corrected as for cellsX) and the cell inside the view
__device__ __forceinline__ uint32_t DecodeView(const DViews& V, uint32_t batchCell, uint32_t& cellInView)
{
	uint32_t view = __umulhi(batchCell, V.magicCellsPerView);
	uint32_t c = batchCell - view * V.cellsPerView;
	while (c >= V.cellsPerView) { c -= V.cellsPerView; ++view; }
	cellInView = c;
	return view;
}
// DecodeJob of a views launch: the pixel of the view's own frame (its stream index and PixelUV are that frame's), the slot of the batch
__device__ __forceinline__ JobPixel DecodeJobViews(const DRenderParams& P, const DViews& V, uint32_t job, uint32_t& view)
{
	JobPixel j;
	const uint32_t p = job & 63u;
	const uint32_t rest = job >> 6;
	uint32_t cellLocal = __umulhi(rest, P.magicSamples);
	uint32_t sLocal = rest - cellLocal * P.sampleCount;
	while (sLocal >= P.sampleCount) { sLocal -= P.sampleCount; ++cellLocal; }
	if (P.activeCells) cellLocal = P.activeCells[cellLocal];
	uint32_t cell;
	view = DecodeView(V, cellLocal, cell);
	uint32_t cy = __umulhi(cell, P.magicCellsX);
	uint32_t cx = cell - cy * P.cellsX;
	while (cx >= P.cellsX) { cx -= P.cellsX; ++cy; }
	j.x = cx * 8u + (p & 7u); j.y = cy * 8u + (p >> 3);
	j.slot = cellLocal * 64u + p;
	j.sample = sLocal;
	j.valid = (j.x < P.width) && (j.y < P.height);
	return j;
}
// DecodeJobBatch of a views launch: the batch is one (cell, sample), so the view is wave-uniform (scalar registers)
__device__ __forceinline__ JobPixel DecodeJobBatchViews(const DRenderParams& P, const DViews& V, uint32_t base, uint32_t lane, uint32_t& view)
{
	JobPixel j;
	const uint32_t rest = (uint32_t)__builtin_amdgcn_readfirstlane((int)base) >> 6;
	uint32_t cellLocal = __umulhi(rest, P.magicSamples);
	uint32_t sLocal = rest - cellLocal * P.sampleCount;
	while (sLocal >= P.sampleCount) { sLocal -= P.sampleCount; ++cellLocal; }
	if (P.activeCells) cellLocal = *(const __attribute__((address_space(4))) uint32_t*)(P.activeCells + cellLocal);
	uint32_t cell;
	view = DecodeView(V, cellLocal, cell);
	uint32_t cy = __umulhi(cell, P.magicCellsX);
	uint32_t cx = cell - cy * P.cellsX;
	while (cx >= P.cellsX) { cx -= P.cellsX; ++cy; }
	j.x = cx * 8u + (lane & 7u); j.y = cy * 8u + (lane >> 3);
	j.slot = cellLocal * 64u + lane;
	j.sample = sLocal;
	j.valid = (j.x < P.width) && (j.y < P.height);
	return j;
}
// A view's camera: per lane (a vector load; the table is at most 64 x 96 bytes and stays in the caches) or, for a wave-uniform view, through the
// scalar cache (the table is written before the launch: constant address space)
__device__ __forceinline__ DCamera LoadViewCamera(const DViews& V, uint32_t view) { return V.cameras[view]; }
__device__ __forceinline__ DCamera LoadViewCameraUniform(const DViews& V, uint32_t view)
{
	DCamera k;
	__builtin_memcpy(&k, (const __attribute__((address_space(4))) DCamera*)(V.cameras + (uint32_t)__builtin_amdgcn_readfirstlane((int)view)), sizeof(DCamera));
	return k;
}

// ---------------------------------------------------------------------------
// The job list, sharded over the chip's XCDs.  An MI355X is 8 XCDs with a private, non-coherent 4 MiB L2 each; workgroups are dealt
// round-robin over them (MI355X_MICROARCH.md "Workgroup dispatch, XCD placement").  The job list (cell-major: all samples of local cell 0,
// then cell 1, ...) is cut into P.numHeads contiguous ranges of P.jobsPerHead jobs -- whole cells, so a range is a horizontal BAND of the
// frame (of this rank's cells) -- each behind a head word of its own, 128 bytes apart.  A wave draws from the head of the XCD it runs
// on (s_getreg HW_REG_XCC_ID): the camera rays an XCD's L2 sees come from one eighth of the image, i.e. they walk one region's part of
// the tree and its triangles, and eight words share the atomic traffic that one hot address took before.  When its own band is used up
// a wave steals from the band with the most jobs left (eight sc1 loads by eight lanes, a 3-step lane max), so the launch's end is
// worked on by everybody.  Heads count RELATIVE to their band's first job, so the host resets the whole queue with one memset.
// Results cannot depend on any of this: streams are keyed by (seed, pixel, sample).
// The reference's analogue is the single LIFO work queue of core/thread_pool.cc:93-112.
#define RL_HEAD_STRIDE 32u   /* uint32 words between two heads (128 B: one L2 line each) */
__device__ __forceinline__ uint32_t XccId()
{
	return (uint32_t)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u;   // GETREG_IMMED(size - 1 = 3, offset 0, XCC_ID = 20): bits 3:0 of XCC_ID
}
struct JobSource { uint32_t cur, dry, left; };   // wave-uniform: the head this wave draws from; bit h: head h is known to be used up (it stays so); jobs that were left in `cur` after this wave's last draw
__device__ __forceinline__ JobSource JobSourceInit(const DRenderParams& P)
{
	JobSource js; js.cur = P.numHeads > 1u ? XccId() % P.numHeads : 0u; js.dry = 0u; js.left = 0xffffffffu;
	return js;
}
__device__ __forceinline__ uint32_t HeadLength(const DRenderParams& P, uint32_t h)
{
	const uint32_t first = h * P.jobsPerHead;   // (numHeads * jobsPerHead stays below 2^32: host side)
	return first < P.numJobs ? min(P.jobsPerHead, P.numJobs - first) : 0u;
}
// `want` (a multiple of 64) consecutive jobs for this wave: true with [base, end) set, false when every band is used up.  Wave-uniform.
__device__ __forceinline__ bool TakeJobs(const DRenderParams& P, unsigned int* __restrict__ heads, JobSource& js, uint32_t want, uint32_t lane, uint32_t& base, uint32_t& end)
{
	for (;;) {
		const uint32_t len = HeadLength(P, js.cur);
		// The end of a band in smaller pieces (P.guideShift > 0): a draw is at most 1 / 2^guideShift of what was left in the band after this
		// wave's previous draw there -- about half of "what is left / waves drawing from it" -- so that when the list runs dry a wave
		// holds a few batches, not a whole chunk of what may be the frame's dearest cells.  No extra read of the head: the size comes from
		// the wave's own last atomic (a stale upper bound: the band only shrinks).
		uint32_t ask = want;
		if (P.guideShift) ask = min(want, max(64u, (js.left >> P.guideShift) & ~63u));
		uint32_t rel = 0;
		if (lane == 0) rel = atomicAdd(&heads[js.cur * RL_HEAD_STRIDE], ask);
		rel = (uint32_t)__builtin_amdgcn_readfirstlane((int)rel);
		if (rel < len) {
			base = js.cur * P.jobsPerHead + rel; end = base + min(ask, len - rel);
			js.left = len - rel - min(ask, len - rel);
			return true;
		}
		js.dry |= 1u << js.cur;
		if (P.numHeads <= 1u) return false;
		// the fullest of the other bands.  A head only grows, so a stale value can only make a band look fuller than it is: the atomic
		// above then says so and the band is marked; "every band looks used up" is never wrong.
		uint32_t key = 0;
		if (lane < P.numHeads && !((js.dry >> lane) & 1u)) {
			const uint32_t nx = __hip_atomic_load(&heads[lane * RL_HEAD_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			const uint32_t ln = HeadLength(P, lane);
			key = nx < ln ? ((ln - nx) | lane) : 0u;   // jobs left (a multiple of 64) with the head's number in the low bits
		}
		key = max(key, (uint32_t)__shfl_xor((int)key, 1));
		key = max(key, (uint32_t)__shfl_xor((int)key, 2));
		key = max(key, (uint32_t)__shfl_xor((int)key, 4));
		key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
		if (key < 64u) return false;
		js.cur = key & 7u; js.left = key & ~63u;
	}
}

__device__ __forceinline__ void WaveLdsSync()
{
	// LDS operations of one wave are executed in issue order; this only stops the compiler from moving LDS
	// accesses of different lanes' data across the point.
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// The megakernels' arguments are ~110 dwords of scalars (render parameters, camera, scene view, sky rotation, pointers).  The compiler loads them
// all at the kernel's entry and keeps them for its whole life -- in 102 SGPRs that the loops' own masks and counters need too: 50 of them went straight
// to VGPR lanes (v_writelane), and every later use was a v_readlane, four VALU issue cycles each, ~400 of them in k_trace's code (6 per record of the
// leaf list's box loop, 7 per pick, 9 per Newton iteration of the sampler ...), on a kernel that is bound by exactly that port.  RL_ARGS() reads them
// again from the kernel-argument segment where a part of the loop needs them (s_load through the scalar cache: no VALU slot, and three other waves
// to cover its latency): the offset goes through an empty asm statement, so that the loads can neither be hoisted out of the loop nor merged with
// the previous part's, and what they fetch dies with the block.  RL_KARG_RELOAD=0: the arguments as the compiler delivers them.
#ifndef RL_KARG_RELOAD
#define RL_KARG_RELOAD 1
#endif
struct KTraceArgs { DRenderParams P; DSceneView S; SkyRot R; SampleRGB* samples; float* pathStack; unsigned long long* counters; unsigned int* jobCounter; };
template <class T> __device__ __forceinline__ T KArg(uint32_t offset)
{
	uint32_t z = 0u;
	asm volatile("" : "+s"(z));
	T v;
	__builtin_memcpy(&v, (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + offset + (z << 2), sizeof(T));   // (z << 2: the compiler must see a dword-aligned address to take the scalar path)
	return v;
}
#if RL_KARG_RELOAD
#define RL_ARGS() \
	const DRenderParams P = KArg<DRenderParams>((uint32_t)offsetof(KTraceArgs, P)); const DSceneView S = KArg<DSceneView>((uint32_t)offsetof(KTraceArgs, S)); \
	const SkyRot R = KArg<SkyRot>((uint32_t)offsetof(KTraceArgs, R)); SampleRGB* const samples = KArg<SampleRGB*>((uint32_t)offsetof(KTraceArgs, samples)); \
	float* const pathStack = KArg<float*>((uint32_t)offsetof(KTraceArgs, pathStack)); unsigned long long* const counters = KArg<unsigned long long*>((uint32_t)offsetof(KTraceArgs, counters)); \
	unsigned int* const jobCounter = KArg<unsigned int*>((uint32_t)offsetof(KTraceArgs, jobCounter)); \
	(void)P; (void)S; (void)R; (void)samples; (void)pathStack; (void)counters; (void)jobCounter
#else
#define RL_ARGS() \
	const DRenderParams& P = Pk; const DSceneView& S = Sk; const SkyRot& R = Rk; SampleRGB* const samples = samplesK; float* const pathStack = pathStackK; \
	unsigned long long* const counters = countersK; unsigned int* const jobCounter = jobCounterK; \
	(void)P; (void)S; (void)R; (void)samples; (void)pathStack; (void)counters; (void)jobCounter
#endif
// The views twins' arguments: KTraceArgs and the view table behind it, so that RL_ARGS() reads the same offsets in both
struct KTraceViewsArgs { KTraceArgs A; DViews V; };
#if RL_KARG_RELOAD
#define RL_VIEWS() const DViews VW = KArg<DViews>((uint32_t)offsetof(KTraceViewsArgs, V)); (void)VW
#else
#define RL_VIEWS() const DViews& VW = Vk; (void)VW
#endif

// The lazy instance's arguments: KTraceArgs and the lit list behind it
struct KTraceLazyArgs { KTraceArgs A; DLitList LL; };
#if RL_KARG_RELOAD
#define RL_LIT_ARGS() const DLitList LL = KArg<DLitList>((uint32_t)offsetof(KTraceLazyArgs, LL)); (void)LL
#else
#define RL_LIT_ARGS() const DLitList& LL = LLk; (void)LL
#endif

// One slot's samples of this batch added to `a` in sample order -- the megakernel's from the sample buffer, or, for a cell outside the scene's silhouette,
// the miss shader's value every one of them comes to -- and each sample's RGB handed to `each` (k_resolve: nothing; k_progressive_resolve: the
// luminance moments of its stopping rule).
template <class EACH>
__device__ __forceinline__ float4 SumSlotBatch(const DRenderParams& P, const DSceneView& S, const SkyRot& R, const SampleRGB* samples,
                                               uint32_t numSlots, uint32_t slot, uint32_t cellLocal, uint32_t x, uint32_t y, float4 a, EACH&& each)
{
	if (P.cellEmpty && P.cellEmpty[cellLocal]) {
		// a cell outside the scene's silhouette (rl_cull.cc): none of its samples can meet the scene, every one of them is the miss shader's value -- the sun's
		// illuminance or nothing, the same for all; with a sky panorama the texel its camera ray points at on top (renderer.cc:155-199), so the ray is
		// generated here exactly as the megakernel generates it (same stream, same draws: jitter, lens, shutter) -- added up sample by sample as if stored
		if (P.emptySky) {
			Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
			for (uint32_t s = 0; s < P.sampleCount; ++s) {
				const uint32_t sidx = P.sampleBegin + s;
				Rng g; g.s = raylib_rng_begin_mixed(P.seedMixed, y * P.width + x, sidx);
				float u, v;
				PixelUV(P, x, y, sidx, g, u, v);
				V3 o, d; float rayTime;
				CameraRay(P.camera, u, v, g, o, d, rayTime);
				V3 L = MissSky(S, R, d, c);
				if (S.hasSun) L = L + ld3(S.sunIlluminance);
				a.x += L.x; a.y += L.y; a.z += L.z;
				each(L.x, L.y, L.z);
			}
		} else
		for (uint32_t s = 0; s < P.sampleCount; ++s) { a.x += P.emptyL[0]; a.y += P.emptyL[1]; a.z += P.emptyL[2]; each(P.emptyL[0], P.emptyL[1], P.emptyL[2]); }
	} else
	for (uint32_t s = 0; s < P.sampleCount; ++s) {
		const SampleRGB v = samples[(size_t)s * numSlots + slot];
		a.x += v.x; a.y += v.y; a.z += v.z;
		each(v.x, v.y, v.z);
	}
	return a;
}

} // namespace rl
