// k_resolve and its views twin (RaylibAMD_RenderViews), one source for both: a translation unit includes this file with RL_VIEWS_TWIN 0 for the
// one-view kernel (rl_render.hip) or 1 for the twin (rl_render_views.hip); prototypes and default template arguments: rl_kernels.h.  The twin takes the view table (DViews) as one more
// trailing argument; everything under RL_VIEWS_TWIN is the twin's alone, so that the
// one-view kernel is the token sequence it always was (a template flag would add an inlining level, which reorders the one-view kernel's code:
// tools/isa_equivalence.py).

// Sequential per-pixel sum of this batch's samples, then (last batch) the mean.
// reference render/renderer.cc:244-248 + core/vec3.h:214-220 (operator/= multiplies by 1/SPP)
__global__ void __launch_bounds__(RL_BLOCK)
#if RL_VIEWS_TWIN
// The twin: the slots are the batch's (DViews), a culled cell's sky lookups use its own view's camera, and the output is view-major (view v's row-major
// frame at out + v * width * height)
k_resolve_views(const DRenderParams Pb, const DSceneView S, const SkyRot R, const SampleRGB* __restrict__ samples, float4* __restrict__ accum, float4* __restrict__ out,
                int firstBatch, int lastBatch, const DViews V)
#else
k_resolve(const DRenderParams P, const DSceneView S, const SkyRot R, const SampleRGB* __restrict__ samples, float4* __restrict__ accum, float4* __restrict__ out, int firstBatch, int lastBatch)
#endif
{
	RL_MATH_PROLOGUE();
#if RL_VIEWS_TWIN
	const uint32_t numSlots = Pb.numLocalCells * 64u;
#else
	const uint32_t numSlots = P.numLocalCells * 64u;
#endif
	const uint32_t slot = blockIdx.x * RL_BLOCK + threadIdx.x;
	if (slot >= numSlots) return;
	const uint32_t p = slot & 63u, cellLocal = slot >> 6;
#if RL_VIEWS_TWIN
	uint32_t cell;
	const uint32_t view = DecodeView(V, cellLocal, cell);
	DRenderParams P = Pb; P.camera = V.cameras[view];   // (SumSlotBatch generates a culled cell's camera rays from P.camera)
#else
	const uint32_t cell = P.cellFirst + cellLocal * P.cellStride;
#endif
	const uint32_t x = (cell % P.cellsX) * 8u + (p & 7u), y = (cell / P.cellsX) * 8u + (p >> 3);
	const bool valid = x < P.width && y < P.height;
	float4 a = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
	if (valid) {
		if (!firstBatch) a = accum[slot];
		a = SumSlotBatch(P, S, R, samples, numSlots, slot, cellLocal, x, y, a, [](float, float, float) __attribute__((always_inline)) {});
		if (lastBatch) {
			const float k = rtm::rcp1_((float)P.spp);
			a.x *= k; a.y *= k; a.z *= k; a.w = 1.0f;
		} else {
			accum[slot] = a;
		}
	}
	if (lastBatch) {
#if RL_VIEWS_TWIN
		if (valid) out[((size_t)view * P.height + y) * P.width + x] = a;
#else
		if (P.rowMajorOutput) { if (valid) out[(size_t)y * P.width + x] = a; }
		else out[slot] = valid ? a : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#endif
	}
}
