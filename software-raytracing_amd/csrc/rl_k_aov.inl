// k_aov and its views twin (RaylibAMD_RenderViews), one source for both: a translation unit includes this file with RL_VIEWS_TWIN 0 for the
// one-view kernel (rl_render.hip) or 1 for the twin (rl_render_views.hip); prototypes and default template arguments: rl_kernels.h.  The twin takes the view table (DViews) as one more
// trailing argument; everything under RL_VIEWS_TWIN is the twin's alone, so that the
// one-view kernel is the token sequence it always was (a template flag would add an inlining level, which reorders the one-view kernel's code:
// tools/isa_equivalence.py).

// Debug render modes (reference render/renderer.cc:62-111, :258-268): one unjittered sample.
// Modes 3 and 6 read an uninitialised tangent frame in the reference; here it is built.
template <int STACK, bool PRIMS>
__global__ void __launch_bounds__(RL_BLOCK)
#if RL_VIEWS_TWIN
// The twin: the slots are the batch's (DViews), each view's rays come from its own camera, and the output is view-major
k_aov_views(const DRenderParams P, const DSceneView S, float4* __restrict__ out, unsigned long long* __restrict__ counters, const DViews V)
#else
k_aov(const DRenderParams P, const DSceneView S, float4* __restrict__ out, unsigned long long* __restrict__ counters)
#endif
{
	RL_TEX_PROLOGUE(S);
	RL_MATH_PROLOGUE();
	__shared__ int s_stack[STACK * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	const uint32_t numSlots = P.numLocalCells * 64u;
	const uint32_t slot = blockIdx.x * RL_BLOCK + threadIdx.x;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	bool valid = false;
	uint32_t x = 0, y = 0;
#if RL_VIEWS_TWIN
	uint32_t view = 0;
	if (slot < numSlots) {
		const uint32_t p = slot & 63u, cellLocal = slot >> 6;
		uint32_t cell;
		view = DecodeView(V, cellLocal, cell);
#else
	if (slot < numSlots) {
		const uint32_t p = slot & 63u, cellLocal = slot >> 6;
		const uint32_t cell = P.cellFirst + cellLocal * P.cellStride;
#endif
		x = (cell % P.cellsX) * 8u + (p & 7u); y = (cell / P.cellsX) * 8u + (p >> 3);
		valid = x < P.width && y < P.height;
	}
	V3 debugValue = v3s(0.0f);
	if (valid) {
		Rng g; g.s = raylib_rng_begin(P.seed, y * P.width + x, 0);
		V3 o, d; float rayTime;
#if RL_VIEWS_TWIN
		CameraRay(LoadViewCamera(V, view), (float)x / (float)P.width, (float)y / (float)P.height, g, o, d, rayTime);
#else
		CameraRay(P.camera, (float)x / (float)P.width, (float)y / (float)P.height, g, o, d, rayTime);
#endif
		c.samples++;
		HitRec h;
		if (Traverse<STACK, false, PRIMS>(S, o, d, rayTime, P.rayTMin, h, stk, c)) {
			Surf s;
			const Mat m = LoadMat(S, BuildSurface<PRIMS>(S, o, d, h, s, true, c));
			const uint32_t mode = P.renderMode;
			if (mode == RAYLIB_RENDERMODE_Albedo) {
				debugValue = GetAlbedo(S, m, s.U, s.V, c);
				if (IsMirrorLike(S, m, s.U, s.V, c)) {
					HitRec h2;
					const V3 d2 = reflect(d, s.n);
					if (Traverse<STACK, false, PRIMS>(S, s.p, d2, rayTime, P.rayTMin, h2, stk, c)) {
						Surf s2;
						const Mat m2 = LoadMat(S, BuildSurface<PRIMS>(S, s.p, d2, h2, s2, false, c));
						debugValue = GetAlbedo(S, m2, s2.U, s2.V, c);
					}
				}
			} else if (mode == RAYLIB_RENDERMODE_SurfaceNormal) {
				debugValue = v3s(0.5f) + 0.5f * s.n;
			} else if (mode == RAYLIB_RENDERMODE_MicrosurfaceNormal) {
				V3 N = GetMicrosurfaceNormal(S, m, s, c);
				N = LocalToWorld(s, N);
				debugValue = 0.5f * N + 0.5f;
			} else if (mode == RAYLIB_RENDERMODE_Texcoord) {
				debugValue = v3(s.U, s.V, 0.0f);
			} else if (mode == RAYLIB_RENDERMODE_Emission) {
				debugValue = Emitted(S, m, s, c);
			} else if (mode == RAYLIB_RENDERMODE_Reflectance) {
				V3 refl = v3(1.0f, 0.75f, 0.8f), outD; float pdf, sp;
				Scatter(S, m, d, s, g, c, refl, outD, pdf, sp);
				debugValue = refl;
			}
		}
	}
	if (slot < numSlots) {
		const float4 px = make_float4(debugValue.x, debugValue.y, debugValue.z, 1.0f);
#if RL_VIEWS_TWIN
		if (valid) out[((size_t)view * P.height + y) * P.width + x] = px;
#else
		if (P.rowMajorOutput) { if (valid) out[(size_t)y * P.width + x] = px; }
		else out[slot] = valid ? px : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#endif
	}
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t vals[CNT_COUNT] = { c.rays, c.nodes, c.tris, c.shaded, c.texels, c.samples, c.trips };
	for (int k = 0; k < CNT_COUNT; ++k) {
		unsigned long long v = vals[k];
		for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
		if (lane == 0 && v) atomicAdd(&counters[k], v);
	}
}

