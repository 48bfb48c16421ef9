// k_radiance: path-traced radiance along a caller's rays (include/raylib_amd.h RaylibAMD_TraceRadiance).  rl_radiance.hip includes this file and
// instantiates the kernel; the other units see the declaration, the records and the instance list of rl_kernels.h, so that the render and query
// kernels stay the code they were (tools/isa_equivalence.py).
//
// It joins what the device library already has: k_query's chunked dealing of a batch (a wave takes RL_QUERY_CHUNK jobs from a global counter with one
// atomic), k_trace's bounce loop of the general instance (walk, BuildSurface / Scatter / Emitted or the miss shader, the vertex record on the path
// stack, the fold back to front) and the stream contract of include/raylib_amd_rng.h with the ray's own `stream` in the place of the pixel index.
//
// One path per lane on a persistent grid.  A job is one ray with its run of Q.sampleCount samples: the lane traces them one after the other and
// sums them in order, from +0, then multiplies by 1 / sampleCount -- k_resolve's accum and its factor.  A lane whose job is finished takes the wave's
// next one at the next trip (ballot + prefix rank, as the 8-wide query does between steps): paths differ in length by the whole maxPathLength, and a
// wave must not wait for its longest.
//
// The candidate rule is the render's (this unit does not set RL_OWN_BOX_WIDEN_TMIN), rayTMin is used as given and the ray is neither normalised nor
// jittered: the camera's rays on the camera's streams give the render's bits.
//
// The path stack is the megakernel's: Q.maxPathLength records of two float4 per RESIDENT lane (not per ray), record k of lane g at
// (k * Q.stackStride + g) * 2 -- a wave's 64 lanes write 2 KiB back to back per record index.
// (RL_QUERY_CHUNK, the jobs a wave takes per atomic on the global counter: rl_kernels.h)
//
// One source for two kernels, as rl_k_resolve.inl is: a translation unit includes this file with RL_GATHER_TWIN 0 for k_radiance (rl_radiance.hip) or 1 for
// k_gather (rl_gather.hip: RaylibAMD_Gather), whose generator template parameter GEN (RL_GEN_HEMISPHERE, RL_GEN_SPHERE) says how a job's ray is made.  The twin
// differs in two places, both under RL_GATHER_TWIN:
//   the `fresh` block   a job is one (point, sample) pair of a launch, sample-major (job = sample * J.numPoints + point, so that a wave's lanes hold
//                       neighbouring points at one sample index); it loads the point and draws the direction from the sample's stream
//   the `done` block    writes the sample's value to slot `job` of the launch's sample buffer instead of summing it -- k_gather_resolve sums the slots in
//                       sample order
// Walk, shading, miss shader, fold, refill and counters are the same lines.  Everything of the twin's is under the macro, so that k_radiance is the token
// sequence it was (a generator parameter on a shared body adds an inlining level, which changes k_radiance's register allocation: tools/isa_equivalence.py).

// (template and kernel arguments: rl_kernels.h)
#if RL_GATHER_TWIN
// points: the call's point records (two float4 each); n: the launch's jobs = J.numPoints * its samples; samples: 2 n float4 for the sphere (L | Wi), n for the hemisphere
template <int TREE, int STACK, bool PRIMS, int GEN>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2))
k_gather(const DSceneView S, const SkyRot R, const DRadianceParams Q, const float4* __restrict__ rays, uint32_t n, const DGatherJobs J, float4* __restrict__ out,
         float* __restrict__ pathStack, unsigned int* __restrict__ rayCounter, unsigned long long* __restrict__ counters)
#else
template <int TREE, int STACK, bool PRIMS>
__global__ void __launch_bounds__(RL_BLOCK, (STACK <= 32 ? RL_TRACE_MIN_WAVES : 2))
k_radiance(const DSceneView S, const SkyRot R, const DRadianceParams Q, const float4* __restrict__ rays, uint32_t n, float4* __restrict__ out,
           float* __restrict__ pathStack, unsigned int* __restrict__ rayCounter, unsigned long long* __restrict__ counters)
#endif
{
#if RL_GATHER_TWIN
	static_assert(GEN == RL_GEN_HEMISPHERE || GEN == RL_GEN_SPHERE, "generator");
#endif
	static_assert(TREE == 2 || TREE == 4, "tree");
	static_assert(TREE == 2 || !PRIMS, "spheres and cubes are walked on the binary tree only");
	RL_TEX_PROLOGUE(S);                      // (empty here: rl_radiance.hip leaves RL_LDS_TEXTURE_TABLE off, texture descriptors are read from global memory)
	RL_MATH_PROLOGUE();
	__shared__ int s_stack[STACK * RL_BLOCK];
	int* stk = s_stack + threadIdx.x;
	const uint32_t gtid = blockIdx.x * RL_BLOCK + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	const unsigned long long laneLt = (1ull << lane) - 1ull;
	Counters c; c.rays = c.nodes = c.tris = c.shaded = c.texels = c.samples = c.trips = 0; RL_DIAG_BIND(c);
	constexpr uint32_t NONE = 0xffffffffu;
	uint32_t my = NONE;                      // this lane's job: the ray's index
	uint32_t sample = 0;                     // of the job's run: 0 .. Q.sampleCount - 1
	bool fresh = false;                      // the next trip starts sample `sample` from the ray record
	V3 acc = v3s(0.0f);                      // the run's sum so far
	Rng g; g.s.state = 0;
	V3 o = v3s(0.0f), d = v3s(0.0f);
	float rayTime = 0.0f;
	int depth = 0;
#if RL_GATHER_TWIN
	float weight = 0.0f;                     // RL_GEN_HEMISPHERE: max(0, dot(N, Wi)) of the sample's direction
#endif
	uint32_t next = 0u, end = 0u;            // the wave's chunk (wave-uniform)
	bool drained = false;                    // the global counter is past n (wave-uniform)
	for (;;) {
		// ---- idle lanes take the wave's next jobs: wave64 ballot + prefix rank ----
		unsigned long long idle = Ballot(my == NONE);
		if (!drained) {
			while (idle != 0ull) {
				if (next >= end) {
					uint32_t b = 0u;
					if (lane == 0u) b = atomicAdd(rayCounter, RL_QUERY_CHUNK);
					b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
					if (b >= n) { drained = true; break; }
					next = b; end = min(b + RL_QUERY_CHUNK, n);
				}
				const uint32_t take = min((uint32_t)__popcll(idle), end - next);
				const uint32_t rank = (uint32_t)__popcll(idle & laneLt);
				if (my == NONE && rank < take) { my = next + rank; sample = 0u; fresh = true; acc = v3s(0.0f); }
				next += take;
				idle = Ballot(my == NONE);
			}
		}
		if (idle == ~0ull) break;             // (only a drained wave leaves the loop above with idle lanes)
		if (lane == 0u) c.trips++;
		if (my != NONE) {
			if (fresh) {
#if RL_GATHER_TWIN
				// the job's (point, sample); the point's record (pos, time | normal, stream); the direction from the sample's first two draws behind the skipped
				// ones (include/raylib_amd.h RaylibAMD_Gather, statement 1): the Lambertian case's three statements of rl_dev_shade.h for the hemisphere, the
				// normalised draw for the sphere
				const uint32_t sIdx = my / J.numPoints, pIdx = my - sIdx * J.numPoints;
				const float4* pp = rays + 2u * ((size_t)J.pointFirst + pIdx);
				const float4 r0 = GLoadF4(pp, 0), r1 = GLoadF4(pp, 1);
				o = v3(r0.x, r0.y, r0.z);
				const V3 N = v3(r1.x, r1.y, r1.z);
				rayTime = fminf(fmaxf(r0.w, Q.timeMin), Q.timeMax);
				g.s = raylib_rng_begin_mixed(Q.seedMixed, __float_as_uint(r1.w), Q.sampleFirst + J.sampleBase + sIdx);
				for (uint32_t k = 0; k < Q.skipDraws; ++k) (void)raylib_rng_next_u32(&g.s);
				V3 w = RandomInUnitSphere(g);
				if constexpr (GEN == RL_GEN_HEMISPHERE) { if ((double)dot(w, N) < 0.0) w = -w; }
				d = normalize(w);
				if constexpr (GEN == RL_GEN_HEMISPHERE) weight = fmaxf(0.0f, dot(N, d));
				else out[(size_t)n + my] = make_float4(d.x, d.y, d.z, 0.0f);   // the resolve's basis functions need Wi: the buffer's second plane
#else
				// the ray as given; its stream (seed, rays[i].stream, sampleFirst + sample) behind the draws the caller made for it
				const float4* rp = rays + 2u * (size_t)my;   // (64-bit offset: n may reach 2^31 - 1)
				const float4 r0 = GLoadF4(rp, 0), r1 = GLoadF4(rp, 1);
				o = v3(r0.x, r0.y, r0.z); d = v3(r1.x, r1.y, r1.z);
				rayTime = fminf(fmaxf(r0.w, Q.timeMin), Q.timeMax);   // (a NaN becomes timeMin: the boxes of moving cubes cover [timeMin, timeMax])
				g.s = raylib_rng_begin_mixed(Q.seedMixed, __float_as_uint(r1.w), Q.sampleFirst + sample);
				for (uint32_t k = 0; k < Q.skipDraws; ++k) (void)raylib_rng_next_u32(&g.s);
#endif
				depth = 0;
				fresh = false;
				c.samples++;
			}
			// ---- one bounce (TraceScene, reference render/renderer.cc:114-208), as k_trace's general instance takes it ----
			HitRec h; h.tri = -1;
			bool hit = false;
			const bool doTrace = depth < Q.maxPathLength;   // renderer.cc:120-123 otherwise
			if (doTrace) {
				if constexpr (TREE == 2) hit = Traverse<STACK, false, PRIMS>(S, o, d, rayTime, Q.rayTMin, h, stk, c);
				else hit = Traverse4<STACK, false, false, false>(S, o, d, rayTime, Q.rayTMin, h, stk, c);
			}
			bool done = false, store = false;
			float4 rec0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rec1 = rec0;
			V3 L = v3s(0.0f);
			if (!doTrace) {
				done = true;
			} else if (hit) {
				Surf s;
				const int mi = BuildSurface<PRIMS>(S, o, d, h, s, true, c);
				const Mat m = LoadMat(S, mi);
				V3 refl = v3s(0.0f), outD = v3s(0.0f);
				float pdf = 0.0f, sp = 0.0f;
				const bool scattered = Scatter(S, m, d, s, g, c, refl, outD, pdf, sp);
				const V3 E = Emitted(S, m, s, c);
				if (scattered && pdf > 0.0f) {
					if (depth + 1 >= Q.maxPathLength) {
						// the next TraceScene returns 0 at once (renderer.cc:120-123): this vertex is the path's last; its step of the fold, from the registers
						V3 radiance = v3s(0.0f);
						radiance = radiance + refl * L * sp / pdf;
						radiance = radiance + E;
						L = radiance;
						done = true;
					} else {
						store = true;
						rec0 = make_float4(refl.x, refl.y, refl.z, sp);
						rec1 = make_float4(pdf, E.x, E.y, E.z);
						o = s.p; d = outD;
					}
				} else {
					L = v3s(0.0f) + E;                        // radiance(0) += Emitted, renderer.cc:137,151
					done = true;
				}
			} else {
				// the miss shader (renderer.cc:155-199): the sky panorama, and the sun unless its shadow ray from the ray's origin is occluded.
				// This restates rl_dev_shade.h MissShader's sun block instead of calling it: MissShader picks its tree from S.nodes4, not from the
				// launch's plan, and would walk the grid nodes under RAYLIB_QUERY_TREE=2.  The two must stay the same arithmetic.
				L = MissSky(S, R, d, c);
				if (S.hasSun) {
					HitRec tmp;
					bool occluded;
					if constexpr (TREE == 2) occluded = Traverse<STACK, true, PRIMS>(S, o, -ld3(S.sunDirection), rayTime, Q.rayTMin, tmp, stk, c);
					else occluded = Traverse4<STACK, true, false, false>(S, o, -ld3(S.sunDirection), rayTime, Q.rayTMin, tmp, stk, c);
					if (!occluded) L = L + ld3(S.sunIlluminance);
				}
				done = true;
			}
			if (done) {
				// fold back to the first vertex: radiance = (0 + refl * Li * sp / pdf) + E at every vertex, the megakernel's arithmetic
				for (int k = depth - 1; k >= 0; --k) {
					const float4* st = (const float4*)pathStack + ((size_t)k * Q.stackStride + gtid) * 2u;
					const float4 q0 = st[0], q1 = st[1];
					const V3 refl = v3(q0.x, q0.y, q0.z);
					const float sp = q0.w, pdf = q1.x;
					const V3 E = v3(q1.y, q1.z, q1.w);
					V3 radiance = v3s(0.0f);
					radiance = radiance + refl * L * sp / pdf;
					radiance = radiance + E;
					L = radiance;
				}
#if RL_GATHER_TWIN
				// the sample's value (statement 3): L * max(0, dot(N, Wi)) for the hemisphere; L itself for the sphere, whose nine products the resolve forms
				if constexpr (GEN == RL_GEN_HEMISPHERE) L = L * weight;
				out[my] = make_float4(L.x, L.y, L.z, 0.0f);
				my = NONE;
#else
				acc = acc + L;
				if (++sample >= Q.sampleCount) {
					const float k = rtm::rcp1_((float)Q.sampleCount);   // k_resolve's factor
					out[my] = make_float4(acc.x * k, acc.y * k, acc.z * k, 1.0f);
					my = NONE;
				} else fresh = true;
#endif
			}
			if (store) {
				// path vertex record: 32 contiguous bytes per lane, two 16-byte stores
				float4* st = (float4*)pathStack + ((size_t)depth * Q.stackStride + gtid) * 2u;
				st[0] = rec0; st[1] = rec1;
				depth++;
			}
		}
	}
	if (counters) {   // wave reduction, one atomic per wave and counter
		const uint32_t vals[CNT_COUNT] = { c.rays, c.nodes, c.tris, c.shaded, c.texels, c.samples, c.trips };
		for (int k = 0; k < CNT_COUNT; ++k) {
			unsigned long long v = vals[k];
			for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
			if (lane == 0u && v) atomicAdd(&counters[k], v);
		}
	}
}

