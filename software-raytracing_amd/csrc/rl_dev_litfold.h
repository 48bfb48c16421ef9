// How the lazy-reflectance kernels (k_trace_lazy, rl_k_trace.inl RL_LAZY_REFL; k_trace_lazy_hitq, rl_k_trace_hitq.inl) finish their lit paths, one copy for both,
// included by rl_render_lazy.hip alone: the reservation of a lit path's entry in the wave's chunk of the lit list (rl_device.h DLitList), the fold of one path, and
// the fold of a chunk by the wave that filled it.  Both kernels are the leaf-list kernel's PLAIN instance (LDS == 2): the materials are read from its LDS copy.
//
// A lit path of at most RL_FOLD_PREFETCH records is written as an entry, and a wave that has written the 64th entry of its chunk reads the chunk back, entry
// `lane` in lane `lane`, and folds it: 64 lanes at work whatever the lanes that ended lit in that trip were.  The wave folds its last, partly filled chunk before it
// leaves.  Nothing reads the list behind the launch.  A path without an entry (more records than an entry holds, or the list used up) folds in place, by its lane alone.
#pragma once

namespace rl {

// A lit path's sample out: stored, and with a lit-sample mask by its rule (rl_lit_mask.h) -- all zero bits, neither stored nor flagged.  numSlots splits outIndex
// into sample and slot.
__device__ __forceinline__ void LitStoreSample(const DLitList& LL, SampleRGB* __restrict__ samples, uint32_t numSlots, uint32_t outIndex, V3 L)
{
	if (!LL.mask) samples[outIndex] = make_sample(L.x, L.y, L.z);
	else if (AnyBitSet(L)) {
		const uint32_t s = outIndex / numSlots;
		samples[outIndex] = make_sample(L.x, L.y, L.z);
		atomicOr(&LL.mask[LitMaskWord(s, numSlots, outIndex - s * numSlots)], LitMaskBit(s));
	}
}

// The fold of one lit path, the one statement of it: from its terminal L over its nrec vertex records, the last first, back to the camera exactly as k_trace
// folds -- each vertex's reflectance evaluated here instead of at its scattering event (FoldLazyVertex) --, then the sample out.  rec(k, r0, r1) fetches record k
// (camera first): from an entry of the list, or from the path stack and the registers.  sm: the kernel's LDS copy of the scene.
template <class REC>
__device__ __forceinline__ void LitFoldPath(const DLitList& LL, const float4* sm, SampleRGB* __restrict__ samples, uint32_t numSlots, uint32_t outIndex, V3 L, int nrec, REC rec)
{
	#pragma nounroll
	for (int k = nrec - 1; k >= 0; --k) {
		float4 r0, r1;
		rec(k, r0, r1);
		const Mat m = MatFrom<true>(sm + LdsAt<2>::MATS + RL_LAZY_REC_MAT(r1.w) * RL_LDS_MSTRIDE(true));
		L = FoldLazyVertex(m, r0, r1, L);
	}
	LitStoreSample(LL, samples, numSlots, outIndex, L);
}

// In place: the path's lane alone, its first `depth` records from its column of the path stack (st0: record 0; step: float4 from a record to the next), a last
// vertex that was recorded in this trip (nrec == depth + 1) from the registers.
__device__ __forceinline__ void LitFoldInPlace(const DLitList& LL, const float4* sm, SampleRGB* __restrict__ samples, uint32_t numSlots, uint32_t outIndex, V3 L, int nrec,
                                               int depth, const float4* st0, size_t step, float4 top0, float4 top1)
{
	LitFoldPath(LL, sm, samples, numSlots, outIndex, L, nrec, [=](int k, float4& r0, float4& r1) __attribute__((always_inline)) {
		r0 = top0; r1 = top1;
		if (k < depth) { const float4* st = st0 + (size_t)k * step; r0 = st[0]; r1 = st[1]; }
	});
}

// The first `count` entries of chunk `chunk`, entry `lane` in lane `lane`: whole waves call it, for a chunk whose entries this wave wrote.  The entries were
// stored by other lanes of the wave than the ones that read them now: the stores are waited for first (the wave's lanes share one vector cache, so what has been
// acknowledged is what a load of the same wave sees).  Inlined at each of its call sites (two in k_trace_lazy, three in k_trace_lazy_hitq).  RL_LIT_FOLD_INLINE=0
// makes it a call, one copy per unit: the callers then keep what lives across the call in the callee-saved registers and spill more around it -- k_trace_lazy 8
// VGPRs spilled and 64 bytes of scratch against 0 and 0, k_trace_lazy_hitq 12 and 80 against 7 and 32 (DESIGN.md section 5 "lit fold").
#ifndef RL_LIT_FOLD_INLINE
#define RL_LIT_FOLD_INLINE 1
#endif
#if RL_LIT_FOLD_INLINE
__device__ __forceinline__
#else
__device__ __noinline__
#endif
void LitFoldChunk(const DLitList LL, const float4* sm, SampleRGB* __restrict__ samples, uint32_t numSlots, uint32_t chunk, uint32_t count, uint32_t lane)
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	if (lane < count) {
		const float4* e = (const float4*)LL.entries + ((size_t)chunk * RL_LIT_CHUNK + lane) * RL_LIT_STRIDE;
		const float4 h0 = e[0];
		const int nrec = __float_as_int(e[1].x);   // (<= RL_FOLD_PREFETCH: a longer path folds in place)
		LitFoldPath(LL, sm, samples, numSlots, __float_as_uint(h0.w), v3(h0.x, h0.y, h0.z), nrec,
		            [e](int k, float4& r0, float4& r1) __attribute__((always_inline)) { r0 = e[2 + 2 * k]; r1 = e[3 + 2 * k]; });
	}
}

// A lit path's entry in the wave's chunk of the lit list, or ~0u when it folds in place: one global atomic per RL_LIT_CHUNK entries (a returning atomic per trip on
// one address would be the rate at which the job counter once bound these kernels).  Whole waves call it.  When the reservation rolls the wave over to a fresh
// chunk, `full` is the chunk it leaves (~0u otherwise): complete once the lanes of this call have written their entries, and the caller folds it there
// (LitFoldChunk, all RL_LIT_CHUNK entries).  The chunk the wave holds at its end is folded up to litFill.
__device__ __forceinline__ uint32_t LitReserve(const DLitList& LL, uint32_t lane, bool wantEntry, uint32_t& litChunk, uint32_t& litFill, bool& litFull, uint32_t& full)
{
	const unsigned long long em = Ballot(wantEntry);
	const uint32_t n = (uint32_t)__popcll(em), rank = (uint32_t)__popcll(em & ((1ull << lane) - 1ull)), room = RL_LIT_CHUNK - litFill;
	uint32_t fresh = ~0u;
	if (n > room && !litFull) {
		if (lane == 0 && LL.numChunks != 0u) fresh = atomicAdd(&LL.ctl[0], 1u);
		fresh = __shfl(fresh, 0);
		if (fresh >= LL.numChunks) { fresh = ~0u; litFull = true; }
	}
	uint32_t entry = ~0u;
	if (wantEntry) {
		if (rank < room) entry = litChunk * RL_LIT_CHUNK + litFill + rank;
		else if (fresh != ~0u) entry = fresh * RL_LIT_CHUNK + (rank - room);
	}
	full = ~0u;
	if (n > room) {   // the wave's chunk is full now, and the fresh one (if any) is the wave's
		full = litChunk;
		litChunk = fresh; litFill = fresh != ~0u ? n - room : RL_LIT_CHUNK;
	} else litFill += n;
	return entry;
}

} // namespace rl
