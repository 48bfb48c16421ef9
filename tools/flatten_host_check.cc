// Sanitizer harness only (tools/host_check.sh flatten): a stand-alone program over FlattenScene (csrc/rl_scene.cc) -- the step that turns a finalized scene into
// the records the devices hold -- on the smallest scenes that reach each of its branches, built through the ABI and linked with tools/nodevice_stub.cc in place
// of the device units.  Never part of libraylib.so.
#include "raylib.h"
#include "raylib_amd.h"
#include "rl_host.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <vector>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "flatten_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static MaterialHandle Material(int type, float shade)
{
	const float albedo[3] = { shade, shade, shade }, zero[3] = { 0, 0, 0 }, one[3] = { 1, 1, 1 };
	return RaylibAMD_CreateMaterial(type, albedo, 0.5f, 0.0f, zero, 1.5f, one, 0.0f);
}
// a scene of loose triangles (nine floats each), triangle i with materials[i]
static rl::Scene* Triangles(const std::vector<std::vector<float>>& tris, const std::vector<MaterialHandle>& materials)
{
	SceneHandle scene = Raylib_CreateScene();
	const float n[3] = { 0, 0, 1 };
	for (size_t i = 0; i < tris.size(); ++i) {
		const float* v = tris[i].data();
		Raylib_AddSceneElement(scene, RaylibAMD_CreateTriangle(v, v + 3, v + 6, n, n, n, NULL, materials[i]));   // (the elements live as long as the program)
	}
	Raylib_FinalizeScene(scene);
	return (rl::Scene*)scene;
}
static float Denom(const rl::DTriIsect& t) { return t.uv * t.uv - t.uu * t.vv; }   // the host's own three operations (this program is built with -ffp-contract=off too)

int main()
{
	const MaterialHandle grey = Material(0, 0.5f);
	CHECK(grey);
	const std::vector<float> ordinary = { 0, 0, 0, 1, 0, 0, 0, 1, 0 }, collinear = { 0, 0, 0, 1, 0, 0, 2, 0, 0 }, tiny = { 0, 0, 0, 1e-5f, 0, 0, 0, 1e-5f, 0 };
	{   // one ordinary triangle, with and without the short divisions
		rl::Scene* s = Triangles({ ordinary }, { grey });
		rl::FlatScene F = rl::FlattenScene(*s);
		CHECK(F.isect.size() == 1 && F.shade.size() == 1 && F.fastBary == 1 && Denom(F.isect[0]) == -1.0f && F.isect[0].rden == 1.0f / Denom(F.isect[0]));
		CHECK(F.isect[0].n[0] == 0.0f && F.isect[0].n[1] == 0.0f && F.isect[0].n[2] == 1.0f && F.shade[0].material == 0);
		CHECK(F.alphaTex.empty() && F.materials.size() == 1 && F.textures.empty() && F.texels.empty() && F.spheres.empty() && F.cubes.empty());
		CHECK(fabsf(F.skyRot.m0[2] + 1.0f) < 1e-6f && fabsf(F.skyRot.m2[0] - 1.0f) < 1e-6f && F.skyRot.m1[1] == 1.0f);   // yaw 90 degrees
		setenv("RAYLIB_FAST_BARY", "0", 1);
		F = rl::FlattenScene(*s);
		unsetenv("RAYLIB_FAST_BARY");
		CHECK(F.fastBary == 0 && F.isect[0].rden == 1.0f / Denom(F.isect[0]));
		Raylib_DestroyScene((SceneHandle)s);
	}
	{   // a triangle without area: denom is 0, which no ray hits in either form -- the scene keeps the short divisions
		rl::Scene* s = Triangles({ ordinary, collinear }, { grey, grey });
		const rl::FlatScene F = rl::FlattenScene(*s);
		CHECK(F.isect.size() == 2 && F.fastBary == 1);
		int nan = 0;
		for (const rl::DTriIsect& t : F.isect) { if (Denom(t) == 0.0f) { CHECK(t.rden != t.rden); ++nan; } else CHECK(t.rden == 1.0f / Denom(t)); }
		CHECK(nan == 1);
		Raylib_DestroyScene((SceneHandle)s);
	}
	{   // |denom| = 1e-20 < 2^-62: its reciprocal is not usable, and the whole scene takes the divisions
		rl::Scene* s = Triangles({ ordinary, tiny }, { grey, grey });
		const rl::FlatScene F = rl::FlattenScene(*s);
		CHECK(F.isect.size() == 2 && F.fastBary == 0);
		int nan = 0;
		for (const rl::DTriIsect& t : F.isect) { if (fabsf(Denom(t)) < 0x1p-62f) { CHECK(Denom(t) != 0.0f && t.rden != t.rden); ++nan; } else CHECK(t.rden == 1.0f / Denom(t)); }
		CHECK(nan == 1);
		Raylib_DestroyScene((SceneHandle)s);
	}
	{   // albedo maps: materials 0 and 1 (microfacet) and 2 (Lambertian) use texture 0, material 3 (microfacet) has no map, triangle 4's material index is out of range
		const MaterialHandle micro0 = Material(3, 0.1f), micro1 = Material(3, 0.2f), lambert = Material(0, 0.3f), bare = Material(3, 0.4f);
		rl::Scene* s = Triangles({ ordinary, ordinary, ordinary, ordinary, ordinary }, { micro0, micro1, lambert, bare, grey });
		auto map = std::make_shared<rl::Image>();
		map->width = 2; map->height = 1; map->rgba = { 0.0f, 0.25f, 0.5f, 1.0f, 2.0f, 0.75f, 1e-3f, 0.5f };
		s->textures.push_back(map);
		for (int m = 0; m < 3; ++m) s->materials[(size_t)m].tex[0] = 0;
		s->triangles[4].material = 99;
		const rl::FlatScene F = rl::FlattenScene(*s);
		CHECK(F.textures.size() == 2 && F.texels.size() == 16 && F.materials.size() == 5);   // exactly one converted copy
		CHECK(F.textures[0].offset == 0 && F.textures[1].offset == 2 && F.textures[1].width == 2 && F.textures[1].height == 1);
		CHECK(F.materials[0].tex[0] == 1 && F.materials[1].tex[0] == 1 && F.materials[2].tex[0] == 0 && F.materials[3].tex[0] == -1);
		for (int i = 0; i < 8; ++i) CHECK(F.texels[(size_t)i] == map->rgba[(size_t)i] && F.texels[8 + (size_t)i] == powf(map->rgba[(size_t)i], 2.2f));
		CHECK(F.alphaTex.size() == 5);
		for (size_t k = 0; k < 5; ++k) {   // slots are in leaf order: the material tells which triangle a slot holds
			const int32_t m = F.shade[k].material;
			CHECK(F.alphaTex[k] == ((m == 0 || m == 1) ? 1 : -1));
		}
		int seen[5] = { 0, 0, 0, 0, 0 };
		for (size_t k = 0; k < 5; ++k) { const int32_t m = F.shade[k].material; ++seen[m == 99 ? 4 : m]; }
		CHECK(seen[0] == 1 && seen[1] == 1 && seen[2] == 1 && seen[3] == 1 && seen[4] == 1);
		Raylib_DestroyScene((SceneHandle)s);
	}
	{   // spheres only: no triangle record at all
		SceneHandle scene = Raylib_CreateScene();
		Raylib_AddSceneElement(scene, RaylibAMD_CreateSphere(0, 0, 0, 0.5f, grey));
		Raylib_AddSceneElement(scene, RaylibAMD_CreateSphere(2, 0, 0, 0.25f, grey));
		Raylib_FinalizeScene(scene);
		const rl::FlatScene F = rl::FlattenScene(*(rl::Scene*)scene);
		CHECK(F.isect.empty() && F.shade.empty() && F.alphaTex.empty() && F.fastBary == 1 && F.cubes.empty());
		CHECK(F.spheres.size() == 2 && F.spheres[1].center[0] == 2.0f && F.spheres[1].radius == 0.25f && F.spheres[1].material == 1 && F.materials.size() == 2);
		Raylib_DestroyScene(scene);
	}
	printf("flatten_host_check: ok\n");
	return 0;
}
