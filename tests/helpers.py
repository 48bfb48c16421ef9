"""Shared test plumbing: scene cases, flat-scene loading, library handles."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "software-raytracing_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ffi, objflat          # noqa: E402  (test infrastructure)
from raylib_amd import scenes            # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def texture_loader(path):
    """What the product must decode from leaf.png, straight from the generator."""
    name = os.path.basename(path)
    if name == "leaf.png":
        return scenes.texture_as_float(scenes.leaf_texture())
    if name in scenes.textured_textures():
        return scenes.texture_as_float(scenes.textured_textures()[name])
    stem, ext = os.path.splitext(name)
    if ext == ".png" and stem in scenes.pbr_textures():
        return scenes.texture_as_float(scenes.pbr_textures()[stem])
    return None


# name -> (generator, kwargs, camera dict, sun, sun_dir, sky?)
CASES = {
    "cornell": dict(gen=scenes.cornell, kw={}, origin=(0, 1, 4), look_at=(0, 1, -1), fov=45.0, aspect=1.0,
                    aperture=0.0, focal=1.0, shutter=(0.0, 0.0), sun=(0, 0, 0), sun_dir=(0.0, -1.0, -0.5), sky=False),
    "cornell_glass_sun": dict(gen=scenes.cornell, kw=dict(short_material=scenes.GLASS), origin=(0.3, 1.2, 4), look_at=(0, 0.9, -1),
                              fov=45.0, aspect=1.0, aperture=0.05, focal=4.0, shutter=(0.0, 1.0),
                              sun=(20, 20, 20), sun_dir=(0.2, -0.3, -1.0), sky=False),
    "cornell_flat_normals": dict(gen=scenes.cornell, kw=dict(with_normals=False, with_uvs=False), origin=(0, 1, 4), look_at=(0, 1, -1),
                                 fov=60.0, aspect=1.0, aperture=0.0, focal=1.0, shutter=(0.0, 0.0),
                                 sun=(0, 0, 0), sun_dir=(0.0, -1.0, -0.5), sky=False),
    "cutout_sky": dict(gen=scenes.cutout, kw={}, origin=(0, 1, 4), look_at=(0, 1, -1), fov=45.0, aspect=1.0,
                       aperture=0.0, focal=1.0, shutter=(0.0, 0.0), sun=(3, 3, 3), sun_dir=(0.1, -0.2, -1.0), sky=True),
    # MicrofacetMaterial away from the Cornell defaults: roughness in (0,1) from Pr and from Ns/Ks, metallic > 0, normal /
    # roughness / metallic / emissive maps, a mirror-like (roughness < 0.1) surface (scenes.pbr_maps)
    "pbr_maps": dict(gen=scenes.pbr_maps, kw={}, origin=(0.1, 1.1, 4), look_at=(0, 0.95, -1), fov=45.0, aspect=1.0,
                     aperture=0.0, focal=1.0, shutter=(0.0, 0.0), sun=(0, 0, 0), sun_dir=(0.0, -1.0, -0.5), sky=False),
}
# cases without a normal map: the microsurface-normal AOV must equal the surface-normal AOV
NO_NORMAL_MAP = ("cornell", "cornell_glass_sun", "cornell_flat_normals")


def build_case(name, tmpdir):
    """Write the OBJ for a case; return (obj_path, case dict)."""
    c = CASES[name]
    d = os.path.join(str(tmpdir), name)
    os.makedirs(d, exist_ok=True)
    obj, _ = c["gen"](os.path.join(d, name + ".obj"), **c["kw"])
    return obj, c


def flat_for_case(name, tmpdir, oracle):
    obj, c = build_case(name, tmpdir)
    flat = objflat.load_obj(obj, oracle, texture_loader=texture_loader, sun_illuminance=c["sun"], sun_direction=c["sun_dir"])
    if c["sky"]:
        flat.textures.append(np.ascontiguousarray(scenes.sky_panorama(), np.float32))
        flat.sky_texture = len(flat.textures) - 1
    return obj, c, flat


def camera_for_case(c):
    return ffi.make_camera(c["origin"], c["look_at"], c["fov"], c["aspect"], c["aperture"], c["focal"], *c["shutter"])


def assert_planned(lib, ses, stats, w, h, spp, max_path=5, tmin=1e-4):
    """The render just made of `ses` (numbers in `stats`) launched what RaylibAMD_PlanRender predicts for it under the same environment (csrc/rl_plan.cc)."""
    import ctypes as C
    from raylib_amd import binding
    st = binding.RendererSettings(int(w), int(h), int(spp), int(max_path), float(tmin), 0)
    p = binding.RenderPlan()
    assert lib.RaylibAMD_PlanRender(ses.scene, C.byref(st), int(getattr(ses, "has_sky", False)), 256, 4, C.byref(p)) == 1
    s = stats if isinstance(stats, dict) else stats.as_dict()
    got = (s["treeWidth"], s["pathsPerWave"], s["nodeBytes"], lib.RaylibAMD_LastTracePlain())
    assert got == (p.treeWidth, p.pathsPerWave, p.nodeBytes, p.plain), (got, p.as_dict())
    return p.as_dict()


def session_for_case(lib, name, tmpdir):
    from raylib_amd import binding
    obj, c = build_case(name, tmpdir)
    return binding.SceneSession(lib, obj, c["origin"], c["look_at"], c["fov"], c["aspect"], sun=c["sun"], sun_dir=c["sun_dir"],
                                aperture=c["aperture"], focal=c["focal"], shutter=c["shutter"],
                                sky_image=scenes.sky_panorama() if c["sky"] else None)


def big_scene(path, objects, mtl_text, oracle, tess, displace_fraction=0.0, sun=(0, 0, 0), sun_dir=(0.0, -1.0, -0.5), arrays=None, textures=None):
    """A large synthetic scene for the BASELINE-size tests: the arrays of scenes.build_arrays (or `arrays`, the same dictionary), written as OBJ
    text by the checker library's multi-threaded writer (the Python writer needs minutes for millions of triangles; same format, same digits),
    and the flat scene the arrays ARE -- every float32 survives its 9 printed digits -- for the oracle.  `textures`: file name -> (H, W, 4)
    uint8, written as PNG next to the OBJ and handed to the oracle as byte / 255 floats, numbered as the reference numbers them (in the order
    the MTL's materials name their albedo maps, obj_loader.cc:372-395).  The caller checks that the product loaded exactly this flat scene.
    Returns (obj path, FlatScene)."""
    A = arrays if arrays is not None else scenes.build_arrays(objects, tess, displace_fraction)
    base = os.path.splitext(path)[0]
    oracle.write_obj(base + ".obj", os.path.basename(base) + ".mtl", A["tri"], A["uv"], A["normal"], A["owner"], A["objects"])
    with open(base + ".mtl", "w") as f:
        f.write(mtl_text)
    if textures:
        scenes.write_textures(os.path.dirname(os.path.abspath(path)), textures)
    mtl = objflat.parse_mtl(base + ".mtl")
    names = [m["name"] for m in mtl]
    mats = np.zeros(len(mtl) + 1, ffi.MAT_DTYPE)
    flat_textures, tex_index = [], {}
    for i, m in enumerate(mtl):
        mats[i] = oracle.material_from_mtl(m["Kd"], m["Ks"], m["Ke"], m["Tf"], m["Ns"], m["Ni"], m["illum"], m["Pr"], m["Pm"], bool(m["map_Kd"]))
        for k in ("texAlbedo", "texNormal", "texRoughness", "texMetallic", "texEmissive"):
            mats[i][k] = -1
        if textures and m["map_Kd"] in textures and mats[i]["type"] == ffi.MAT_MICROFACET:
            if m["map_Kd"] not in tex_index:
                tex_index[m["map_Kd"]] = len(flat_textures)
                flat_textures.append(scenes.texture_as_float(textures[m["map_Kd"]]))
            mats[i]["texAlbedo"] = tex_index[m["map_Kd"]]
    mats[-1]["type"] = ffi.MAT_LAMBERTIAN; mats[-1]["albedo"] = (0.5, 0.5, 0.5)
    for k in ("texAlbedo", "texNormal", "texRoughness", "texMetallic", "texEmissive"):
        mats[-1][k] = -1
    n = len(A["tri"])
    tris = np.zeros(n, ffi.TRI_DTYPE)
    tris["v0"], tris["v1"], tris["v2"] = A["tri"][:, 0], A["tri"][:, 1], A["tri"][:, 2]
    tris["n0"] = tris["n1"] = tris["n2"] = A["normal"]
    tris["st"] = A["uv"].reshape(n, 6)
    per_object = np.array([names.index(m) if m in names else len(mtl) for _, m in A["objects"]], np.int32)
    tris["material"] = per_object[A["owner"]]
    tris["shape"] = A["owner"]
    flat = ffi.FlatScene(tris, mats, flat_textures, num_shapes=len(A["objects"]), sun_illuminance=sun, sun_direction=sun_dir)
    return base + ".obj", flat


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """Element-wise: the same float32 bits, or NaN on both sides.  (The reference itself produces NaN radiance on some paths --
    e.g. a near-specular Beckmann lobe, roughness 0.05 -- and a NaN's payload / sign is not part of parity: x86 SSE makes
    0xFFC00000, the GPU 0x7FC00000.)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def l2(a, b):
    """RMS per-pixel L2 distance over the pixels that are finite on both sides (NaN must meet NaN: `helpers.same`)."""
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    d = d[np.isfinite(d).all(-1)]
    return float(np.sqrt((d * d).sum(-1).mean())) if len(d) else 0.0


def z_statistics(run_images, ref_mean, ref_std, runs):
    """`runs` independent renders (different seeds, the same samples per pixel each) by the renderer under test against the statistics of
    `runs` independent renders of the UNTOUCHED reference (tests/golden/native_stats.npz: per pixel and channel the mean and the standard
    deviation of the run means).  If -- and only if -- both sample the same per-sample distribution, the two sets of run means are two
    samples of one distribution, so the difference of their means is SYMMETRIC around 0 whatever that distribution's skew (path-traced
    pixels are heavy-tailed: a one-sample z against the reference mean is biased by the skew, measured: 14 sigma on the Cornell box).
        z = (mean_here - mean_ref) / sqrt((var_here + var_ref) / runs)
    Returned: summaries over the pixels that vary on either side (n of them): mean z and the share of positive differences (both
    centred under the hypothesis, with standard errors ~1.1 / sqrt(n) and 0.5 / sqrt(n)), the median |z| (0.68 for a normal z), the
    whole-image sums, and the worst deviation among the pixels that are constant on both sides."""
    g = np.asarray(run_images, np.float64)[..., :3]
    assert g.shape[0] == runs
    gm, gs = g.mean(0), g.std(0, ddof=1)
    m, sd = np.asarray(ref_mean, np.float64), np.asarray(ref_std, np.float64)
    finite = np.isfinite(gm) & np.isfinite(gs) & np.isfinite(m) & np.isfinite(sd)
    vary = finite & ((sd > 0) | (gs > 0))
    se = np.sqrt((gs[vary] ** 2 + sd[vary] ** 2) / float(runs))
    d = gm[vary] - m[vary]
    z = d / se
    const = finite & ~vary
    dev = np.abs(gm[const] - m[const]) / np.maximum(np.abs(m[const]), 1e-3)
    n = int(vary.sum())
    return {"n": n, "mean_z": float(z.mean()), "mean_z_in_sigmas": float(z.mean() * np.sqrt(n) / 1.1), "positive_share": float((d > 0).mean()),
            "positive_share_in_sigmas": float(((d > 0).mean() - 0.5) * 2.0 * np.sqrt(n)), "median_abs_z": float(np.median(np.abs(z))),
            "share_abs_z_gt_5": float((np.abs(z) > 5).mean()),
            "image_sum_rel_err": float(d.sum() / m[vary].sum()), "image_sum_err_in_sigmas": float(d.sum() / np.sqrt((se * se).sum())),
            "n_const": int(const.sum()), "max_const_rel_dev": float(dev.max()) if dev.size else 0.0,
            "nonfinite_here": int((~np.isfinite(gm)).sum()), "nonfinite_ref": int((~np.isfinite(m)).sum())}


def frac_bit_equal(a, b):
    return float((bits(a[..., :3]) == bits(b[..., :3])).all(-1).mean())



def window_mismatches_without_a_tie(oracle, scene, cam, st, img, x0, y0, size):
    """Compare a window with the oracle; a pixel may differ only if one of its samples met two surfaces at exactly the same t
    (there the reference's own answer depends on its randomly shaped BVH; the oracle counts such events, the device breaks the tie
    by the lower triangle slot).  Returns (pixels equal, pixels differing with a tie, pixels differing WITHOUT one)."""
    want = oracle.render_region(scene, cam, st, x0, y0, size, size, seed=1)
    got = img[y0:y0 + size, x0:x0 + size]
    e = same(got[..., :3], want[..., :3]).all(-1)
    tied = untied = 0
    for (py, px) in zip(*np.nonzero(~e)):
        oracle.render_region(scene, cam, st, x0 + int(px), y0 + int(py), 1, 1, seed=1)
        cn = oracle.counters(scene)
        if cn["closest_hit_ties"] > 0 or cn["hits_outside_own_box"] > 0:
            tied += 1
        else:
            untied += 1
    return int(e.sum()), tied, untied, l2(got, want)


def random_rays(n, seed, extent=4.0):
    rng = np.random.RandomState(seed)
    o = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return np.concatenate([o, d.astype(np.float32)], axis=1).astype(np.float32)


def procedural_case():
    """Analytic scene in the spirit of the reference's FourSpheres / RandomSpheres demos (src/main.cc:913-984):
    every material class, a moving cube (shutter open), depth of field, a sun."""
    mats = np.zeros(6, ffi.MAT_DTYPE)
    for m in mats:
        for k in ("texAlbedo", "texNormal", "texRoughness", "texMetallic", "texEmissive"):
            m[k] = -1
        m["transmission"] = (1, 1, 1)
    mats[0]["type"] = ffi.MAT_MICROFACET; mats[0]["albedo"] = (1, 1, 1); mats[0]["roughness"] = 0.0
    mats[1]["type"] = ffi.MAT_DIELECTRIC; mats[1]["ior"] = 1.5; mats[1]["transmission"] = (1, 0.5, 0.5)
    mats[2]["type"] = ffi.MAT_LAMBERTIAN; mats[2]["albedo"] = (0.8, 0.3, 0.3)
    mats[3]["type"] = ffi.MAT_METAL; mats[3]["albedo"] = (0.8, 0.6, 0.2); mats[3]["fuzziness"] = 0.3
    mats[4]["type"] = ffi.MAT_DIFFUSE_LIGHT; mats[4]["albedo"] = (4, 4, 4)
    mats[5]["type"] = ffi.MAT_MIRROR; mats[5]["albedo"] = (0.9, 0.9, 0.95)
    sph = np.zeros(5, ffi.SPHERE_DTYPE)
    sph[0] = ((0, -100.5, -1), 100.0, 0); sph[1] = ((-1, 0.02, -1), 0.5, 1); sph[2] = ((0, 0.02, -1), 0.5, 2)
    sph[3] = ((1, 0.02, -1), 0.5, 3); sph[4] = ((0, 2.5, -1), 0.7, 4)
    cub = np.zeros(2, ffi.CUBE_DTYPE)
    cub[0] = ((-0.3, -0.45, 0.2), (0.3, -0.1, 0.6), 0.0, (0.5, 0, 0), 2)
    cub[1] = ((1.2, -0.45, -0.3), (1.6, 0.4, 0.1), 0.0, (0, 0, 0), 5)
    cam = dict(origin=(0, 0.5, 3), look_at=(0, 0, -1), fov=45.0, aspect=1.5, aperture=0.05, focal=4.0, shutter=(0.0, 1.0),
               sun=(1, 1, 1), sun_dir=(0.0, -1.0, -0.3))
    return mats, sph, cub, cam


def procedural_flat():
    mats, sph, cub, cam = procedural_case()
    return ffi.FlatScene(np.zeros(0, ffi.TRI_DTYPE), mats, spheres=sph, cubes=cub, num_shapes=0,
                         sun_illuminance=cam["sun"], sun_direction=cam["sun_dir"]), cam


# ---- GPU parity helpers shared by the test files ---------------------------------------------------------------------------------
L2_TOL = 1e-4
FLT_MAX = 3.4028234663852886e38


def tie_mask(oracle, flat, cam, w, h):
    """Pixels whose unjittered primary ray has two or more triangles at the minimum t."""
    ys, xs = np.mgrid[0:h, 0:w]
    uv = np.stack([xs.ravel() / np.float32(w), ys.ravel() / np.float32(h)], 1).astype(np.float32)
    rays = oracle.camera_rays(cam, uv, seed=1)[:, :6]
    tmin = np.full(len(rays), np.inf, np.float32)
    count = np.zeros(len(rays), np.int32)
    for tri in flat.triangles:
        hts = oracle.triangle_hit(np.repeat(tri[None], len(rays)), rays, 1e-4, FLT_MAX)
        t = np.where(hts["hit"] == 1, hts["t"], np.inf).astype(np.float32)
        closer = t < tmin
        same = (t == tmin) & np.isfinite(t)
        count = np.where(closer, 1, count + same.astype(np.int32))
        tmin = np.minimum(tmin, t)
    return (count > 1).reshape(h, w)


def assert_same_outside_ties(img, want, ties, what):
    assert ties.mean() < 0.02, "too many tie pixels for a meaningful comparison"
    eq = same(img, want)[~ties]
    assert eq.all(), "%s: %d of %d non-tie pixels differ (L2 %.3e)" % (what, (~eq).any(-1).sum(), len(eq), l2(img, want))


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ---- ray-query intervals (tests/test_ray_query_host.py, tests/test_gpu_ray_query_intervals.py) -------------------------------------------
F32_MAX = np.float32(3.4028235e38)
F32_DENORM = np.float32(1e-45)          # the least positive denormal


def nextup(x):
    return np.nextafter(np.asarray(x, np.float32), np.float32(np.inf))


def nextdown(x):
    return np.nextafter(np.asarray(x, np.float32), np.float32(-np.inf))


def rays8(o, d, tmin=1e-4, tmax=F32_MAX):
    """n x (org, tMin, dir, tMax), the layout of RaylibAMDRay"""
    d = np.asarray(d, np.float32)
    r = np.zeros((len(d), 8), np.float32)
    r[:, 0:3] = o; r[:, 3] = tmin; r[:, 4:7] = d; r[:, 7] = tmax
    return r


def with_interval(rays, tmin=None, tmax=None):
    r = np.array(rays, np.float32, copy=True)
    if tmin is not None:
        r[:, 3] = tmin
    if tmax is not None:
        r[:, 7] = tmax
    return r


def peel(oracle, scene, rays, layers, tmin0=0.0, ray_time=0.0):
    """The first `layers` surfaces of each ray by the brute-force oracle alone: layer k+1 is interval_hits over [nextup(t_k), FLT_MAX].
    Returns (layers, n) float32, +inf from the layer at which a ray runs out of surfaces."""
    n = len(rays)
    T = np.full((layers, n), np.inf, np.float32)
    lo = np.full(n, tmin0, np.float32)
    alive = np.ones(n, bool)
    for k in range(layers):
        idx = np.nonzero(alive)[0]
        if not len(idx):
            break
        got = oracle.interval_hits(scene, with_interval(rays[idx], lo[idx], F32_MAX), ray_time)
        T[k, idx] = got["t"]
        alive[idx] = np.isfinite(got["t"])
        lo[idx] = nextup(got["t"])
    return T
