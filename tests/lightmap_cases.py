"""Shared by tests/test_lightmap_host.py and tests/test_gpu_lightmap.py (RaylibAMD_BakeLightmap, include/raylib_amd.h): statements 1 to 6 and 8 to 9 of the
header's contract restated in NumPy -- int64 for the integers, one float32 operation at a time for the floats, float64 for the barycentrics' division --, and
the two UV generators of the tests.  Statement 7, the gather, is RaylibAMD_Gather's."""
import numpy as np

F = np.float32
I = np.int64
NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]   # (dx, dy), statement 9's order
TRI_DTYPE = np.dtype([("v", "f4", (3, 3)), ("n", "f4", (3, 3)), ("st", "f4", 6), ("material", "i4"), ("shape", "i4")])
assert TRI_DTYPE.itemsize == 104


def scene_triangles(lib, scene):
    """The scene's triangles in RaylibAMD_SceneExportTriangles order."""
    tris = np.zeros(lib.RaylibAMD_SceneNumTriangles(scene), TRI_DTYPE)
    lib.RaylibAMD_SceneExportTriangles(scene, tris.ctypes.data)
    return tris


# ---- the UV generators ----
def grid_uv(n_tris, margin=0.05):
    """"grid": triangles 2p and 2p + 1 (a quad's pair) get cell p of a g x g grid, g = ceil(sqrt(pairs)), shrunk by `margin` of a cell on every side; the two
    share the cell's diagonal exactly, and with margin 0 neighbouring cells share their edges exactly.  (n_tris, 6) float32."""
    pairs = (n_tris + 1) // 2
    g = int(np.ceil(np.sqrt(pairs)))
    p = np.arange(pairs)
    cx, cy = (p % g).astype(np.float64), (p // g).astype(np.float64)
    x0, x1, y0, y1 = [a.astype(F) for a in ((cx + margin) / g, (cx + 1 - margin) / g, (cy + margin) / g, (cy + 1 - margin) / g)]
    uv = np.zeros((pairs, 2, 6), F)
    uv[:, 0] = np.stack([x0, y0, x1, y0, x1, y1], 1)
    uv[:, 1] = np.stack([x0, y0, x1, y1, x0, y1], 1)
    return np.ascontiguousarray(uv.reshape(-1, 6)[:n_tris])


def own_uv(tris):
    """"own": what uv = NULL stands for."""
    return np.ascontiguousarray(tris["st"], F)


# ---- statements 1 to 3 ----
def snap(uv, w, h):
    """Statements 1 and 2: X, Y (n, 3) int64, A2 (n,) int64 and which triangles are kept."""
    uv = np.ascontiguousarray(uv, F).reshape(-1, 6)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = ((uv[:, 0::2] * F(w)).astype(F) * F(256)).astype(F)
        fy = ((uv[:, 1::2] * F(h)).astype(F) * F(256)).astype(F)
        f = np.concatenate([fx, fy], 1)
        ok = (np.isfinite(f) & ~(np.abs(f) > F(16777216))).all(1)
        X = np.where(ok[:, None], np.floor((fx + F(0.5)).astype(F)), 0).astype(I)
        Y = np.where(ok[:, None], np.floor((fy + F(0.5)).astype(F)), 0).astype(I)
    A2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    return X, Y, A2, ok & (A2 != 0)


def _orient(qx, qy, rx, ry, px, py):
    return (rx - qx) * (py - qy) - (ry - qy) * (px - qx)


def weights(X, Y, A2, px, py):
    """Statement 3's wA, wB, wC of triangles (X, Y, A2: (..., 3), (..., 3), (...)) at the points px, py (sub-texel units), broadcast."""
    s = np.sign(A2)
    wA = s * _orient(X[..., 1], Y[..., 1], X[..., 2], Y[..., 2], px, py)
    wB = s * _orient(X[..., 2], Y[..., 2], X[..., 0], Y[..., 0], px, py)
    wC = s * _orient(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], px, py)
    return wA, wB, wC


def owners(uv, w, h):
    """Statement 3: per texel the lowest-indexed covering triangle of the range, -1 where none; (h, w) int64."""
    X, Y, A2, keep = snap(uv, w, h)
    owner = np.full((h, w), -1, I)
    for k in np.nonzero(keep)[0]:
        # the texels whose centres 256 x + 128 lie in the box: ceil((min - 128) / 256) .. floor((max - 128) / 256), inside the atlas
        x0, x1 = max(0, -((128 - int(X[k].min())) // 256)), min(w - 1, (int(X[k].max()) - 128) // 256)
        y0, y1 = max(0, -((128 - int(Y[k].min())) // 256)), min(h - 1, (int(Y[k].max()) - 128) // 256)
        if x1 < x0 or y1 < y0:
            continue
        px = (256 * np.arange(x0, x1 + 1, dtype=I) + 128)[None, :]
        py = (256 * np.arange(y0, y1 + 1, dtype=I) + 128)[:, None]
        wA, wB, wC = weights(X[k], Y[k], A2[k], px, py)
        sub = owner[y0:y1 + 1, x0:x1 + 1]
        sub[(wA >= 0) & (wB >= 0) & (wC >= 0) & (sub < 0)] = k
    return owner


# ---- statements 4 to 6 ----
def _dot(a, b):
    return ((a[:, 0] * b[:, 0]).astype(F) + (a[:, 1] * b[:, 1]).astype(F) + (a[:, 2] * b[:, 2]).astype(F)).astype(F)


def _cross(a, b):
    m = lambda p, q: (p * q).astype(F)
    return np.stack([(m(a[:, 1], b[:, 2]) - m(a[:, 2], b[:, 1])).astype(F), (m(a[:, 2], b[:, 0]) - m(a[:, 0], b[:, 2])).astype(F),
                     (m(a[:, 0], b[:, 1]) - m(a[:, 1], b[:, 0])).astype(F)], 1)


def points(tris, uv, w, h, time=0.0):
    """Statements 1 to 6: (points (n, 8) float32 with the stream's bits in the last column, texel indices (n,) uint32, the owner map)."""
    uv = own_uv(tris) if uv is None else np.ascontiguousarray(uv, F).reshape(-1, 6)
    owner = owners(uv, w, h)
    X, Y, A2, _ = snap(uv, w, h)
    texel = np.nonzero(owner.ravel() >= 0)[0]
    k = owner.ravel()[texel]
    px, py = 256 * (texel % w) + 128, 256 * (texel // w) + 128
    _, wB, wC = weights(X[k], Y[k], A2[k], px, py)
    area = np.abs(A2[k]).astype(np.float64)
    b1 = (wB.astype(np.float64) / area).astype(F)[:, None]
    b2 = (wC.astype(np.float64) / area).astype(F)[:, None]
    v, n = tris["v"][k], tris["n"][k]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e1, e2 = (v[:, 1] - v[:, 0]).astype(F), (v[:, 2] - v[:, 0]).astype(F)
        pos = ((v[:, 0] + (b1 * e1).astype(F)).astype(F) + (b2 * e2).astype(F)).astype(F)
        nn = ((n[:, 0] + (b1 * (n[:, 1] - n[:, 0]).astype(F)).astype(F)).astype(F) + (b2 * (n[:, 2] - n[:, 0]).astype(F)).astype(F)).astype(F)
        d = _dot(nn, nn)
        bad = ~(np.isfinite(d) & (d > 0))
        face = _cross(e1, e2)
        nn = np.where(bad[:, None], face, nn).astype(F)
        d = np.where(bad, _dot(face, face), d).astype(F)
        full = np.isfinite(d) & (d > 0) & np.isfinite(pos).all(1)
        normal = (nn * (F(1) / np.sqrt(d).astype(F)).astype(F)[:, None]).astype(F)
    out = np.zeros((len(texel), 8), F)
    out[:, 0:3] = pos; out[:, 3] = F(time); out[:, 4:7] = normal; out[:, 7] = texel.astype(np.uint32).view(F)
    return np.ascontiguousarray(out[full]), texel[full].astype(np.uint32), owner


# ---- statements 8 and 9 ----
def scatter(values, texel, w, h):
    """Statement 8: the atlas (h, w, C) and its coverage (h, w) uint8 from the points' values (n, C) and texel indices."""
    values = np.ascontiguousarray(values, F)
    c = values.shape[1]
    atlas = np.zeros((h * w, c), F)
    cov = np.zeros(h * w, np.uint8)
    atlas[texel] = values
    cov[texel] = 1
    return atlas.reshape(h, w, c), cov.reshape(h, w)


def dilate(atlas, cov, passes):
    """Statement 9 (C == 4 is IRRADIANCE: channel 3 of a filled texel becomes 1)."""
    atlas, cov = np.array(atlas, F), np.array(cov, np.uint8)
    h, w, c = atlas.shape
    for k in range(1, passes + 1):
        pa = np.zeros((h + 2, w + 2, c), F); pa[1:-1, 1:-1] = atlas
        pc = np.zeros((h + 2, w + 2), np.uint8); pc[1:-1, 1:-1] = cov
        s = np.zeros((h, w, c), F)
        m = np.zeros((h, w), np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            for dx, dy in NEIGHBOURS:
                on = pc[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != 0
                s = np.where(on[..., None], (s + pa[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]).astype(F), s)
                m += on
            fill = (cov == 0) & (m > 0)
            val = (s * (F(1) / np.maximum(m, 1).astype(F)).astype(F)[..., None]).astype(F)
        if c == 4:
            val[..., 3] = F(1)
        atlas = np.where(fill[..., None], val, atlas).astype(F)
        cov = np.where(fill, np.uint8(1 + k), cov).astype(np.uint8)
    return atlas, cov


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- constructed edge inputs, on a range of n_tris triangles (every triangle not named below has all-zero UVs: zero area, skipped) ----
def edge_inputs(n_tris=36):
    """name -> (w, h, uv (n_tris, 6) float32)."""
    nan = float("nan")
    T = lambda *c: np.array(c, np.float64) / 8.0
    out = {}

    def case(name, w, h, tris):
        uv = np.zeros((n_tris, 6), F)
        for k, t in tris.items():
            uv[k] = np.asarray(t, F)
        out[name] = (w, h, uv)
    case("vertex_on_centre", 8, 8, {3: T(2.5, 3.5, 6, 3.5, 2.5, 7)})
    case("shared_edge_through_centres", 8, 8, {0: T(0.5, 0.5, 7.5, 0.5, 7.5, 7.5), 1: T(0.5, 0.5, 7.5, 7.5, 0.5, 7.5)})
    case("shared_edge_reversed_order", 8, 8, {4: T(0.5, 0.5, 7.5, 7.5, 0.5, 7.5), 9: T(7.5, 7.5, 0.5, 0.5, 7.5, 0.5)})
    case("overlap_lowest_wins", 16, 16, {5: T(1, 1, 7, 1, 1, 7), 2: T(0, 0, 5, 0, 0, 5), 7: T(0, 0, 8, 0, 0, 8)})
    case("zero_area", 8, 8, {0: T(1, 1, 3, 3, 5, 5), 1: T(2, 2, 2, 2, 2, 2), 2: T(0, 0, 8, 0, 0, 8)})
    case("nan_uv", 8, 8, {0: [nan, 0, 1, 0, 0, 1], 1: [0, 0, 1, 0, 0, float("inf")], 2: T(0, 0, 8, 0, 0, 8)})
    case("far_outside_skipped", 8, 8, {0: [1e6, 0, 1, 0, 0, 1], 1: [0, -1e6, 1, 0, 0, 1], 2: T(1, 1, 6, 1, 1, 6)})
    case("far_outside_clipped", 8, 8, {0: T(6, 6, 100, 6, 6, 100), 1: T(-50, 3, 4, 3, 4, 4), 5: T(-24, -24, 40, -24, -24, 40)})
    case("box_is_whole_atlas", 13, 7, {6: [-0.5, -0.5, 2.5, -0.5, -0.5, 2.5]})
    case("negative_area", 8, 8, {0: T(0, 0, 0, 8, 8, 0)})
    return out


def big_and_small(n_tris):
    """The dealing's worst case on a 128 x 128 atlas: n_tris - 1 triangles smaller than a texel each and, last, one triangle that fills the atlas."""
    uv = (grid_uv(n_tris, 0.05) * F(0.3)).astype(F)
    uv[-1] = [-0.5, -0.5, 2.5, -0.5, -0.5, 2.5]
    return 128, 128, uv


ATLASES = [(61, 47), (128, 128), (1, 1)]


def triangle_scene(lib, triangles):
    """A scene of loose triangles (v (3, 3), n (3, 3), uv (6,)) through RaylibAMD_CreateTriangle."""
    import ctypes as C
    from raylib_amd import binding
    mat = binding.create_material(lib, dict(type=0, albedo=(0.5, 0.5, 0.5), roughness=0.0, metallic=0.0, emissive=(0, 0, 0), ior=1.0, transmission=(0, 0, 0), fuzziness=0.0))
    assert mat
    scene = lib.Raylib_CreateScene()
    elems = []
    fp = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
    for v, n, uv in triangles:
        v, n, uv = np.asarray(v, F), np.asarray(n, F), np.asarray(uv, F)
        e = lib.RaylibAMD_CreateTriangle(fp(v[0]), fp(v[1]), fp(v[2]), fp(n[0]), fp(n[1]), fp(n[2]), fp(uv), mat)
        assert e
        elems.append(e); lib.Raylib_AddSceneElement(scene, e)
    lib.Raylib_FinalizeScene(scene)

    def close():
        lib.Raylib_DestroyScene(scene)
        for e in elems:
            lib.RaylibAMD_DestroySceneElement(e)
        lib.RaylibAMD_DestroyMaterial(mat)
    return scene, close
