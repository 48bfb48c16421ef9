"""The query families share one ring of work counters (RL_QUERY_RING of csrc/rl_rt.h) and one set of staging buffers (qRays, qOut, qPrim, qContact): here they
alternate.  2 * RL_QUERY_RING + 2 calls cycle over the ray queries (ANY, CLOSEST, SURFACE with primitives), the multi-hit queries, the nearest-point queries
(WITHIN, CLOSEST), the K-nearest queries, the overlap queries (ANY, LIST), the contact segments and a signed distance-field bake -- once through the device
entries, spread over three caller streams and all enqueued before any wait, and once through the host-memory entries back to back, which re-uses the staging
buffers at 16-, 32- and 48-byte records and at every output size.  Every call's outputs equal, byte for byte, what one call of its family gave before the
sequence: the family's host oracle where it has one, a single call through the same entry where it has none (the ray queries)."""
import os

import numpy as np
import pytest
import torch    # before the library is loaded: the device entry is handed torch's tensors

import helpers
import nearest_cases as nc
import overlap_cases as oc
import sdf_cases as sc
from raylib_amd import binding

pytestmark = pytest.mark.gpu

RING = 64                      # RL_QUERY_RING
CALLS = 2 * RING + 2
N = 256
DIMS = (8, 8, 8)


def _bytes(out):
    """A call's outputs as one byte string: arrays or tensors, alone or in a tuple (None: an output not asked for)."""
    parts = out if isinstance(out, tuple) else (out,)
    return b"".join((p.cpu().numpy() if isinstance(p, torch.Tensor) else p).tobytes() for p in parts if p is not None)


def _families(lib, scene, rays, points, queries, grid, **kw):
    """name -> call, on the given inputs (NumPy arrays: the host-memory entries, or with host=True in kw the oracles; tensors: the device entries)."""
    bake_kw = dict(kw) if isinstance(rays, np.ndarray) else {"device": True}
    return [
        ("TraceRays ANY", lambda: binding.trace_rays(lib, scene, rays, binding.QUERY_ANY)),
        ("TraceRays CLOSEST", lambda: binding.trace_rays(lib, scene, rays, binding.QUERY_CLOSEST)),
        ("TraceRays SURFACE", lambda: binding.trace_rays(lib, scene, rays, binding.QUERY_SURFACE, with_prim=True)),
        ("TraceRaysAll", lambda: binding.trace_rays_all(lib, scene, rays, 3, count=True, **kw)),
        ("NearestPoints WITHIN", lambda: binding.nearest_points(lib, scene, points, binding.NEAREST_WITHIN, **kw)),
        ("NearestPoints CLOSEST", lambda: binding.nearest_points(lib, scene, points, binding.NEAREST_CLOSEST, **kw)),
        ("NearestPointsAll", lambda: binding.nearest_points_all(lib, scene, points, 3, count=True, **kw)),
        ("OverlapTriangles ANY", lambda: binding.overlap_triangles(lib, scene, queries, binding.OVERLAP_ANY, **kw)),
        ("OverlapTriangles LIST", lambda: binding.overlap_triangles(lib, scene, queries, binding.OVERLAP_LIST, 0, 4, count=True, **kw)),
        ("OverlapContacts", lambda: binding.overlap_contacts(lib, scene, queries, 0, 4, **kw)),
        ("BakeDistanceField", lambda: binding.bake_distance_field(lib, scene, grid[0], grid[1], DIMS, float("inf"), binding.SDF_SIGN_MAJORITY, prim=True, **bake_kw)),
    ]


def test_families_alternate_past_the_ring(gpu_lib, workdir, monkeypatch):
    monkeypatch.delenv("RAYLIB_QUERY_TREE", raising=False)
    d = os.path.join(str(workdir), "query_mix"); os.makedirs(d, exist_ok=True)
    ses = nc.session(gpu_lib, nc.write_soup(os.path.join(d, "soup.obj"), 2000))
    try:
        tris = ses.export_flat()[0]
        rng = np.random.RandomState(71)
        r6 = helpers.random_rays(N, 72)
        rays = helpers.rays8(r6[:, :3], r6[:, 3:])
        points = nc.with_max_dist(nc.point_set(rng, tris, N), 1.5)       # (a finite radius: WITHIN answers both ways, the K-nearest counts differ)
        queries = oc.query_set(rng, tris, N - 11)                        # (... and the 11 special records)
        assert len(rays) == N and len(points) == N and len(queries) == N
        grid = sc.grid_around(DIMS, lo=-4.2, hi=4.2, shift=sc.IRRATIONAL)
        host = _families(gpu_lib, ses.scene, rays, points, queries, grid)
        oracle = _families(gpu_lib, ses.scene, rays, points, queries, grid, host=True)
        want = {name: _bytes(call()) for name, call in oracle if not name.startswith("TraceRays ")}
        assert len(host) == 11 and len(want) == 8

        # the device entries: three caller streams, every call enqueued before any wait
        as_words = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(len(a), -1)).cuda()
        dev = _families(gpu_lib, ses.scene, as_words(rays), as_words(points), as_words(queries), grid)
        torch.cuda.synchronize()
        single = {name: _bytes(call()) for name, call in dev if name not in want}     # (on torch's default stream: synchronous)
        streams = [torch.cuda.Stream() for _ in range(3)]
        outs = []
        for i in range(CALLS):
            with torch.cuda.stream(streams[i % 3]):
                outs.append(dev[i % len(dev)][1]())
        for s in streams:
            s.synchronize()
        for i, out in enumerate(outs):
            name = dev[i % len(dev)][0]
            assert _bytes(out) == want.get(name, single.get(name)), "device entries: call %d (%s) on stream %d" % (i, name, i % 3)
        assert single["TraceRays ANY"] != bytes(len(single["TraceRays ANY"])), "some ray hits"

        # the host-memory entries, back to back through the staging buffers
        single = {name: _bytes(call()) for name, call in host if name not in want}
        for i in range(CALLS):
            name, call = host[i % len(host)]
            assert _bytes(call()) == want.get(name, single.get(name)), "host-memory entries: call %d (%s)" % (i, name)
    finally:
        ses.close()
