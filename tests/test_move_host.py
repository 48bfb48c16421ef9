"""RaylibAMD_SceneMoveTriangles without a device: what the entry refuses before it reaches one, and the host side of the refit -- the box ids the builder
records for the wide formats, the grid rule shared with the device against the builder's former quantiser, the leaf order's inverse (tools/move_host_check.cc)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import helpers
import move_cases as mc
import stack_edges
from raylib_amd import binding

ROOT = helpers.ROOT


def test_box_ids_grid_rule_and_leaf_order(tmp_path):
    """tools/move_host_check.cc compiled with g++ (no FMA contraction, as the library) against rl_bvh.cc alone, and run: every wide child's recorded box id names
    the binary tree's box with the child's bits; the builder's DNode4Q / DNode8 planes are what its former quantiser, restated in the program, makes of the same
    boxes; the re-derivation from the binary tree's boxes gives the builder's DNode4Q / DNode8 / leaf-list records and SAH cost back byte for byte; the leaf order is a permutation; after a third of the triangles has moved and the binary boxes are refitted, the re-derived formats pass the builder's
    validators, cost at least a fresh build, and moved back are the builder's bytes again."""
    exe = str(tmp_path / "move_host_check")
    src = os.path.join(ROOT, "software-raytracing_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DRAYLIB_EXPORTS=1", "-I" + os.path.join(ROOT, "include"), "-I" + src,
                           os.path.join(ROOT, "tools", "move_host_check.cc"), os.path.join(src, "rl_bvh.cc"), os.path.join(src, "rl_log.cc"), "-o", exe, "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "move_host_check: ok" in out.stdout


def test_refusals_that_need_no_device(lib, workdir):
    """Checked before anything is touched: an unknown scene, a scene not finalized, a range outside the scene, null positions, a value that is not finite (host
    entry).  count == 0 is 1 whatever the pointers.  Every refusal leaves the host's triangles as they were."""
    ses = mc.soup_session(lib, workdir, "move_refusals", mc.soup_triangles(40, seed=2))
    n = lib.RaylibAMD_SceneNumTriangles(ses.scene)
    assert n == 40
    before = mc.export(ses).tobytes()
    P = mc.pos9(mc.export(ses)[:4]) + np.float32(0.5)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    move, moved = lib.RaylibAMD_SceneMoveTriangles, lib.RaylibAMD_SceneMoveTrianglesDevice
    assert move(ses.scene, 0, 0, None, None) == 1 and move(ses.scene, n, 0, None, None) == 1 and moved(ses.scene, 3, 0, None, None, None) == 1
    assert move(0, 0, 4, fp(P), None) == 0 and move(12345, 0, 4, fp(P), None) == 0
    loose = lib.Raylib_CreateScene()
    assert move(loose, 0, 0, None, None) == 0 and move(loose, 0, 4, fp(P), None) == 0      # not finalized
    assert lib.Raylib_DestroyScene(loose) == 1
    for first, count in ((-1, 4), (0, -1), (n - 3, 4), (n, 1), (0, n + 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert move(ses.scene, first, count, fp(P), None) == 0, (first, count)
        assert moved(ses.scene, first, count, fp(P), None, None) == 0, (first, count)
    assert move(ses.scene, 0, 4, None, None) == 0 and moved(ses.scene, 0, 4, None, None, None) == 0
    for bad in (np.nan, np.inf, -np.inf):
        Q = P.copy(); Q[2, 5] = bad
        assert move(ses.scene, 0, 4, fp(Q), None) == 0
        assert move(ses.scene, 0, 4, fp(P), fp(Q)) == 0
    assert binding.move_triangles(lib, ses.scene, 0, np.zeros((0, 9), np.float32)) == 1
    assert mc.export(ses).tobytes() == before
    assert lib.RaylibAMD_SceneRebuild(0) == 0 and lib.RaylibAMD_SceneCheckTrees(0, None) == 0
    ses.close()


def test_a_rebuild_of_an_unmoved_scene_is_the_same_tree(lib, workdir):
    """RaylibAMD_SceneRebuild of an unmoved scene is the build again: the same hashes, the same nodes."""
    ses = mc.soup_session(lib, workdir, "move_rebuild", mc.soup_triangles(40, seed=3))
    h0, t0, n0 = lib.RaylibAMD_SceneBVHHash(ses.scene), lib.RaylibAMD_SceneTopologyHash(ses.scene), mc.bvh_nodes(lib, ses.scene).tobytes()
    assert t0 not in (0, h0)
    assert lib.RaylibAMD_SceneRebuild(ses.scene) == 1
    assert (lib.RaylibAMD_SceneBVHHash(ses.scene), lib.RaylibAMD_SceneTopologyHash(ses.scene), mc.bvh_nodes(lib, ses.scene).tobytes()) == (h0, t0, n0)
    assert lib.RaylibAMD_SceneTopologyHash(0) == 0 and lib.RaylibAMD_SceneExportBVHNodes(0, None) == 0
    ses.close()


def _fresh_scenes(lib, workdir):
    """(name, session) of freshly finalized scenes: a 300-triangle soup, the Cornell box, and the deepest tree the suite builds (stack_edges.deepest_triangles)."""
    yield "soup", mc.soup_session(lib, workdir, "restate_soup", mc.soup_triangles(300, seed=12))
    obj, _ = helpers.build_case("cornell", os.path.join(str(workdir), "restate_cornell"))
    yield "cornell", mc.case_session(lib, "cornell", obj)
    yield "deepest", mc.soup_session(lib, workdir, "restate_deepest", stack_edges.deepest_triangles())


def test_the_refit_restated_reproduces_the_builders_boxes(lib, workdir):
    """move_cases.refit_boxes (csrc/rl_k_refit.inl k_refit_level in NumPy), applied to the builder's own nodes of a fresh scene, gives the builder's boxes back
    as values: the restatement is held to an independent implementation before the device is held to the restatement (tests/test_gpu_move.py assert_trees,
    tests/test_gpu_refit_exact.py).  Compared with ==: the builder grows an inner node's box over its primitives, the refit over its two child boxes, and on a
    face that holds zeros of both signs the two may pick different ones.  And the restatement is not the identity: with one triangle moved it changes the boxes
    on that triangle's path and no other."""
    for name, ses in _fresh_scenes(lib, workdir):
        nodes, tris, order = mc.bvh_nodes(lib, ses.scene), mc.export(ses), mc.tri_order(lib, ses.scene)
        assert sorted(order.tolist()) == list(range(len(tris))), name
        if name == "deepest":
            assert mc.bvh_info(lib, ses.scene)[2] == stack_edges.DEEPEST_DEPTH
        want = mc.refit_boxes(nodes, tris, order)
        for k in mc.BOXES:
            assert (nodes[k] == want[k]).all(), (name, k, np.nonzero(~(nodes[k] == want[k]).all(1))[0][:4])
        assert all(nodes[k].tobytes() == want[k].tobytes() for k in ("left", "right", "pad")), name
        moved = tris.copy()
        moved["v1"][len(tris) // 2] = np.float32(2.0 ** 40)           # far outside every box: each box on the path to it grows, the root's included
        got = mc.refit_boxes(nodes, moved, order)
        changed = np.zeros(len(nodes), bool)
        for k in mc.BOXES:
            changed |= (got[k] != nodes[k]).any(1)
        assert changed[0] and 1 <= changed.sum() <= mc.node_levels(nodes).max() + 1, (name, changed.sum())
        ses.close()


NO_DEVICE_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import move_cases as mc
from raylib_amd import binding
lib = binding.load()
assert lib.RaylibAMD_DeviceAvailable() == 0, "the devices are not hidden from this process"
ses = mc.soup_session(lib, sys.argv[1], "move_nodevice", mc.soup_triangles(40, seed=3))
before, h0 = mc.export(ses), lib.RaylibAMD_SceneBVHHash(ses.scene)
P = mc.pos9(before[:4]) + np.float32(0.5)
assert binding.move_triangles(lib, ses.scene, 0, P) == 0
assert mc.export(ses).tobytes() == before.tobytes() and lib.RaylibAMD_SceneBVHHash(ses.scene) == h0
assert lib.RaylibAMD_SceneCheckTrees(ses.scene, None) == 0 and lib.RaylibAMD_SceneRebuild(ses.scene) == 1
ses.close()
print("refused without a device")
"""


def test_a_move_without_a_device_is_refused(workdir):
    """No device: the host entry returns 0 and changes nothing (the library has no CPU path).  In a process of its own from which every device is hidden, so that
    the path is the one taken on a machine with a GPU too; the move with a device is tests/test_gpu_move.py's."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", RAYLIB_QUIET="1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD % os.path.dirname(os.path.abspath(__file__)), str(workdir)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused without a device" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
