"""The lazy-reflectance instance leaves a scattering event's pdf unevaluated where two compares decide what the kernel reads of it (csrc/rl_dev_shade.h
LazyPdfQuick, LazyScatterPdf); the fold recomputes it from the vertex record on lit paths (LazyRecordPdf).  The decision and both record forms are swept on the
device (RaylibAMD_VerifyLazyPdf); frames that consume every record, and frames full of grazing events, must be the eager instance's bit for bit."""
import ctypes as C
import os

import pytest

from helpers import scenes
from test_gpu_lazy_refl import H, W, _binding, render_both
from test_lazy_refl_host import MTL, box_with

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [7, 20261019])
def test_pdf_guard_sweep(gpu_lib, seed):
    """No quick event with a pdf that is not positive, a non-finite sp or half vector, or a record that folds to other bits; the edge inputs reach the
    fallback, and the quick path is the common one (the cap is no measurement: LazyVertexSafe refuses 11.3 % of this distribution)."""
    n = 1 << 22
    ev, wrong, refused = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert gpu_lib.RaylibAMD_VerifyLazyPdf(n, seed, C.byref(ev), C.byref(wrong), C.byref(refused)) == 1
    print("pdf guard sweep, seed %d: %d events, %d wrong, %d refused (%.3f %%)" % (seed, ev.value, wrong.value, refused.value, 100.0 * refused.value / max(1, ev.value)))
    assert ev.value == n
    assert wrong.value == 0
    assert refused.value > 0
    assert refused.value <= 0.20 * n


@pytest.fixture(scope="module")
def bright(gpu_lib, workdir):
    """Ceiling, floor and walls all emit (the bright box of test_gpu_lazy_refl.py): nearly every path is lit, nearly every record is folded."""
    d = os.path.join(str(workdir), "lazy_pdf_gpu"); os.makedirs(d, exist_ok=True)
    mtl = MTL.replace("Ns 10\nillum 2", "Ns 10\nKe 0.5 0.25 0.125\nillum 2") % dict(kd="0.725 0.71 0.68", ks="0 0 0", ns="10", pr="Ke 0.25 0.5 1")
    obj = scenes.write_obj(os.path.join(d, "bright.obj"), scenes.cornell_objects(scenes.WHITE, scenes.WHITE), mtl)[0]
    ses = _binding().SceneSession(gpu_lib, obj, (0, 1, 4), (0, 1, -1), 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    yield ses
    ses.close()


@pytest.mark.parametrize("max_path", [5, 12])
@pytest.mark.parametrize("entries", ["0", None])
def test_every_record_folded(gpu_lib, bright, monkeypatch, entries, max_path):
    """RAYLIB_LIT_LIST=0: every fold in place, inside k_trace_lazy; the default list: k_fold_lit, and in place for the paths of more than five vertices."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    if entries is not None:
        monkeypatch.setenv("RAYLIB_LIT_LIST", entries)
    st = render_both(bright, gpu_lib, monkeypatch, max_path=max_path)
    assert st.litPaths * 2 > st.cameraSamples, (st.litPaths, st.cameraSamples)
    if entries == "0":
        assert st.litFoldedInPlace == st.litPaths
    else:
        # (the default list holds an entry per 32 jobs: a frame this bright overflows it, and what does not fit folds in place as well)
        assert st.litPaths > st.litFoldedInPlace, (st.litPaths, st.litFoldedInPlace)
        assert st.litFoldedInPlace > 0 or max_path == 5


@pytest.mark.parametrize("name,pr", [("low", "Pr 0.0009765625\nPm 0.75"), ("high", "Pr 1\nPm 1")])
def test_grazing_view(gpu_lib, workdir, monkeypatch, name, pr):
    """The camera 2^-11 above the floor (below the boxes, which float 2^-10 above it), looking along it: the lower half of the frame meets the floor at
    grazing angles, |Wo.z| down to 1e-3, where half vectors graze too.  Roughness at both ends of the lazy interval."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    d = os.path.join(str(workdir), "lazy_pdf_gpu"); os.makedirs(d, exist_ok=True)
    y = 2.0 ** -11
    ses = _binding().SceneSession(gpu_lib, box_with(os.path.join(d, "graze_%s.obj" % name), pr=pr), (0, y, 0.96875), (0, y, -1), 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 1
    st = render_both(ses, gpu_lib, monkeypatch)
    assert st.litPaths > 0 and st.shadedHits > st.cameraSamples
    ses.close()


def test_refused_scene_stays_eager(gpu_lib, workdir, monkeypatch):
    """A roughness just below the interval: the planner refuses, the eager plain instance renders, with or without RAYLIB_LAZY_REFL."""
    monkeypatch.setenv("RAYLIB_POOL", "0")
    d = os.path.join(str(workdir), "lazy_pdf_gpu"); os.makedirs(d, exist_ok=True)
    ses = _binding().SceneSession(gpu_lib, box_with(os.path.join(d, "rough_out.obj"), pr="Pr 0.00097"), (0, 1, 4), (0, 1, -1), 45.0, W / H)
    assert gpu_lib.RaylibAMD_SceneLazyRefl(ses.scene) == 0 and gpu_lib.RaylibAMD_ScenePlain(ses.scene) == 1
    st = render_both(ses, gpu_lib, monkeypatch, want_lazy=0)
    assert st.litPaths == 0 and st.litFoldedInPlace == 0
    ses.close()
