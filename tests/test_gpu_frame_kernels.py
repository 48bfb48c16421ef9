"""The small kernels behind the megakernel past their first chunk: k_progressive_compact over more than one trip of 8192 entries, and k_pp_max / k_pp_map over
more than one stride of 524 288 pixels, each against a plain reference.

Compaction (RaylibAMD_ProgressiveCompactTest launches the kernel as a pass does) against NumPy:
    keep = live[~stopped[live]];  trace = keep[~empty[keep]] (keep without `empty`);  pixels = the valid pixels of keep[empty[keep]]
Both lists element for element, in order; the counts equal; what lies beyond the counts untouched.

Post-process (Raylib_PostProcess on images made from host pixels and on frames that live on the device) against oracle.postprocess, bit for bit; the images
are tests/postprocess_cases.py's, which the host suite runs through the same entry point.  No comparison here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import helpers
import postprocess_cases as pc
from helpers import bits

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

CHUNK = 8192                                             # RL_COMPACT_BLOCK * RL_COMPACT_PER: the entries of one trip
FRAMES = [(1445, 723), (1024, 512), (44, 36)]            # 16 471 cells: three trips, ragged right and bottom cells; 8192: exactly one full trip; 30: one
NUM_LIVE = (0, 1, 63, 64, 65, 8191, 8192, 8193, 16383, 16384, 16385, 16471)
STOP_PATTERNS = ("none", "all", "every other", "random 10", "random 50", "random 90", "entries 8191 and 8192", "first chunk only", "all but the first chunk",
                 "all but the last entry")
EMPTY_KINDS = ("null", "zeros", "ones", "random", "ring")


def _binding():
    from raylib_amd import binding
    return binding


def _cells(w, h):
    return (w + 7) // 8, (h + 7) // 8


def _stop_mask(pattern, n, rng):
    """which ENTRIES of the list stop"""
    m = np.zeros(n, bool)
    i = np.arange(n)
    if pattern == "all":
        m[:] = True
    elif pattern == "every other":
        m = i % 2 == 0
    elif pattern.startswith("random"):
        m = rng.random_sample(n) < int(pattern.split()[1]) / 100.0
    elif pattern == "entries 8191 and 8192":
        m = (i == CHUNK - 1) | (i == CHUNK)
    elif pattern == "first chunk only":
        m = i < CHUNK
    elif pattern == "all but the first chunk":
        m = i >= CHUNK
    elif pattern == "all but the last entry":
        m = i < n - 1
    return m


def _empty(kind, w, h, rng):
    cx, cy = _cells(w, h)
    if kind == "null":
        return None
    if kind == "zeros":
        return np.zeros(cx * cy, np.uint8)
    if kind == "ones":
        return np.ones(cx * cy, np.uint8)
    if kind == "random":
        return (rng.random_sample(cx * cy) < 0.5).astype(np.uint8)
    ring = np.zeros((cy, cx), np.uint8)                      # the frame's outer ring of cells: the ragged ones enter the pixel count
    ring[0, :] = ring[-1, :] = 1
    ring[:, 0] = ring[:, -1] = 1
    return ring.reshape(-1)


def _reference(w, h, live, stopped, empty):
    cx, _ = _cells(w, h)
    live = live.astype(np.int64)
    keep = live[stopped[live] == 0]
    if empty is None:
        return keep, keep, 0
    outside = empty[keep] != 0
    c = keep[outside]
    pixels = int((np.minimum(8, w - 8 * (c % cx)) * np.minimum(8, h - 8 * (c // cx))).sum())
    return keep, keep[~outside], pixels


def _check(lib, w, h, live, stopped, empty, what):
    """one launch against the reference; returns the device's live list"""
    binding = _binding()
    r, out_live, out_trace, counts = binding.progressive_compact_test(lib, w, h, live, stopped, empty)
    assert r == 1, what
    keep, trace, pixels = _reference(w, h, live, stopped, empty)
    assert (int(counts[0]), int(counts[1]), int(counts[2]) | int(counts[3]) << 32) == (len(keep), len(trace), pixels), (what, counts.tolist())
    assert np.array_equal(out_live[:len(keep)], keep), (what, "live", int((out_live[:len(keep)] != keep).argmax()))
    assert np.array_equal(out_trace[:len(trace)], trace), (what, "trace", int((out_trace[:len(trace)] != trace).argmax()))
    assert (out_live[len(keep):] == binding.COMPACT_SENTINEL).all() and (out_trace[len(trace):] == binding.COMPACT_SENTINEL).all(), (what, "written past the counts")
    return out_live[:len(keep)].copy()


@pytest.mark.parametrize("subset", [False, True], ids=["prefix", "subset"])
@pytest.mark.parametrize("frame", FRAMES, ids=["%dx%d" % f for f in FRAMES])
def test_compaction_against_numpy(gpu_lib, frame, subset):
    """Every list length around the trip boundaries x every stop pattern x every kind of `empty`, and each result fed back in three more times with more cells
    stopped: the life of a session's lists.  `subset`: the list is a sorted random subset of the cells (earlier passes thinned it) instead of a prefix."""
    w, h = frame
    cx, cy = _cells(w, h)
    cells = cx * cy
    rng = np.random.RandomState(cells + subset)
    empties = [(kind, _empty(kind, w, h, rng)) for kind in EMPTY_KINDS]
    launches = 0
    for n in sorted(set(k for k in NUM_LIVE if k <= cells) | {cells}):
        live = np.sort(rng.choice(cells, n, replace=False)).astype(np.uint32) if subset else np.arange(n, dtype=np.uint32)
        for pattern in STOP_PATTERNS:
            # cells that are not listed: stopped long ago (a thinned list) or never looked at (a prefix); the kernel must not care
            stopped = np.full(cells, 1 if subset else 0, np.uint8)
            stopped[live] = _stop_mask(pattern, n, rng)
            for kind, empty in empties:
                what = (frame, "subset" if subset else "prefix", n, pattern, kind)
                kept = _check(gpu_lib, w, h, live, stopped, empty, what)
                launches += 1
                again = stopped.copy()
                for round_ in range(3):
                    again[kept[rng.random_sample(len(kept)) < 0.4]] = 1
                    kept = _check(gpu_lib, w, h, kept, again, empty, what + ("fed back", round_))
                    launches += 1
    print("\ncompaction %dx%d (%d cells, %d trips) %s: %d launches equal the NumPy reference" % (w, h, cells, -(-cells // CHUNK), "subset" if subset else "prefix", launches))


# ---- post-process ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", [pc.SMALL] + [(n,) for n in pc.LARGE] + [(pc.FRAME[0] * pc.FRAME[1],)],
                         ids=["small"] + [str(n) for n in pc.LARGE] + ["%dx%d" % pc.FRAME])
def test_post_process_edge_images_match_oracle(gpu_lib, oracle, pixels):
    """Images uploaded from host pixels (DevicePostProcess's upload path): the white point decided by the first pixel, the last, a lane of the last wave,
    a pixel only the second or the third stride reads; images in which no wave, or exactly one, runs its atomic; the cut, the clamp and powf at their edges."""
    for n in pixels:
        images = pc.check_pixel_count(gpu_lib, oracle, n)
        print("\npost-process %d pixels: %d images equal the oracle bit for bit" % (n, images))
        assert images >= 8


def _render_into(lib, ses, w, h, spp):
    img = lib.Raylib_CreateImage(w, h)
    lib.Raylib_Render(C.byref(ses.settings(w, h, spp)), ses.scene, ses.camera, img)
    return img


def _rgba(lib, img, w, h):
    out = np.full((h, w, 4), -7.0, np.float32)
    lib.RaylibAMD_DumpImageRGBA(img, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def test_post_process_of_device_resident_frames(gpu_lib, oracle, sessions, full_size):
    """A frame that Raylib_Render left on the device, two strides long; the same twice in a row; and the 1920 x 1080 frame (four strides) from host pixels."""
    lib = gpu_lib
    w, h = pc.FRAME
    img = _render_into(lib, sessions["cornell"], w, h, 2)
    raw = _rgba(lib, img, w, h)
    assert pc.lum32(raw[..., :3]).max() > 1.0                # the lamp: the white point is found on the device
    lib.Raylib_PostProcess(img)
    once = oracle.postprocess(raw)
    pc.assert_post_processed(_rgba(lib, img, w, h), once, raw, "rendered %d x %d" % (w, h))
    lib.Raylib_PostProcess(img)                              # (its own output: every luminance at most 1 now)
    pc.assert_post_processed(_rgba(lib, img, w, h), oracle.postprocess(once), raw, "post-processed twice")
    lib.Raylib_DestroyImage(img)
    frame = full_size[1]
    pc.assert_post_processed(pc.post_process(lib, frame), oracle.postprocess(frame), frame, "1920 x 1080")


def test_render_after_post_process(gpu_lib, sessions):
    """Raylib_PostProcess keeps its white point, float bits, in the job counter; the next render must start its heads from zero all the same."""
    lib = gpu_lib
    ses = sessions["cornell"]
    w, h = pc.FRAME
    before = ses.render(w, h, 2)
    img = _render_into(lib, ses, w, h, 2)
    lib.Raylib_PostProcess(img)
    after = ses.render(w, h, 2)
    lib.Raylib_DestroyImage(img)
    assert np.array_equal(bits(after), bits(before))
