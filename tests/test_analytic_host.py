"""Spheres and cubes at their degenerate rays, on the CPU (tests/analytic_cases.py; the device side is tests/test_gpu_analytic_edges.py).

The oracle is the reference: oracle.closest_hit gives the records tests/golden/analytic_edges.npz holds from the reference -- the records of a fixed subsample of
every family and the SHA-256 of the records of every ray -- on every machine, and ref.closest_hit's own records where oracle/_ref was built.  A cube at ray time tau
is asked at ray time 0 of the time-shifted scene (analytic_cases.Scene.at), whose float32 movement is asserted equal.  Each family reaches the edge it is named
for (counts), and the excused set -- rays whose answer depends on the tree -- stays below 0.1 % of every family.

What the fixture catches (each change made to a scratch copy of oracle/oracle.cc, the fixture comparison below run on it; the families whose records change):
    SphereHit  D > 0 -> D >= 0                       tangent_axis, tangent_generic
    SphereHit  t_min < temp -> t_min <= temp         on_surface
    SphereHit  temp < t_max -> temp <= t_max         flt_max
    CubeHit    t_min <= t[7] -> t_min < t[7]         cube_axis, cube_onface, special (and the moved-cube sets)
    CubeHit    std::min / std::max -> fminf / fmaxf  cube_axis, special (and the moved-cube sets)
    CubeHit    the == chain with y before x          cube_corner, cube_axis, special (and the moved-cube sets)
    CubeHit    movement without std::max(0, ...)     regular_many, special"""
import os

import numpy as np
import pytest

import helpers
from helpers import ffi, bits, nextup
import analytic_cases as ac

F = np.float32


@pytest.fixture(scope="module")
def S():
    return ac.scenes()


@pytest.fixture(scope="module")
def fams(S):
    return ac.families(S)


@pytest.fixture(scope="module")
def handles(oracle, S):
    H = {}

    def get(sc):
        if sc.name not in H:
            H[sc.name] = oracle.scene_create(ac.flat_scene(sc, ffi), 1)
        return H[sc.name]
    yield get
    for h in H.values():
        oracle.scene_destroy(h)


def fixture_differences(got, want):
    """Keys of two analytic_cases.recorded() dictionaries that differ"""
    bad = [k for k in want if k not in got or np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes() or np.asarray(got[k]).dtype != np.asarray(want[k]).dtype]
    return bad + [k for k in got if k not in want]


def test_the_oracle_gives_the_references_records(oracle, ref):
    """The fixture always; the reference itself where it was built.  Every family, every tMin, every ray (by hash) -- and the subsample record for record, so
    that a failure names rays."""
    want = dict(np.load(os.path.join(helpers.GOLDEN, "analytic_edges.npz")))
    got = ac.recorded(oracle, ffi)
    stale = [k for k in want if k.endswith("/rays") and str(got[k]) != str(want[k])]
    assert not stale, "the rays of %s are not the bytes the fixture was recorded for (tests/golden/gen_golden.py analytic_edges)" % stale
    bad = fixture_differences(got, want)
    for k in bad:
        if k.endswith("/sub") and k in got:
            i = np.nonzero((got[k].view(np.uint8).reshape(len(got[k]), -1) != want[k].view(np.uint8).reshape(len(want[k]), -1)).any(1))[0]
            print("%s: %d of %d stored records differ, first at subsample %d: oracle %s reference %s" % (k, len(i), len(want[k]), i[0], got[k][i[0]], want[k][i[0]]))
    assert not bad, "the oracle differs from the reference's recorded results: %s" % sorted(set(k.split("/")[0] if not k.startswith("tau") else "/".join(k.split("/")[:2]) for k in bad))
    if ref is None:
        print("oracle/_ref is not built: compared with the fixture only")
        return
    live = ac.recorded(ref, ffi)
    bad = fixture_differences(got, live)
    assert not bad, "the oracle differs from the reference: %s" % bad
    print("the oracle, the reference and the fixture agree on %d arrays" % len(live))


def test_a_shifted_start_time_gives_the_same_movement(oracle, S, handles):
    """ref.closest_hit runs at ray time 0; a cube with timeStartMove' = -fl(tau - timeStartMove) (0 if that is not positive) computes there the float32
    movement the cube computes at tau -- in the arithmetic, and through the oracle's CubeHit on rays at the moved cube's planes."""
    for name in ("cube1m", "many"):
        sc = S[name]
        for tau in ac.TAUS:
            a, b = sc.movement(tau), sc.at(tau).movement(0.0)
            assert a.dtype == F and np.array_equal(bits(a), bits(b)), (name, float(tau), a, b)
            if tau > 0.25 or name == "cube1m" and tau > 0:
                assert (a != 0).any(), (name, float(tau))
    sc = S["cube1m"]
    for tau in ac.TAUS:
        for k, r6 in ac.moved_cube_families(tau).items():
            a = oracle.interval_hits(handles(sc), ac.rays8(r6, 0.0), float(tau))
            b = oracle.interval_hits(handles(sc.at(tau)), ac.rays8(r6, 0.0), 0.0)
            assert a.tobytes() == b.tobytes(), (float(tau), k)
            if k in ("cube_axis", "cube_onface"):
                assert (np.isfinite(a["t"]) & (a["t"] == 0)).sum() > 20, (float(tau), k)      # the planes followed the cube


def test_each_family_reaches_its_edge(oracle, S, fams, handles):
    rec = {k: ac.closest(oracle, handles(S[sn]), r, 0.0) for k, (sn, r) in fams.items()}
    hit = {k: v["hit"] == 1 for k, v in rec.items()}
    count = {}
    p = rec["poles"]
    count["poles: NaN paramU"] = int((hit["poles"] & np.isnan(p["paramU"])).sum())
    count["poles: NaN paramV"] = int((hit["poles"] & np.isnan(p["paramV"])).sum())
    assert count["poles: NaN paramU"] >= 240 and count["poles: NaN paramV"] >= 100, count      # (the 250 rays along the z axis land on a pole: atan(0 / 0))
    for k in ("cube_axis", "cube_onface", "cube_axis_m", "cube_onface_m", "special"):
        z = hit[k] & (bits(rec[k]["t"]) == 0); nz = hit[k] & (bits(rec[k]["t"]) == 0x80000000)
        count[k + ": t == +0"], count[k + ": t == -0"] = int(z.sum()), int(nz.sum())
        assert z.sum() >= 100 and nz.sum() >= 100, (k, count)
    tiny = ac.closest(oracle, handles(S["cube1"]), fams["cube_onface"][1], 1e-4)
    assert not (tiny["hit"] == 1).any()                                                        # with tMin 1e-4 a ray from a face never meets its cube
    for k in ("cube_inside", "cube_inside_m"):
        for tmin in ac.TMINS:
            assert not (ac.closest(oracle, handles(S[fams[k][0]]), fams[k][1], tmin)["hit"] == 1).any(), (k, float(tmin))
    # corner rays: two entry planes at the same t
    r = fams["cube_corner"][1]
    with np.errstate(all="ignore"):
        lo = [np.minimum((ac.MN1[a] - r[:, a]) / r[:, 3 + a], (ac.MX1[a] - r[:, a]) / r[:, 3 + a]) for a in range(3)]
    t1t3 = (lo[0] == lo[1]) & (lo[0] == rec["cube_corner"]["t"])
    count["cube_corner: t1 == t3 == t"] = int(t1t3.sum())
    assert t1t3.sum() >= 512 and hit["cube_corner"].all(), count
    # tangents: a hit and a miss one ulp apart
    a = rec["tangent_axis"]["hit"].reshape(-1, 129)
    count["tangent_axis: groups with a hit and a miss one ulp apart"] = int((a[:, 1:] != a[:, :-1]).any(1).sum())
    a = rec["tangent_generic"]["hit"].reshape(-1, 2)
    count["tangent_generic: pairs with a hit and a miss one ulp apart"] = int((a[:, 0] != a[:, 1]).sum())
    assert count["tangent_axis: groups with a hit and a miss one ulp apart"] >= 48 and count["tangent_generic: pairs with a hit and a miss one ulp apart"] >= 50, count
    # the origin on the surface exactly: a root at t = 0, outside the open interval
    o = rec["on_surface"]
    assert not (o["hit"][-120::20] == 1).any() and (o["hit"][-119::20] == 1).all()      # (straight out: the far root is 0; straight in: the near one is)
    # FLT_MAX: the sphere's open interval ends before it, the cube's closed one holds it
    f = rec["flt_max"]
    assert f["hit"].tolist() == [0, 1, 0] * 6 + [1, 0, 1] and bits(f["t"][18]) == bits(ac.FLT_MAX) and (bits(f["t"][1:18:3]) == bits(ac.FLT_MAX) - 1).all()
    for k in sorted(count):
        print("%-64s %d" % (k, count[k]))


def test_tie_rays_meet_both_primitives_at_one_t(oracle, S, handles):
    for name in ac.TIE_SCENES:
        sc, r6 = S[name], ac.tie_rays(S[name])
        full = oracle.interval_hits(handles(sc), ac.rays8(r6, 0.0), 0.0)
        assert np.isfinite(full["t"]).all()
        up = oracle.interval_hits(handles(sc), ac.rays8(r6, 0.0, nextup(full["t"])), 0.0)
        at = oracle.interval_hits(handles(sc), ac.rays8(r6, 0.0, full["t"]), 0.0)
        below = oracle.interval_hits(handles(sc), ac.rays8(r6, 0.0, helpers.nextdown(full["t"])), 0.0)
        assert (up["count"] == 2).all() and (np.sort(up["prims"][:, :2], 1) == (ac.PRIM_SPHERE, ac.PRIM_CUBE)).all(), name
        assert (at["count"] == 1).all() and (at["prims"][:, 0] == ac.PRIM_CUBE).all() and np.array_equal(bits(at["t"]), bits(full["t"])), name
        assert not np.isfinite(below["t"]).any(), name


def test_the_box_test_restated_in_numpy_is_the_oracles(oracle, S, fams):
    """analytic_cases.box_hit, which gives the excused set its per-ray intervals, against oracle.aabb_hit"""
    for k, (sn, r6) in fams.items():
        for box in S[sn].boxes(0.0):
            for tmin, tmax in ((F(0.0), ac.FLT_MAX), (F(1e-4), F(3.0)), (F(-0.0), F(0.0))):
                want = oracle.aabb_hit(np.tile(box, (len(r6), 1)), r6, tmin, tmax) == 1
                assert np.array_equal(ac.box_hit(box, ac.rays8(r6, tmin, tmax)), want), (k, box, tmin, tmax)


def test_the_excused_set_stays_below_a_thousandth(oracle, S, fams):
    """A ray is excused only if a primitive the float test accepts in its interval fails the box test on its own box (analytic_cases.Excuser).  Counted on
    every set the device is asked: each family at each tMin, its interval re-runs, and the moved cube at each ray time."""
    ex = {sn: ac.Excuser(oracle, S[sn], lambda s: ac.flat_scene(s, ffi)) for sn in set(sn for sn, _ in fams.values())}
    full = {sn: oracle.scene_create(ac.flat_scene(S[sn], ffi), 1) for sn in ex}
    over = []
    for k, (sn, r6) in fams.items():
        n = total = 0
        for tmin in ac.TMINS:
            sets = [("full", ac.rays8(r6, tmin))] + ac.interval_sets(r6, tmin, oracle.interval_hits(full[sn], ac.rays8(r6, tmin), 0.0)["t"])
            for label, r8 in sets:
                e = int(ex[sn](r8).sum())
                n += e; total += len(r8)
                if e > 0.001 * len(r6):
                    over.append((k, float(tmin), label, e, len(r8)))
        print("%-16s excused %d of %d rays asked" % (k, n, total))
    sc = S["cube1m"]
    for tau in ac.TAUS:
        n = 0
        for k, r6 in ac.moved_cube_families(tau).items():
            e = int(ex["cube1m"](ac.rays8(r6, 0.0), tau).sum())
            n += e
            if e > 0.001 * len(r6):
                over.append((k, float(tau), e, len(r6)))
        print("cube1m at ray time %-12r excused %d" % (float(tau), n))
    for e in ex.values():
        e.close()
    for h in full.values():
        oracle.scene_destroy(h)
    assert not over, over
