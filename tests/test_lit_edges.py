"""Light sampling on every axis and at K = 8, without a GPU: the plain-Python reading (tests/_lit.py), which is all the lit
kernels are compared with, is held to geometry.rs on a rectangle of each axis -- its samples to literals, its densities to solid
angles computed without it -- and the inputs of tests/test_gpu_lit_edges.py are shown, from the reading alone, to reach what
that file is there to compare."""
import numpy as np
import pytest

import _lit
import test_gpu_lit_edges as E
from test_lit import mean_inverse_density

F = np.float64
RECTS = {r[0]: r[1:] for r in _lit.LAMP_BOX_RECTS}


def test_the_lamp_box_is_what_the_gpu_tests_take_it_for():
    """Twelve objects: the local-pool route's size (one record of the gate tree, at most 16 primitives and surfaces:
    include/rayrs_hip.h rayrs_tuning.local_pool) and not compact; a lamp on each of the six axes, unequal and off-centre ranges,
    none of the rectangles Lambertian; two sphere lamps, the first Lambertian; the list is the eight emitters."""
    import rayrs_amd
    from rayrs_amd.api import MAT_LAMBERTIAN, Axis
    i = E.inputs("box")
    cam, objs, heur, names = _lit.lamp_box()
    info = i.host_info
    assert info["gate_n_wide"] == 1 and info["n_prims"] == info["n_surfaces"] == 12 and info["compact"] == 0
    assert i.lists["all"] == tuple(rayrs_amd.emitters(objs)) and len(i.lists["all"]) == 8
    prims = i.reading.prims
    assert [int(prims.axis[names["rect"][a]]) for a in E.AXES] == [int(getattr(Axis, a)) for a in E.AXES] == list(range(6))
    for a in E.AXES:
        k = names["rect"][a]
        umin, umax, vmin, vmax, pos = RECTS[a]
        assert tuple(prims.rect[k]) == RECTS[a] and objs[k].mat.kind != MAT_LAMBERTIAN and objs[k].emission.emissive
        assert umax - umin != vmax - vmin and umin + umax != 0.0 and vmin + vmax != 0.0 and (umin, umax) != (vmin, vmax)
    s0, s1 = names["sphere_lamps"]
    assert objs[s0].mat.kind == MAT_LAMBERTIAN and objs[s1].mat.kind != MAT_LAMBERTIAN
    assert [int(prims.kind[k]) for k in i.lists["all"]] == [1] * 6 + [0] * 2
    assert [objs[names[n]].mat.kind for n in ("floor", "dark_sphere")] == [MAT_LAMBERTIAN] * 2


# ---- the reading reads geometry.rs

def test_a_rectangles_sample_is_geometry_rs_on_every_axis():
    """Plane::sample, geometry.rs:288-299: u from the first draw and the u range, v from the second and the v range, and
    Vec3::new(pos, u, v) | (u, pos, v) | (u, v, pos) for X and XRev | Y and YRev | Z and ZRev.  The draws 0.25 and 0.75; every
    value below is exact in binary."""
    i = E.inputs("box")
    want = {"X": (-3.5, 0.75, -0.125), "XRev": (3.5, 1.5, 0.75), "Y": (2.25, 0.25, -1.875), "YRev": (-1.75, 3.5, 2.5),
            "Z": (-2.375, 1.0625, -3.5), "ZRev": (0.625, 3.0, 3.0)}
    for a in E.AXES:
        got = i.reading.light_sample(i.lists[a][0], F(0.25), F(0.75))
        assert tuple(float(x) for x in got) == want[a], (a, got, want[a])
    # the corners: u1 = 0, u2 = 1 is (umin, vmax)
    corners = {"X": (-3.5, 0.5, 0.5), "XRev": (3.5, 1.0, 1.0), "Y": (2.0, 0.25, -1.5), "YRev": (-2.0, 3.5, 3.0), "Z": (-3.0, 1.25, -3.5),
               "ZRev": (0.5, 3.5, 3.0)}
    for a in E.AXES:
        got = i.reading.light_sample(i.lists[a][0], F(0.0), F(1.0))
        assert tuple(float(x) for x in got) == corners[a], (a, got, corners[a])


# ---- the densities are densities, on every axis

def solid_angle(axis, umin, umax, vmin, vmax, pos, position, m=400000, seed=4):
    """(omega, its standard error) of the rectangle seen from `position`: the share of m uniform directions whose line meets the
    plane in front (t > 0) within the ranges, times 4 pi.  Plain numpy slab arithmetic; u is the lower of the two other axes, v
    the higher (geometry.rs:294-298)."""
    rng = np.random.default_rng(seed)
    z = 1.0 - 2.0 * rng.random(m)
    phi = 2.0 * np.pi * rng.random(m)
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s * np.cos(phi), z, s * np.sin(phi)], axis=1)
    a = {"X": 0, "Y": 1, "Z": 2}[axis[0]]
    ua, va = [x for x in range(3) if x != a]
    with np.errstate(all="ignore"):
        t = (pos - position[a]) / d[:, a]
        u, v = position[ua] + t * d[:, ua], position[va] + t * d[:, va]
    hit = (t > 0.0) & (u >= umin) & (u <= umax) & (v >= vmin) & (v <= vmax)
    share = hit.mean()
    return 4.0 * np.pi * share, 4.0 * np.pi * np.sqrt(share * (1.0 - share) / m), int(hit.sum())


@pytest.mark.parametrize("axis", E.AXES)
def test_the_densities_are_densities_on_every_axis(axis):
    """E[1 / p_k(l)] over 4000 generated l is the rectangle's solid angle, within 4 combined standard errors -- and at least 8
    away from the solid angle of the rectangle with its u and v ranges exchanged, so the check tells the two apart."""
    i = E.inputs("box")
    position = (0.3, 1.1, -0.4)
    umin, umax, vmin, vmax, pos = RECTS[axis]
    assert all(position[{"X": 0, "Y": 1, "Z": 2}[a[0]]] != r[4] for a, r in RECTS.items())   # off every lamp's plane
    mean, se = mean_inverse_density(i.reading, i.lists[axis][0], _lit.f3(position), 4000, 30 + E.AXES.index(axis))
    omega, omega_se, hits = solid_angle(axis, umin, umax, vmin, vmax, pos, position)
    other, other_se, other_hits = solid_angle(axis, vmin, vmax, umin, umax, pos, position)
    print(axis, "solid angle", omega, "+-", omega_se, "mean 1/p", mean, "+-", se, "| ranges exchanged", other, "+-", other_se,
          "away by", abs(mean - other) / np.hypot(se, other_se), "combined standard errors")
    assert hits >= 100 and other_hits >= 100   # (enough for the share's standard error to mean something)
    assert abs(mean - omega) <= 4.0 * np.hypot(se, omega_se)
    assert abs(mean - other) >= 8.0 * np.hypot(se, other_se)


# ---- non-vacuity of tests/test_gpu_lit_edges.py, from the reading alone, on the default walk

def test_the_gpu_comparisons_are_not_vacuous():
    i = E.inputs("box")
    lights = i.lists["all"]
    for what in E.FORMS:
        values, _ = E.expected("box", "all", what)
        assert np.isfinite(values).all(), what   # (the room makes no NaN of its own)
    t = i.tally
    by_light = [t["by_light"].get(k, 0) for k in range(len(lights))]
    print("lamp box tally", t, "sampled by place in the list", by_light)
    assert len(lights) == 8 and min(by_light) >= 50
    assert t["ndl_negative"] >= 50 and t["plastic_diffuse"] >= 20 and t["plastic_specular"] >= 20
    assert t["light_arm"] >= 500 and t["cosine_arm"] >= 500
    # aimed rays that arrive, over the radiance and irradiance cases together (the image's primary rays are the radiance's own)
    arrive = _lit.new_tally()
    _lit.radiance_paths(i.reading, i.o, i.d, E.S, 50, E.SEED, lights, tally=arrive)
    _lit.irradiance_paths(i.reading, i.p, i.nrm, E.S, E.BIAS, 50, E.SEED, lights, tally=arrive)
    print("aimed rays that arrive at their rectangle", arrive["hit"][1], "of", arrive["sampled"][1], "at their sphere", arrive["hit"][0],
          "of", arrive["sampled"][0])
    assert arrive["hit"][1] >= 20 and arrive["hit"][0] >= 10
    unlit, _ = _lit.radiance_paths(i.reading, i.o, i.d, E.S, 50, E.SEED, [])
    q50 = E.expected("box", "all", "radiance")
    print("rays the lights change", E.rays_differing(q50, (unlit, q50[1])))
    # the budget
    v3, q3 = E.expected("box", "all", "radiance", False, 3)
    at_budget = int((q3 == 3).sum())
    differ = int((E.bits(v3) != E.bits(q50[0])).any(axis=2).sum())
    print("max_bounces = 3: paths of exactly 3 queries", at_budget, "paths whose value differs from 50 bounces", differ)
    assert at_budget >= 200 and differ >= 50
    for what in E.FORMS:
        assert (E.expected("box", "all", what, False, 1)[1] == 1).all(), what
    # the K = 1 lists tell the axes apart: any two of them give other answers at half of the 64 points and more
    ones = [E.expected("box", a, "irradiance") for a in E.AXES]
    apart = [[E.rays_differing(ones[a], ones[b]) for b in range(6)] for a in range(6)]
    print("points whose answers differ between the lists of one rectangle", apart)
    assert all(apart[a][b] >= 32 for a in range(6) for b in range(6) if a != b)


def test_the_points_and_normals_as_given_touch_what_they_are_for():
    p, n = E.edge_points()
    length = np.linalg.norm(n, axis=1)
    assert np.allclose(length[:64], 1.0) and (np.abs(n[:64]) > 0.05).all(axis=1).sum() >= 32      # oblique
    assert np.allclose(length[64::2], 0.5) and np.allclose(length[65::2], 3.0)
    cp, cn, touched = E.corrupted_points()
    print("corrupted (point, normal) pairs", int(touched.sum()), "of", len(cp), "non-finite", int((~np.isfinite(cp) | ~np.isfinite(cn)).any(axis=1).sum()))
    assert touched.sum() >= 100 and len(cp) % 64 != 0
