"""A plain-Python reading of include/rayrs_hip.h LIGHT SAMPLING, independent of the library under test: radiance()'s loop
(lib.rs:521-560) written out with Material::evaluate taking Some(pdf), composed from the oracle's pieces -- OracleScene.intersect
for the loop's query, the second reading of geometry.rs (tests/_geometry_reading.py) for normals and the lights' own
intersections, _oracle.material_evaluate's entry point for the materials the mix does not touch, OracleScene.background, the
oracle's sin and cos and orthonormal basis, and tests/_ao.py's keys and draws.  Every step is one numpy f64 operation, nothing
fused, in the header's order.  Plastic's arm is told from the oracle's answer: its diffuse arm's direction is a Lambertian's
evaluated at the next draw."""
import ctypes as C

import numpy as np

import _ao
import _geometry_reading as G
import _oracle
import _radiance
from rayrs_amd.api import MAT_LAMBERTIAN, MAT_PLASTIC, Material

F = np.float64
PI = F(_ao.PI)
FRAC_1_PI = F(0.318309886183790671537767526745028724)
ONES = (F(1.0), F(1.0), F(1.0))
ZEROS = (F(0.0), F(0.0), F(0.0))


def f3(v):
    return tuple(F(x) for x in v)


def mul(a, b):  # impl Mul for Vector<f64>: componentwise
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def div(a, s):  # Div<f64>, vecmath.rs:690-698: multiplies by the reciprocal
    return G.scale(a, F(1.0) / s)


def uniform(key, draw):
    return F(_ao.uniform(int(key), int(draw)))


def new_tally():
    return dict(light_arm=0, cosine_arm=0, ndl_negative=0, sampled={0: 0, 1: 0}, hit={0: 0, 1: 0}, blocked_by_mesh=0,
                plastic_diffuse=0, plastic_specular=0, by_light={})


class Reading:
    """The scene of the reading: the objects in the scene's numbering (a mesh is its triangles), an oracle scene for the
    loop's query and the background, and the walk it asks the oracle for."""

    def __init__(self, objs, z_near, z_far, heuristic, hdri, osc=None, traversal=0):
        self.prims = G.Prims(objs)
        self.z_near, self.z_far = float(z_near), float(z_far)
        self.osc = osc if osc is not None else _oracle.OracleScene(objs, z_near, z_far, heuristic, hdri)
        self.traversal = traversal
        self._mat = {}

    # ---- Hittable

    def normal(self, k, position):
        kind = int(self.prims.kind[k])
        if kind == 0:
            return G.sphere_normal(f3(self.prims.c[k]), position)
        if kind == 1:
            return f3(G.plane_normal(int(self.prims.axis[k])))
        return f3(self.prims.normal[k])

    def light_sample(self, k, u1, u2):
        """Hittable::sample on the draws u1 then u2: geometry.rs:288-299 (plane), :142-152 (sphere)."""
        if int(self.prims.kind[k]) == 1:
            umin, umax, vmin, vmax, pos = (F(x) for x in self.prims.rect[k])
            u = u1 * (umax - umin) + umin
            v = u2 * (vmax - vmin) + vmin
            return {0: (pos, u, v), 1: (u, pos, v), 2: (u, v, pos)}[int(self.prims.axis[k]) >> 1]
        radius2 = F(self.prims.radius[k]) * F(self.prims.radius[k])  # Sphere::new
        phi = F(2.0) * PI * u2
        r = np.sqrt(u1 * (F(1.0) - u1))
        x = F(_oracle.math_fn(1, [phi])[0]) * F(2.0) * r
        y = F(_oracle.math_fn(0, [phi])[0]) * F(2.0) * r
        z = F(1.0) - F(2.0) * u1
        return G.add(G.scale((x, y, z), np.sqrt(radius2)), f3(self.prims.c[k]))

    def crossing(self, position, l, t, nk, area):
        pt = G.point(position, l, t)
        away = G.sub(position, pt)
        return G.dot(away, away) / (np.abs(G.dot(nk, l)) * area)

    def light_density(self, k, position, l, near_root_only=False):
        """p_k(l), the true solid-angle density of light_sample's directions at `position`.  near_root_only: the reference's
        reading of a sphere (Sphere::intersect's one root), kept to show that it is no density."""
        p = F(0.0)
        if int(self.prims.kind[k]) == 1:
            umin, umax, vmin, vmax, pos = (F(x) for x in self.prims.rect[k])
            axis = int(self.prims.axis[k])
            some, t = G.plane_intersect(axis, umin, umax, vmin, vmax, pos, position, l)
            if some and t > 0.0:
                p = self.crossing(position, l, t, f3(G.plane_normal(axis)), (umax - umin) * (vmax - vmin))
            return p
        c = f3(self.prims.c[k])
        radius2 = F(self.prims.radius[k]) * F(self.prims.radius[k])
        area = (F(4.0) * PI) * radius2
        odiff = G.sub(position, c)
        a = G.dot(l, l)
        b = F(2.0) * G.dot(l, odiff)
        cc = G.dot(odiff, odiff) - radius2
        desc = b * b - F(4.0) * a * cc
        if desc > 0.0:
            sq = np.sqrt(desc)
            t1 = (-b - sq) / (F(2.0) * a)
            t2 = (-b + sq) / (F(2.0) * a)
            if near_root_only:
                t = t2 if t1 < 0.0 else t1
                if not (t1 < 0.0 and t2 < 0.0):
                    p = p + self.crossing(position, l, t, G.sphere_normal(c, G.point(position, l, t)), area)
                return p
            if t1 > 0.0:
                p = p + self.crossing(position, l, t1, G.sphere_normal(c, G.point(position, l, t1)), area)
            if t2 > 0.0:
                p = p + self.crossing(position, l, t2, G.sphere_normal(c, G.point(position, l, t2)), area)
        return p

    # ---- Material::evaluate

    def cosine_direction(self, normal, key, draw):
        """Pdf::Cosine.generate (material.rs:982-993) on the draws `draw` and `draw + 1`."""
        e1, e2 = (f3(e) for e in _oracle.orthonormal_basis(normal))
        u = uniform(key, draw)
        phi = F(2.0) * PI * uniform(key, draw + 1)
        su = np.sqrt(u)
        x = F(_oracle.math_fn(1, [phi])[0]) * su
        y = F(_oracle.math_fn(0, [phi])[0]) * su
        z = np.sqrt(F(1.0) - u)
        return G.add(G.add(G.scale(e1, x), G.scale(e2, y)), G.scale(normal, z))

    def lit_lambertian(self, albedo, position, normal, key, draw, lights, tally=None):
        """LambertianDiffuse::scatter with Some(pdf): (color, l, next draw, index into `lights` of the sampled light or None)."""
        K = len(lights)
        a = uniform(key, draw)
        picked = None
        if a < 0.5:
            b = uniform(key, draw + 1)
            picked = min(int(b * F(K)), K - 1)
            u1, u2 = uniform(key, draw + 2), uniform(key, draw + 3)
            q = self.light_sample(lights[picked], u1, u2)
            l = G.unit(G.sub(q, position))
            draw += 4
        else:
            l = self.cosine_direction(normal, key, draw + 1)
            draw += 3
        ndl = G.dot(normal, l)
        if ndl < 0.0:
            pdf = F(np.inf)
        else:
            p_l = None
            for k in lights:
                p = self.light_density(k, position, l)
                p_l = p if p_l is None else p_l + p
            p_l = p_l / F(K)
            pdf = F(0.5) * p_l + F(0.5) * (ndl * FRAC_1_PI)
        color = div(G.scale(G.scale(albedo, FRAC_1_PI), ndl), pdf)
        if tally is not None:
            tally["light_arm" if picked is not None else "cosine_arm"] += 1
            tally["ndl_negative"] += int(ndl < 0.0)
            if picked is not None:
                tally["sampled"][int(self.prims.kind[lights[picked]])] += 1
                tally["by_light"][picked] = tally["by_light"].get(picked, 0) + 1   # (by its place in the list)
        return color, l, draw, picked

    def oracle_evaluate(self, mat, normal, view, key, draw):
        """Material::evaluate(.., None) by the oracle, from draw `draw`: (scattered, color, l, next draw)."""
        m = self._mat.get(mat)
        if m is None:
            m = self._mat[mat] = (_oracle.mat_desc(mat),)
        c, d = (C.c_double * 3)(), (C.c_double * 3)()
        dr = C.c_uint32(int(draw))
        r = _oracle.lib().orc_material_evaluate(C.byref(m[0]), _oracle.d3((0, 0, 0)), _oracle.d3(normal), _oracle.d3(view), int(key),
                                                C.byref(dr), c, d)
        assert r >= 0
        return bool(r), f3(c), f3(d), dr.value

    def evaluate(self, k, position, normal, view, key, draw, lights, tally=None):
        """(scattered, color, l, next draw, sampled light or None)."""
        mat = self.prims.list[k].mat
        if len(lights) and mat.kind == MAT_LAMBERTIAN:
            return (True,) + self.lit_lambertian(f3(mat.color), position, normal, key, draw, lights, tally)
        ans = self.oracle_evaluate(mat, normal, view, key, draw)
        if len(lights) and mat.kind == MAT_PLASTIC:
            diffuse = self.oracle_evaluate(Material.LambertianDiffuse(mat.color), normal, view, key, draw + 1)
            if ans[0] and ans[3] == draw + 3 and np.array(ans[2]).tobytes() == np.array(diffuse[2]).tobytes():
                if tally is not None:
                    tally["plastic_diffuse"] += 1
                return (True,) + self.lit_lambertian(f3(mat.color), position, normal, key, draw + 1, lights, tally)
            if tally is not None:
                tally["plastic_specular"] += 1
        return ans + (None,)

    # ---- radiance(), lib.rs:521-560

    def path(self, o, d, max_bounces, key, draw, lights, tally=None, aimed=None):
        """(L (3,) f64, Bvh::intersect calls, next draw).  aimed: the light (object index) the ray's direction was sampled
        from, for the tally."""
        o, d = f3(o), f3(d)
        thr, light = ONES, ZEROS
        queries = 0
        with np.errstate(all="ignore"):
            for _ in range(int(max_bounces)):
                obj, t = self.osc.intersect(o, d, self.z_near, self.z_far, self.traversal)
                queries += 1
                if tally is not None and aimed is not None:
                    if obj == aimed:
                        tally["hit"][int(self.prims.kind[aimed])] += 1
                    elif obj >= 0 and int(self.prims.kind[obj]) == 2:
                        tally["blocked_by_mesh"] += 1
                if obj < 0:
                    bg = f3(self.osc.background(np.array([d]))[0])
                    return np.array(G.add(light, mul(thr, bg))), queries, draw
                position = G.point(o, d, F(t))
                normal = self.normal(obj, position)
                view = G.unit(G.scale(d, F(-1.0)))
                scattered, color, l, draw, picked = self.evaluate(obj, position, normal, view, key, draw, lights, tally)
                if not scattered:
                    return np.array(light), queries, draw
                aimed = None if picked is None else lights[picked]
                e = self.prims.list[obj].emission
                emit = G.scale(f3(e.color), F(e.strength)) if e.emissive else ZEROS
                light = G.add(light, mul(thr, emit))
                thr = mul(thr, color)
                p = np.fmax(np.fmax(thr[0], thr[1]), thr[2])
                u = uniform(key, draw)
                draw += 1
                if u > p:
                    return np.array(light), queries, draw
                thr = (thr[0] / p, thr[1] / p, thr[2] / p)  # DivAssign, vecmath.rs:708-714
                o, d = position, l
        return np.array(light), queries, draw


def _collect(n, samples, one):
    values, queries = np.zeros((n, samples, 3)), np.zeros((n, samples), dtype=np.int64)
    for i in range(n):
        for s in range(samples):
            values[i, s], queries[i, s] = one(i, s)
    values.setflags(write=False), queries.setflags(write=False)
    return values, queries


def radiance_paths(R, origins, directions, samples, max_bounces, seed, lights, index_base=0, tally=None):
    """RADIANCE, LIT: (values (n, S, 3), queries (n, S)) of a call; the sums are _radiance.answers'."""
    lights = [int(k) for k in lights]

    def one(i, s):
        return R.path(origins[i], directions[i], max_bounces, _ao.path_key(int(seed), int(index_base) + i, s), 0, lights, tally)[:2]
    return _collect(len(origins), samples, one)


def irradiance_paths(R, points, normals, samples, bias, max_bounces, seed, lights, index_base=0, tally=None):
    """IRRADIANCE, LIT.  With lights the first direction is the operation's at (p + n * bias, n), albedo (1, 1, 1), and the
    path's value is multiplied by its colour; without, IRRADIANCE's ray on draws 0 and 1 and no multiplication."""
    lights = [int(k) for k in lights]

    def one(i, s):
        key = _ao.path_key(int(seed), int(index_base) + i, s)
        p, n = f3(points[i]), f3(normals[i])
        with np.errstate(all="ignore"):
            position = G.add(p, G.scale(n, F(bias)))
            if not lights:
                value, q, _ = R.path(position, R.cosine_direction(n, key, 0), max_bounces, key, 2, lights, tally)
                return value, q
            color, l, draw, picked = R.lit_lambertian(ONES, position, n, key, 0, lights, tally)
            if max_bounces == 0:
                return np.zeros(3), 0
            value, q, _ = R.path(position, l, max_bounces, key, draw, lights, tally, None if picked is None else lights[picked])
            return np.array(mul(color, f3(value))), q
    return _collect(len(points), samples, one)


def image_paths(R, ocam, samples, max_bounces, seed, lights, tally=None, pixels=None):
    """The image form: pixel (row, col) is ray row * W + col, the primary ray sample_ray's on draws 0 and 1.  pixels: the
    pixel indices to read (in that order) where the whole image is too many."""
    lights = [int(k) for k in lights]
    h, w = ocam.y_pixels(), ocam.x_pixels()
    pixels = range(h * w) if pixels is None else [int(i) for i in pixels]

    def one(j, s):
        i = pixels[j]
        row, col = divmod(i, w)
        key = _ao.path_key(int(seed), i, s)
        o, d, draw = ocam.primary_ray(h - row, w - col, key)
        return R.path(o, d, max_bounces, key, draw, lights, tally)[:2]
    return _collect(len(pixels), samples, one)


answers = _radiance.answers


# ---- the small lit room of the tests (the local-pool-sized route)

def lit_room():
    """(camera args, objects, heuristic, names): a Lambertian floor, a Plastic sphere, a glass sphere, a small sphere lamp, a
    rectangle lamp facing down, and a dark sphere that a light list may name as well.  names maps each to its object index.
    The rectangle lamp is a mirror that emits: a LAMBERTIAN rectangle in the list that a path scatters on can draw itself, l
    then lies in its plane, ndl = 0 and pdf = 0, and the colour is 0 * inf -- NaN by the header's "whatever IEEE gives" (the
    mesh3_light tests meet it); a room for the statistics keeps clear of it."""
    from rayrs_amd.api import Axis, BvhHeuristic, Emission, Object
    white = Material.LambertianDiffuse((0.8, 0.8, 0.8))
    objs = [
        Object.plane(Axis.Y, -4.0, 4.0, -4.0, 4.0, 0.0, Material.LambertianDiffuse((0.7, 0.7, 0.6)), Emission.Dark()),
        Object.sphere(0.8, (-1.5, 0.8, 0.0), Material.Plastic((0.7, 0.2, 0.2), (1.0, 1.0, 1.0), 0.2, 1.5), Emission.Dark()),
        Object.sphere(0.6, (1.2, 0.6, 0.8), Material.Glass((1.0, 1.0, 1.0), 1.5), Emission.Dark()),
        Object.sphere(0.25, (0.0, 2.5, 0.0), white, Emission.new(20.0, (1.0, 0.9, 0.8))),
        Object.plane(Axis.YRev, 1.0, 2.0, -2.0, -1.0, 3.5, Material.Reflect((0.8, 0.8, 0.8)), Emission.new(15.0, (0.8, 0.9, 1.0))),
        Object.sphere(0.4, (-0.5, 0.4, 1.6), Material.LambertianDiffuse((0.3, 0.5, 0.3)), Emission.Dark()),
    ]
    names = dict(floor=0, plastic=1, glass=2, sphere_lamp=3, rect_lamp=4, dark_sphere=5)
    cam = ((0.0, 2.2, 7.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 50.0, 32.0 / 254.0, 24.0 / 254.0, 100)
    return cam, objs, BvhHeuristic.Sah(1000), names


# ---- the lamp box: a rectangle lamp on every axis and K = 8

LAMP_BOX_RECTS = (("X", 0.5, 1.5, -2.0, 0.5, -3.5), ("XRev", 1.0, 3.0, 0.0, 1.0, 3.5), ("Y", 2.0, 3.0, -3.0, -1.5, 0.25),
                  ("YRev", -2.0, -1.0, 1.0, 3.0, 3.5), ("Z", -3.0, -0.5, 0.5, 1.25, -3.5), ("ZRev", 0.5, 1.0, 1.5, 3.5, 3.0))


def lamp_box():
    """(camera args, objects, heuristic, names): lit_room()'s floor, its three spheres and its camera, six rectangle lamps -- one
    on each of Axis.X, XRev, Y, YRev, Z, ZRev, (umin, umax, vmin, vmax, pos) as LAMP_BOX_RECTS has them: the u and v ranges
    of every one unequal in length and not symmetric about 0, so a u taken for a v, or one axis's point for another's, is
    another point -- and two sphere lamps.  names["lights"] is the eight lamps, K = RAYRS_MAX_LIGHTS; names["rect"][axis name]
    one rectangle.  Every rectangle is a mirror that emits, as lit_room's is: none is Lambertian, so the room makes no NaN of its
    own (lit_room's docstring), and none is NoReflect, whose emission no path collects (lib.rs:550) -- an aimed ray that arrives
    would then be worth the same 0 at every lamp.  The first sphere lamp is Lambertian, as lit_room's is."""
    from rayrs_amd.api import Axis, BvhHeuristic, Emission, Object
    cam, room, heur, _ = lit_room()
    objs = [room[0], room[1], room[2], room[5]]
    names = dict(floor=0, plastic=1, glass=2, dark_sphere=3, rect={}, sphere_lamps=[])
    tints = ((1.0, 0.9, 0.8), (0.8, 0.9, 1.0), (0.9, 1.0, 0.8))
    for i, (axis, umin, umax, vmin, vmax, pos) in enumerate(LAMP_BOX_RECTS):
        mat = Material.Reflect((0.8, 0.8, 0.8))
        names["rect"][axis] = len(objs)
        objs.append(Object.plane(getattr(Axis, axis), umin, umax, vmin, vmax, pos, mat, Emission.new(10.0 + 2.0 * i, tints[i % 3])))
    names["sphere_lamps"] = [len(objs), len(objs) + 1]
    objs.append(Object.sphere(0.25, (0.0, 2.5, 0.0), Material.LambertianDiffuse((0.8, 0.8, 0.8)), Emission.new(20.0, (1.0, 0.9, 0.8))))
    objs.append(Object.sphere(0.15, (2.5, 1.0, 2.0), Material.Reflect((0.8, 0.8, 0.8)), Emission.new(30.0, (0.9, 0.8, 1.0))))
    names["lights"] = tuple(names["rect"][a[0]] for a in LAMP_BOX_RECTS) + tuple(names["sphere_lamps"])
    # Sah(4): twelve objects in at most four leaf groups, one record of the gate tree -- the local-pool route's size, as
    # lit_room() is (Sah(1000) makes five groups of these and the room would stream)
    return cam, objs, BvhHeuristic.Sah(4), names
