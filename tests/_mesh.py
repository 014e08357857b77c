"""A plain-Python reading of include/rayrs_hip.h MESH LIGHTS, independent of the library under test: the group's table,
mesh_sample, p_tri and DIRECT LIGHTING's / SKY SAMPLING's turn with the group as light number K.  It builds on tests/_sky.py's and
tests/_direct.py's Reading -- the lamps' samples and densities, the sky's table, the unlit Material::evaluate with Plastic's arm
told, the oracle's query and background.  Every step is one numpy f64 operation, nothing fused, in the header's order."""
import numpy as np

import _ao
import _geometry_reading as G
import _lit
import _sky
from _lit import F, FRAC_1_PI, ONES, ZEROS, div, f3, mul, uniform

INF = F(np.inf)


class Table:
    """The table of the listed triangles `tris` (object indices) of a G.Prims: per entry the vertices, n_j and A_j by
    Triangle::new's arithmetic (geometry.rs:341-353), the inclusive prefix P in list order, and T."""

    def __init__(self, prims, tris):
        self.tris = [int(t) for t in tris]
        self.p, self.n, self.A, self.P = [], [], [], []
        with np.errstate(all="ignore"):
            for t in self.tris:
                assert int(prims.kind[t]) == 2, t
                p1, p2, p3 = (f3(v) for v in prims.p[t])
                nrm = G.cross(G.sub(p2, p1), G.sub(p3, p1))
                self.p.append((p1, p2, p3))
                self.n.append(G.unit(nrm))
                self.A.append(G.mag(nrm) / F(2.0))
                self.P.append(self.A[-1] if not self.P else self.P[-1] + self.A[-1])
        self.T = self.P[-1] if self.P else F(0.0)

    def __len__(self):
        return len(self.tris)

    def sample(self, u1, u2):
        """mesh_sample(u1, u2): (j, q)."""
        with np.errstate(all="ignore"):
            ty = u1 * self.T
            j = _sky.Table.first_above(self.P, ty)
            below = self.P[j - 1] if j > 0 else F(0.0)
            r = (ty - below) / self.A[j]
            su = np.sqrt(r)
            b0 = F(1.0) - su
            b1 = su * (F(1.0) - u2)
            b2 = su * u2
            p1, p2, p3 = self.p[j]
            return j, G.add(G.add(G.scale(p1, b0), G.scale(p2, b1)), G.scale(p3, b2))

    def aim(self, position, j, q):
        """(l_s, p_tri) of a shadow sample from `position` to the point q of entry j."""
        with np.errstate(all="ignore"):
            l_s = G.unit(G.sub(q, position))
            away = G.sub(position, q)
            return l_s, G.dot(away, away) / (np.abs(G.dot(self.n[j], l_s)) * self.T)


def new_tally():
    """Shadow samples by what was drawn (the group, a lamp, the sky) and what became of them; listed triangles, unlisted emissive
    triangles and the sky met by a path's own ray, by their weight."""
    keys = ("group_credited", "group_blocked_unlisted", "group_blocked_listed", "group_blocked_lamp", "group_missed", "group_skipped_ndl",
            "group_skipped_den", "lamp_credited", "lamp_blocked", "lamp_met_listed", "lamp_missed", "lamp_skipped", "sky_credited",
            "sky_blocked", "sky_met_lamp", "sky_met_listed", "sky_skipped", "met_listed_weighted", "met_listed_unweighted",
            "met_unlisted_emissive_triangle", "miss_weighted", "miss_unweighted", "plastic_diffuse", "plastic_specular", "taken")
    return {k: 0 for k in keys}


class Reading(_sky.Reading):
    """_sky.Reading with a group: `tris` are the listed triangles' object indices, in list order (at least one)."""

    def __init__(self, objs, z_near, z_far, heuristic, hdri, tris, osc=None, traversal=0):
        super().__init__(objs, z_near, z_far, heuristic, hdri, osc=osc, traversal=traversal)
        self.mesh = Table(self.prims, tris)
        assert len(self.mesh) >= 1
        self.listed = {t: j for j, t in enumerate(self.mesh.tris)}

    def rest_density(self, lights, sky, position, l):
        """p_R(position, l): the lamps in list order, then (sky) p_env(l) last, over (double)M; 0.0 without either."""
        if not lights and not sky:
            return F(0.0)
        p_r = None
        for k in lights:
            p = self.light_density(k, position, l)
            p_r = p if p_r is None else p_r + p
        if sky:
            p_e = self.sky.density(l)
            p_r = p_e if p_r is None else p_r + p_e
        return p_r / F(len(lights) + 1 + int(sky))

    def mesh_bounce(self, albedo, thr, position, normal, l, key, draw, lights, member, sky, tally=None):
        """The diffuse branch of the turn: (what the shadow sample adds to light or None, its queries (0 or 1), w_next, pc, next
        draw)."""
        K = len(lights)
        M = K + 1 + int(sky)
        b, u1, u2 = uniform(key, draw), uniform(key, draw + 1), uniform(key, draw + 2)
        draw += 3
        k = min(int(b * F(M)), M - 1)
        j = None
        if k == K:
            drawn = "group"
            j, q = self.mesh.sample(u1, u2)
            l_s, p_tri = self.mesh.aim(position, j, q)
        elif k == K + 1:
            drawn = "sky"
            l_s = self.sky.sample(u1, u2)
        else:
            drawn = "lamp"
            l_s = G.unit(G.sub(self.light_sample(lights[k], u1, u2), position))
        ndl_s = G.dot(normal, l_s)
        added, queries, what = None, 0, None
        if ndl_s > 0.0:
            p_light = p_tri / F(M) if j is not None else self.rest_density(lights, sky, position, l_s)
            den = p_light + ndl_s * FRAC_1_PI
            if den < INF:
                c = div(G.scale(G.scale(albedo, FRAC_1_PI), ndl_s), den)
                obj, _ = self.osc.intersect(position, l_s, self.z_near, self.z_far, self.traversal)
                queries = 1
                if j is not None:
                    if obj == self.mesh.tris[j]:
                        added = mul(mul(thr, c), self.emit(obj))
                        what = "group_credited"
                    else:
                        what = ("group_missed" if obj < 0 else "group_blocked_listed" if obj in self.listed else
                                "group_blocked_lamp" if obj in member else "group_blocked_unlisted")
                elif obj >= 0 and obj in member:
                    added = mul(mul(thr, c), self.emit(obj))
                    what = "sky_met_lamp" if drawn == "sky" else "lamp_credited"
                elif obj < 0 and sky:
                    added = mul(mul(thr, c), self.background(l_s))
                    what = "sky_credited" if drawn == "sky" else "lamp_missed"
                elif obj >= 0 and obj in self.listed:
                    what = drawn + "_met_listed"
                else:
                    what = "lamp_missed" if obj < 0 else drawn + "_blocked"
                if tally is not None:
                    tally["taken"] += 1
            else:
                what = "group_skipped_den" if j is not None else drawn + "_skipped"
        else:
            what = "group_skipped_ndl" if j is not None else drawn + "_skipped"
        if tally is not None:
            tally[what] += 1
        ndl = G.dot(normal, l)
        pc = ndl * FRAC_1_PI
        pr = self.rest_density(lights, sky, position, l)
        w_next = pc / (pc + pr) if pr > 0.0 else F(1.0)
        return added, queries, w_next, pc, draw

    def path(self, o, d, max_bounces, key, draw, lights, sky, tally=None, w=F(1.0), pc=None):
        """(L (3,) f64, Bvh::intersect calls -- the shadow queries among them --, next draw).  w: the weight of a listed lamp, or
        of the sky, met by the first ray; pc: the cosine arm's density of the first ray where it leaves a diffuse bounce
        (IRRADIANCE's virtual one), else None."""
        o, d = f3(o), f3(d)
        member = set(lights)
        M = F(len(lights) + 1 + int(sky))
        thr, light = ONES, ZEROS
        queries = 0
        with np.errstate(all="ignore"):
            for _ in range(int(max_bounces)):
                obj, t = self.osc.intersect(o, d, self.z_near, self.z_far, self.traversal)
                queries += 1
                if obj < 0:
                    if not sky:
                        return np.array(G.add(light, mul(thr, self.background(d)))), queries, draw
                    if tally is not None:
                        tally["miss_weighted" if w < 1.0 else "miss_unweighted"] += 1
                    return np.array(G.add(light, mul(thr, G.scale(self.background(d), w)))), queries, draw
                position = G.point(o, d, F(t))
                normal = self.normal(obj, position)
                view = G.unit(G.scale(d, F(-1.0)))
                scattered, color, l, draw, diffuse = self.evaluate_unlit(obj, normal, view, key, draw, tally)
                if not scattered:
                    return np.array(light), queries, draw
                e = self.emit(obj)
                if obj in self.listed:
                    wt = F(1.0)
                    if pc is not None:
                        away = G.sub(o, position)
                        p = G.dot(away, away) / (np.abs(G.dot(normal, d)) * self.mesh.T)
                        wt = pc / (pc + p / M) if p > 0.0 else F(1.0)
                        e = G.scale(e, wt)
                    if tally is not None:
                        tally["met_listed_weighted" if wt < 1.0 else "met_listed_unweighted"] += 1
                elif obj in member:
                    e = G.scale(e, w)
                elif tally is not None and int(self.prims.kind[obj]) == 2 and self.prims.list[obj].emission.emissive:
                    tally["met_unlisted_emissive_triangle"] += 1
                light = G.add(light, mul(thr, e))
                w_next, pc_next = F(1.0), None
                if diffuse:
                    albedo = f3(self.prims.list[obj].mat.color)
                    added, q, w_next, pc_next, draw = self.mesh_bounce(albedo, thr, position, normal, l, key, draw, lights, member, sky, tally)
                    queries += q
                    if added is not None:
                        light = G.add(light, added)
                thr = mul(thr, color)
                p = np.fmax(np.fmax(thr[0], thr[1]), thr[2])
                u = uniform(key, draw)
                draw += 1
                if u > p:
                    return np.array(light), queries, draw
                thr = (thr[0] / p, thr[1] / p, thr[2] / p)  # DivAssign, vecmath.rs:708-714
                w, pc = w_next, pc_next
                o, d = position, l
        return np.array(light), queries, draw


def split_sky(lights):
    """A light list as the interface takes it -> (the lamps, whether SKY is among them)."""
    lights = [int(k) for k in lights]
    return [k for k in lights if k != 0xFFFFFFFF], any(k == 0xFFFFFFFF for k in lights)


def radiance_paths(R, origins, directions, samples, max_bounces, seed, lights, index_base=0, tally=None):
    """RADIANCE with the group: (values (n, S, 3), queries (n, S)) of a call; `lights` are the lamps and, maybe, SKY."""
    lamps, sky = split_sky(lights)

    def one(i, s):
        return R.path(origins[i], directions[i], max_bounces, _ao.path_key(int(seed), int(index_base) + i, s), 0, lamps, sky, tally)[:2]
    return _lit._collect(len(origins), samples, one)


def irradiance_paths(R, points, normals, samples, bias, max_bounces, seed, lights, index_base=0, tally=None):
    """IRRADIANCE with the group: the virtual bounce -- the cosine ray on draws 0 and 1, b, u1, u2 on draws 2 to 4, no roulette,
    the path from draw 5."""
    lamps, sky = split_sky(lights)
    member = set(lamps)

    def one(i, s):
        key = _ao.path_key(int(seed), int(index_base) + i, s)
        p, n = f3(points[i]), f3(normals[i])
        with np.errstate(all="ignore"):
            position = G.add(p, G.scale(n, F(bias)))
            l = R.cosine_direction(n, key, 0)
            if max_bounces == 0:
                return np.zeros(3), 0
            added, q, w, pc, draw = R.mesh_bounce(ONES, ONES, position, n, l, key, 2, lamps, member, sky, tally)
            value, q_path, _ = R.path(position, l, max_bounces, key, draw, lamps, sky, tally, w, pc)
            credit = ZEROS if added is None else added   # (the virtual bounce's credit: +0 where nothing was credited)
            return np.array(G.add(credit, f3(value))), q + q_path
    return _lit._collect(len(points), samples, one)


def image_paths(R, ocam, samples, max_bounces, seed, lights, tally=None, pixels=None):
    """The image form: pixel (row, col) is ray row * W + col, the primary ray sample_ray's on draws 0 and 1."""
    lamps, sky = split_sky(lights)
    h, w = ocam.y_pixels(), ocam.x_pixels()
    pixels = range(h * w) if pixels is None else [int(i) for i in pixels]

    def one(j, s):
        i = pixels[j]
        row, col = divmod(i, w)
        key = _ao.path_key(int(seed), i, s)
        o, d, draw = ocam.primary_ray(h - row, w - col, key)
        return R.path(o, d, max_bounces, key, draw, lamps, sky, tally)[:2]
    return _lit._collect(len(pixels), samples, one)


answers = _lit.answers


def mesh_room(small=False):
    """(camera args, objects, heuristic, names): tests/_lit.py's lit room plus an emissive two-triangle quad (a tilted panel over
    the floor), a second, smaller quad directly behind it as seen from the floor (a listed triangle behind a listed one), a small
    emissive octahedron above the sphere lamp (a listed triangle behind a lamp as seen from the floor), and an emissive triangle
    that stays outside the group.  names maps each to its object indices; names["group"] are the listed triangles.  small: the
    first quad and the unlisted triangle only -- few enough objects for the local-pool route."""
    from rayrs_amd.api import Emission, Material, Object
    cam, objs, heur, names = _lit.lit_room()
    objs = list(objs)
    white = Material.LambertianDiffuse((0.8, 0.8, 0.8))
    glow = Emission.new(8.0, (1.0, 0.8, 0.6))
    names = dict(names)
    count = [len(objs)]

    def add(tag, verts, idx, emission=glow):
        objs.extend(Object.from_triangles(np.array(verts, dtype=np.float64), np.array(idx, dtype=np.uint32), white, emission))
        names[tag] = list(range(count[0], count[0] + len(idx)))
        count[0] += len(idx)
    add("quad", [(-1.1, 1.7, -0.5), (-0.1, 2.1, -0.5), (-0.1, 2.1, 0.9), (-1.1, 1.7, 0.9)], [(0, 1, 2), (0, 2, 3)])
    names["group"] = list(names["quad"])
    if not small:
        add("behind", [(-0.9, 2.08, -0.3), (-0.3, 2.32, -0.3), (-0.3, 2.32, 0.7), (-0.9, 2.08, 0.7)], [(0, 1, 2), (0, 2, 3)])
        c, r = (0.0, 3.2, 0.0), 0.3
        v = [(c[0] + r, c[1], c[2]), (c[0] - r, c[1], c[2]), (c[0], c[1] + r, c[2]), (c[0], c[1] - r, c[2]), (c[0], c[1], c[2] + r),
             (c[0], c[1], c[2] - r)]
        add("octahedron", v, [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)],
            Emission.new(12.0, (0.7, 0.9, 1.0)))
        names["group"] += names["behind"] + names["octahedron"]
    add("unlisted", [(2.5, 0.3, -2.5), (3.5, 0.3, -2.5), (3.0, 1.4, -2.8)], [(0, 1, 2)], Emission.new(6.0, (0.9, 1.0, 0.7)))
    return cam, objs, heur, names
