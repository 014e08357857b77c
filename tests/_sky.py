"""A plain-Python reading of include/rayrs_hip.h SKY SAMPLING, independent of the library under test: the sky's table, sky_sample,
p_env and DIRECT LIGHTING's turn with the sky as light number K.  It builds on tests/_direct.py's Reading -- the lamps' samples
and densities, the unlit Material::evaluate with Plastic's arm told, the oracle's query and background -- and on the oracle's
elementary functions (_oracle.math_fn).  Every step is one numpy f64 operation, nothing fused, in the header's order."""
import numpy as np

import _ao
import _direct
import _geometry_reading as G
import _lit
import _oracle
from _lit import F, FRAC_1_PI, ONES, PI, ZEROS, div, f3, mul, uniform

INF = F(np.inf)
SIN, COS, ACOS, ATAN2, SQRT = 0, 1, 5, 6, 7


def fn(code, x, y=0.0):
    return F(_oracle.math_fn(code, [x], [y])[0])


def as_usize(x):
    """Rust `as usize`: NaN and negatives are 0."""
    return int(x) if x > 0.0 else 0


class Table:
    """The table of an (h, w, 3) f32 map: A, C (h-1, w-1), M (h-1,), T.  texel(i, j) is the map clipped to [0, 3]
    (clip = min(max).max(min), vecmath.rs:388-396, on the f32 widened to f64)."""

    def __init__(self, hdri):
        tex = np.fmax(np.fmin(np.asarray(hdri, dtype=np.float32).astype(F), F(3.0)), F(0.0))
        self.h, self.w = int(tex.shape[0]), int(tex.shape[1])
        h, w = self.h, self.w
        lum = (tex[..., 0] + tex[..., 1]) + tex[..., 2]
        s = np.array([fn(SIN, (F(i) + F(0.5)) * PI / F(h - 1)) for i in range(h - 1)])
        self.A = s[:, None] * (((lum[:-1, :-1] + lum[1:, :-1]) + lum[:-1, 1:]) + lum[1:, 1:])
        self.C = np.add.accumulate(self.A, axis=1)   # (strictly left to right: the first assigned, then one add per cell)
        self.R = self.C[:, w - 2].copy()
        self.M = np.add.accumulate(self.R)
        self.T = F(self.M[h - 2])
        for a in (self.A, self.C, self.R, self.M):
            a.setflags(write=False)

    def usable(self):
        return bool(self.T > 0.0 and np.isfinite(self.T))

    @staticmethod
    def first_above(prefix, t):
        """The first index whose prefix exceeds t, or the last index if there is none (a linear scan: any search finds it)."""
        for k in range(len(prefix)):
            if prefix[k] > t:
                return k
        return len(prefix) - 1

    def sample(self, u1, u2):
        h, w = self.h, self.w
        with np.errstate(all="ignore"):
            ty = u1 * self.T
            i = self.first_above(self.M, ty)
            below = self.M[i - 1] if i > 0 else F(0.0)
            y = F(i) + (ty - below) / self.R[i]
            tx = u2 * self.R[i]
            j = self.first_above(self.C[i], tx)
            below = self.C[i, j - 1] if j > 0 else F(0.0)
            x = F(j) + (tx - below) / self.A[i, j]
            theta = y / F(h - 1) * PI
            phi = x / F(w - 1) * (F(2.0) * PI)
            psi = phi - PI
            st, ct = fn(SIN, theta), fn(COS, theta)
            sp, cp = fn(SIN, psi), fn(COS, psi)
            return (cp * st, ct, sp * st)

    def cell(self, l):
        """(i, j, dir.y) of p_env(l): the bilinear cell Scene::background reads for l."""
        h, w = self.h, self.w
        d = G.unit(f3(l))
        phi = fn(ATAN2, d[2], d[0]) + PI
        theta = fn(ACOS, d[1])
        x = phi / (F(2.0) * PI) * F(w - 1)
        y = theta / PI * F(h - 1)
        return min(as_usize(np.floor(y)), h - 2), min(as_usize(np.floor(x)), w - 2), d[1]

    def density(self, l):
        h, w = self.h, self.w
        with np.errstate(all="ignore"):
            i, j, dy = self.cell(l)
            sn = np.sqrt(F(1.0) - dy * dy)
            return ((self.A[i, j] / self.T) * (F(w - 1) * F(h - 1))) / (((F(2.0) * PI) * PI) * sn)

    def lit_solid_angle(self):
        """The solid angle of the cells with A > 0: the sum of dphi * (cos theta_i - cos theta_{i+1}) (float arithmetic: a
        statistic's expectation, not an operation)."""
        h, w = self.h, self.w
        theta = np.arange(h) * np.pi / (h - 1)
        band = np.cos(theta[:-1]) - np.cos(theta[1:])
        return float(((self.A > 0.0) * band[:, None]).sum() * (2.0 * np.pi / (w - 1)))


def new_tally():
    """Shadow samples by what was drawn (the sky or a lamp) and what became of them; misses of a path's own ray by their weight."""
    return dict(sky_credited=0, sky_blocked=0, sky_skipped_ndl=0, sky_skipped_den=0, sky_met_lamp=0, lamp_credited=0, lamp_blocked=0,
                lamp_missed=0, lamp_skipped=0, miss_weighted=0, miss_unweighted=0, plastic_diffuse=0, plastic_specular=0, taken=0)


class Reading(_direct.Reading):
    def __init__(self, objs, z_near, z_far, heuristic, hdri, osc=None, traversal=0):
        super().__init__(objs, z_near, z_far, heuristic, hdri, osc=osc, traversal=traversal)
        self.sky = Table(hdri)

    def background(self, d):
        return f3(self.osc.background(np.array([d]))[0])

    def mix_density(self, lights, position, l):
        """p_M(position, l): the lamps in list order, then p_env(l) last, over (double)M."""
        p_m = None
        for k in lights:
            p = self.light_density(k, position, l)
            p_m = p if p_m is None else p_m + p
        p_e = self.sky.density(l)
        p_m = p_e if p_m is None else p_m + p_e
        return p_m / F(len(lights) + 1)

    def sky_bounce(self, albedo, thr, position, normal, l, key, draw, lights, member, tally=None):
        """The diffuse branch of the turn, K >= 0: (what the shadow sample adds to light or None, its queries (0 or 1), w_next,
        next draw)."""
        K = len(lights)
        M = K + 1
        b, u1, u2 = uniform(key, draw), uniform(key, draw + 1), uniform(key, draw + 2)
        draw += 3
        k = min(int(b * F(M)), M - 1)
        sky = k == K
        if sky:
            l_s = self.sky.sample(u1, u2)
        else:
            l_s = G.unit(G.sub(self.light_sample(lights[k], u1, u2), position))
        ndl_s = G.dot(normal, l_s)
        added, queries = None, 0
        what = None
        if ndl_s > 0.0:
            den = self.mix_density(lights, position, l_s) + ndl_s * FRAC_1_PI
            if den < INF:
                c = div(G.scale(G.scale(albedo, FRAC_1_PI), ndl_s), den)
                obj, _ = self.osc.intersect(position, l_s, self.z_near, self.z_far, self.traversal)
                queries = 1
                if obj >= 0 and obj in member:
                    added = mul(mul(thr, c), self.emit(obj))
                    what = "sky_met_lamp" if sky else "lamp_credited"
                elif obj < 0:
                    added = mul(mul(thr, c), self.background(l_s))
                    what = "sky_credited" if sky else "lamp_missed"
                else:
                    what = "sky_blocked" if sky else "lamp_blocked"
                if tally is not None:
                    tally["taken"] += 1
            else:
                what = "sky_skipped_den" if sky else "lamp_skipped"
        else:
            what = "sky_skipped_ndl" if sky else "lamp_skipped"
        if tally is not None:
            tally[what] += 1
        ndl = G.dot(normal, l)
        pc = ndl * FRAC_1_PI
        pm = self.mix_density(lights, position, l)
        w_next = pc / (pc + pm) if pm > 0.0 else F(1.0)
        return added, queries, w_next, draw

    def path(self, o, d, max_bounces, key, draw, lights, tally=None, w=F(1.0)):
        """(L (3,) f64, Bvh::intersect calls -- the shadow queries among them --, next draw).  w: the weight of what the first ray
        meets, a listed object or the sky (1.0 but after IRRADIANCE's virtual bounce)."""
        o, d = f3(o), f3(d)
        member = set(lights)
        thr, light = ONES, ZEROS
        queries = 0
        with np.errstate(all="ignore"):
            for _ in range(int(max_bounces)):
                obj, t = self.osc.intersect(o, d, self.z_near, self.z_far, self.traversal)
                queries += 1
                if obj < 0:
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
                if obj in member:
                    e = G.scale(e, w)
                light = G.add(light, mul(thr, e))
                w_next = F(1.0)
                if diffuse:
                    albedo = f3(self.prims.list[obj].mat.color)
                    added, q, w_next, draw = self.sky_bounce(albedo, thr, position, normal, l, key, draw, lights, member, tally)
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
                w = w_next
                o, d = position, l
        return np.array(light), queries, draw


def radiance_paths(R, origins, directions, samples, max_bounces, seed, lights, index_base=0, tally=None):
    """RADIANCE with the sky: (values (n, S, 3), queries (n, S)) of a call; `lights` are the lamps, the sky is always on."""
    lights = [int(k) for k in lights]

    def one(i, s):
        return R.path(origins[i], directions[i], max_bounces, _ao.path_key(int(seed), int(index_base) + i, s), 0, lights, tally)[:2]
    return _lit._collect(len(origins), samples, one)


def irradiance_paths(R, points, normals, samples, bias, max_bounces, seed, lights, index_base=0, tally=None):
    """IRRADIANCE with the sky: the virtual bounce whatever K is -- the cosine ray on draws 0 and 1, b, u1, u2 on draws 2 to 4, no
    roulette, the path from draw 5."""
    lights = [int(k) for k in lights]
    member = set(lights)

    def one(i, s):
        key = _ao.path_key(int(seed), int(index_base) + i, s)
        p, n = f3(points[i]), f3(normals[i])
        with np.errstate(all="ignore"):
            position = G.add(p, G.scale(n, F(bias)))
            l = R.cosine_direction(n, key, 0)
            if max_bounces == 0:
                return np.zeros(3), 0
            added, q, w, draw = R.sky_bounce(ONES, ONES, position, n, l, key, 2, lights, member, tally)
            value, q_path, _ = R.path(position, l, max_bounces, key, draw, lights, tally, w)
            credit = ZEROS if added is None else added   # (the virtual bounce's credit: +0 where nothing was credited)
            return np.array(G.add(credit, f3(value))), q + q_path
    return _lit._collect(len(points), samples, one)


def image_paths(R, ocam, samples, max_bounces, seed, lights, tally=None, pixels=None):
    """The image form: pixel (row, col) is ray row * W + col, the primary ray sample_ray's on draws 0 and 1."""
    lights = [int(k) for k in lights]
    h, w = ocam.y_pixels(), ocam.x_pixels()
    pixels = range(h * w) if pixels is None else [int(i) for i in pixels]

    def one(j, s):
        i = pixels[j]
        row, col = divmod(i, w)
        key = _ao.path_key(int(seed), i, s)
        o, d, draw = ocam.primary_ray(h - row, w - col, key)
        return R.path(o, d, max_bounces, key, draw, lights, tally)[:2]
    return _lit._collect(len(pixels), samples, one)


answers = _lit.answers
