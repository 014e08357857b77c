"""A plain-Python reading of include/rayrs_hip.h LIGHT TREE, independent of the library under test: the entries' powers, the
build, one step of the descent, tree_sample, tree_probability and MESH LIGHTS' turn with its two substituted lines.  It builds on
tests/_mesh.py's Table and Reading and changes neither.  Every step is one numpy f64 operation, nothing fused, in the header's
order."""
import numpy as np

import _geometry_reading as G
import _mesh
from _lit import F, FRAC_1_PI, ONES, ZEROS, div, f3, mul, uniform

INF = F(np.inf)
NONE = 0xFFFFFFFF


def emit_of(obj):
    e = obj.emission
    return G.scale(f3(e.color), F(e.strength)) if e.emissive else ZEROS


class Tree(_mesh.Table):
    """_mesh.Table with the tree over it.  w[j], path[j], depth[j] per entry; the nodes in preorder as (m, r2, W, right, entry)
    with right / entry None where there is none (the left child of node i is i + 1)."""

    def __init__(self, prims, tris):
        super().__init__(prims, tris)
        n = len(self.tris)
        self.prims_list = prims.list
        with np.errstate(all="ignore"):
            self.w = []
            for j, t in enumerate(self.tris):
                e = emit_of(prims.list[t])
                self.w.append(self.A[j] * ((e[0] + e[1]) + e[2]))
            self.key = [G.add(G.add(p1, p2), p3) for p1, p2, p3 in self.p]
            self.path, self.depth = [0] * n, [0] * n
            self.nodes = []
            if n:
                self._node(list(range(n)), 0, 0)

    def _node(self, entries, depth, path):
        i = len(self.nodes)
        self.nodes.append(None)
        lo, hi = list(self.p[entries[0]][0]), list(self.p[entries[0]][0])
        for j in entries:
            for v in self.p[j]:
                for c in range(3):
                    if v[c] < lo[c]:
                        lo[c] = v[c]
                    if v[c] > hi[c]:
                        hi[c] = v[c]
        m = tuple((lo[c] + hi[c]) * F(0.5) for c in range(3))
        h = G.sub(tuple(hi), m)
        r2 = G.dot(h, h)
        if len(entries) == 1:
            j = entries[0]
            self.path[j], self.depth[j] = path, depth
            self.nodes[i] = (m, r2, self.w[j], None, j)
            return self.w[j]
        klo, khi = list(self.key[entries[0]]), list(self.key[entries[0]])
        for j in entries:
            for c in range(3):
                if self.key[j][c] < klo[c]:
                    klo[c] = self.key[j][c]
                if self.key[j][c] > khi[c]:
                    khi[c] = self.key[j][c]
        axis = 0
        for c in (1, 2):
            if khi[c] - klo[c] > khi[axis] - klo[axis]:
                axis = c
        order = sorted(entries, key=lambda j: (self.key[j][axis], j))
        half = (len(order) + 1) // 2
        w_l = self._node(order[:half], depth + 1, path)
        right = len(self.nodes)
        w_r = self._node(order[half:], depth + 1, path | (1 << depth))
        W = w_l + w_r
        self.nodes[i] = (m, r2, W, right, None)
        return W

    def importance(self, c, x):
        m, r2, W = self.nodes[c][:3]
        if not W > 0.0:
            return F(0.0)
        d = G.sub(x, m)
        return W / np.fmax(G.dot(d, d), r2)

    def left_probability(self, i, x):
        l, r = i + 1, self.nodes[i][3]
        i_l = self.importance(l, x)
        s = i_l + self.importance(r, x)
        if s > 0.0 and s < INF:
            return i_l / s
        return self.nodes[l][2] / (self.nodes[l][2] + self.nodes[r][2])

    def descend(self, x, u):
        """(j, u at the leaf, p)."""
        i, p = 0, F(1.0)
        with np.errstate(all="ignore"):
            while self.nodes[i][4] is None:
                p_l = self.left_probability(i, x)
                p_r = F(1.0) - p_l
                if u < p_l:
                    u, p, i = u / p_l, p * p_l, i + 1
                else:
                    u, p, i = (u - p_l) / p_r, p * p_r, self.nodes[i][3]
        return self.nodes[i][4], u, p

    def tree_sample(self, x, u1, u2):
        """(j, q, p_sel)."""
        with np.errstate(all="ignore"):
            j, u, p = self.descend(x, u1)
            r = np.fmin(u, F(1.0))
            su = np.sqrt(r)
            b0 = F(1.0) - su
            b1 = su * (F(1.0) - u2)
            b2 = su * u2
            p1, p2, p3 = self.p[j]
            return j, G.add(G.add(G.scale(p1, b0), G.scale(p2, b1)), G.scale(p3, b2)), p

    def tree_probability(self, x, j):
        i, p = 0, F(1.0)
        with np.errstate(all="ignore"):
            for k in range(self.depth[j]):
                p_l = self.left_probability(i, x)
                p_r = F(1.0) - p_l
                if (self.path[j] >> k) & 1:
                    p, i = p * p_r, self.nodes[i][3]
                else:
                    p, i = p * p_l, i + 1
        assert self.nodes[i][4] == j
        return p

    def tree_aim(self, position, j, q, p_sel):
        """(l_s, p_tri) of a shadow sample from `position` to the point q of entry j, chosen with p_sel."""
        with np.errstate(all="ignore"):
            l_s = G.unit(G.sub(q, position))
            away = G.sub(position, q)
            return l_s, (G.dot(away, away) / (np.abs(G.dot(self.n[j], l_s)) * self.A[j])) * p_sel


class Reading(_mesh.Reading):
    """_mesh.Reading with the group chosen by the tree: mesh_bounce and path are _mesh.Reading's with the two substituted lines."""

    def __init__(self, objs, z_near, z_far, heuristic, hdri, tris, osc=None, traversal=0):
        super().__init__(objs, z_near, z_far, heuristic, hdri, tris, osc=osc, traversal=traversal)
        self.mesh = Tree(self.prims, tris)

    def mesh_bounce(self, albedo, thr, position, normal, l, key, draw, lights, member, sky, tally=None):
        K = len(lights)
        M = K + 1 + int(sky)
        b, u1, u2 = uniform(key, draw), uniform(key, draw + 1), uniform(key, draw + 2)
        draw += 3
        k = min(int(b * F(M)), M - 1)
        j = None
        if k == K:
            drawn = "group"
            j, q, p_sel = self.mesh.tree_sample(position, u1, u2)          # substituted
            l_s, p_tri = self.mesh.tree_aim(position, j, q, p_sel)         # substituted
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
                        j = self.listed[obj]
                        away = G.sub(o, position)
                        p = (G.dot(away, away) / (np.abs(G.dot(normal, d)) * self.mesh.A[j])) * self.mesh.tree_probability(o, j)  # substituted
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


radiance_paths, irradiance_paths, image_paths, answers = _mesh.radiance_paths, _mesh.irradiance_paths, _mesh.image_paths, _mesh.answers
