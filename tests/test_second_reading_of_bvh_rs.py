"""A second, independent reading of Bvh::build (rayrs-lib/src/bvh.rs:7-38, :81-185, :227-389) and of the bounding
boxes it is built from (geometry.rs:544-550, :577-582, :640-645, :674-683, :686-732), in plain Python written from
the Rust text, against the product's exported tree (host-only scene: no GPU).  What the tree decides -- and all it
decides, since the closest hit does not depend on the topology otherwise -- is (1) the depth-first order of the
primitives (equal-t ties: the first leaf wins, bvh.rs:62) and (2) which box gates which leaves (a leaf is reached iff
the box of its parent Node is entered; a flat box never is, geometry.rs:474).  Both are compared exactly: Python's
floats are the same IEEE doubles, list.sort is stable like slice::sort_by."""
import bisect
import math

import numpy as np
import pytest

import rayrs_amd
from rayrs_amd import procedural, scenes
from rayrs_amd.api import BvhHeuristic, Emission, Material, Object, flatten_objects
from test_bvh_builder import reference_groups

HDRI = procedural.make_hdri(8, 4)
NR, DARK = Material.NoReflect(), Emission.Dark()


def bbox_of(o):  # impl From<&Sphere / &Plane / &Triangle> for AxisAlignedBoundingBox, geometry.rs:686-732
    if o.kind == "sphere":
        r = math.sqrt(o.radius * o.radius)  # the sphere keeps radius^2 (geometry.rs:99) and takes its root here
        c = o.origin
        return (c[0] - r, c[0] + r, c[1] - r, c[1] + r, c[2] - r, c[2] + r)
    if o.kind == "plane":
        ax = o.axis >> 1
        if ax == 0:
            return (o.pos, o.pos, o.umin, o.umax, o.vmin, o.vmax)
        if ax == 1:
            return (o.umin, o.umax, o.pos, o.pos, o.vmin, o.vmax)
        return (o.umin, o.umax, o.vmin, o.vmax, o.pos, o.pos)
    p1, p2, p3 = o.p
    return (min(p1[0], min(p2[0], p3[0])), max(p1[0], max(p2[0], p3[0])), min(p1[1], min(p2[1], p3[1])),
            max(p1[1], max(p2[1], p3[1])), min(p1[2], min(p2[2], p3[2])), max(p1[2], max(p2[2], p3[2])))


def expand(a, b):  # geometry.rs:674-683
    return (min(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]), min(a[4], b[4]), max(a[5], b[5]))


def bbox_list(items):  # from_object_list, geometry.rs:544-550
    out = items[0][1]
    for _, b in items[1:]:
        out = expand(out, b)
    return out


def center(b):  # geometry.rs:577-582
    return ((b[1] - b[0]) / 2.0 + b[0], (b[3] - b[2]) / 2.0 + b[2], (b[5] - b[4]) / 2.0 + b[4])


def area(b):  # geometry.rs:640-645
    x, y, z = b[1] - b[0], b[3] - b[2], b[5] - b[4]
    return 2.0 * x * y + 2.0 * y * z + 2.0 * x * z


class Node:  # BvhTree::Node(AxisAlignedBoundingBox, Vec<BvhTree>), bvh.rs:222
    def __init__(self, box, children):
        self.box, self.children = box, children


class LeafNode:  # BvhTree::LeafNode(Object), bvh.rs:223
    def __init__(self, obj):
        self.object = obj


def build(items, splits, order, groups):
    """BvhTree::build_sah (splits > 0, bvh.rs:227-317) / build_midpoint (:319-389).  items: [(object index, bbox)].
    Appends the objects to `order` depth-first and the bottom Nodes / direct leaves to `groups` as (first position
    in the order, count, gating box).  Returns the tree: Node(box, children) / LeafNode(object index)."""
    box = bbox_list(items)
    if len(items) > 4:
        x, y, z = box[1] - box[0], box[3] - box[2], box[5] - box[4]
        ax = 0 if (x >= y and x >= z) else 1 if y >= z else 2
        items = sorted(items, key=lambda it: center(it[1])[ax])  # stable, like sort_by on the centres
        cs = [center(it[1])[ax] for it in items]
        first_above = lambda v: next((k for k, c in enumerate(cs) if c > v), None)  # split_ind, bvh.rs:7-13
        if splits:
            mn, ln = box[2 * ax], (x, y, z)[ax]
            dist = ln / (splits - 1)
            best, best_sah = None, math.inf
            # the boxes of items[:k + 1] and items[k:] once, not once per split (a min / max is exact, so only the sign of a
            # zero bound can depend on the order of the fold, and no surface area, hence no cost, depends on that sign);
            # the centres are sorted, so split_ind is a bisection
            pre, suf = [items[0][1]], [items[-1][1]]
            for it in items[1:]:
                pre.append(expand(pre[-1], it[1]))
            for it in items[-2::-1]:
                suf.append(expand(it[1], suf[-1]))
            suf.reverse()
            sorted_ok = not any(c != c for c in cs)
            for i in range(1, splits + 1):
                v = mn + i * dist
                ind = bisect.bisect_right(cs, v) if sorted_ok else first_above(v)
                if ind is not None and ind < len(cs):
                    pl = area(pre[ind - 1]) / area(box) if ind else 0.0  # calculate_sah(0.3, 1., ...), bvh.rs:15-38
                    pr = area(suf[ind]) / area(box)
                    s = 0.3 + 1.0 * (pl * ind + pr * (len(items) - ind))
                    if s < best_sah:
                        best_sah, best = s, ind
        else:
            best = first_above(center(box)[ax])
        ind = len(items) // 2 if (best is None or best == 0 or best == len(items) - 1) else best
        children = []
        for side in (items[:ind], items[ind:]):
            if len(side) > 1:
                children.append(build(side, splits, order, groups))
            else:  # LeafNode directly under this Node: no box of its own (bvh.rs:297, :302) -- this Node's gates it
                groups.append((len(order), 1, box))
                order.append(side[0][0])
                children.append(LeafNode(side[0][0]))
        return Node(box, children)
    groups.append((len(order), len(items), box))
    order.extend(i for i, _ in items)
    return Node(box, [LeafNode(i) for i, _ in items])


def singles(objs):
    out = []
    for o in flatten_objects(objs):
        if o.kind == "mesh":
            v = np.asarray(o.verts, dtype=np.float64)
            out += [Object.triangle(tuple(v[a]), tuple(v[b]), tuple(v[c]), o.mat, o.emission) for a, b, c in o.idx]
        else:
            out.append(o)
    return out


CASES = [("single_sphere", scenes.diffuse_single_sphere), ("sphere_row", scenes.cook_torrance_spheres_metallic),
         ("mesh320", lambda: scenes.mesh_scene(2)), ("mesh1280_light", lambda: scenes.mesh_scene(3, area_light=True))]


def soup():
    r = np.random.default_rng(8)
    objs = []
    for i in range(240):
        c = r.uniform(-5, 5, 3)
        if i % 3 == 0:
            objs.append(Object.sphere(float(r.uniform(0.05, 0.6)), c, NR, DARK))
        elif i % 3 == 1:
            objs.append(Object.plane(int(r.integers(0, 6)), c[0], c[0] + 0.5, c[1], c[1] + 0.7, c[2], NR, DARK))
        else:
            objs.append(Object.triangle(c, c + r.uniform(-1, 1, 3), c + r.uniform(-1, 1, 3), NR, DARK))
    objs += [Object.sphere(0.3, (1.0, 1.0, 1.0), NR, DARK) for _ in range(9)]  # coincident centres: the median fallback
    return None, objs, None


@pytest.mark.parametrize("name,fn", CASES + [("soup", soup)], ids=[c[0] for c in CASES] + ["soup"])
@pytest.mark.parametrize("heur", [BvhHeuristic.Sah(1000), BvhHeuristic.Sah(7), BvhHeuristic.Midpoint],
                         ids=["sah1000", "sah7", "midpoint"])
def test_product_tree_is_the_second_reading(name, fn, heur):
    objs = fn()[1]
    prod = rayrs_amd.Scene(objs, 1e-6, 1e6, heur, HDRI, device=-1)
    box, ref, prim_object = prod.export_bvh()
    info = prod.info()
    flat = singles(objs)
    items = [(i, bbox_of(o)) for i, o in enumerate(flat)]
    order, groups = [], []
    if len(items) == 1:
        groups.append((0, 1, items[0][1])), order.append(0)
    else:
        build(items, heur[1] if heur[0] == "sah" else 0, order, groups)
    assert list(prim_object) == order                                   # (1) the depth-first order
    want = {(1 << 30) | (first << 2) | (count - 1): np.array(b, dtype=np.float64).tobytes() for first, count, b in groups}
    assert reference_groups(box, ref, info) == want                     # (2) every group behind exactly its gating box
    assert tuple(info["root_box"]) == bbox_list(items)
