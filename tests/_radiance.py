"""A plain-Python reading of include/rayrs_hip.h RADIANCE QUERY and IRRADIANCE, independent of the library under test: the
keys and the irradiance rays come from tests/_ao.py, a path's value and its number of queries from the oracle's radiance()
(OracleScene.radiance, one call per path, the rng at draw 0 or 2), and the sums are written out in the header's order with one
numpy f64 operation each -- nothing fused."""
import numpy as np

import _ao


def chunks(samples, sample_chunk):
    """The (first, end) sample ranges of a ray's chunks: c' = S if c == 0 or c >= S, else c."""
    c = samples if sample_chunk == 0 or sample_chunk >= samples else sample_chunk
    return [(k, min(k + c, samples)) for k in range(0, samples, c)]


def mean(values, sample_chunk):
    """radiance_i of one ray from its samples' values (S, 3): C_k = zeros, += in sample order; sum = C_0 assigned, then += C_k
    in chunk order; sum * (1.0 / S)."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    samples = len(values)
    total = None
    with np.errstate(all="ignore"):
        for first, end in chunks(samples, sample_chunk):
            c = np.zeros(3)
            for s in range(first, end):
                c = c + values[s]
            total = c if total is None else total + c
        return total * (np.float64(1.0) / np.float64(samples))


def paths(osc, origins, directions, samples, max_bounces, seed, index_base=0, draw=0, traversal=0, per_sample_rays=False):
    """Every path of a call: (values (n, S, 3) f64, queries (n, S) int64).  per_sample_rays: origins and directions hold a ray
    per (ray, sample), n * S of them (the irradiance's), else one per ray."""
    n = len(origins) // samples if per_sample_rays else len(origins)
    values, queries = np.zeros((n, samples, 3)), np.zeros((n, samples), dtype=np.int64)
    for i in range(n):
        for s in range(samples):
            k = i * samples + s if per_sample_rays else i
            values[i, s], queries[i, s], _ = osc.radiance(origins[k], directions[k], max_bounces,
                                                          _ao.path_key(int(seed), int(index_base) + i, s), draw, traversal)
    values.setflags(write=False), queries.setflags(write=False)
    return values, queries


def answers(values, queries, sample_chunk):
    """(radiance (n, 3) f64, queries (n,) uint32) of a call from paths()."""
    rad = np.stack([mean(v, sample_chunk) for v in values]) if len(values) else np.zeros((0, 3))
    return rad, queries.sum(axis=1).astype(np.uint32)


def radiance_paths(osc, origins, directions, samples, max_bounces, seed, index_base=0, traversal=0):
    return paths(osc, np.ascontiguousarray(origins, dtype=np.float64), np.ascontiguousarray(directions, dtype=np.float64), samples,
                 max_bounces, seed, index_base, 0, traversal)


def irradiance_paths(osc, points, normals, samples, bias, max_bounces, seed, index_base=0, traversal=0):
    """Draws 0 and 1 make the ray as AMBIENT OCCLUSION does (_ao.rays); the path's rng goes on at draw 2."""
    o, d = _ao.rays(points, normals, samples, bias, seed, index_base=index_base)
    return paths(osc, o, d, samples, max_bounces, seed, index_base, 2, traversal, per_sample_rays=True)
