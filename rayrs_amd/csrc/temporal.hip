// temporal.hip -- the reprojection kernel of temporal accumulation (include/rayrs_hip.h TEMPORAL ACCUMULATION).  It is no
// part of a render.  It streams through memory: no LDS, no scratch, and at most 128 vector registers, so that four waves fit
// a SIMD and the four divergent taps of one wave are covered by the other three.
#include <hip/hip_runtime.h>

#include "../../include/rayrs_hip.h"
#include "temporal_kernels.h"

namespace rayrs {

// One lane per pixel of A, a wave 64 consecutive pixels of a row (as the a-trous kernels): neighbouring pixels of A land on
// neighbouring pixels of B, so the four taps of a wave's lanes fall in a few neighbouring 128-byte lines of each of B's
// planes.  A tap's depth, coverage, object, normal, variance and weight decide whether it is valid; its colour -- the widest
// plane -- is fetched only then.  (The header lists the tap's skips in another order; every one of them is a plain skip, so
// the order they are tried in changes no result.)  About fourteen f64 divisions per pixel, none of them in a loop longer
// than the four taps.
constexpr uint32_t TEMPORAL_BX = 64, TEMPORAL_BY = 4;

namespace {
__device__ __forceinline__ double dot3(double ax, double ay, double az, const double* b) {
    return (ax * b[0] + ay * b[1]) + az * b[2];
}
}  // namespace

__global__ void __launch_bounds__(TEMPORAL_BX * TEMPORAL_BY) temporal_kernel(TemporalDev t) {
    const uint32_t col = blockIdx.x * TEMPORAL_BX + threadIdx.x;
    const uint32_t r = blockIdx.y * TEMPORAL_BY + threadIdx.y;
    const CameraDev& ca = t.cam_a;
    const CameraDev& cb = t.cam_b;
    if (col >= ca.W || r >= ca.H) return;
    const size_t p = (size_t)r * ca.W + col;
    uint32_t op = t.a_object[p];
    if (t.prim_object) {  // (uniform) a features pass numbers depth-first slots: the history keeps objects
        if (op != 0xffffffffu) op = op < t.n_prims ? t.prim_object[op] : 0xffffffffu;
        t.out_object[p] = op;
    }
    const double cx = t.a_color[3 * p], cy = t.a_color[3 * p + 1], cz = t.a_color[3 * p + 2];
    const double v_in = t.a_variance[p];
    const double wc = t.a_weight ? t.a_weight[p] : (double)t.a_tile_n[(size_t)(r >> 3) * t.a_tiles_x + (col >> 3)];
    // "no history": the frame's own values
    double ox = cx, oy = cy, oz = cz, ov = v_in, ow = wc;
    const bool blendable = __builtin_isfinite(cx) && __builtin_isfinite(cy) && __builtin_isfinite(cz) && wc > 0.0;
    if (!blendable) ow = wc > 0.0 ? wc : 0.0;  // 1. pass-through
    if (blendable && t.has_b) {
        // 2. the centre ray of the pixel
        const double x = ((double)(ca.W - col) + 0.5) / ca.ppc - ca.width / 2.;
        const double y = ((double)(ca.H - r) + 0.5) / ca.ppc - ca.height / 2.;
        const double dx = (ca.z[0] + x * ca.e_x[0]) + y * ca.e_y[0];
        const double dy = (ca.z[1] + x * ca.e_x[1]) + y * ca.e_y[1];
        const double dz = (ca.z[2] + x * ca.e_x[2]) + y * ca.e_y[2];
        // 3. the source vector
        const double kp = t.a_coverage[p];
        const bool hit = kp > 0.0;
        bool history = hit || kp == 0.0;
        double ux = dx, uy = dy, uz = dz;
        double npx = 0.0, npy = 0.0, npz = 0.0;
        if (hit) {
            const double big_t = t.a_depth[p] / kp;
            ux = (ca.origin[0] + dx * big_t) - cb.origin[0];
            uy = (ca.origin[1] + dy * big_t) - cb.origin[1];
            uz = (ca.origin[2] + dz * big_t) - cb.origin[2];
            npx = t.a_normal[3 * p], npy = t.a_normal[3 * p + 1], npz = t.a_normal[3 * p + 2];
        }
        // 4. into B
        const double s = dot3(ux, uy, uz, cb.z), zz = dot3(cb.z[0], cb.z[1], cb.z[2], cb.z);
        history = history && s > 0.0;
        if (history) {
            const double tp = s / zz;
            const double xp = (dot3(ux, uy, uz, cb.e_x) * zz) / s, yp = (dot3(ux, uy, uz, cb.e_y) * zz) / s;
            const double fx = ((double)cb.W + 0.5) - (xp + cb.width / 2.) * cb.ppc;
            const double fy = ((double)cb.H + 0.5) - (yp + cb.height / 2.) * cb.ppc;
            if (fx >= -1.0 && fx < (double)cb.W && fy >= -1.0 && fy < (double)cb.H) {
                const double x0f = __builtin_floor(fx), y0f = __builtin_floor(fy);
                const double ax = fx - x0f, ay = fy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;  // -1 .. 65534
                const double tol_z = t.tz2 * (tp * tp);
                // 5. the taps
                double bs = 0.0, hx = 0.0, hy = 0.0, hz = 0.0, hv = 0.0, hm = 0.0;
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int qy = y0 + j;
                    if (qy < 0 || qy >= (int)cb.H) continue;
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int qx = x0 + i;
                        if (qx < 0 || qx >= (int)cb.W) continue;
                        const double b = (i ? ax : 1.0 - ax) * (j ? ay : 1.0 - ay);
                        if (b == 0.0) continue;
                        const size_t q = (size_t)qy * cb.W + (uint32_t)qx;
                        const double kq = t.b_coverage[q];
                        if (hit) {
                            if (!(kq > 0.0) || t.b_object[q] != op) continue;
                            const double dt = t.b_depth[q] / kq - tp;
                            if (!(dt * dt <= tol_z)) continue;
                            const double ex = npx - t.b_normal[3 * q], ey = npy - t.b_normal[3 * q + 1], ez = npz - t.b_normal[3 * q + 2];
                            if (!((ex * ex + ey * ey) + ez * ez <= t.tn2)) continue;
                        } else if (!(kq == 0.0)) {
                            continue;
                        }
                        const double vq = t.b_variance[q], mq = t.b_weight[q];
                        if (!(vq >= 0.0) || !(mq > 0.0)) continue;
                        const double qcx = t.b_color[3 * q], qcy = t.b_color[3 * q + 1], qcz = t.b_color[3 * q + 2];
                        if (!(__builtin_isfinite(qcx) && __builtin_isfinite(qcy) && __builtin_isfinite(qcz))) continue;
                        bs += b;
                        hx += qcx * b, hy += qcy * b, hz += qcz * b;
                        hv += vq * b;
                        hm += mq * b;
                    }
                }
                if (bs != 0.0) {  // (6. no valid tap: no history)
                    // 7. the history's values
                    const double hcx = hx / bs, hcy = hy / bs, hcz = hz / bs;
                    double big_v = hv / bs;
                    const double m0 = hm / bs;
                    const double m = m0 < t.max_weight ? m0 : t.max_weight;
                    // 8. healing
                    const double inf = __builtin_huge_val();
                    double vp = v_in >= 0.0 ? v_in : inf;
                    if (vp == inf && big_v < inf) vp = (big_v * m0) / wc;
                    else if (big_v == inf && vp < inf) big_v = (vp * wc) / m0;
                    // 9. the blend
                    const double alpha = wc / (wc + m), beta = 1.0 - alpha;
                    ox = hcx * beta + cx * alpha, oy = hcy * beta + cy * alpha, oz = hcz * beta + cz * alpha;
                    const double bb = beta * beta, aa = alpha * alpha;
                    const double tb = bb == 0.0 ? 0.0 : big_v * bb;  // (0 x infinity)
                    const double ta = aa == 0.0 ? 0.0 : vp * aa;
                    ov = tb + ta;
                    ow = m + wc;
                }
            }
        }
    }
    t.out_color[3 * p] = ox, t.out_color[3 * p + 1] = oy, t.out_color[3 * p + 2] = oz;
    t.out_variance[p] = ov;
    t.out_weight[p] = ow;
}

hipError_t launch_temporal(const TemporalDev& t, hipStream_t stream) {
    if (t.cam_a.W == 0u || t.cam_a.H == 0u) return hipSuccess;
    // (H <= 65535: the grid's y dimension holds it)
    hipLaunchKernelGGL(temporal_kernel, dim3((t.cam_a.W + TEMPORAL_BX - 1u) / TEMPORAL_BX, (t.cam_a.H + TEMPORAL_BY - 1u) / TEMPORAL_BY),
                       dim3(TEMPORAL_BX, TEMPORAL_BY), 0, stream, t);
    return hipGetLastError();
}

}  // namespace rayrs
