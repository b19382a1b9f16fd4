// Efficient multi-scale attention (EMA, models/common.py:5263-5292): the passes over the (B,H,W,C) map that are EMA's own.  With g = factor,
// cg = C / g, channel c = gi * cg + j, N = H * W and the small tensors sg = sigmoid(conv1x1(means)) (B, H + W, C) and x2 = conv3x3(x):
//   stats     mean and sum of squared deviations of t = x * sg_h[b,h,c] * sg_w[b,w,c] per (b, c), and the mean of x2            (x, x2 read once)
//             -> vec (B, 4, C): mean, rstd = 1 / sqrt(M2 / N + eps), x21 = softmax_j(mean x2), x11 = softmax_j(beta)
//   gate      x1 = gamma * (t - mean) * rstd + beta in registers; wgt[b,gi,h,w] = sum_j x11[j] x2[j] + x21[b,gi,j] x1[j]; out = [res +] x * sigmoid(wgt)
//   bwd gate  the same rebuild + dout: dx = [dx +] dout * s, dwgt = s (1 - s) sum_j dout[j] x[j] (written over the group's channels of dw), and
//             per (b, c) the sums P = sum dwgt * that, Q = sum dwgt, R = sum dwgt * x2  -> bvec (B, 3, C): the constants of the next pass; dgamma, dbeta
//   bwd norm  dt = rstd * gamma * (dx1 - mean dx1 - that * mean(dx1 * that)), dx1 = dwgt * x21, written to y; dw becomes dx2 = dwgt * x11 + c2 in
//             place; and the row / column sums of dt * t, times (1 - sg): the gradient of conv1x1's output in sg's layout
// x11 uses mean(x1) = beta (the mean of a normalised map is its shift); its gradient lands on beta alone, as autograd's does up to rounding.
//
// Geometry: the map pass of common.h (map_plan, map_lane): a workgroup takes RH rows x NL columns of one image, lane (l, q) of its
// 256 = NL x QW owns column w0 + l and channel quad q and walks the rows four at a time.  A group of cg channels is L = cg / 4 adjacent lanes: the reduction over a group goes through LDS,
// every lane of the group adding the same L values in the same order, so all of them hold the same bits.  Reductions over the map: the lane
// keeps its column's sum over the rows it walks, the workgroup adds its NL columns in order through LDS and writes one partial per (b, c); a
// second launch folds the partials in order.  No float atomics: two launches are bit-identical.
// The variance uses a pivot: t at pixel (0, 0) of the same (b, c), which every lane can form; mean = pivot + S1 / N, M2 = S2 - S1^2 / N with
// S1, S2 the sums of (t - pivot) and its square.  On a 1x1 map both are exactly zero.
#include "common.h"

// no fused multiply-adds here: t - pivot, t - mean and dx1 - mean dx1 must cancel exactly where both sides are the same product (1x1 maps)
#pragma clang fp contract(off)

namespace somi {

constexpr int EM_RU = 4;          // rows in flight per lane
constexpr int EM_MAX_CG = 64;     // channels of a group: at most 16 lanes

struct EmArgs {
    somi_slice x, x2, sg, y, res, dx, dw, dsg;
    const float *gamma, *beta;
    float *stats, *vec, *sums, *bvec, *dgamma, *dbeta;
    float *part, *rowpart, *colpart;
    float eps;
    int accumulate;
    int B, H, W, C4, L, QW, NL, nQc, nWc, nHc, RH, nP;
};

__device__ __forceinline__ f32x4 em_vec(const float *p, long row, int C4, int q) { return ld4(p + (row * C4 + q) * 4); }
__device__ __forceinline__ float em_sum4(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }

// the workgroup's NL columns added in order, one partial per (b, partial, k, c): part[((b * nP + p) * K + k) * C + c]
template <int K>
__device__ __forceinline__ void em_fold_columns(const EmArgs &a, const MapLane &l, f32x4 (*sm)[256], const f32x4 (&s)[K]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) sm[k][t] = s[k];
    __syncthreads();
    const int q = (blockIdx.z % a.nQc) * 256 + t;
    if (t < a.QW && q < a.C4) {
        const long p = (long)l.b * a.nP + blockIdx.y * a.nWc + blockIdx.x;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            f32x4 r = sm[k][t];
            for (int c = 1; c < a.NL; ++c) r += sm[k][c * a.QW + t];
            st4(a.part + ((p * K + k) * a.C4 + q) * 4, r);
        }
    }
}

// ------------------------------------------------------------------------------------------------ statistics
__global__ __launch_bounds__(256) void em_stats_kernel(EmArgs a) {
    __shared__ f32x4 sm[3][256];
    const MapLane l = map_lane(a);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 s[3] = {zero, zero, zero};
    if (l.on) {
        const long row0 = (long)l.b * (a.H + a.W);
        const f32x4 piv = ld4(at(a.x, (long)l.b * a.H * a.W, l.q)) * ld4(at(a.sg, row0, l.q)) * ld4(at(a.sg, row0 + a.H, l.q));
        const f32x4 sw = ld4(at(a.sg, row0 + a.H + l.w, l.q));
        for (int g = l.h0; g < l.h1; g += EM_RU) {
            f32x4 v[EM_RU], sh[EM_RU], v2[EM_RU];
#pragma unroll
            for (int r = 0; r < EM_RU; ++r) {
                v[r] = sh[r] = v2[r] = zero;
                if (g + r < l.h1) {
                    const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
                    v[r] = ld4(at(a.x, pix, l.q));
                    sh[r] = ld4(at(a.sg, row0 + g + r, l.q));
                    if (a.x2.p) v2[r] = ld4(at(a.x2, pix, l.q));
                }
            }
#pragma unroll
            for (int r = 0; r < EM_RU; ++r) {
                if (g + r >= l.h1) continue;
                const f32x4 d = v[r] * sh[r] * sw - piv;
                s[0] += d;
                s[1] += d * d;
                s[2] += v2[r];
            }
        }
    }
    em_fold_columns<3>(a, l, sm, s);
}

// one lane per (b, quad): the partials in order -> stats (B, 3, C): mean of t, M2 of t, mean of x2
__global__ __launch_bounds__(256) void em_stats_finish_kernel(EmArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.B * a.C4) return;
    const int q = (int)(i % a.C4), b = (int)(i / a.C4);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 s[3] = {zero, zero, zero};
    for (int p = 0; p < a.nP; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += em_vec(a.part, ((long)b * a.nP + p) * 3 + k, a.C4, q);
    const long row0 = (long)b * (a.H + a.W);
    const f32x4 piv = ld4(at(a.x, (long)b * a.H * a.W, q)) * ld4(at(a.sg, row0, q)) * ld4(at(a.sg, row0 + a.H, q));
    const float n = (float)a.H * (float)a.W;
    f32x4 m2 = s[1] - s[0] * s[0] / n;
    m2.x = fmaxf(m2.x, 0.f); m2.y = fmaxf(m2.y, 0.f); m2.z = fmaxf(m2.z, 0.f); m2.w = fmaxf(m2.w, 0.f);
    float *o = a.stats + (long)b * 3 * a.C4 * 4 + 4 * q;
    st4(o, piv + s[0] / n);
    st4(o + a.C4 * 4, m2);
    st4(o + 2 * a.C4 * 4, s[2] / n);
}

// softmax over the cg values v[j0 .. j0 + cg) (stride 1), the maximum subtracted: the value at j
__device__ __forceinline__ float em_softmax_at(const float *v, int cg, int j) {
    float mx = v[0];
    for (int k = 1; k < cg; ++k) mx = fmaxf(mx, v[k]);
    float den = 0.f;
    for (int k = 0; k < cg; ++k) den += expf(v[k] - mx);
    return expf(v[j] - mx) / den;
}

// one lane per (b, c): vec (B, 4, C) = mean, rstd, x21, x11
__global__ __launch_bounds__(256) void em_vectors_kernel(EmArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int C = a.C4 * 4, cg = a.L * 4;
    if (i >= (long)a.B * C) return;
    const int c = (int)(i % C), b = (int)(i / C), j = c % cg;
    const float *st = a.stats + (long)b * 3 * C;
    float *o = a.vec + (long)b * 4 * C;
    const float n = (float)a.H * (float)a.W;
    o[c] = st[c];
    o[C + c] = 1.0f / sqrtf(st[C + c] / n + a.eps);
    o[2 * C + c] = em_softmax_at(st + 2 * C + (c - j), cg, j);
    o[3 * C + c] = em_softmax_at(a.beta, cg, j);
}

// ------------------------------------------------------------------------------------------------ the gate, forward and backward
template <bool BWD>
__global__ __launch_bounds__(256) void em_gate_kernel(EmArgs a) {
    __shared__ float sred[BWD ? 2 : 1][EM_RU][256];
    __shared__ f32x4 sm[BWD ? 3 : 1][256];
    const int t = threadIdx.x;
    const MapLane l = map_lane(a);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int gb = t - (l.q % a.L);                                // the first lane of this lane's group
    f32x4 mean = zero, rstd = zero, x21 = zero, x11 = zero, gam = zero, bet = zero, sw = zero;
    f32x4 s[3] = {zero, zero, zero};
    const long row0 = (long)l.b * (a.H + a.W);
    if (l.on) {
        mean = em_vec(a.vec, (long)l.b * 4, a.C4, l.q);
        rstd = em_vec(a.vec, (long)l.b * 4 + 1, a.C4, l.q);
        x21 = em_vec(a.vec, (long)l.b * 4 + 2, a.C4, l.q);
        x11 = em_vec(a.vec, (long)l.b * 4 + 3, a.C4, l.q);
        gam = ld4(a.gamma + 4 * (l.q % a.L));
        bet = ld4(a.beta + 4 * (l.q % a.L));
        sw = ld4(at(a.sg, row0 + a.H + l.w, l.q));
    }
    const bool add = BWD ? a.accumulate != 0 : a.res.p != nullptr;
    for (int g = l.h0; g < l.h1; g += EM_RU) {
        f32x4 v[EM_RU], v2[EM_RU], th[EM_RU], d[EM_RU], e[EM_RU];
#pragma unroll
        for (int r = 0; r < EM_RU; ++r) {
            v[r] = v2[r] = th[r] = d[r] = e[r] = zero;
            if (l.on && g + r < l.h1) {
                const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
                v[r] = ld4(at(a.x, pix, l.q));
                v2[r] = ld4(at(a.x2, pix, l.q));
                th[r] = ld4(at(a.sg, row0 + g + r, l.q));
                if (BWD) d[r] = ld4(at(a.y, pix, l.q));
                if (add) e[r] = BWD ? ld4(at(a.dx, pix, l.q)) : ld4(at(a.res, pix, l.q));
            }
        }
#pragma unroll
        for (int r = 0; r < EM_RU; ++r) {
            th[r] = (v[r] * th[r] * sw - mean) * rstd;
            const f32x4 x1 = gam * th[r] + bet;
            sred[0][r][t] = em_sum4(x11 * v2[r] + x21 * x1);
            if (BWD) sred[1][r][t] = em_sum4(d[r] * v[r]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < EM_RU; ++r) {
            if (!(l.on && g + r < l.h1)) continue;
            const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
            float wgt = sred[0][r][gb];
            for (int k = 1; k < a.L; ++k) wgt += sred[0][r][gb + k];
            const float sig = sigmoidf_(wgt);
            if (!BWD) {
                const f32x4 o = v[r] * sig + e[r];
                st4(at_w(a.y, pix, l.q), o);
            } else {
                float dd = sred[1][r][gb];
                for (int k = 1; k < a.L; ++k) dd += sred[1][r][gb + k];
                const float dwgt = dd * (sig * (1.0f - sig));
                const f32x4 o = d[r] * sig + e[r];
                st4(at_w(a.dx, pix, l.q), o);
                st4(at_w(a.dw, pix, l.q), splat4(dwgt));
                s[0] += dwgt * th[r];
                s[1] += splat4(dwgt);
                s[2] += dwgt * v2[r];
            }
        }
        __syncthreads();
    }
    if constexpr (BWD) em_fold_columns<3>(a, l, sm, s);
}

// one lane per (b, quad): the partials in order -> sums (B, 3, C): P, Q, R
__global__ __launch_bounds__(256) void em_sums_finish_kernel(EmArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.B * a.C4) return;
    const int q = (int)(i % a.C4), b = (int)(i / a.C4);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 s[3] = {zero, zero, zero};
    for (int p = 0; p < a.nP; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += em_vec(a.part, ((long)b * a.nP + p) * 3 + k, a.C4, q);
#pragma unroll
    for (int k = 0; k < 3; ++k) st4(a.sums + (((long)b * 3 + k) * a.C4 + q) * 4, s[k]);
}

// one lane per (b, c): bvec (B, 3, C) = c2 (what every pixel of dx2 gets from the softmax over mean x2), mean dx1, mean (dx1 * that)
__global__ __launch_bounds__(256) void em_bwd_vectors_kernel(EmArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int C = a.C4 * 4, cg = a.L * 4;
    if (i >= (long)a.B * C) return;
    const int c = (int)(i % C), b = (int)(i / C), j = c % cg;
    const float *sm = a.sums + (long)b * 3 * C, *x21 = a.vec + (long)b * 4 * C + 2 * C;
    const float n = (float)a.H * (float)a.W;
    // the softmax backward as x21[j] * sum_k x21[k] (s1[j] - s1[k]): no 1 - x21[j] where one mean dominates
    const float s1 = a.gamma[j] * sm[c] + a.beta[j] * sm[C + c];
    float acc = 0.f;
    for (int k = 0; k < cg; ++k) {
        const int ck = c - j + k;
        acc += x21[ck] * (s1 - (a.gamma[k] * sm[ck] + a.beta[k] * sm[C + ck]));
    }
    float *o = a.bvec + (long)b * 3 * C;
    o[c] = x21[c] * acc / n;
    o[C + c] = (x21[c] * sm[C + c]) / n;
    o[2 * C + c] = (x21[c] * sm[c]) / n;
}

// one workgroup: dgamma[j] += sum_(b,gi) x21 P, dbeta[j] += sum_(b,gi) x21 Q + the softmax backward of sum_(b,gi) R over beta.  Lane (s, j) of the
// 256 / cg slices adds the pairs (b, gi) number s, s + S, ... in order; lane (0, j) then adds the slices in order: a fixed order for a given shape
__global__ __launch_bounds__(256) void em_param_grads_kernel(EmArgs a) {
    __shared__ float sg[256], sb[256], sd[256], sx[EM_MAX_CG];
    const int t = threadIdx.x, C = a.C4 * 4, cg = a.L * 4, S = 256 / cg, j = t % cg, sl = t / cg, G = C / cg, n = a.B * G;
    float dg = 0.f, db = 0.f, d11 = 0.f;
    if (sl < S)
        for (int i = sl; i < n; i += S) {
            const int b = i / G, c = (i - b * G) * cg + j;
            const float *sm = a.sums + (long)b * 3 * C, *x21 = a.vec + (long)b * 4 * C + 2 * C;
            dg += x21[c] * sm[c];
            db += x21[c] * sm[C + c];
            d11 += sm[2 * C + c];
        }
    sg[t] = dg; sb[t] = db; sd[t] = d11;
    __syncthreads();
    if (t < cg)
        for (int k = 1; k < S; ++k) { dg += sg[k * cg + t]; db += sb[k * cg + t]; d11 += sd[k * cg + t]; }
    const float x11 = t < cg ? a.vec[3 * C + t] : 0.f;
    __syncthreads();
    if (t < cg) { sd[t] = d11; sx[t] = x11; }
    __syncthreads();
    if (t < cg) {
        float acc = 0.f;                                          // the softmax backward in em_bwd_vectors_kernel's form
        for (int k = 0; k < cg; ++k) acc += sx[k] * (d11 - sd[k]);
        a.dgamma[t] += dg;
        a.dbeta[t] += db + x11 * acc;
    }
}

// ------------------------------------------------------------------------------------------------ the instance-norm backward
__global__ __launch_bounds__(256) void em_norm_bwd_kernel(EmArgs a) {
    __shared__ f32x4 srow[EM_RU][256];
    const int t = threadIdx.x;
    const MapLane l = map_lane(a);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 mean = zero, rstd = zero, x21 = zero, x11 = zero, gam = zero, c2 = zero, k1 = zero, k2 = zero, sw = zero, col = zero;
    const long row0 = (long)l.b * (a.H + a.W);
    if (l.on) {
        mean = em_vec(a.vec, (long)l.b * 4, a.C4, l.q);
        rstd = em_vec(a.vec, (long)l.b * 4 + 1, a.C4, l.q);
        x21 = em_vec(a.vec, (long)l.b * 4 + 2, a.C4, l.q);
        x11 = em_vec(a.vec, (long)l.b * 4 + 3, a.C4, l.q);
        c2 = em_vec(a.bvec, (long)l.b * 3, a.C4, l.q);
        k1 = em_vec(a.bvec, (long)l.b * 3 + 1, a.C4, l.q);
        k2 = em_vec(a.bvec, (long)l.b * 3 + 2, a.C4, l.q);
        gam = ld4(a.gamma + 4 * (l.q % a.L));
        sw = ld4(at(a.sg, row0 + a.H + l.w, l.q));
    }
    for (int g = l.h0; g < l.h1; g += EM_RU) {
        f32x4 v[EM_RU], dwg[EM_RU], sh[EM_RU];
#pragma unroll
        for (int r = 0; r < EM_RU; ++r) {
            v[r] = dwg[r] = sh[r] = zero;
            if (l.on && g + r < l.h1) {
                const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
                v[r] = ld4(at(a.x, pix, l.q));
                dwg[r] = ld4(at(a.dw, pix, l.q));
                sh[r] = ld4(at(a.sg, row0 + g + r, l.q));
            }
        }
#pragma unroll
        for (int r = 0; r < EM_RU; ++r) {
            const f32x4 tt = v[r] * sh[r] * sw;
            const f32x4 th = (tt - mean) * rstd;
            const f32x4 dx1 = dwg[r] * x21;
            const f32x4 dt = rstd * gam * (dx1 - k1 - th * k2);
            const f32x4 u = dt * tt;
            srow[r][t] = u;
            if (l.on && g + r < l.h1) {
                const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
                const f32x4 dx2 = dwg[r] * x11 + c2;
                st4(at_w(a.y, pix, l.q), dt);
                st4(at_w(a.dw, pix, l.q), dx2);
                col += u;
            }
        }
        __syncthreads();
        for (int it = t; it < EM_RU * a.QW; it += 256) {
            const int r = it / a.QW, qq = it - r * a.QW;
            const int q = (blockIdx.z % a.nQc) * 256 + qq;
            if (g + r < l.h1 && q < a.C4) {
                f32x4 s = srow[r][qq];
                for (int k = 1; k < a.NL; ++k) s += srow[r][k * a.QW + qq];
                st4(a.rowpart + (((long)l.b * a.H + g + r) * a.nWc + blockIdx.x) * (4 * a.C4) + 4 * q, s);
            }
        }
        __syncthreads();
    }
    if (l.on) st4(a.colpart + (((long)l.b * a.nHc + blockIdx.y) * a.W + l.w) * (4 * a.C4) + 4 * l.q, col);
}

// one lane per (b, row of the (H + W)-row layout, quad): its partials in order, times (1 - sg): d t / d hw = t (1 - sigmoid(hw))
__global__ __launch_bounds__(256) void em_norm_bwd_finish_kernel(EmArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.B * (a.H + a.W) * a.C4) return;
    const int q = (int)(i % a.C4);
    const long br = i / a.C4;
    const int r = (int)(br % (a.H + a.W)), b = (int)(br / (a.H + a.W));
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (r < a.H) {
        const float *p = a.rowpart + ((long)b * a.H + r) * a.nWc * (4 * a.C4) + 4 * q;
        for (int k = 0; k < a.nWc; ++k) s += ld4(p + (long)k * (4 * a.C4));
    } else {
        const float *p = a.colpart + ((long)b * a.nHc * a.W + (r - a.H)) * (4 * a.C4) + 4 * q;
        for (int k = 0; k < a.nHc; ++k) s += ld4(p + (long)k * a.W * (4 * a.C4));
    }
    const f32x4 d = s * (1.0f - ld4(at(a.sg, br, q)));
    st4(at_w(a.dsg, br, q), d);
}

enum EmOp { EM_STATS, EM_GATE, EM_BWD_GATE, EM_BWD_NORM };

static size_t em_workspace_floats(int B, int H, int W, int C) {
    const MapPlan p = map_plan(B, H, W, C, EM_RU);
    const size_t part = (size_t)B * p.nHc * p.nWc * 3 * C, rc = ((size_t)B * H * p.nWc + (size_t)B * p.nHc * W) * C;
    return part > rc ? part : rc;
}

// checks the descriptor for `op` and fills the kernel arguments; nothing is launched on an error
static int em_unpack(const somi_ema_desc *d, EmOp op, EmArgs &a, MapPlan &p, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->factor > 0 && (long)d->B * d->H * d->W < (1L << 31) &&
                 (long)d->B * (d->H + d->W) * cdiv(d->C, 4) < (1L << 31) && (long)d->B * cdiv(cdiv(d->C, 4), 256) <= 65535 && d->H <= EM_RU * 65535,
                 SOMI_EINVAL, "%s: bad sizes", who);
    const int C = d->C;
    SOMI_REQUIRE(C % d->factor == 0, SOMI_ENOTIMPL, "%s: %d channels do not divide into %d groups", who, C, d->factor);
    const int cg = C / d->factor;
    SOMI_REQUIRE(cg % 4 == 0, SOMI_ENOTIMPL, "%s: %d channels per group: a multiple of 4 is needed", who, cg);
    SOMI_REQUIRE(cg <= EM_MAX_CG, SOMI_ENOTIMPL, "%s: %d channels per group: the group reduction holds at most %d", who, cg, EM_MAX_CG);
    SOMI_REQUIRE(C / 4 <= 256 || 256 % (cg / 4) == 0, SOMI_ENOTIMPL, "%s: %d channels per group do not tile a chunk of 1024 channels", who, cg);
    const somi_slice *maps[] = {&d->x, &d->x2, &d->y, &d->res, &d->dx, &d->dw};
    for (const somi_slice *m : maps)
        SOMI_REQUIRE(!m->p || (long)d->B * d->H * d->W * (m->cs > 0 ? m->cs : 1) <= (1L << 30), SOMI_ENOTIMPL,
                     "%s: a tensor of more than 2^30 floats", who);
    SOMI_REQUIRE_SLICES(who, {"x", d->x.p, d->x.cs, d->x.coff, C}, {"sg", d->sg.p, d->sg.cs, d->sg.coff, C});
    SOMI_REQUIRE(d->gamma && d->beta && d->vec, SOMI_EINVAL, "%s: gamma, beta and vec are required", who);
    if (op == EM_STATS) {
        SOMI_REQUIRE_SLICES(who, {"x2", d->x2.p, d->x2.cs, d->x2.coff, C, kOptional});
        SOMI_REQUIRE(d->stats, SOMI_EINVAL, "%s: stats is required", who);
    }
    if (op == EM_GATE)
        SOMI_REQUIRE_SLICES(who, {"x2", d->x2.p, d->x2.cs, d->x2.coff, C}, {"out", d->y.p, d->y.cs, d->y.coff, C},
                            {"res", d->res.p, d->res.cs, d->res.coff, C, kOptional});
    if (op == EM_BWD_GATE) {
        SOMI_REQUIRE_SLICES(who, {"x2", d->x2.p, d->x2.cs, d->x2.coff, C}, {"dout", d->y.p, d->y.cs, d->y.coff, C},
                            {"dx", d->dx.p, d->dx.cs, d->dx.coff, C}, {"dw", d->dw.p, d->dw.cs, d->dw.coff, C});
        SOMI_REQUIRE(d->sums && d->bvec && d->dgamma && d->dbeta, SOMI_EINVAL, "%s: sums, bvec, dgamma and dbeta are required", who);
    }
    if (op == EM_BWD_NORM) {
        SOMI_REQUIRE_SLICES(who, {"dw", d->dw.p, d->dw.cs, d->dw.coff, C}, {"dt", d->y.p, d->y.cs, d->y.coff, C},
                            {"dsg", d->dsg.p, d->dsg.cs, d->dsg.coff, C});
        SOMI_REQUIRE(d->bvec, SOMI_EINVAL, "%s: bvec is required", who);
    }
    if (op != EM_GATE) {
        SOMI_REQUIRE(d->workspace && aligned16(d->workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
        SOMI_REQUIRE(d->workspace_floats >= em_workspace_floats(d->B, d->H, d->W, C), SOMI_EWORKSPACE, "%s: workspace too small", who);
    }
    p = map_plan(d->B, d->H, d->W, C, EM_RU);
    a = EmArgs{};
    a.x = d->x; a.x2 = d->x2; a.sg = d->sg; a.y = d->y; a.res = d->res;
    a.dx = d->dx; a.dw = d->dw; a.dsg = d->dsg;
    a.gamma = d->gamma; a.beta = d->beta;
    a.stats = d->stats; a.vec = d->vec; a.sums = d->sums; a.bvec = d->bvec; a.dgamma = d->dgamma; a.dbeta = d->dbeta;
    a.part = a.rowpart = d->workspace;
    a.colpart = d->workspace ? d->workspace + (size_t)d->B * d->H * p.nWc * C : nullptr;
    a.eps = d->eps;
    a.accumulate = d->accumulate;
    a.B = d->B; a.H = d->H; a.W = d->W; a.C4 = C / 4; a.L = cg / 4;
    a.QW = p.QW; a.NL = p.NL; a.nQc = p.nQc; a.nWc = p.nWc; a.nHc = p.nHc; a.RH = p.RH; a.nP = p.nHc * p.nWc;
    return 0;
}

static dim3 em_grid(const somi_ema_desc *d, const MapPlan &p) { return dim3(p.nWc, p.nHc, d->B * p.nQc); }

}  // namespace somi

using namespace somi;

extern "C" size_t somi_ema_desc_bytes(void) { return sizeof(somi_ema_desc); }

static bool em_sizes_ok(int B, int H, int W, int C) { return B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0; }

extern "C" size_t somi_ema_workspace_floats(int B, int H, int W, int C) { return em_sizes_ok(B, H, W, C) ? em_workspace_floats(B, H, W, C) : 0; }

extern "C" int somi_ema_partials(int B, int H, int W, int C) {
    if (!em_sizes_ok(B, H, W, C)) return 0;
    const MapPlan p = map_plan(B, H, W, C, EM_RU);
    return p.nHc * p.nWc;
}

extern "C" int somi_ema_stats_nhwc_f32(const somi_ema_desc *d, somi_stream_t stream) {
    EmArgs a;
    MapPlan p;
    if (int rc = em_unpack(d, EM_STATS, a, p, "ema stats")) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(em_stats_kernel, em_grid(d, p), dim3(256), 0, s, a);
    hipLaunchKernelGGL(em_stats_finish_kernel, dim3(cdiv((long)a.B * a.C4, 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(em_vectors_kernel, dim3(cdiv((long)a.B * d->C, 256)), dim3(256), 0, s, a);
    return launch_status("somi_ema_stats_nhwc_f32");
}

extern "C" int somi_ema_gate_nhwc_f32(const somi_ema_desc *d, somi_stream_t stream) {
    EmArgs a;
    MapPlan p;
    if (int rc = em_unpack(d, EM_GATE, a, p, "ema gate")) return rc;
    hipLaunchKernelGGL(em_gate_kernel<false>, em_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_ema_gate_nhwc_f32");
}

extern "C" int somi_ema_bwd_gate_nhwc_f32(const somi_ema_desc *d, somi_stream_t stream) {
    EmArgs a;
    MapPlan p;
    if (int rc = em_unpack(d, EM_BWD_GATE, a, p, "ema bwd gate")) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(em_gate_kernel<true>, em_grid(d, p), dim3(256), 0, s, a);
    hipLaunchKernelGGL(em_sums_finish_kernel, dim3(cdiv((long)a.B * a.C4, 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(em_bwd_vectors_kernel, dim3(cdiv((long)a.B * d->C, 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(em_param_grads_kernel, dim3(1), dim3(256), 0, s, a);
    return launch_status("somi_ema_bwd_gate_nhwc_f32");
}

extern "C" int somi_ema_bwd_norm_nhwc_f32(const somi_ema_desc *d, somi_stream_t stream) {
    EmArgs a;
    MapPlan p;
    if (int rc = em_unpack(d, EM_BWD_NORM, a, p, "ema bwd norm")) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(em_norm_bwd_kernel, em_grid(d, p), dim3(256), 0, s, a);
    hipLaunchKernelGGL(em_norm_bwd_finish_kernel, dim3(cdiv((long)a.B * (a.H + a.W) * a.C4, 256)), dim3(256), 0, s, a);
    return launch_status("somi_ema_bwd_norm_nhwc_f32");
}
