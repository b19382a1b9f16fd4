// ASF-YOLO neck (Zoom_cat, models/common.py:4312-4327; ScalSeq, :4330-4355; attention_model, :4358-4424).  One channel quad per lane, every
// map a channel slice.
//
// Zoom_cat     forward, one kernel: lane (output pixel, quad of the Cl + Cm + Cs output channels); l's quads read the 2x2 window (max, first in
//              row-major order on a tie, + mean) and leave a code byte, m's quads copy, s's quads read (h >> 1, w >> 1).
//              backward, one kernel, owner-computes: a lane per element of dl, dm and ds.
// ScalSeq      the tail behind u_i = conv3d(.) at their own resolutions.  The virtual (B,C,3,H,W) stack holds u3 once, u4 4 times, u5 16 times:
//   stats      a workgroup of 256 = NL pixel lanes x QW quads takes SS_K * NL pixels of the list [u3 | u4 | u5] and leaves the weighted sums
//              of (u - pivot) and (u - pivot)^2, lanes merged by a fixed tree; a second kernel, one workgroup per channel quad, adds the
//              workgroups' rows in double: lane l the rows l, l + 256, ... in order, then the lanes by a fixed tree.
//   fuse       out = max_i leaky(scale u_i + shift), lane (P3 pixel, quad), a code byte per lane.
//   route      lane (4x4 tile of P3, quad): 16 dout / code / u3 reads, 4 u4, 1 u5; writes g3 (16), g4 (4), g5 (1) and, through the same tree,
//              the workgroup's partial of sum g and sum g xhat; a second kernel adds the partials the same way (sums, dgamma, dbeta).
//   apply      du_i = scale (g_i - w_i (m1 + xhat_i m2)) in place, lane (pixel of the list, quad).
// attention    the ECA gate on (B, C); t = x1 gate + x2 with the row and column means of t in the map-pass geometry of common.h (a workgroup
//              takes RH rows x NL columns, a lane walks the rows; row sums through LDS, columns in order; partials, then a fixed-order second
//              kernel); ds = sum dt x1 per (image, channel) in the same geometry; dx1 = dt gate + davg / HW.
// No float atomics: two launches are bit-identical.
#include "common.h"

namespace somi {

__device__ __forceinline__ float as_slope(float v) { return v > 0.f ? 1.f : 0.1f; }

// the sum over the NL lanes of a workgroup, fixed tree: at width s lane l takes lane l + s.  Every thread of the workgroup calls it; the
// result is valid on lane 0.  buf: 256 entries; the caller synchronises before reusing it.
__device__ __forceinline__ f32x4 as_tree(f32x4 v, f32x4 *buf, int t, int lane, int QW, int NL) {
    int top = 1;
    while (top < NL) top *= 2;
    buf[t] = v;
    for (int s = top / 2; s >= 1; s /= 2) {
        __syncthreads();
        if (lane < s && lane + s < NL) {
            v += buf[t + s * QW];
            buf[t] = v;
        }
    }
    return v;
}

// ================================================================================================ Zoom_cat
struct ZcArgs {
    somi_slice l, m, s, out;
    uint8_t *codes;
    int H, W, Hs, Ws, Ql, Qm, Qs;
    int acc_l, acc_m, acc_s;
    long n_l, n_m, n_s;           // backward: lanes per segment
};

__global__ __launch_bounds__(256) void zc_fwd_kernel(ZcArgs a, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Q = a.Ql + a.Qm + a.Qs;
    const int q = (int)(i % Q);
    const long pix = i / Q;
    const int w = (int)(pix % a.W);
    const long bh = pix / a.W;
    const int h = (int)(bh % a.H);
    const long b = bh / a.H;
    float *o = at_w(a.out, pix, q);
    if (q < a.Ql) {
        const long p00 = (b * 2 * a.H + 2 * h) * (2L * a.W) + 2 * w;
        f32x4 v[4];
        v[0] = ld4(at(a.l, p00, q));
        v[1] = ld4(at(a.l, p00 + 1, q));
        v[2] = ld4(at(a.l, p00 + 2L * a.W, q));
        v[3] = ld4(at(a.l, p00 + 2L * a.W + 1, q));
        f32x4 r;
        unsigned code = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float mx = v[0][j];
            unsigned best = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k][j] > mx) { mx = v[k][j]; best = k; }     // strictly greater: the first pixel in row-major order keeps a tie
            r[j] = mx + 0.25f * (v[0][j] + v[1][j] + v[2][j] + v[3][j]);
            code |= best << (2 * j);
        }
        st4(o, r);
        if (a.codes) a.codes[pix * a.Ql + q] = (uint8_t)code;
    } else if (q < a.Ql + a.Qm) {
        if (a.m.p) st4(o, ld4(at(a.m, pix, q - a.Ql)));
    } else {
        const long ps = (b * a.Hs + (h >> 1)) * a.Ws + (w >> 1);
        st4(o, ld4(at(a.s, ps, q - a.Ql - a.Qm)));
    }
}

__global__ __launch_bounds__(256) void zc_bwd_kernel(ZcArgs a, long total) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (i < a.n_l) {                                              // dl: (b, y, x, q) of the (B,2H,2W) map
        const int q = (int)(i % a.Ql);
        const long pl = i / a.Ql;
        const int x = (int)(pl % (2 * a.W));
        const long by = pl / (2 * a.W);
        const int y = (int)(by % (2 * a.H));
        const long b = by / (2 * a.H);
        const long pix = (b * a.H + (y >> 1)) * a.W + (x >> 1);
        const f32x4 d = ld4(at(a.out, pix, q));
        const unsigned code = a.codes[pix * a.Ql + q], pos = (unsigned)((y & 1) * 2 + (x & 1));
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = d[j] * (0.25f + (((code >> (2 * j)) & 3u) == pos ? 1.f : 0.f));
        float *o = at_w(a.l, pl, q);
        if (a.acc_l) r += ld4(o);
        st4(o, r);
        return;
    }
    i -= a.n_l;
    if (i < a.n_m) {                                              // dm = dout's middle slice
        const int q = (int)(i % a.Qm);
        const long pix = i / a.Qm;
        f32x4 r = ld4(at(a.out, pix, a.Ql + q));
        float *o = at_w(a.m, pix, q);
        if (a.acc_m) r += ld4(o);
        st4(o, r);
        return;
    }
    i -= a.n_m;                                                   // ds: the children that exist, in row-major order
    const int q = (int)(i % a.Qs);
    const long ps = i / a.Qs;
    const int ws = (int)(ps % a.Ws);
    const long bh = ps / a.Ws;
    const int hs = (int)(bh % a.Hs);
    const long b = bh / a.Hs;
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    for (int di = 0; di < 2; ++di)
        for (int dj = 0; dj < 2; ++dj) {
            const int h = 2 * hs + di, w = 2 * ws + dj;
            if (h < a.H && w < a.W) r += ld4(at(a.out, (b * a.H + h) * a.W + w, a.Ql + a.Qm + q));
        }
    float *o = at_w(a.s, ps, q);
    if (a.acc_s) r += ld4(o);
    st4(o, r);
}

static int zc_unpack(const somi_zoomcat_desc *d, bool bwd, ZcArgs &a, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Cl > 0 && d->Cm > 0 && d->Cs > 0 && d->Cl % 4 == 0 && d->Cm % 4 == 0 && d->Cs % 4 == 0 &&
                 4L * d->B * d->H * d->W < (1L << 31),
                 SOMI_EINVAL, "%s: bad sizes (Cl, Cm, Cs multiples of 4, fewer than 2^31 pixels in l)", who);
    const int Ct = d->Cl + d->Cm + d->Cs;
    SOMI_REQUIRE_SLICES(who, {bwd ? "dout" : "out", d->out.p, d->out.cs, d->out.coff, Ct});
    if (!bwd) {
        SOMI_REQUIRE_SLICES(who, {"l", d->l.p, d->l.cs, d->l.coff, d->Cl}, {"m", d->m.p, d->m.cs, d->m.coff, d->Cm, kOptional},
                            {"s", d->s.p, d->s.cs, d->s.coff, d->Cs});
    } else {
        SOMI_REQUIRE_SLICES(who, {"dl", d->l.p, d->l.cs, d->l.coff, d->Cl, kOptional}, {"dm", d->m.p, d->m.cs, d->m.coff, d->Cm, kOptional},
                            {"ds", d->s.p, d->s.cs, d->s.coff, d->Cs, kOptional});
        SOMI_REQUIRE(!d->l.p || d->codes, SOMI_EINVAL, "%s: dl needs the forward's codes", who);
    }
    a = ZcArgs{};
    a.l = d->l; a.m = d->m; a.s = d->s; a.out = d->out;
    a.codes = d->codes;
    a.H = d->H; a.W = d->W; a.Hs = (d->H + 1) / 2; a.Ws = (d->W + 1) / 2;
    a.Ql = d->Cl / 4; a.Qm = d->Cm / 4; a.Qs = d->Cs / 4;
    a.acc_l = d->accumulate[0]; a.acc_m = d->accumulate[1]; a.acc_s = d->accumulate[2];
    const long npix = (long)d->B * d->H * d->W;
    a.n_l = d->l.p ? 4 * npix * a.Ql : 0;
    a.n_m = d->m.p ? npix * a.Qm : 0;
    a.n_s = d->s.p ? (long)d->B * a.Hs * a.Ws * a.Qs : 0;
    return 0;
}

// ================================================================================================ ScalSeq
constexpr int SS_K = 16;          // pixels a lane of the statistics kernel sums

struct SsArgs {
    somi_slice u[3], out, g[3];
    uint8_t *codes;
    const float *gamma, *beta;
    float *mean, *rstd, *scale, *shift, *rm, *rv, *sums, *dgamma, *dbeta, *part;
    int B, H, W, C4, QW, NL, nQc;
    long n3, n4, n5;              // pixels of the three maps
    int nparts;
    float eps, momentum;
};

// pixel p of the list [u3 | u4 | u5] -> (map, pixel inside it)
__device__ __forceinline__ int ss_map(const SsArgs &a, long &p) {
    if (p < a.n3) return 0;
    p -= a.n3;
    if (p < a.n4) return 1;
    p -= a.n4;
    return 2;
}

__global__ __launch_bounds__(256) void ss_stats_kernel(SsArgs a) {
    __shared__ f32x4 buf[256];
    const int t = threadIdx.x, lane = t / a.QW, q = blockIdx.y * 256 + (t - lane * a.QW);
    const bool on = lane < a.NL && q < a.C4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 s1 = zero, s2 = zero, piv = zero;
    if (on && a.rm) piv = ld4(a.rm + 4 * q);
    const long total = a.n3 + a.n4 + a.n5;
    const long p0 = (long)blockIdx.x * (SS_K * a.NL) + lane;
    f32x4 v[SS_K];
    float wgt[SS_K];
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
        long p = p0 + (long)k * a.NL;
        v[k] = piv;
        wgt[k] = 0.f;
        if (on && p < total) {
            const int mp = ss_map(a, p);
            v[k] = ld4(at(a.u[mp], p, q));
            wgt[k] = mp == 0 ? 1.f : (mp == 1 ? 4.f : 16.f);
        }
    }
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
        const f32x4 dlt = v[k] - piv;
        s1 += wgt[k] * dlt;
        s2 += wgt[k] * dlt * dlt;
    }
    s1 = as_tree(s1, buf, t, lane, a.QW, a.NL);
    __syncthreads();
    s2 = as_tree(s2, buf, t, lane, a.QW, a.NL);
    if (on && lane == 0) {
        float *dst = a.part + (long)blockIdx.x * 2 * (4 * a.C4) + 4 * q;
        st4(dst, s1);
        st4(dst + 4 * a.C4, s2);
    }
}

// the sum of the workgroups' partial rows [nparts][2][C] for the channel quad blockIdx.x, in double: lane l adds the rows l, l + 256, ... in
// order, then the 256 lanes by a fixed tree.  Valid on thread 0.
__device__ __forceinline__ void ss_sum_parts(const SsArgs &a, double (&s1)[4], double (&s2)[4]) {
    __shared__ double sh[8][256];
    const int t = threadIdx.x, q = blockIdx.x;
    for (int j = 0; j < 4; ++j) s1[j] = s2[j] = 0.0;
    for (int k = t; k < a.nparts; k += 256) {
        const float *src = a.part + (long)k * 2 * (4 * a.C4) + 4 * q;
        const f32x4 v1 = ld4(src), v2 = ld4(src + 4 * a.C4);
        for (int j = 0; j < 4; ++j) { s1[j] += (double)v1[j]; s2[j] += (double)v2[j]; }
    }
    for (int j = 0; j < 4; ++j) { sh[j][t] = s1[j]; sh[4 + j][t] = s2[j]; }
    for (int s = 128; s >= 1; s /= 2) {
        __syncthreads();
        if (t < s)
            for (int j = 0; j < 8; ++j) sh[j][t] += sh[j][t + s];
    }
    for (int j = 0; j < 4; ++j) { s1[j] = sh[j][0]; s2[j] = sh[4 + j][0]; }
}

__global__ __launch_bounds__(256) void ss_stats_finish_kernel(SsArgs a) {
    double s1[4], s2[4];
    ss_sum_parts(a, s1, s2);
    if (threadIdx.x != 0) return;
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * blockIdx.x + j;
        const double N = 3.0 * (double)a.n3, piv = a.rm ? (double)a.rm[c] : 0.0;
        const double m = s1[j] / N;
        double var = s2[j] / N - m * m;
        if (var < 0.0) var = 0.0;
        const double mean = piv + m;
        const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
        const float sc = a.gamma[c] * rstd;
        a.mean[c] = (float)mean;
        a.rstd[c] = rstd;
        a.scale[c] = sc;
        a.shift[c] = a.beta[c] - (float)mean * sc;
        if (a.rm) a.rm[c] = (float)((1.0 - (double)a.momentum) * piv + (double)a.momentum * mean);
        if (a.rv) a.rv[c] = (float)((1.0 - (double)a.momentum) * (double)a.rv[c] + (double)a.momentum * var * (N / (N - 1.0)));
    }
}

__global__ __launch_bounds__(256) void ss_fuse_kernel(SsArgs a, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % a.C4);
    const long pix = i / a.C4;
    const int w = (int)(pix % a.W);
    const long bh = pix / a.W;
    const int h = (int)(bh % a.H);
    const long b = bh / a.H;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (a.scale) { sc = ld4(a.scale + 4 * q); sh = ld4(a.shift + 4 * q); }
    f32x4 v[3];
    v[0] = ld4(at(a.u[0], pix, q));
    v[1] = ld4(at(a.u[1], (b * (a.H / 2) + (h >> 1)) * (a.W / 2) + (w >> 1), q));
    v[2] = ld4(at(a.u[2], (b * (a.H / 4) + (h >> 2)) * (a.W / 4) + (w >> 2), q));
    f32x4 r;
    unsigned code = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float mx = apply_act<SOMI_ACT_LEAKY>(sc[j] * v[0][j] + sh[j]);
        unsigned best = 0;
#pragma unroll
        for (int k = 1; k < 3; ++k) {
            const float z = apply_act<SOMI_ACT_LEAKY>(sc[j] * v[k][j] + sh[j]);
            if (z > mx) { mx = z; best = k; }                     // strictly greater: the first depth index keeps a tie
        }
        r[j] = mx;
        code |= best << (2 * j);
    }
    st4(at_w(a.out, pix, q), r);
    if (a.codes) a.codes[pix * a.C4 + q] = (uint8_t)code;
}

__global__ __launch_bounds__(256) void ss_route_kernel(SsArgs a, long tiles) {
    __shared__ f32x4 buf[256];
    const int t = threadIdx.x, lane = t / a.QW, q = blockIdx.y * 256 + (t - lane * a.QW);
    const long tile = (long)blockIdx.x * a.NL + lane;
    const bool on = lane < a.NL && q < a.C4 && tile < tiles;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 sg = zero, sgx = zero;
    if (on) {
        const int H4 = a.H / 4, W4 = a.W / 4, H2 = a.H / 2, W2 = a.W / 2;
        const int tx = (int)(tile % W4);
        const long bt = tile / W4;
        const int ty = (int)(bt % H4);
        const long b = bt / H4;
        const f32x4 sc = ld4(a.scale + 4 * q), sh = ld4(a.shift + 4 * q), mu = ld4(a.mean + 4 * q), rs = ld4(a.rstd + 4 * q);
        const long p5 = (b * H4 + ty) * W4 + tx;
        const f32x4 u5 = ld4(at(a.u[2], p5, q));
        f32x4 g5 = zero;
        for (int cy = 0; cy < 2; ++cy)
            for (int cx = 0; cx < 2; ++cx) {
                const long p4 = (b * H2 + 2 * ty + cy) * W2 + 2 * tx + cx;
                const f32x4 u4 = ld4(at(a.u[1], p4, q));
                f32x4 g4 = zero;
                f32x4 d[4], u3[4];
                unsigned code[4];
                long p3[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    p3[k] = (b * a.H + 4 * ty + 2 * cy + (k >> 1)) * a.W + 4 * tx + 2 * cx + (k & 1);
                    d[k] = ld4(at(a.out, p3[k], q));
                    u3[k] = ld4(at(a.u[0], p3[k], q));
                    code[k] = a.codes[p3[k] * a.C4 + q];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    f32x4 g3;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned sel = (code[k] >> (2 * j)) & 3u;
                        g3[j] = sel == 0 ? d[k][j] * as_slope(sc[j] * u3[k][j] + sh[j]) : 0.f;
                        g4[j] += sel == 1 ? d[k][j] : 0.f;
                        g5[j] += sel == 2 ? d[k][j] : 0.f;
                    }
                    st4(at_w(a.g[0], p3[k], q), g3);
                    sg += g3;
                    sgx += g3 * ((u3[k] - mu) * rs);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) g4[j] *= as_slope(sc[j] * u4[j] + sh[j]);
                st4(at_w(a.g[1], p4, q), g4);
                sg += g4;
                sgx += g4 * ((u4 - mu) * rs);
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) g5[j] *= as_slope(sc[j] * u5[j] + sh[j]);
        st4(at_w(a.g[2], p5, q), g5);
        sg += g5;
        sgx += g5 * ((u5 - mu) * rs);
    }
    sg = as_tree(sg, buf, t, lane, a.QW, a.NL);
    __syncthreads();
    sgx = as_tree(sgx, buf, t, lane, a.QW, a.NL);
    if (lane == 0 && q < a.C4) {
        float *dst = a.part + (long)blockIdx.x * 2 * (4 * a.C4) + 4 * q;
        st4(dst, sg);
        st4(dst + 4 * a.C4, sgx);
    }
}

__global__ __launch_bounds__(256) void ss_route_finish_kernel(SsArgs a) {
    double s1[4], s2[4];
    ss_sum_parts(a, s1, s2);
    if (threadIdx.x != 0) return;
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * blockIdx.x + j;
        a.sums[c] = (float)s1[j];
        a.sums[4 * a.C4 + c] = (float)s2[j];
        if (a.dbeta) a.dbeta[c] += (float)s1[j];
        if (a.dgamma) a.dgamma[c] += (float)s2[j];
    }
}

__global__ __launch_bounds__(256) void ss_apply_kernel(SsArgs a, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % a.C4);
    long p = i / a.C4;
    const int mp = ss_map(a, p);
    const float wgt = mp == 0 ? 1.f : (mp == 1 ? 4.f : 16.f);
    const float invN = 1.0f / (3.0f * (float)a.n3);
    const f32x4 sc = ld4(a.scale + 4 * q), mu = ld4(a.mean + 4 * q), rs = ld4(a.rstd + 4 * q);
    const f32x4 m1 = ld4(a.sums + 4 * q) * invN, m2 = ld4(a.sums + 4 * a.C4 + 4 * q) * invN;
    const f32x4 xh = (ld4(at(a.u[mp], p, q)) - mu) * rs;
    float *g = at_w(a.g[mp], p, q);
    st4(g, sc * (ld4(g) - wgt * (m1 + xh * m2)));
}

enum SsOp { SS_STATS, SS_FUSE, SS_ROUTE, SS_APPLY };

static int ss_nparts(SsOp op, int B, int H, int W, const MapShape &g) {
    const long n3 = (long)B * H * W;
    if (op == SS_STATS) return cdiv(n3 + n3 / 4 + n3 / 16, (long)SS_K * g.NL);
    return cdiv(n3 / 16, g.NL);
}

static int ss_unpack(const somi_scalseq_desc *d, SsOp op, SsArgs &a, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C % 4 == 0 && d->H % 4 == 0 && d->W % 4 == 0 &&
                 2L * d->B * d->H * d->W < (1L << 31) && cdiv(d->C / 4, 256) <= 65535,
                 SOMI_EINVAL, "%s: bad sizes (C, H and W multiples of 4, fewer than 2^30 pixels)", who);
    const int C = d->C;
    SOMI_REQUIRE_SLICES(who, {"u3", d->u3.p, d->u3.cs, d->u3.coff, C}, {"u4", d->u4.p, d->u4.cs, d->u4.coff, C},
                        {"u5", d->u5.p, d->u5.cs, d->u5.coff, C});
    if (op == SS_FUSE || op == SS_ROUTE) SOMI_REQUIRE_SLICES(who, {op == SS_FUSE ? "out" : "dout", d->out.p, d->out.cs, d->out.coff, C});
    if (op == SS_ROUTE || op == SS_APPLY)
        SOMI_REQUIRE_SLICES(who, {"g3", d->g3.p, d->g3.cs, d->g3.coff, C}, {"g4", d->g4.p, d->g4.cs, d->g4.coff, C},
                            {"g5", d->g5.p, d->g5.cs, d->g5.coff, C});
    if (op == SS_STATS) SOMI_REQUIRE(d->gamma && d->beta && d->eps > 0.f, SOMI_EINVAL, "%s: gamma, beta and a positive eps are required", who);
    if (op == SS_FUSE) {
        SOMI_REQUIRE(!d->scale == !d->shift, SOMI_EINVAL, "%s: scale and shift come together", who);
        SOMI_REQUIRE(!d->scale || (aligned16(d->scale) && aligned16(d->shift)), SOMI_EINVAL, "%s: scale and shift must be 16-byte aligned", who);
    } else {
        SOMI_REQUIRE(d->mean && d->rstd && d->scale && d->shift && aligned16(d->mean) && aligned16(d->rstd) && aligned16(d->scale) &&
                     aligned16(d->shift), SOMI_EINVAL, "%s: mean, rstd, scale and shift (C floats, 16-byte aligned) are required", who);
    }
    SOMI_REQUIRE(!d->running_mean || aligned16(d->running_mean), SOMI_EINVAL, "%s: running_mean must be 16-byte aligned", who);
    if (op == SS_ROUTE) SOMI_REQUIRE(d->codes, SOMI_EINVAL, "%s: the forward's codes are required", who);
    if (op == SS_ROUTE || op == SS_APPLY)
        SOMI_REQUIRE(d->sums && aligned16(d->sums), SOMI_EINVAL, "%s: sums (2, C), 16-byte aligned, is required", who);
    if (op == SS_STATS || op == SS_ROUTE) {
        SOMI_REQUIRE(d->workspace && aligned16(d->workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
        SOMI_REQUIRE(d->workspace_floats >= somi_scalseq_workspace_floats(d->B, d->H, d->W, C), SOMI_EWORKSPACE, "%s: workspace too small", who);
    }
    const MapShape g = map_shape(C);
    a = SsArgs{};
    a.u[0] = d->u3; a.u[1] = d->u4; a.u[2] = d->u5;
    a.out = d->out;
    a.g[0] = d->g3; a.g[1] = d->g4; a.g[2] = d->g5;
    a.codes = d->codes;
    a.gamma = d->gamma; a.beta = d->beta;
    a.mean = d->mean; a.rstd = d->rstd; a.scale = d->scale; a.shift = d->shift;
    a.rm = d->running_mean; a.rv = d->running_var;
    a.sums = d->sums; a.dgamma = d->dgamma; a.dbeta = d->dbeta; a.part = d->workspace;
    a.B = d->B; a.H = d->H; a.W = d->W; a.C4 = C / 4;
    a.QW = g.QW; a.NL = g.NL; a.nQc = g.nQc;
    a.n3 = (long)d->B * d->H * d->W; a.n4 = a.n3 / 4; a.n5 = a.n3 / 16;
    a.nparts = (op == SS_STATS || op == SS_ROUTE) ? ss_nparts(op, d->B, d->H, d->W, g) : 0;
    a.eps = d->eps; a.momentum = d->momentum;
    return 0;
}

// ================================================================================================ attention_model
constexpr int ECA_KMAX = 9;

__global__ __launch_bounds__(256) void eca_fwd_kernel(const float *avg, const float *w, int k, float *gate, int B, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * C) return;
    const int c = (int)(i % C);
    const float *row = avg + (i - c);
    float s = 0.f;
    for (int j = 0; j < k; ++j) {
        const int cc = c + j - k / 2;
        if (cc >= 0 && cc < C) s += w[j] * row[cc];
    }
    gate[i] = sigmoidf_(s);
}

__global__ __launch_bounds__(256) void eca_davg_kernel(const float *w, int k, const float *gate, const float *dgate, float *davg, int B, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * C) return;
    const int c = (int)(i % C);
    const long r0 = i - c;
    float s = 0.f;
    for (int j = 0; j < k; ++j) {
        const int cc = c - j + k / 2;
        if (cc >= 0 && cc < C) {
            const float g = gate[r0 + cc];
            s += w[j] * dgate[r0 + cc] * g * (1.f - g);
        }
    }
    davg[i] = s;
}

// one workgroup: thread t takes the elements t, t + 256, ... in order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void eca_dw_kernel(const float *avg, int k, const float *gate, const float *dgate, float *dw, int B, int C) {
    __shared__ float buf[ECA_KMAX][256];
    const int t = threadIdx.x;
    float acc[ECA_KMAX];
#pragma unroll
    for (int j = 0; j < ECA_KMAX; ++j) acc[j] = 0.f;
    const long n = (long)B * C;
    for (long i = t; i < n; i += 256) {
        const int c = (int)(i % C);
        const long r0 = i - c;
        const float g = gate[i], dz = dgate[i] * g * (1.f - g);
#pragma unroll
        for (int j = 0; j < ECA_KMAX; ++j) {
            const int cc = c + j - k / 2;
            if (j < k && cc >= 0 && cc < C) acc[j] += dz * avg[r0 + cc];
        }
    }
#pragma unroll
    for (int j = 0; j < ECA_KMAX; ++j) buf[j][t] = acc[j];
    for (int s = 128; s >= 1; s /= 2) {
        __syncthreads();
        if (t < s) {
#pragma unroll
            for (int j = 0; j < ECA_KMAX; ++j) buf[j][t] += buf[j][t + s];
        }
    }
    if (t < k) dw[t] = buf[t][0];
}

constexpr int AM_RU = 4;          // rows in flight per lane

struct AmArgs {
    somi_slice x1, x2, t, pool, dx1;
    const float *gate, *davg;
    float *ds, *rowpart, *colpart;
    int accumulate;
    int B, H, W, C4, QW, NL, nQc, nWc, nHc, RH;
};

// t = x1 gate + x2 written; row partials [B][H][nWc][C], column partials [B][nHc][W][C]
__global__ __launch_bounds__(256) void am_mix_kernel(AmArgs a) {
    __shared__ f32x4 srow[AM_RU][256];
    const int t = threadIdx.x;
    const MapLane l = map_lane(a);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 col = zero, gt = zero;
    if (l.on) gt = ld4(a.gate + (long)l.b * (4 * a.C4) + 4 * l.q);
    for (int g = l.h0; g < l.h1; g += AM_RU) {
        f32x4 v1[AM_RU], v2[AM_RU];
#pragma unroll
        for (int r = 0; r < AM_RU; ++r) {
            v1[r] = v2[r] = zero;
            if (l.on && g + r < l.h1) {
                const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
                v1[r] = ld4(at(a.x1, pix, l.q));
                v2[r] = ld4(at(a.x2, pix, l.q));
            }
        }
#pragma unroll
        for (int r = 0; r < AM_RU; ++r) {
            const f32x4 m = v1[r] * gt + v2[r];
            if (l.on && g + r < l.h1) st4(at_w(a.t, ((long)l.b * a.H + g + r) * a.W + l.w, l.q), m);
            col += m;
            srow[r][t] = m;
        }
        __syncthreads();
        for (int it = t; it < AM_RU * a.QW; it += 256) {          // the row sums over this workgroup's columns, columns in order
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

__global__ __launch_bounds__(256) void am_mix_finish_kernel(AmArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.B * (a.H + a.W) * a.C4) return;
    const int q = (int)(i % a.C4);
    const long br = i / a.C4;
    const int r = (int)(br % (a.H + a.W)), b = (int)(br / (a.H + a.W));
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (r < a.H) {
        const float *p = a.rowpart + ((long)b * a.H + r) * a.nWc * (4 * a.C4) + 4 * q;
        for (int k = 0; k < a.nWc; ++k) s += ld4(p + (long)k * (4 * a.C4));
        s = s / (float)a.W;
    } else {
        const float *p = a.colpart + ((long)b * a.nHc * a.W + (r - a.H)) * (4 * a.C4) + 4 * q;
        for (int k = 0; k < a.nHc; ++k) s += ld4(p + (long)k * a.W * (4 * a.C4));
        s = s / (float)a.H;
    }
    st4(at_w(a.pool, br, q), s);
}

// ds partials [B][nHc][nWc][C]: a lane's rows in order, then the workgroup's columns by the fixed tree
__global__ __launch_bounds__(256) void am_sums_kernel(AmArgs a) {
    __shared__ f32x4 buf[256];
    const int t = threadIdx.x;
    const MapLane l = map_lane(a);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc = zero;
    for (int g = l.h0; g < l.h1; g += AM_RU) {
        f32x4 v1[AM_RU], dt[AM_RU];
#pragma unroll
        for (int r = 0; r < AM_RU; ++r) {
            v1[r] = dt[r] = zero;
            if (l.on && g + r < l.h1) {
                const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
                v1[r] = ld4(at(a.x1, pix, l.q));
                dt[r] = ld4(at(a.t, pix, l.q));
            }
        }
#pragma unroll
        for (int r = 0; r < AM_RU; ++r) acc += v1[r] * dt[r];
    }
    acc = as_tree(acc, buf, t, l.lane, a.QW, a.NL);
    if (l.lane == 0 && l.q < a.C4)
        st4(a.rowpart + (((long)l.b * a.nHc + blockIdx.y) * a.nWc + blockIdx.x) * (4 * a.C4) + 4 * l.q, acc);
}

__global__ __launch_bounds__(256) void am_sums_finish_kernel(AmArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.B * a.C4) return;
    const int q = (int)(i % a.C4);
    const long b = i / a.C4;
    const int n = a.nHc * a.nWc;
    const float *p = a.rowpart + b * n * (4 * a.C4) + 4 * q;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < n; ++k) s += ld4(p + (long)k * (4 * a.C4));
    st4(a.ds + b * (4 * a.C4) + 4 * q, s);
}

__global__ __launch_bounds__(256) void am_input_kernel(AmArgs a, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % a.C4);
    const long pix = i / a.C4;
    const long b = pix / ((long)a.H * a.W);
    const f32x4 gt = ld4(a.gate + b * (4 * a.C4) + 4 * q), da = ld4(a.davg + b * (4 * a.C4) + 4 * q);
    f32x4 r = ld4(at(a.t, pix, q)) * gt + da / (float)(a.H * a.W);
    float *o = at_w(a.dx1, pix, q);
    if (a.accumulate) r += ld4(o);
    st4(o, r);
}

enum AmOp { AM_MIX, AM_SUMS, AM_INPUT };

static int am_unpack(const somi_asfatt_desc *d, AmOp op, AmArgs &a, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C % 4 == 0 && (long)d->B * d->H * d->W < (1L << 31) &&
                 (long)d->B * (d->H + d->W) * (d->C / 4) < (1L << 31) && (long)d->B * cdiv(d->C / 4, 256) <= 65535 && d->H <= AM_RU * 65535,
                 SOMI_EINVAL, "%s: bad sizes (C a multiple of 4, fewer than 2^31 pixels)", who);
    const int C = d->C;
    if (op == AM_MIX)
        SOMI_REQUIRE_SLICES(who, {"x1", d->x1.p, d->x1.cs, d->x1.coff, C}, {"x2", d->x2.p, d->x2.cs, d->x2.coff, C},
                            {"t", d->t.p, d->t.cs, d->t.coff, C}, {"pool", d->pool.p, d->pool.cs, d->pool.coff, C});
    if (op == AM_SUMS) SOMI_REQUIRE_SLICES(who, {"x1", d->x1.p, d->x1.cs, d->x1.coff, C}, {"dt", d->t.p, d->t.cs, d->t.coff, C});
    if (op == AM_INPUT) SOMI_REQUIRE_SLICES(who, {"dt", d->t.p, d->t.cs, d->t.coff, C}, {"dx1", d->dx1.p, d->dx1.cs, d->dx1.coff, C});
    if (op == AM_MIX || op == AM_INPUT) SOMI_REQUIRE(d->gate && aligned16(d->gate), SOMI_EINVAL, "%s: gate (B, C), 16-byte aligned, is required", who);
    if (op == AM_SUMS) SOMI_REQUIRE(d->ds && aligned16(d->ds), SOMI_EINVAL, "%s: ds (B, C), 16-byte aligned, is required", who);
    if (op == AM_INPUT) SOMI_REQUIRE(d->davg && aligned16(d->davg), SOMI_EINVAL, "%s: davg (B, C), 16-byte aligned, is required", who);
    if (op == AM_MIX || op == AM_SUMS) {
        SOMI_REQUIRE(d->workspace && aligned16(d->workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
        SOMI_REQUIRE(d->workspace_floats >= somi_asfatt_workspace_floats(d->B, d->H, d->W, C), SOMI_EWORKSPACE, "%s: workspace too small", who);
    }
    const MapPlan p = map_plan(d->B, d->H, d->W, C, AM_RU);
    a = AmArgs{};
    a.x1 = d->x1; a.x2 = d->x2; a.t = d->t; a.pool = d->pool; a.dx1 = d->dx1;
    a.gate = d->gate; a.davg = d->davg; a.ds = d->ds;
    a.rowpart = d->workspace;
    a.colpart = d->workspace ? d->workspace + (size_t)d->B * d->H * p.nWc * C : nullptr;
    a.accumulate = d->accumulate;
    a.B = d->B; a.H = d->H; a.W = d->W; a.C4 = C / 4;
    a.QW = p.QW; a.NL = p.NL; a.nQc = p.nQc; a.nWc = p.nWc; a.nHc = p.nHc; a.RH = p.RH;
    return 0;
}

static int eca_check(const float *avg, const float *w, int k, const float *gate, int B, int C, const char *who) {
    SOMI_REQUIRE(avg && w && gate, SOMI_EINVAL, "%s: avg, w and gate are required", who);
    SOMI_REQUIRE(B > 0 && C > 0 && (long)B * C < (1L << 31), SOMI_EINVAL, "%s: bad sizes", who);
    SOMI_REQUIRE(k >= 1 && k % 2 == 1 && k <= ECA_KMAX, SOMI_ENOTIMPL, "%s: the kernel size must be odd and at most %d, got %d", who, ECA_KMAX, k);
    return 0;
}

}  // namespace somi

using namespace somi;

extern "C" size_t somi_zoomcat_desc_bytes(void) { return sizeof(somi_zoomcat_desc); }
extern "C" size_t somi_scalseq_desc_bytes(void) { return sizeof(somi_scalseq_desc); }
extern "C" size_t somi_asfatt_desc_bytes(void) { return sizeof(somi_asfatt_desc); }

extern "C" int somi_zoomcat_nhwc_f32(const somi_zoomcat_desc *d, somi_stream_t stream) {
    ZcArgs a;
    if (int rc = zc_unpack(d, false, a, "zoomcat")) return rc;
    const long total = (long)d->B * d->H * d->W * (a.Ql + a.Qm + a.Qs);
    SOMI_REQUIRE(cdiv(total, 256) > 0 && total < (1L << 39), SOMI_EINVAL, "zoomcat: too many elements");
    hipLaunchKernelGGL(zc_fwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a, total);
    return launch_status("somi_zoomcat_nhwc_f32");
}

extern "C" int somi_zoomcat_bwd_nhwc_f32(const somi_zoomcat_desc *d, somi_stream_t stream) {
    ZcArgs a;
    if (int rc = zc_unpack(d, true, a, "zoomcat bwd")) return rc;
    const long total = a.n_l + a.n_m + a.n_s;
    if (total == 0) return 0;
    SOMI_REQUIRE(total < (1L << 39), SOMI_EINVAL, "zoomcat bwd: too many elements");
    hipLaunchKernelGGL(zc_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a, total);
    return launch_status("somi_zoomcat_bwd_nhwc_f32");
}

extern "C" size_t somi_scalseq_workspace_floats(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || H % 4 || W % 4) return 0;
    const MapShape g = map_shape(C);
    const int n = ss_nparts(SS_STATS, B, H, W, g), m = ss_nparts(SS_ROUTE, B, H, W, g);
    return (size_t)(n > m ? n : m) * 2 * C;
}

extern "C" int somi_scalseq_stats_f32(const somi_scalseq_desc *d, somi_stream_t stream) {
    SsArgs a;
    if (int rc = ss_unpack(d, SS_STATS, a, "scalseq stats")) return rc;
    hipLaunchKernelGGL(ss_stats_kernel, dim3(a.nparts, a.nQc), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(ss_stats_finish_kernel, dim3(a.C4), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_scalseq_stats_f32");
}

extern "C" int somi_scalseq_fuse_nhwc_f32(const somi_scalseq_desc *d, somi_stream_t stream) {
    SsArgs a;
    if (int rc = ss_unpack(d, SS_FUSE, a, "scalseq fuse")) return rc;
    const long total = a.n3 * a.C4;
    hipLaunchKernelGGL(ss_fuse_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a, total);
    return launch_status("somi_scalseq_fuse_nhwc_f32");
}

extern "C" int somi_scalseq_route_bwd_nhwc_f32(const somi_scalseq_desc *d, somi_stream_t stream) {
    SsArgs a;
    if (int rc = ss_unpack(d, SS_ROUTE, a, "scalseq route bwd")) return rc;
    hipLaunchKernelGGL(ss_route_kernel, dim3(a.nparts, a.nQc), dim3(256), 0, (hipStream_t)stream, a, a.n5);
    hipLaunchKernelGGL(ss_route_finish_kernel, dim3(a.C4), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_scalseq_route_bwd_nhwc_f32");
}

extern "C" int somi_scalseq_apply_bwd_f32(const somi_scalseq_desc *d, somi_stream_t stream) {
    SsArgs a;
    if (int rc = ss_unpack(d, SS_APPLY, a, "scalseq apply bwd")) return rc;
    const long total = (a.n3 + a.n4 + a.n5) * a.C4;
    hipLaunchKernelGGL(ss_apply_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a, total);
    return launch_status("somi_scalseq_apply_bwd_f32");
}

extern "C" size_t somi_asfatt_workspace_floats(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return 0;
    const MapPlan p = map_plan(B, H, W, C, AM_RU);
    return ((size_t)B * H * p.nWc + (size_t)B * p.nHc * W) * C;      // also covers the B * nHc * nWc rows of the backward sums
}

extern "C" int somi_eca_gate_f32(const float *avg, const float *w, int k, float *gate, int B, int C, somi_stream_t stream) {
    if (int rc = eca_check(avg, w, k, gate, B, C, "eca gate")) return rc;
    hipLaunchKernelGGL(eca_fwd_kernel, dim3(cdiv((long)B * C, 256)), dim3(256), 0, (hipStream_t)stream, avg, w, k, gate, B, C);
    return launch_status("somi_eca_gate_f32");
}

extern "C" int somi_eca_gate_bwd_f32(const float *avg, const float *w, int k, const float *gate, const float *dgate, float *davg, float *dw, int B,
                                     int C, somi_stream_t stream) {
    if (int rc = eca_check(avg, w, k, gate, B, C, "eca gate bwd")) return rc;
    SOMI_REQUIRE(dgate && davg && dw, SOMI_EINVAL, "eca gate bwd: dgate, davg and dw are required");
    hipLaunchKernelGGL(eca_davg_kernel, dim3(cdiv((long)B * C, 256)), dim3(256), 0, (hipStream_t)stream, w, k, gate, dgate, davg, B, C);
    hipLaunchKernelGGL(eca_dw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, avg, k, gate, dgate, dw, B, C);
    return launch_status("somi_eca_gate_bwd_f32");
}

extern "C" int somi_asf_mix_means_nhwc_f32(const somi_asfatt_desc *d, somi_stream_t stream) {
    AmArgs a;
    if (int rc = am_unpack(d, AM_MIX, a, "asf mix means")) return rc;
    hipLaunchKernelGGL(am_mix_kernel, dim3(a.nWc, a.nHc, d->B * a.nQc), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(am_mix_finish_kernel, dim3(cdiv((long)d->B * (d->H + d->W) * a.C4, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_asf_mix_means_nhwc_f32");
}

extern "C" int somi_asf_mix_bwd_sums_nhwc_f32(const somi_asfatt_desc *d, somi_stream_t stream) {
    AmArgs a;
    if (int rc = am_unpack(d, AM_SUMS, a, "asf mix bwd sums")) return rc;
    hipLaunchKernelGGL(am_sums_kernel, dim3(a.nWc, a.nHc, d->B * a.nQc), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(am_sums_finish_kernel, dim3(cdiv((long)d->B * a.C4, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_asf_mix_bwd_sums_nhwc_f32");
}

extern "C" int somi_asf_mix_bwd_input_nhwc_f32(const somi_asfatt_desc *d, somi_stream_t stream) {
    AmArgs a;
    if (int rc = am_unpack(d, AM_INPUT, a, "asf mix bwd input")) return rc;
    const long total = (long)d->B * d->H * d->W * a.C4;
    hipLaunchKernelGGL(am_input_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a, total);
    return launch_status("somi_asf_mix_bwd_input_nhwc_f32");
}
