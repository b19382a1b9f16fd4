// Grouped and depthwise convolution, NHWC fp32 (models/common.py:53-70 with g > 1: DWConv :9580-9583, GhostConv :2001-2011).
//
// The dense implicit GEMM cannot express groups, and a depthwise layer has no GEMM to speak of: k*k multiply-adds per output element
// against one read of the input, so these kernels are streaming stencils.  One lane owns one channel quad (float4) of one pixel; a
// workgroup of 256 lanes is nq quads wide (a power of two <= 64, the smallest that covers the layer's channels) and pp = 256 / nq pixels
// tall, and walks `iters` such pixel rows.  Adjacent lanes read adjacent quads of one pixel, then the next pixel: a wave reads 1 KiB of
// contiguous NHWC for any channel count from 4 up, which is what the narrow layers of yolov5s-ghost (8 channels at 160x160) need.
// Channels beyond 256 take a second grid dimension.
//
// Reductions (BatchNorm partial sums, weight gradient) are fixed trees: xor-shuffles inside a wave, then the four waves in order through
// LDS, one row per workgroup; the rows are summed in order by a second pass.  No float atomics: every launch is bit-identical.
#include "common.h"

namespace somi {
namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_MAXQ = 64;                                       // quads per channel chunk: 256 channels
constexpr int GC_MAX_CIN_G = 16;

struct GPlan {
    int nq, pp, iters, nblk, nchunk;
};

static int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// target: about `want` workgroups in all (pixel blocks x channel chunks)
static GPlan gplan(long npix, int cw, int want) {
    GPlan p;
    const int cq = cw / 4;
    p.nchunk = cdiv(cq, GC_MAXQ);
    p.nq = pow2_at_least(cq < GC_MAXQ ? cq : GC_MAXQ);
    p.pp = GC_THREADS / p.nq;
    const long passes = (npix + p.pp - 1) / p.pp;
    long it = passes * p.nchunk / want;
    p.iters = (int)(it < 1 ? 1 : (it > 64 ? 64 : it));
    p.nblk = (int)((passes + p.iters - 1) / p.iters);
    return p;
}

constexpr int FWD_BLOCKS = 2048, WGRAD_BLOCKS = 512;

struct FwdArgs {
    const float *x, *w, *bias, *res;
    float *y, *ssum, *ssq;
    const float *pivot;
    int x_cs, x_coff, B, H, W, C1, w_cs, y_cs, y_coff, Ho, Wo, C2, Cw, act, res_cs, res_coff, cin_g, cout_g;
    GPlan p;
};

template <int K, int S, bool DW>
__global__ __launch_bounds__(GC_THREADS) void gconv_fwd_kernel(FwdArgs a) {
    __shared__ f32x4 red[2][GC_THREADS];
    constexpr int P = K / 2;
    const int ql = threadIdx.x % a.p.nq, psub = threadIdx.x / a.p.nq;
    const int co0 = (blockIdx.y * GC_MAXQ + ql) * 4;
    const bool active = co0 < a.Cw;
    const long npix = (long)a.B * a.Ho * a.Wo;
    const bool stats = a.ssum != nullptr;
    f32x4 wreg[DW ? K * K : 1];
    if constexpr (DW) {
#pragma unroll
        for (int t = 0; t < K * K; ++t) wreg[t] = active ? ld4(a.w + (size_t)t * a.w_cs + co0) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 bias = {0.f, 0.f, 0.f, 0.f}, piv = bias, st1 = bias, st2 = bias;
    if (active && a.bias) bias = ld4(a.bias + co0);
    if (active && stats && a.pivot) piv = ld4(a.pivot + co0);
    const bool load = active && co0 < a.C1;                      // quads of pad channels compute zeros (their weights are zero)
    for (int it = 0; it < a.p.iters; ++it) {
        const long pix = ((long)blockIdx.x * a.p.iters + it) * a.p.pp + psub;
        if (!active || pix >= npix) continue;
        const int wo = (int)(pix % a.Wo);
        const long t0 = pix / a.Wo;
        const int ho = (int)(t0 % a.Ho), b = (int)(t0 / a.Ho);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *xb = a.x + (size_t)b * a.H * a.W * a.x_cs + a.x_coff;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int hi = ho * S - P + r;
            if (hi < 0 || hi >= a.H) continue;
#pragma unroll
            for (int q = 0; q < K; ++q) {
                const int wi = wo * S - P + q;
                if (wi < 0 || wi >= a.W) continue;
                const float *xp = xb + ((size_t)hi * a.W + wi) * a.x_cs;
                if constexpr (DW) {
                    if (load) acc += ld4(xp + co0) * wreg[r * K + q];
                } else {
                    const float *wt = a.w + (size_t)(r * K + q) * a.cin_g * a.w_cs;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int co = co0 + e;
                        if (co >= a.C2) break;
                        const int ci0 = (co / a.cout_g) * a.cin_g;
                        float s = 0.f;
                        for (int c = 0; c < a.cin_g; ++c) s += xp[ci0 + c] * wt[(size_t)c * a.w_cs + co];
                        acc[e] += s;
                    }
                }
            }
        }
        f32x4 v = acc + bias;
        if (a.act == SOMI_ACT_SILU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f + __expf(-v[e]));
        } else if (a.act != SOMI_ACT_NONE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = apply_act_rt(v[e], a.act);
        }
        if (a.res) v += ld4(a.res + (size_t)pix * a.res_cs + a.res_coff + co0);
        st4(a.y + (size_t)pix * a.y_cs + a.y_coff + co0, v);
        if (stats) {
            const f32x4 t = v - piv;
            st1 += t;
            st2 += t * t;
        }
    }
    if (!stats) return;                                           // uniform over the workgroup
    const f32x4 s1 = block_quad_sum<GC_THREADS>(st1, a.p.nq, red[0]);
    const f32x4 s2 = block_quad_sum<GC_THREADS>(st2, a.p.nq, red[1]);
    if (threadIdx.x < a.p.nq && active) {
        st4(a.ssum + (size_t)blockIdx.x * a.Cw + co0, s1);
        st4(a.ssq + (size_t)blockIdx.x * a.Cw + co0, s2);
    }
}

struct DgradArgs {
    const float *dy, *w, *acc1, *acc2;
    float *dx;
    int dy_cs, dy_coff, B, Ho, Wo, C2, w_cs, dx_cs, dx_coff, H, W, C1, Cx, acc1_cs, acc1_coff, acc2_cs, acc2_coff, cin_g, cout_g;
    GPlan p;
};

// dx[b,h,w,ci] = sum over the taps whose output pixel (h + P - r) / S, (w + P - q) / S exists, and over the cout_g outputs of ci's group
template <int K, int S, bool DW>
__global__ __launch_bounds__(GC_THREADS) void gconv_dgrad_kernel(DgradArgs a) {
    constexpr int P = K / 2;
    const int ql = threadIdx.x % a.p.nq, psub = threadIdx.x / a.p.nq;
    const int ci0 = (blockIdx.y * GC_MAXQ + ql) * 4;
    if (ci0 >= a.Cx) return;
    const long npix = (long)a.B * a.H * a.W;
    const bool load = ci0 < a.C1;
    for (int it = 0; it < a.p.iters; ++it) {
        const long pix = ((long)blockIdx.x * a.p.iters + it) * a.p.pp + psub;
        if (pix >= npix) return;
        const int w = (int)(pix % a.W);
        const long t0 = pix / a.W;
        const int h = (int)(t0 % a.H), b = (int)(t0 / a.H);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *db = a.dy + (size_t)b * a.Ho * a.Wo * a.dy_cs + a.dy_coff;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int hs = h + P - r;
            if (hs < 0 || hs % S) continue;
            const int ho = hs / S;
            if (ho >= a.Ho) continue;
#pragma unroll
            for (int q = 0; q < K; ++q) {
                const int ws = w + P - q;
                if (ws < 0 || ws % S) continue;
                const int wo = ws / S;
                if (wo >= a.Wo) continue;
                const float *dp = db + ((size_t)ho * a.Wo + wo) * a.dy_cs;
                const float *wt = a.w + (size_t)(r * K + q) * a.cin_g * a.w_cs;
                if constexpr (DW) {
                    if (load) acc += ld4(dp + ci0) * ld4(wt + ci0);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ci = ci0 + e;
                        if (ci >= a.C1) break;
                        const int g = ci / a.cin_g, cl = ci - g * a.cin_g;
                        const float *wc = wt + (size_t)cl * a.w_cs + g * a.cout_g;
                        const float *dc = dp + g * a.cout_g;
                        float s = 0.f;
                        for (int j = 0; j < a.cout_g; ++j) s += dc[j] * wc[j];
                        acc[e] += s;
                    }
                }
            }
        }
        if (a.acc1) acc += ld4(a.acc1 + (size_t)pix * a.acc1_cs + a.acc1_coff + ci0);
        if (a.acc2) acc += ld4(a.acc2 + (size_t)pix * a.acc2_cs + a.acc2_coff + ci0);
        st4(a.dx + (size_t)pix * a.dx_cs + a.dx_coff + ci0, acc);
    }
}

struct WgradArgs {
    const float *x, *dy;
    float *part;
    int x_cs, x_coff, B, H, W, C1, dy_cs, dy_coff, Ho, Wo, C2, C2r, cin_g, cout_g;
    GPlan p;
};

// stage 1: one row of partial weight gradients per workgroup, part[row][(tap * cin_g + c) * C2r + co]
template <int K, int S, bool DW>
__global__ __launch_bounds__(GC_THREADS) void gconv_wgrad_kernel(WgradArgs a) {
    __shared__ f32x4 red[GC_THREADS];
    constexpr int P = K / 2, KK = K * K;
    const int ql = threadIdx.x % a.p.nq, psub = threadIdx.x / a.p.nq;
    const int co0 = (blockIdx.y * GC_MAXQ + ql) * 4;
    const bool active = co0 < a.C2r;
    const long npix = (long)a.B * a.Ho * a.Wo;
    const long pix0 = (long)blockIdx.x * a.p.iters * a.p.pp + psub;
    float *row = a.part + (size_t)blockIdx.x * KK * a.cin_g * a.C2r;
    if constexpr (DW) {                                           // every tap at once: dy read once per pixel
        f32x4 acc[KK];
#pragma unroll
        for (int t = 0; t < KK; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < a.p.iters; ++it) {
            const long pix = pix0 + (long)it * a.p.pp;
            if (!active || pix >= npix) break;
            const int wo = (int)(pix % a.Wo);
            const long t0 = pix / a.Wo;
            const int ho = (int)(t0 % a.Ho), b = (int)(t0 / a.Ho);
            const f32x4 d = ld4(a.dy + (size_t)pix * a.dy_cs + a.dy_coff + co0);
            const float *xb = a.x + (size_t)b * a.H * a.W * a.x_cs + a.x_coff + co0;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int hi = ho * S - P + r;
                if (hi < 0 || hi >= a.H) continue;
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const int wi = wo * S - P + q;
                    if (wi < 0 || wi >= a.W) continue;
                    acc[r * K + q] += d * ld4(xb + ((size_t)hi * a.W + wi) * a.x_cs);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < KK; ++t) {
            const f32x4 s = block_quad_sum<GC_THREADS>(acc[t], a.p.nq, red);
            if (threadIdx.x < a.p.nq && active) st4(row + (size_t)t * a.C2r + co0, s);
        }
    } else {
        for (int t = 0; t < KK; ++t) {
            const int r = t / K, q = t % K;
            for (int c = 0; c < a.cin_g; ++c) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int it = 0; it < a.p.iters; ++it) {
                    const long pix = pix0 + (long)it * a.p.pp;
                    if (!active || pix >= npix) break;
                    const int wo = (int)(pix % a.Wo);
                    const long t0 = pix / a.Wo;
                    const int ho = (int)(t0 % a.Ho), b = (int)(t0 / a.Ho);
                    const int hi = ho * S - P + r, wi = wo * S - P + q;
                    if (hi < 0 || hi >= a.H || wi < 0 || wi >= a.W) continue;
                    const float *dp = a.dy + (size_t)pix * a.dy_cs + a.dy_coff;
                    const float *xp = a.x + (((size_t)b * a.H + hi) * a.W + wi) * a.x_cs + a.x_coff;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int co = co0 + e;
                        if (co < a.C2) acc[e] += dp[co] * xp[(co / a.cout_g) * a.cin_g + c];
                    }
                }
                const f32x4 s = block_quad_sum<GC_THREADS>(acc, a.p.nq, red);
                if (threadIdx.x < a.p.nq && active) st4(row + (size_t)(t * a.cin_g + c) * a.C2r + co0, s);
            }
        }
    }
}

// stage 2: dw[co][c][r][q] (+)= sum of the rows in order
__global__ __launch_bounds__(GC_THREADS) void gconv_wgrad_fold_kernel(const float *__restrict__ part, int rows, int KK, int cin_g, int C2, int C2r,
                                                                     float *__restrict__ dw, int accumulate) {
    const int idx = blockIdx.x * GC_THREADS + threadIdx.x;
    const int cols = KK * cin_g;
    if (idx >= cols * C2) return;
    const int co = idx % C2, col = idx / C2;                     // col = tap * cin_g + c
    const int t = col / cin_g, c = col - t * cin_g;
    const float *p = part + (size_t)col * C2r + co;
    const size_t stride = (size_t)cols * C2r;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += p[(size_t)r * stride];
    float *o = dw + ((size_t)co * cin_g + c) * KK + t;
    *o = accumulate ? *o + s : s;
}

#define GC_SWITCH(K_, S_, DW_, KERNEL, GRID, ARGS, STREAM)                                                                      \
    do {                                                                                                                        \
        if (K_ == 1 && S_ == 1 && DW_) hipLaunchKernelGGL((KERNEL<1, 1, true>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);   \
        else if (K_ == 1 && S_ == 1) hipLaunchKernelGGL((KERNEL<1, 1, false>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);    \
        else if (K_ == 1 && DW_) hipLaunchKernelGGL((KERNEL<1, 2, true>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);         \
        else if (K_ == 1) hipLaunchKernelGGL((KERNEL<1, 2, false>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);               \
        else if (K_ == 3 && S_ == 1 && DW_) hipLaunchKernelGGL((KERNEL<3, 1, true>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS); \
        else if (K_ == 3 && S_ == 1) hipLaunchKernelGGL((KERNEL<3, 1, false>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);    \
        else if (K_ == 3 && DW_) hipLaunchKernelGGL((KERNEL<3, 2, true>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);         \
        else if (K_ == 3) hipLaunchKernelGGL((KERNEL<3, 2, false>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);               \
        else if (S_ == 1 && DW_) hipLaunchKernelGGL((KERNEL<5, 1, true>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);         \
        else if (S_ == 1) hipLaunchKernelGGL((KERNEL<5, 1, false>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);               \
        else if (DW_) hipLaunchKernelGGL((KERNEL<5, 2, true>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);                    \
        else hipLaunchKernelGGL((KERNEL<5, 2, false>), GRID, dim3(GC_THREADS), 0, STREAM, ARGS);                            \
    } while (0)

static int check_geometry(int C1, int C2, int groups, int k, int stride) {
    SOMI_REQUIRE(k == 1 || k == 3 || k == 5, SOMI_ENOTIMPL, "grouped conv: kernel size %d (1, 3 or 5 only)", k);
    SOMI_REQUIRE(stride == 1 || stride == 2, SOMI_ENOTIMPL, "grouped conv: stride %d (1 or 2 only)", stride);
    SOMI_REQUIRE(groups >= 1 && C1 > 0 && C2 > 0 && C1 % groups == 0 && C2 % groups == 0, SOMI_EINVAL,
                 "grouped conv: %d and %d channels are not divisible into %d groups", C1, C2, groups);
    SOMI_REQUIRE(C1 / groups <= GC_MAX_CIN_G, SOMI_ENOTIMPL, "grouped conv: %d input channels per group (at most %d)", C1 / groups, GC_MAX_CIN_G);
    return 0;
}

}  // namespace
}  // namespace somi

using namespace somi;

extern "C" int somi_gconv2d_stat_rows(int B, int Ho, int Wo, int Cw) {
    if (B <= 0 || Ho <= 0 || Wo <= 0 || Cw <= 0 || Cw % 4) return 0;
    return gplan((long)B * Ho * Wo, Cw, FWD_BLOCKS).nblk;
}

extern "C" int somi_gconv2d_nhwc_f32(const float *x, int x_cs, int x_coff, int B, int H, int W, int C1, const float *w, int w_cs, const float *bias,
                                     int groups, int k, int stride, float *y, int y_cs, int y_coff, int C2, int Cw, int act, const float *residual,
                                     int res_cs, int res_coff, float *stat_sum, float *stat_sumsq, const float *stat_pivot, somi_stream_t stream) {
    if (int rc = check_geometry(C1, C2, groups, k, stride)) return rc;
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && Cw % 4 == 0 && Cw >= C2 && (!bias || aligned16(bias)), SOMI_EINVAL, "grouped conv: bad sizes or bias");
    SOMI_REQUIRE(w && aligned16(w) && w_cs % 4 == 0 && w_cs >= Cw, SOMI_EINVAL, "grouped conv: w must be 16 B aligned, its row stride w_cs (%d) a multiple of 4 >= Cw (%d)", w_cs, Cw);
    SOMI_REQUIRE_SLICES("grouped conv", {"x", x, x_cs, x_coff, r4(C1)}, {"y", y, y_cs, y_coff, Cw}, {"residual", residual, res_cs, res_coff, Cw, kOptional});
    SOMI_REQUIRE(act >= 0 && act <= 4, SOMI_EINVAL, "grouped conv: bad activation");
    SOMI_REQUIRE(!stat_sum == !stat_sumsq && (!stat_sum || (aligned16(stat_sum) && aligned16(stat_sumsq))) && (!stat_pivot || aligned16(stat_pivot)),
                 SOMI_EINVAL, "grouped conv: bad statistics buffers");
    const int P = k / 2, Ho = (H + 2 * P - k) / stride + 1, Wo = (W + 2 * P - k) / stride + 1;
    FwdArgs a;
    a.x = x; a.w = w; a.bias = bias; a.res = residual; a.y = y; a.ssum = stat_sum; a.ssq = stat_sumsq; a.pivot = stat_pivot;
    a.x_cs = x_cs; a.x_coff = x_coff; a.B = B; a.H = H; a.W = W; a.C1 = C1; a.w_cs = w_cs; a.y_cs = y_cs; a.y_coff = y_coff; a.Ho = Ho; a.Wo = Wo;
    a.C2 = C2; a.Cw = Cw; a.act = act; a.res_cs = res_cs; a.res_coff = res_coff; a.cin_g = C1 / groups; a.cout_g = C2 / groups;
    a.p = gplan((long)B * Ho * Wo, Cw, FWD_BLOCKS);
    const bool dw = a.cin_g == 1 && a.cout_g == 1;
    hipStream_t s = (hipStream_t)stream;
    GC_SWITCH(k, stride, dw, gconv_fwd_kernel, dim3(a.p.nblk, a.p.nchunk), a, s);
    return launch_status("somi_gconv2d_nhwc_f32");
}

extern "C" int somi_gconv2d_dgrad_nhwc_f32(const float *dy, int dy_cs, int dy_coff, int B, int Ho, int Wo, int C2, const float *w, int w_cs, int groups,
                                           int k, int stride, float *dx, int dx_cs, int dx_coff, int H, int W, int C1, int Cx, const float *acc1,
                                           int acc1_cs, int acc1_coff, const float *acc2, int acc2_cs, int acc2_coff, somi_stream_t stream) {
    if (int rc = check_geometry(C1, C2, groups, k, stride)) return rc;
    const int P = k / 2;
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && Ho == (H + 2 * P - k) / stride + 1 && Wo == (W + 2 * P - k) / stride + 1, SOMI_EINVAL,
                 "grouped conv dgrad: output size does not match the input size");
    SOMI_REQUIRE(Cx % 4 == 0 && Cx >= C1, SOMI_EINVAL, "grouped conv dgrad: Cx is C1 rounded up to a multiple of 4, or more");
    SOMI_REQUIRE(w && aligned16(w) && w_cs % 4 == 0 && w_cs >= r4(C2), SOMI_EINVAL,
                 "grouped conv dgrad: w must be 16 B aligned, its row stride w_cs (%d) a multiple of 4 >= C2 (%d) rounded up to 4", w_cs, C2);
    SOMI_REQUIRE_SLICES("grouped conv dgrad", {"dy", dy, dy_cs, dy_coff, r4(C2)}, {"dx", dx, dx_cs, dx_coff, Cx},
                        {"acc1", acc1, acc1_cs, acc1_coff, Cx, kOptional}, {"acc2", acc2, acc2_cs, acc2_coff, Cx, kOptional});
    DgradArgs a;
    a.dy = dy; a.w = w; a.acc1 = acc1; a.acc2 = acc2; a.dx = dx;
    a.dy_cs = dy_cs; a.dy_coff = dy_coff; a.B = B; a.Ho = Ho; a.Wo = Wo; a.C2 = C2; a.w_cs = w_cs; a.dx_cs = dx_cs; a.dx_coff = dx_coff; a.H = H;
    a.W = W; a.C1 = C1; a.Cx = Cx; a.acc1_cs = acc1_cs; a.acc1_coff = acc1_coff; a.acc2_cs = acc2_cs; a.acc2_coff = acc2_coff;
    a.cin_g = C1 / groups; a.cout_g = C2 / groups;
    a.p = gplan((long)B * H * W, Cx, FWD_BLOCKS);
    const bool dw = a.cin_g == 1 && a.cout_g == 1;
    hipStream_t s = (hipStream_t)stream;
    GC_SWITCH(k, stride, dw, gconv_dgrad_kernel, dim3(a.p.nblk, a.p.nchunk), a, s);
    return launch_status("somi_gconv2d_dgrad_nhwc_f32");
}

extern "C" size_t somi_gconv2d_wgrad_workspace_floats(int B, int Ho, int Wo, int C2, int cin_g, int k) {
    if (B <= 0 || Ho <= 0 || Wo <= 0 || C2 <= 0 || cin_g <= 0 || k <= 0) return 0;
    const GPlan p = gplan((long)B * Ho * Wo, r4(C2), WGRAD_BLOCKS);
    return (size_t)p.nblk * k * k * cin_g * r4(C2);
}

extern "C" int somi_gconv2d_wgrad_nhwc_f32(const float *x, int x_cs, int x_coff, int B, int H, int W, int C1, const float *dy, int dy_cs, int dy_coff,
                                           int Ho, int Wo, int C2, int groups, int k, int stride, float *dw, int accumulate, float *workspace,
                                           size_t workspace_floats, somi_stream_t stream) {
    if (int rc = check_geometry(C1, C2, groups, k, stride)) return rc;
    const int P = k / 2;
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && Ho == (H + 2 * P - k) / stride + 1 && Wo == (W + 2 * P - k) / stride + 1, SOMI_EINVAL,
                 "grouped conv wgrad: output size does not match the input size");
    SOMI_REQUIRE_SLICES("grouped conv wgrad", {"x", x, x_cs, x_coff, r4(C1)}, {"dy", dy, dy_cs, dy_coff, r4(C2)});
    SOMI_REQUIRE(dw && workspace && aligned16(workspace), SOMI_EINVAL, "grouped conv wgrad: dw and a 16-byte aligned workspace are needed");
    const int cin_g = C1 / groups;
    SOMI_REQUIRE(workspace_floats >= somi_gconv2d_wgrad_workspace_floats(B, Ho, Wo, C2, cin_g, k), SOMI_EWORKSPACE,
                 "grouped conv wgrad: workspace too small");
    WgradArgs a;
    a.x = x; a.dy = dy; a.part = workspace;
    a.x_cs = x_cs; a.x_coff = x_coff; a.B = B; a.H = H; a.W = W; a.C1 = C1; a.dy_cs = dy_cs; a.dy_coff = dy_coff; a.Ho = Ho; a.Wo = Wo; a.C2 = C2;
    a.C2r = r4(C2); a.cin_g = cin_g; a.cout_g = C2 / groups;
    a.p = gplan((long)B * Ho * Wo, a.C2r, WGRAD_BLOCKS);
    const bool depthwise = a.cin_g == 1 && a.cout_g == 1;
    hipStream_t s = (hipStream_t)stream;
    GC_SWITCH(k, stride, depthwise, gconv_wgrad_kernel, dim3(a.p.nblk, a.p.nchunk), a, s);
    const int n = k * k * cin_g * C2;
    hipLaunchKernelGGL(gconv_wgrad_fold_kernel, dim3(cdiv(n, GC_THREADS)), dim3(GC_THREADS), 0, s, (const float *)workspace, a.p.nblk, k * k, cin_g,
                       C2, a.C2r, dw, accumulate);
    return launch_status("somi_gconv2d_wgrad_nhwc_f32");
}
