// Large-kernel depthwise convolution, NHWC fp32, K = 7 or 9, stride 1, pad K / 2 (ConvNextBlock's 7x7, models/common.py:6755; ConvMix's 9x9,
// :7153).
//
// gconv.hip's depthwise stencil holds all K * K taps of a channel quad in registers and issues one load per tap per output: at K = 9 that is
// 324 registers of taps and 81 loads per output quad.  Here a lane owns one channel quad of a STRIP of DL_T = 8 adjacent outputs of one image
// row.  It walks the K tap rows; per tap row it holds that row's K taps (K float4) and slides over the DL_T + K - 1 inputs the strip reads
// from that image row, each input loaded once and multiplied into every output of the strip it reaches: (K + DL_T + K - 1) loads for DL_T * K
// multiply-adds per quad - 25 loads for 72 at K = 9, where the direct stencil issues 72 for 72.  Live registers: DL_T accumulators + K taps +
// the inputs in flight, independent of K * K.
//
// A workgroup of 256 lanes is nq quads wide (a power of two <= 64, the smallest that covers the channels) and 256 / nq strips tall, and walks
// `iters` such rows of strips (somi_dwlk_strips_per_workgroup); strips are numbered (image, row, strip of the row), so the lanes of a
// workgroup read neighbouring strips.  Channels beyond 256 take a second grid dimension, as in gconv.hip.
//
// The data gradient is the same stencil with the taps mirrored.  The weight gradient turns the loop inside out: per tap row a lane keeps K
// accumulators (one per tap of the row), loads the strip's DL_T gradients and slides over the same DL_T + K - 1 inputs; the workgroup's sums
// go to one partial row per workgroup, tap row by tap row, and a second kernel adds the rows in a fixed order.  Reductions are fixed trees
// (xor-shuffles in a wave, the four waves in order through LDS): no float atomics, every launch is bit-identical.
#include "common.h"

namespace somi {
namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_MAXQ = 64;                                       // quads per channel chunk: 256 channels
constexpr int DL_T = 8;                                           // outputs per strip
constexpr int DL_G = 2;                                           // inputs loaded together (two such groups in flight)
constexpr int DL_FWD_BLOCKS = 2048, DL_WGRAD_BLOCKS = 512;        // about this many workgroups in all
constexpr int DL_MAX_ITERS = 64;

struct DPlan {
    int nq, pp, iters, nblk, nchunk;
    unsigned nstrip, nitem;
};

static DPlan dplan(int B, int H, int W, int C, int want) {
    DPlan p;
    const int cq = C / 4;
    p.nchunk = cdiv(cq, DL_MAXQ);
    p.nq = 1;
    while (p.nq < cq && p.nq < DL_MAXQ) p.nq <<= 1;
    p.pp = DL_THREADS / p.nq;
    p.nstrip = cdiv(W, DL_T);
    p.nitem = (unsigned)((long)B * H * p.nstrip);
    const long passes = ((long)p.nitem + p.pp - 1) / p.pp;
    const long it = passes * p.nchunk / want;
    p.iters = (int)(it < 1 ? 1 : (it > DL_MAX_ITERS ? DL_MAX_ITERS : it));
    p.nblk = (int)((passes + p.iters - 1) / p.iters);
    return p;
}

// DL_G adjacent pixels of an image row, zero outside the row.  o: float index (relative to `base`, which is uniform over the workgroup; a
// tensor is below 2^30 floats, check_size) of the first of them - it may lie outside the row -, advanced past the group; [lo, hi]: the
// indices of the row's first and last pixel.  The index is clamped into the row and the value dropped where it was clamped: no branch, and
// one running index in place of one address per pixel.
__device__ __forceinline__ void load_group(f32x4 (&xv)[DL_G], const float *base, int &o, int lo, int hi, int cs) {
#pragma unroll
    for (int i = 0; i < DL_G; ++i) {
        const int oc = min(max(o, lo), hi);
        const f32x4 v = ld4(base + (unsigned)oc);
        xv[i] = o == oc ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        o += cs;
    }
}

struct StencilArgs {
    const float *x, *w, *bias, *ps, *pt, *r1, *r2, *pivot;
    float *y, *ssum, *ssq;
    int x_cs, x_coff, B, H, W, C, w_cs, y_cs, y_coff, act, r1_cs, r1_coff, r2_cs, r2_coff, flip;
    DPlan p;
};

// forward (flip = 0) and data gradient (flip = 1: taps mirrored, r1 / r2 = acc1 / acc2).  Bounded at THREE waves a SIMD (168 registers):
// at four (128) the compiler spills 22 - 44 registers, some inside the tap loop, and the kernel is 1.2 - 1.8x slower.
template <int K, int ACT, bool STATS>
__global__ __launch_bounds__(DL_THREADS, 3) void dwlk_stencil_kernel(StencilArgs a) {
    __shared__ f32x4 stage[DL_T][DL_THREADS];
    constexpr int P = K / 2, NG = (DL_T + K - 1 + DL_G - 1) / DL_G;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int ql = threadIdx.x % a.p.nq, psub = threadIdx.x / a.p.nq;
    const int c0 = (blockIdx.y * DL_MAXQ + ql) * 4;
    const bool active = c0 < a.C;
    constexpr bool stats = STATS;
    f32x4 st1 = zero, st2 = zero;
    for (int it = 0; it < a.p.iters; ++it) {
        const unsigned item = (blockIdx.x * a.p.iters + it) * a.p.pp + psub;   // below 2^31 (check_size)
        if (!active || item >= a.p.nitem) continue;
        const unsigned row = item / a.p.nstrip, sw = item - row * a.p.nstrip;   // row = b * H + h
        const int h = (int)(row % a.H);
        const int w0 = (int)sw * DL_T;
        const float *xbase = a.x + a.x_coff;
        f32x4 acc[DL_T];
#pragma unroll
        for (int t = 0; t < DL_T; ++t) acc[t] = zero;
        const int r0 = h < P ? P - h : 0, r1 = a.H + P - h < K ? a.H + P - h : K;   // the tap rows inside the image
#pragma unroll 1
        for (int r = r0; r < r1; ++r) {
            const int hi = h - P + r;
            const float *wr = a.w + (size_t)((a.flip ? K - 1 - r : r) * K) * a.w_cs + c0;
            f32x4 wt[K];
#pragma unroll
            for (int q = 0; q < K; ++q) wt[q] = ld4(wr + (size_t)(a.flip ? K - 1 - q : q) * a.w_cs);
            const int lo = (int)((row - h + hi) * a.W) * a.x_cs + c0, up = lo + (a.W - 1) * a.x_cs;
            int o = lo + (w0 - P) * a.x_cs;
            f32x4 xv[2][DL_G];
            load_group(xv[0], xbase, o, lo, up, a.x_cs);
#pragma unroll
            for (int g = 0; g < NG; ++g) {                        // the next group's loads fly while this group's products issue
                if (g + 1 < NG) load_group(xv[(g + 1) & 1], xbase, o, lo, up, a.x_cs);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < DL_G; ++i)
#pragma unroll
                    for (int q = 0; q < K; ++q) {
                        const int t = g * DL_G + i - q;
                        if (t >= 0 && t < DL_T) acc[t] += xv[g & 1][i] * wt[q];
                    }
            }
        }
        // The epilogue runs as a rolled loop over the strip, the accumulators handed over through the lane's own LDS slots: unrolled, its eight
        // copies (exact GELU included) cost more registers than the tap loop and the compiler spilled the accumulators to make room.
#pragma unroll
        for (int t = 0; t < DL_T; ++t) stage[t][threadIdx.x] = acc[t];
        const size_t pix0 = (size_t)row * a.W + w0;
        const int nt = a.W - w0 < DL_T ? a.W - w0 : DL_T;
        f32x4 bias = zero, ps = {1.f, 1.f, 1.f, 1.f}, pt = zero, piv = zero;
        if (a.bias) bias = ld4(a.bias + c0);
        if (!stats && a.ps) ps = ld4(a.ps + c0);
        if (!stats && a.pt) pt = ld4(a.pt + c0);
        if (stats && a.pivot) piv = ld4(a.pivot + c0);
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            f32x4 v = stage[t][threadIdx.x] + bias;
            const size_t pix = pix0 + t;
            float *yp = a.y + pix * a.y_cs + a.y_coff + c0;
            if constexpr (stats) st4(yp, v); // the pre-activation is what is stored; the sums are of act(.)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = apply_act<ACT>(v[e]);
            if constexpr (stats) {
                const f32x4 d = v - piv;
                st1 += d;
                st2 += d * d;
            } else {
                v = v * ps + pt;
                if (a.r1) v += ld4(a.r1 + pix * a.r1_cs + a.r1_coff + c0);
                if (a.r2) v += ld4(a.r2 + pix * a.r2_cs + a.r2_coff + c0);
                st4(yp, v);
            }
        }
    }
    if constexpr (!stats) return;
    __syncthreads();                                              // the reduction reuses the staging rows
    const f32x4 s1 = block_quad_sum<DL_THREADS>(st1, a.p.nq, stage[0]);
    const f32x4 s2 = block_quad_sum<DL_THREADS>(st2, a.p.nq, stage[1]);
    if (threadIdx.x < a.p.nq && active) {
        st4(a.ssum + (size_t)blockIdx.x * a.C + c0, s1);
        st4(a.ssq + (size_t)blockIdx.x * a.C + c0, s2);
    }
}

struct WgradArgs {
    const float *x, *dy;
    float *part;
    int x_cs, x_coff, dy_cs, dy_coff, B, H, W, C;
    DPlan p;
};

// stage 1: one row of partial sums per workgroup, part[row][(tap | K * K: the bias) * C + c]
template <int K>
__global__ __launch_bounds__(DL_THREADS, 4) void dwlk_wgrad_kernel(WgradArgs a) {
    __shared__ f32x4 red[K + 1][DL_THREADS];
    constexpr int P = K / 2, NG = (DL_T + K - 1 + DL_G - 1) / DL_G;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int ql = threadIdx.x % a.p.nq, psub = threadIdx.x / a.p.nq;
    const int c0 = (blockIdx.y * DL_MAXQ + ql) * 4;
    const bool active = c0 < a.C;
    float *prow = a.part + (size_t)blockIdx.x * (K * K + 1) * a.C;
#pragma unroll 1
    for (int r = 0; r < K; ++r) {
        f32x4 acc[K], bsum = zero;
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] = zero;
        for (int it = 0; it < a.p.iters; ++it) {
            const unsigned item = (blockIdx.x * a.p.iters + it) * a.p.pp + psub;
            if (!active || item >= a.p.nitem) break;
            const unsigned row = item / a.p.nstrip, sw = item - row * a.p.nstrip;
            const int h = (int)(row % a.H);
            const int w0 = (int)sw * DL_T;
            const int hi = h - P + r;
            if (r != 0 && (hi < 0 || hi >= a.H)) continue;
            const float *dp = a.dy + ((size_t)row * a.W + w0) * a.dy_cs + a.dy_coff + c0;
            f32x4 d[DL_T];
#pragma unroll
            for (int t = 0; t < DL_T; ++t) d[t] = w0 + t < a.W ? ld4(dp + (size_t)t * a.dy_cs) : zero;
            if (r == 0) {
#pragma unroll
                for (int t = 0; t < DL_T; ++t) bsum += d[t];
                if (hi < 0) continue;                             // hi >= H cannot happen at r = 0
            }
            const float *xbase = a.x + a.x_coff;
            const int lo = (int)((row - h + hi) * a.W) * a.x_cs + c0, up = lo + (a.W - 1) * a.x_cs;
            int o = lo + (w0 - P) * a.x_cs;
            f32x4 xv[2][DL_G];
            load_group(xv[0], xbase, o, lo, up, a.x_cs);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 1 < NG) load_group(xv[(g + 1) & 1], xbase, o, lo, up, a.x_cs);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < DL_G; ++i)
#pragma unroll
                    for (int q = 0; q < K; ++q) {
                        const int t = g * DL_G + i - q;
                        if (t >= 0 && t < DL_T) acc[q] += d[t] * xv[g & 1][i];
                    }
            }
        }
        // the tap row's k sums (and, at tap row 0, the bias sum) through the tree together: one pair of barriers a tap row, not one a tap
        for (int off = a.p.nq; off < 64; off <<= 1) {
#pragma unroll
            for (int q = 0; q < K; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[q][e] += __shfl_xor(acc[q][e], off);
#pragma unroll
            for (int e = 0; e < 4; ++e) bsum[e] += __shfl_xor(bsum[e], off);
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane < a.p.nq) {
#pragma unroll
            for (int q = 0; q < K; ++q) red[q][wave * 64 + lane] = acc[q];
            red[K][wave * 64 + lane] = bsum;
        }
        __syncthreads();
        if (threadIdx.x < a.p.nq && active) {
#pragma unroll
            for (int q = 0; q <= K; ++q) {
                if (q == K && r != 0) break;
                f32x4 s = red[q][threadIdx.x];
#pragma unroll
                for (int wv = 1; wv < DL_THREADS / 64; ++wv) s += red[q][wv * 64 + threadIdx.x];
                st4(prow + (size_t)(q == K ? K * K : r * K + q) * a.C + c0, s);
            }
        }
        __syncthreads();
    }
}

// stage 2: dw[c][tap] and db[c] (+)= the rows summed in a fixed order
__global__ __launch_bounds__(DL_THREADS) void dwlk_wgrad_fold_kernel(const float *__restrict__ part, int rows, int KK, int C, float *__restrict__ dw,
                                                                    float *__restrict__ db, int accumulate) {
    const int idx = blockIdx.x * DL_THREADS + threadIdx.x;
    if (idx >= (KK + 1) * C) return;
    const int c = idx % C, col = idx / C;
    if (col == KK && !db) return;
    const float *p = part + idx;
    const size_t stride = (size_t)(KK + 1) * C;
    float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};         // eight interleaved running sums: eight loads in flight, the order still fixed
    int r = 0;
    for (; r + 8 <= rows; r += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] += p[(size_t)(r + j) * stride];
    for (int j = 0; r < rows; ++r, ++j) t[j] += p[(size_t)r * stride];
    const float s = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    float *o = col == KK ? db + c : dw + (size_t)c * KK + col;
    *o = accumulate ? *o + s : s;
}

static int check_size(const char *who, int B, int H, int W, int C, int k, int cs_max) {
    SOMI_REQUIRE(k == 7 || k == 9, SOMI_ENOTIMPL, "%s: kernel size %d (7 or 9 only; 1, 3 and 5 are somi_gconv2d_*'s)", who, k);
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, SOMI_EINVAL, "%s: bad sizes (%d, %d, %d, %d)", who, B, H, W, C);
    SOMI_REQUIRE(C % 4 == 0, SOMI_ENOTIMPL, "%s: %d channels (a multiple of 4 only)", who, C);
    SOMI_REQUIRE((long)B * H * W * cs_max <= (1L << 30), SOMI_ENOTIMPL, "%s: a tensor of more than 2^30 floats (%d x %d x %d x %d)", who, B, H, W, cs_max);
    return 0;
}

static int check_weight(const char *who, const float *w, int w_cs, int C) {
    SOMI_REQUIRE(w && aligned16(w) && w_cs % 4 == 0 && w_cs >= C, SOMI_EINVAL,
                 "%s: w must be 16 B aligned, its row stride w_cs (%d) a multiple of 4 >= C (%d)", who, w_cs, C);
    return 0;
}

template <int K>
static void launch_stencil_k(const StencilArgs &a, hipStream_t s) {
    const dim3 grid(a.p.nblk, a.p.nchunk), block(DL_THREADS);
    const bool gelu = a.act == SOMI_ACT_GELU;
    if (a.ssum) {
        if (gelu) hipLaunchKernelGGL((dwlk_stencil_kernel<K, SOMI_ACT_GELU, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((dwlk_stencil_kernel<K, SOMI_ACT_NONE, true>), grid, block, 0, s, a);
    } else {
        if (gelu) hipLaunchKernelGGL((dwlk_stencil_kernel<K, SOMI_ACT_GELU, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((dwlk_stencil_kernel<K, SOMI_ACT_NONE, false>), grid, block, 0, s, a);
    }
}

static void launch_stencil(int k, const StencilArgs &a, hipStream_t s) {
    if (k == 7) launch_stencil_k<7>(a, s);
    else launch_stencil_k<9>(a, s);
}

}  // namespace
}  // namespace somi

using namespace somi;

extern "C" int somi_dwlk_strip_length(void) { return DL_T; }

extern "C" int somi_dwlk_strips_per_workgroup(int B, int H, int W, int C, int wgrad) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return 0;
    return dplan(B, H, W, C, wgrad ? DL_WGRAD_BLOCKS : DL_FWD_BLOCKS).iters;
}

extern "C" int somi_dwlk_stat_rows(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return 0;
    return dplan(B, H, W, C, DL_FWD_BLOCKS).nblk;
}

extern "C" int somi_dwlk_nhwc_f32(somi_slice x, const float *w, int w_cs, const float *bias, int k, int act, const float *post_scale,
                                  const float *post_shift, somi_slice y, somi_slice residual, int B, int H, int W, int C, float *stat_sum,
                                  float *stat_sumsq, const float *stat_pivot, somi_stream_t stream) {
    const char *who = "dwlk";
    if (int rc = check_size(who, B, H, W, C, k, x.cs > y.cs ? x.cs : y.cs)) return rc;
    if (int rc = check_weight(who, w, w_cs, C)) return rc;
    SOMI_REQUIRE(act == SOMI_ACT_NONE || act == SOMI_ACT_GELU, SOMI_ENOTIMPL, "%s: activation %d (none or gelu only)", who, act);
    SOMI_REQUIRE((!bias || aligned16(bias)) && (!post_scale || aligned16(post_scale)) && (!post_shift || aligned16(post_shift)), SOMI_EINVAL,
                 "%s: bias, post_scale and post_shift must be 16 B aligned", who);
    SOMI_REQUIRE_SLICES(who, {"x", x.p, x.cs, x.coff, C}, {"y", y.p, y.cs, y.coff, C}, {"residual", residual.p, residual.cs, residual.coff, C, kOptional});
    SOMI_REQUIRE(!stat_sum == !stat_sumsq && (!stat_sum || (aligned16(stat_sum) && aligned16(stat_sumsq))) && (!stat_pivot || aligned16(stat_pivot)),
                 SOMI_EINVAL, "%s: bad statistics buffers", who);
    SOMI_REQUIRE(!stat_sum || (!post_scale && !post_shift && !residual.p), SOMI_EINVAL,
                 "%s: with statistics the pre-activation is written: no post_scale, post_shift or residual", who);
    StencilArgs a;
    a.x = x.p; a.w = w; a.bias = bias; a.ps = post_scale; a.pt = post_shift; a.r1 = residual.p; a.r2 = nullptr; a.pivot = stat_pivot;
    a.y = y.p; a.ssum = stat_sum; a.ssq = stat_sumsq;
    a.x_cs = x.cs; a.x_coff = x.coff; a.B = B; a.H = H; a.W = W; a.C = C; a.w_cs = w_cs; a.y_cs = y.cs; a.y_coff = y.coff; a.act = act;
    a.r1_cs = residual.cs; a.r1_coff = residual.coff; a.r2_cs = 0; a.r2_coff = 0; a.flip = 0;
    a.p = dplan(B, H, W, C, DL_FWD_BLOCKS);
    launch_stencil(k, a, (hipStream_t)stream);
    return launch_status("somi_dwlk_nhwc_f32");
}

extern "C" int somi_dwlk_dgrad_nhwc_f32(somi_slice dy, const float *w, int w_cs, int k, somi_slice dx, somi_slice acc1, somi_slice acc2, int B, int H,
                                        int W, int C, somi_stream_t stream) {
    const char *who = "dwlk dgrad";
    if (int rc = check_size(who, B, H, W, C, k, dy.cs > dx.cs ? dy.cs : dx.cs)) return rc;
    if (int rc = check_weight(who, w, w_cs, C)) return rc;
    SOMI_REQUIRE_SLICES(who, {"dy", dy.p, dy.cs, dy.coff, C}, {"dx", dx.p, dx.cs, dx.coff, C}, {"acc1", acc1.p, acc1.cs, acc1.coff, C, kOptional},
                        {"acc2", acc2.p, acc2.cs, acc2.coff, C, kOptional});
    StencilArgs a;
    a.x = dy.p; a.w = w; a.bias = nullptr; a.ps = nullptr; a.pt = nullptr; a.r1 = acc1.p; a.r2 = acc2.p; a.pivot = nullptr;
    a.y = dx.p; a.ssum = nullptr; a.ssq = nullptr;
    a.x_cs = dy.cs; a.x_coff = dy.coff; a.B = B; a.H = H; a.W = W; a.C = C; a.w_cs = w_cs; a.y_cs = dx.cs; a.y_coff = dx.coff; a.act = SOMI_ACT_NONE;
    a.r1_cs = acc1.cs; a.r1_coff = acc1.coff; a.r2_cs = acc2.cs; a.r2_coff = acc2.coff; a.flip = 1;
    a.p = dplan(B, H, W, C, DL_FWD_BLOCKS);
    launch_stencil(k, a, (hipStream_t)stream);
    return launch_status("somi_dwlk_dgrad_nhwc_f32");
}

extern "C" size_t somi_dwlk_wgrad_workspace_floats(int B, int H, int W, int C, int k) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || k <= 0) return 0;
    return (size_t)dplan(B, H, W, C, DL_WGRAD_BLOCKS).nblk * (k * k + 1) * C;
}

extern "C" int somi_dwlk_wgrad_nhwc_f32(somi_slice x, somi_slice dy, int B, int H, int W, int C, int k, float *dw, float *db, int accumulate,
                                        float *workspace, size_t workspace_floats, somi_stream_t stream) {
    const char *who = "dwlk wgrad";
    if (int rc = check_size(who, B, H, W, C, k, x.cs > dy.cs ? x.cs : dy.cs)) return rc;
    SOMI_REQUIRE_SLICES(who, {"x", x.p, x.cs, x.coff, C}, {"dy", dy.p, dy.cs, dy.coff, C});
    SOMI_REQUIRE(dw && workspace && aligned16(workspace), SOMI_EINVAL, "%s: dw and a 16-byte aligned workspace are needed", who);
    SOMI_REQUIRE(workspace_floats >= somi_dwlk_wgrad_workspace_floats(B, H, W, C, k), SOMI_EWORKSPACE, "%s: workspace too small", who);
    WgradArgs a;
    a.x = x.p; a.dy = dy.p; a.part = workspace;
    a.x_cs = x.cs; a.x_coff = x.coff; a.dy_cs = dy.cs; a.dy_coff = dy.coff; a.B = B; a.H = H; a.W = W; a.C = C;
    a.p = dplan(B, H, W, C, DL_WGRAD_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(a.p.nblk, a.p.nchunk);
    if (k == 7) hipLaunchKernelGGL(dwlk_wgrad_kernel<7>, grid, dim3(DL_THREADS), 0, s, a);
    else hipLaunchKernelGGL(dwlk_wgrad_kernel<9>, grid, dim3(DL_THREADS), 0, s, a);
    hipLaunchKernelGGL(dwlk_wgrad_fold_kernel, dim3(cdiv((long)(k * k + 1) * C, DL_THREADS)), dim3(DL_THREADS), 0, s, (const float *)workspace, a.p.nblk,
                       k * k, C, dw, db, accumulate);
    return launch_status("somi_dwlk_wgrad_nhwc_f32");
}
