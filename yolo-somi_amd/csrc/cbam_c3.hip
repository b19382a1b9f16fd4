// Tail attention of the CBAM C3 family (SCBAMBottleneck, models/common.py:975-995; the bare C3CBAM row, :494-504): the pass that
// combines a map t with its channel gate ca (B, C) and its spatial gate sa (B, H, W) and writes a channel slice (+ a shortcut), and
// that pass's backward in the A / C shape of train_blocks.hip, with the spatial gate's own backward pluggable between the two.
//
//   product (mode 0):      out = t * ca * sa [+ res]
//   sigmoid-sum (mode 1):  out = sigmoid(t * (ca + sa)) [+ res]          (SCBAM: yc = ca * t, ys = sa * t, out = sigmoid(yc + ys))
//
// Backward, given dout:
//   pixel   per pixel:    dsa = sum_c g * t * (mode 0: ca, mode 1: 1),  g = dout (mode 0) or dout * o * (1 - o), o = sigmoid(t * (ca + sa));
//                         written raw, or times sa * (1 - sa) (the plain conv gate: somi_spatial_attn_bwd_f32 starts at the logit);
//                         amaxc = first argmax_c (t * ca);  amaxp = the first pixel of every (image, channel) maximum of t (step A's idiom)
//   chan    per element:  dt1 = (mode 0: dout * sa) + dstats0 / C + [c == amaxc] * dstats1
//                         mode 0: dca = sum_p dt1 * t,         dt = dt1 * ca
//                         mode 1: dca = sum_p (g + dt1) * t,   dt = g * (ca + sa) + dt1 * ca
// Every float sum is per-workgroup partials + a fixed-order finish (no float atomics): two launches are bit-identical.
#include "common.h"

namespace somi {

constexpr int GC_CHUNK = 256;        // pixels per workgroup in the per-image reduction of the chan pass

struct GcFwdArgs {
    somi_slice t, res, out;
    const float *ca, *sa;
    long n4;                         // pixels x channel quads
    int HW, C4;
};

template <int MODE>
__global__ __launch_bounds__(256) void gc_forward_kernel(GcFwdArgs a) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= a.n4) return;
    const long pix = i / a.C4;
    const int q = (int)(i - pix * a.C4);
    const long b = pix / a.HW;
    const f32x4 tv = ld4(at(a.t, pix, q)), cav = ld4(a.ca + b * a.C4 * 4 + 4 * q);
    const float sav = a.sa[pix];
    f32x4 o;
    if constexpr (MODE == 0) {
        o = tv * cav * sav;
    } else {
        const f32x4 z = tv * (cav + sav);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = sigmoidf_(z[e]);
    }
    if (a.res.p) o += ld4(at(a.res, pix, q));
    st4(at_w(a.out, pix, q), o);
}

struct GcPixArgs {
    somi_slice dout, t;
    const float *ca, *sa, *mxv;      // mxv NULL: no arg-max pixels
    float *dsa;
    int *amaxc, *amaxp;
    int B, HW, C, logit;
};

// Step A's geometry: LG lanes per pixel, the smallest power of two that covers the C / 4 quads; a wave takes 64 / LG pixels a trip.
template <int MODE>
__global__ __launch_bounds__(256) void gc_bwd_pixel_kernel(GcPixArgs a) {
    const int C = a.C, HW = a.HW;
    int LG = 64;
    while (LG > 1 && (LG >> 1) * 4 >= C) LG >>= 1;
    const int lane = threadIdx.x & 63, sub = lane / LG, sl = lane % LG, ppw = 64 / LG;
    const long wave_id = (blockIdx.x * 256L + threadIdx.x) >> 6, nwave = (long)gridDim.x * 4;
    const long npix = (long)a.B * HW;
    for (long p0 = wave_id * ppw; p0 < npix; p0 += nwave * ppw) {        // every lane of a wave makes the same trips: the shuffles below are whole
        const long p = p0 + sub;
        const bool on = p < npix;
        float s = 0.f, m = -__builtin_huge_valf();
        int mi = 0x7fffffff;
        if (on) {
            const long b = p / HW;
            const float *cr = a.ca + b * C;
            const float sav = a.sa[p];
            for (int c = sl * 4; c < C; c += LG * 4) {
                const f32x4 tq = ld4(at_ch(a.t, p, c));
                const f32x4 cq = ld4(cr + c);
                const f32x4 v = tq * cq;
                f32x4 g = ld4(at_ch(a.dout, p, c));
                if (a.mxv) {
                    const f32x4 mq = ld4(a.mxv + b * C + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (tq[e] == mq[e]) atomicMin(a.amaxp + b * C + c + e, (int)(p - b * HW));      // integer: order-independent
                }
                if constexpr (MODE == 0) {
                    s += (g[0] * v[0] + g[1] * v[1]) + (g[2] * v[2] + g[3] * v[3]);
                } else {
                    const f32x4 z = tq * (cq + sav);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float o = sigmoidf_(z[e]);
                        g[e] *= o * (1.f - o);
                    }
                    s += (g[0] * tq[0] + g[1] * tq[1]) + (g[2] * tq[2] + g[3] * tq[3]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v[e] > m) { m = v[e]; mi = c + e; }                  // first maximum inside the lane (ascending c)
            }
        }
        for (int o = LG >> 1; o > 0; o >>= 1) {
            s += __shfl_xor(s, o);
            const float om = __shfl_xor(m, o);
            const int oi = __shfl_xor(mi, o);
            if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }       // lowest index on ties (torch.max)
        }
        if (on && sl == 0) {
            const float sav = a.sa[p];
            a.dsa[p] = a.logit ? s * sav * (1.f - sav) : s;
            a.amaxc[p] = mi;
        }
    }
}

struct GcChanArgs {
    somi_slice dout, t, dt;          // dt may be dout itself (every element is read, then written, by one lane)
    const float *ca, *sa, *dstats;
    const int *amaxc;
    float *part;                     // [B][nchunk][C]
    int HW, C, nchunk, accumulate;
};

// grid (nchunk, B): lanes over channel quads, rows over the chunk's pixels (step C's geometry)
template <int MODE>
__global__ __launch_bounds__(256) void gc_bwd_chan_kernel(GcChanArgs a) {
    __shared__ f32x4 l1[256];
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int C = a.C, C4 = C >> 2, HW = a.HW;
    const int p0 = chunk * GC_CHUNK, p1 = min(p0 + GC_CHUNK, HW);
    const float inv_c = 1.f / (float)C;
    for (int cq0 = 0; cq0 < C4; cq0 += 256) {
        const int ncq = min(256, C4 - cq0);
        const int rows_par = 256 / ncq;
        const int cq = threadIdx.x % ncq, rr = threadIdx.x / ncq;
        const int c = (cq0 + cq) * 4;
        f32x4 s1 = {0.f, 0.f, 0.f, 0.f};
        if (rr < rows_par) {
            const f32x4 cav = ld4(a.ca + (long)b * C + c);
            auto one = [&](long p, const f32x4 tv, f32x4 g, const float2 ds, int am, float sav) {
                f32x4 d1 = splat4(ds.x * inv_c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e == am) d1[e] += ds.y;
                f32x4 r;
                if constexpr (MODE == 0) {
                    d1 += g * sav;
                    s1 += d1 * tv;
                    r = d1 * cav;
                } else {
                    const f32x4 w = cav + sav, z = tv * w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float o = sigmoidf_(z[e]);
                        g[e] *= o * (1.f - o);
                    }
                    s1 += (g + d1) * tv;
                    r = g * w + d1 * cav;
                }
                float *dst = at_ch_w(a.dt, p, c);
                if (a.accumulate) r += ld4(dst);
                st4(dst, r);
            };
            int pl = p0 + rr;
            for (; pl + 3 * rows_par < p1; pl += 4 * rows_par) {          // four pixels' loads go out together; sums and stores in pixel order
                f32x4 tv[4], g[4];
                float2 ds[4];
                int am[4];
                float sav[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long p = (long)b * HW + pl + u * rows_par;
                    tv[u] = ld4(at_ch(a.t, p, c));
                    g[u] = ld4(at_ch(a.dout, p, c));
                    ds[u] = *reinterpret_cast<const float2 *>(a.dstats + p * 2);
                    am[u] = a.amaxc[p];
                    sav[u] = a.sa[p];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) one((long)b * HW + pl + u * rows_par, tv[u], g[u], ds[u], am[u], sav[u]);
            }
            for (; pl < p1; pl += rows_par) {
                const long p = (long)b * HW + pl;
                one(p, ld4(at_ch(a.t, p, c)), ld4(at_ch(a.dout, p, c)), *reinterpret_cast<const float2 *>(a.dstats + p * 2), a.amaxc[p], a.sa[p]);
            }
        }
        l1[threadIdx.x] = s1;
        __syncthreads();
        if (threadIdx.x < ncq) {
            for (int r2 = 1; r2 < rows_par; ++r2) s1 += l1[r2 * ncq + cq];
            st4(a.part + ((long)b * a.nchunk + chunk) * C + c, s1);
        }
        __syncthreads();
    }
}

// dca[b][c] = the chunk partials in ascending order, fp64: one lane per (image, channel)
__global__ __launch_bounds__(256) void gc_finish_kernel(const float *__restrict__ part, int nchunk, int C, int BC, float *__restrict__ dca) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const int b = i / C, c = i - b * C;
    const float *pp = part + (long)b * nchunk * C + c;
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += (double)pp[(long)k * C];
    dca[i] = (float)s;
}

// the per-pixel pass: a wave per 64 / LG pixels and trip (LG = the lanes a pixel takes), at most GC_PIXEL_MAX_WG workgroups of four waves
constexpr int GC_PIXEL_MAX_WG = 2048;
static long gc_pixel_grid(int B, int HW) {
    const long g = ((long)B * HW * 64 + 255) / 256;
    return g > GC_PIXEL_MAX_WG ? GC_PIXEL_MAX_WG : g;
}
static int gc_pixel_lanes(int C) {
    int LG = 64;
    while (LG > 1 && (LG >> 1) * 4 >= C) LG >>= 1;
    return LG;
}

static int gc_sizes_ok(const char *who, int B, int HW, int C, int mode) {
    SOMI_REQUIRE(B > 0 && B <= 65535 && HW > 0 && (long)B * HW < (1L << 31), SOMI_EINVAL, "%s: bad sizes (batch <= 65535, fewer than 2^31 pixels)", who);
    SOMI_REQUIRE((long)B * C < (1L << 31), SOMI_EINVAL, "%s: bad sizes (B * C = %ld, fewer than 2^31 gate values)", who, (long)B * C);
    SOMI_REQUIRE(C > 0 && C % 4 == 0, SOMI_EINVAL, "%s: C = %d is not a multiple of 4 (a lane owns a channel quad)", who, C);
    SOMI_REQUIRE(mode == SOMI_GATE_PRODUCT || mode == SOMI_GATE_SIGMOID_SUM, SOMI_EINVAL, "%s: mode %d is neither product (0) nor sigmoid-sum (1)", who, mode);
    return 0;
}

}  // namespace somi

using namespace somi;

extern "C" int somi_gate_combine_nhwc_f32(somi_slice t, const float *ca, const float *sa, somi_slice residual, somi_slice out, int B, int HW, int C,
                                          int mode, somi_stream_t stream) {
    const char *who = "gate combine";
    if (int rc = gc_sizes_ok(who, B, HW, C, mode)) return rc;
    SOMI_REQUIRE_SLICES(who, {"t", t.p, t.cs, t.coff, C}, {"out", out.p, out.cs, out.coff, C},
                        {"residual", residual.p, residual.cs, residual.coff, C, kOptional});
    SOMI_REQUIRE(ca && sa && aligned16(ca), SOMI_EINVAL, "%s: ca (16-byte aligned) and sa are required", who);
    GcFwdArgs a;
    a.t = t; a.res = residual; a.out = out; a.ca = ca; a.sa = sa; a.HW = HW; a.C4 = C / 4;
    a.n4 = (long)B * HW * (C / 4);
    SOMI_REQUIRE(cdiv(a.n4, 256) > 0 && a.n4 / 256 < (1L << 31) - 1, SOMI_EINVAL, "%s: map too large", who);
    if (mode == SOMI_GATE_PRODUCT) hipLaunchKernelGGL(gc_forward_kernel<0>, dim3(cdiv(a.n4, 256)), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gc_forward_kernel<1>, dim3(cdiv(a.n4, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_gate_combine_nhwc_f32");
}

extern "C" int somi_gate_combine_bwd_pixel_f32(somi_slice dout, somi_slice t, const float *ca, const float *sa, const float *t_max, float *dsa,
                                               int32_t *amaxc, int32_t *amaxp, int B, int HW, int C, int mode, int logit, somi_stream_t stream) {
    const char *who = "gate combine bwd pixel";
    if (int rc = gc_sizes_ok(who, B, HW, C, mode)) return rc;
    SOMI_REQUIRE_SLICES(who, {"dout", dout.p, dout.cs, dout.coff, C}, {"t", t.p, t.cs, t.coff, C});
    SOMI_REQUIRE(ca && sa && dsa && amaxc && aligned16(ca), SOMI_EINVAL, "%s: ca (16-byte aligned), sa, dsa and amaxc are required", who);
    SOMI_REQUIRE((t_max == nullptr) == (amaxp == nullptr) && aligned16(t_max), SOMI_EINVAL, "%s: t_max (16-byte aligned) and amaxp come together", who);
    hipStream_t s = (hipStream_t)stream;
    if (amaxp && hipMemsetAsync(amaxp, 0x7f, (size_t)B * C * sizeof(int32_t), s) != hipSuccess) return launch_status(who);   // above every pixel index
    GcPixArgs a;
    a.dout = dout; a.t = t; a.ca = ca; a.sa = sa; a.mxv = t_max; a.dsa = dsa; a.amaxc = amaxc; a.amaxp = amaxp;
    a.B = B; a.HW = HW; a.C = C; a.logit = logit != 0;
    const long g = gc_pixel_grid(B, HW);
    if (mode == SOMI_GATE_PRODUCT) hipLaunchKernelGGL(gc_bwd_pixel_kernel<0>, dim3((int)g), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(gc_bwd_pixel_kernel<1>, dim3((int)g), dim3(256), 0, s, a);
    return launch_status("somi_gate_combine_bwd_pixel_f32");
}

extern "C" int somi_gate_combine_pixel_trips(int B, int HW, int C) {
    if (B <= 0 || B > 65535 || HW <= 0 || (long)B * HW >= (1L << 31) || C <= 0 || C % 4) return 0;
    const long per_trip = gc_pixel_grid(B, HW) * 4 * (64 / gc_pixel_lanes(C));
    return (int)(((long)B * HW + per_trip - 1) / per_trip);
}

extern "C" size_t somi_gate_combine_bwd_workspace_floats(int B, int HW, int C) {
    if (B <= 0 || HW <= 0 || C <= 0 || C % 4) return 0;
    return (size_t)B * cdiv(HW, GC_CHUNK) * C;
}

extern "C" int somi_gate_combine_bwd_chan_f32(somi_slice dout, somi_slice t, const float *ca, const float *sa, const float *dstats,
                                              const int32_t *amaxc, somi_slice dt, float *dca, float *workspace, size_t workspace_floats, int B,
                                              int HW, int C, int mode, int accumulate, somi_stream_t stream) {
    const char *who = "gate combine bwd chan";
    if (int rc = gc_sizes_ok(who, B, HW, C, mode)) return rc;
    SOMI_REQUIRE_SLICES(who, {"dout", dout.p, dout.cs, dout.coff, C}, {"t", t.p, t.cs, t.coff, C}, {"dt", dt.p, dt.cs, dt.coff, C});
    SOMI_REQUIRE(ca && sa && dstats && amaxc && dca && aligned16(ca) && (reinterpret_cast<uintptr_t>(dstats) & 7u) == 0, SOMI_EINVAL,
                 "%s: ca (16-byte aligned), sa, dstats (8-byte aligned), amaxc and dca are required", who);
    SOMI_REQUIRE(workspace && aligned16(workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
    SOMI_REQUIRE(workspace_floats >= somi_gate_combine_bwd_workspace_floats(B, HW, C), SOMI_EWORKSPACE, "%s: workspace too small", who);
    hipStream_t s = (hipStream_t)stream;
    GcChanArgs a;
    a.dout = dout; a.t = t; a.dt = dt; a.ca = ca; a.sa = sa; a.dstats = dstats; a.amaxc = amaxc; a.part = workspace;
    a.HW = HW; a.C = C; a.nchunk = cdiv(HW, GC_CHUNK); a.accumulate = accumulate != 0;
    if (mode == SOMI_GATE_PRODUCT) hipLaunchKernelGGL(gc_bwd_chan_kernel<0>, dim3(a.nchunk, B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(gc_bwd_chan_kernel<1>, dim3(a.nchunk, B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(gc_finish_kernel, dim3(cdiv((long)B * C, 256)), dim3(256), 0, s, workspace, a.nchunk, C, B * C, dca);
    return launch_status("somi_gate_combine_bwd_chan_f32");
}

// =================================================================================================================
// The depthwise-separable spatial gate of CBAMBottleneckDWC (SpatialAttentionModuleDWC / DepthWiseConv, models/common.py:361-389, 425-438) on
// the (B,H,W,2) map stats = [mean_c, max_c]:
//   u = depthwise k x k conv (2 channels, bias, pad k / 2);  v = relu(BN(u));  p = 1x1 conv 2 -> 1 (bias);  q = relu(BN1(p));  sa = sigmoid(q)
// params (2 k k + 11 floats): depth_conv.weight (2,1,k,k), depth_conv.bias (2), bn.weight (2), bn.bias (2), point_conv.weight (2),
// point_conv.bias (1), bn1.weight (1), bn1.bias (1); run (6): bn.running_mean (2), bn.running_var (2), bn1.running_mean, bn1.running_var;
// st (8): mean (2), rstd (2) of u, mean, rstd of p, two unused.
// The maps are tiny (2 N and N floats, N = B H W), so launches are the cost: the two training BatchNorms are two grid-wide reductions that
// follow one another, each closed by a kernel boundary - three launches forward.  At most DWC_MAX_WG workgroups walk the pixels grid-stride and
// leave fp64 partial sums; EVERY workgroup of the next launch adds them in the same fixed order (no float atomics, bit-identical launches),
// workgroup 0 also writes the statistics and the running statistics.
namespace somi {

constexpr int DWC_MAX_WG = 128;          // <= 256: a workgroup finishes the partials with one lane per partial row
constexpr int DWC_WCHUNK = 4096;         // pixels per workgroup of the weight-gradient partials

static int dwc_blocks(long N) { const long g = (N + 255) / 256; return (int)(g > DWC_MAX_WG ? DWC_MAX_WG : (g < 1 ? 1 : g)); }
static int dwc_wchunks(long N) { return (int)((N + DWC_WCHUNK - 1) / DWC_WCHUNK); }

struct DwcArgs {
    const float *stats, *params, *dsa;
    float *u, *p, *st, *run, *sa, *dz, *du, *dstats, *dparams;
    double *part;                        // this launch's partial rows (written) ...
    const double *prev;                  // ... and the previous launch's (read), nprev rows
    int nprev;
    int B, H, W, k;
    long N;
    float eps, momentum;
};

// offsets into params / dparams
__host__ __device__ inline int dwc_o_db(int k) { return 2 * k * k; }          // depth_conv.bias, then bn.weight +2, bn.bias +4, point w +6, point b +8, bn1 w +9, bn1 b +10

// sum over the workgroup, fixed order; every lane gets it
__device__ __forceinline__ double dwc_block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// column idx of the nprev partial rows (ncol wide), rows in ascending order
__device__ __forceinline__ double dwc_finish(const double *prev, int nprev, int ncol, int idx, double *red) {
    return dwc_block_sum((int)threadIdx.x < nprev ? prev[(long)threadIdx.x * ncol + idx] : 0.0, red);
}
__device__ __forceinline__ float dwc_conv_at(const DwcArgs &a, long pix, int j) {
    const int k = a.k, pad = k >> 1;
    const int wv = (int)(pix % a.W), hv = (int)((pix / a.W) % a.H);
    float acc = a.params[dwc_o_db(k) + j];
    for (int r = 0; r < k; ++r) {
        const int hi = hv + r - pad;
        if ((unsigned)hi >= (unsigned)a.H) continue;
        for (int q = 0; q < k; ++q) {
            const int wi = wv + q - pad;
            if ((unsigned)wi >= (unsigned)a.W) continue;
            acc += a.params[(j * k + r) * k + q] * a.stats[(pix + (long)(r - pad) * a.W + (q - pad)) * 2 + j];
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void dwc_fwd_conv_kernel(DwcArgs a) {
    __shared__ double red[4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long pix = blockIdx.x * 256L + threadIdx.x; pix < a.N; pix += (long)gridDim.x * 256) {
        const float u0 = dwc_conv_at(a, pix, 0), u1 = dwc_conv_at(a, pix, 1);
        *reinterpret_cast<float2 *>(a.u + pix * 2) = make_float2(u0, u1);
        s[0] += u0; s[1] += (double)u0 * u0; s[2] += u1; s[3] += (double)u1 * u1;
    }
    for (int i = 0; i < 4; ++i) {
        const double t = dwc_block_sum(s[i], red);
        if (threadIdx.x == 0) a.part[(long)blockIdx.x * 4 + i] = t;
    }
}

// mean / rstd of one channel from its finished sum and sum of squares; workgroup 0's lane 0 records them and moves the running statistics
__device__ __forceinline__ void dwc_bn_stats(const DwcArgs &a, double sum, double sumsq, int st_mean, int st_rstd, int run_mean, int run_var,
                                             float &mean, float &rstd) {
    const double m = sum / (double)a.N;
    double var = sumsq / (double)a.N - m * m;
    var = var < 0.0 ? 0.0 : var;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.st[st_mean] = mean;
        a.st[st_rstd] = rstd;
        if (a.run) {
            a.run[run_mean] = (1.f - a.momentum) * a.run[run_mean] + a.momentum * mean;
            a.run[run_var] = (1.f - a.momentum) * a.run[run_var] + a.momentum * (float)(var * (double)a.N / (double)(a.N - 1));
        }
    }
}

__global__ __launch_bounds__(256) void dwc_fwd_point_kernel(DwcArgs a) {
    __shared__ double red[4];
    const float *pr = a.params + dwc_o_db(a.k);
    float mean[2], rstd[2];
    for (int j = 0; j < 2; ++j) {
        const double sum = dwc_finish(a.prev, a.nprev, 4, 2 * j, red), sumsq = dwc_finish(a.prev, a.nprev, 4, 2 * j + 1, red);
        dwc_bn_stats(a, sum, sumsq, j, 2 + j, j, 2 + j, mean[j], rstd[j]);
    }
    double s0 = 0.0, s1 = 0.0;
    for (long pix = blockIdx.x * 256L + threadIdx.x; pix < a.N; pix += (long)gridDim.x * 256) {
        const float2 uu = *reinterpret_cast<const float2 *>(a.u + pix * 2);
        const float v0 = fmaxf(pr[2] * ((uu.x - mean[0]) * rstd[0]) + pr[4], 0.f), v1 = fmaxf(pr[3] * ((uu.y - mean[1]) * rstd[1]) + pr[5], 0.f);
        const float pv = pr[6] * v0 + pr[7] * v1 + pr[8];
        a.p[pix] = pv;
        s0 += pv; s1 += (double)pv * pv;
    }
    const double t0 = dwc_block_sum(s0, red), t1 = dwc_block_sum(s1, red);
    if (threadIdx.x == 0) { a.part[(long)blockIdx.x * 2] = t0; a.part[(long)blockIdx.x * 2 + 1] = t1; }
}

__global__ __launch_bounds__(256) void dwc_fwd_gate_kernel(DwcArgs a) {
    __shared__ double red[4];
    const float *pr = a.params + dwc_o_db(a.k);
    float mean, rstd;
    const double sum = dwc_finish(a.prev, a.nprev, 2, 0, red), sumsq = dwc_finish(a.prev, a.nprev, 2, 1, red);
    dwc_bn_stats(a, sum, sumsq, 4, 5, 4, 5, mean, rstd);
    for (long pix = blockIdx.x * 256L + threadIdx.x; pix < a.N; pix += (long)gridDim.x * 256)
        a.sa[pix] = sigmoidf_(fmaxf(pr[9] * ((a.p[pix] - mean) * rstd) + pr[10], 0.f));
}

// inference: running statistics, everything per pixel in one launch
__global__ __launch_bounds__(256) void dwc_eval_kernel(DwcArgs a) {
    const float *pr = a.params + dwc_o_db(a.k);
    const float r0 = rsqrtf(a.run[2] + a.eps), r1 = rsqrtf(a.run[3] + a.eps), r2 = rsqrtf(a.run[5] + a.eps);
    for (long pix = blockIdx.x * 256L + threadIdx.x; pix < a.N; pix += (long)gridDim.x * 256) {
        const float u0 = dwc_conv_at(a, pix, 0), u1 = dwc_conv_at(a, pix, 1);
        const float v0 = fmaxf(pr[2] * ((u0 - a.run[0]) * r0) + pr[4], 0.f), v1 = fmaxf(pr[3] * ((u1 - a.run[1]) * r1) + pr[5], 0.f);
        const float pv = pr[6] * v0 + pr[7] * v1 + pr[8];
        a.sa[pix] = sigmoidf_(fmaxf(pr[9] * ((pv - a.run[4]) * r2) + pr[10], 0.f));
    }
}

// ------------------------------------------------------------------------------------------------ backward
// d z1 of one pixel (z1 = BN1(p), q = relu(z1), sa = sigmoid(q)) from the raw dsa, and xhat1
__device__ __forceinline__ float dwc_dz1(const DwcArgs &a, const float *pr, long pix, float &xh) {
    xh = (a.p[pix] - a.st[4]) * a.st[5];
    const float z = pr[9] * xh + pr[10];
    if (!(z > 0.f)) return 0.f;
    const float s = sigmoidf_(z);
    return a.dsa[pix] * s * (1.f - s);
}

__global__ __launch_bounds__(256) void dwc_bwd_bn1_kernel(DwcArgs a) {
    __shared__ double red[4];
    const float *pr = a.params + dwc_o_db(a.k);
    double s1 = 0.0, s2 = 0.0;
    for (long pix = blockIdx.x * 256L + threadIdx.x; pix < a.N; pix += (long)gridDim.x * 256) {
        float xh;
        const float dz = dwc_dz1(a, pr, pix, xh);
        s1 += dz; s2 += (double)dz * xh;
    }
    const double t1 = dwc_block_sum(s1, red), t2 = dwc_block_sum(s2, red);
    if (threadIdx.x == 0) { a.part[(long)blockIdx.x * 2] = t1; a.part[(long)blockIdx.x * 2 + 1] = t2; }
}

__global__ __launch_bounds__(256) void dwc_bwd_point_kernel(DwcArgs a) {
    __shared__ double red[4];
    const float *pr = a.params + dwc_o_db(a.k);
    float *dp_ = a.dparams + dwc_o_db(a.k);
    const double S1 = dwc_finish(a.prev, a.nprev, 2, 0, red), S2 = dwc_finish(a.prev, a.nprev, 2, 1, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) { dp_[9] += (float)S2; dp_[10] += (float)S1; }
    // the two means stay in fp64: rounded to fp32 they would shift every pixel's dp the same way, N roundings that add up in the sums below
    const double m1 = S1 / (double)a.N, m2 = S2 / (double)a.N, g1r = (double)pr[9] * (double)a.st[5];
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long pix = blockIdx.x * 256L + threadIdx.x; pix < a.N; pix += (long)gridDim.x * 256) {
        float xh1;
        const float dz1 = dwc_dz1(a, pr, pix, xh1);
        const float dp = (float)(g1r * ((double)dz1 - m1 - (double)xh1 * m2));
        const float2 uu = *reinterpret_cast<const float2 *>(a.u + pix * 2);
        const float xh[2] = {(uu.x - a.st[0]) * a.st[2], (uu.y - a.st[1]) * a.st[3]};
        float dzv[2];
        s[0] += dp;
        for (int j = 0; j < 2; ++j) {
            const float z = pr[2 + j] * xh[j] + pr[4 + j];
            const bool on = z > 0.f;
            s[1 + j] += on ? (double)dp * z : 0.0;               // d point_conv.weight[j] = sum dp * v_j, v_j = relu(z)
            dzv[j] = on ? dp * pr[6 + j] : 0.f;
            s[3 + 2 * j] += dzv[j];
            s[4 + 2 * j] += (double)dzv[j] * xh[j];
        }
        *reinterpret_cast<float2 *>(a.dz + pix * 2) = make_float2(dzv[0], dzv[1]);
    }
    for (int i = 0; i < 7; ++i) {
        const double t = dwc_block_sum(s[i], red);
        if (threadIdx.x == 0) a.part[(long)blockIdx.x * 7 + i] = t;
    }
}

__global__ __launch_bounds__(256) void dwc_bwd_bn_kernel(DwcArgs a) {
    __shared__ double red[4];
    const float *pr = a.params + dwc_o_db(a.k);
    float *dp_ = a.dparams + dwc_o_db(a.k);
    double S[7];
    for (int i = 0; i < 7; ++i) S[i] = dwc_finish(a.prev, a.nprev, 7, i, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        dp_[8] += (float)S[0];                                    // point_conv.bias
        dp_[6] += (float)S[1]; dp_[7] += (float)S[2];             // point_conv.weight
        dp_[4] += (float)S[3]; dp_[2] += (float)S[4];             // bn.bias[0], bn.weight[0]
        dp_[5] += (float)S[5]; dp_[3] += (float)S[6];             // bn.bias[1], bn.weight[1]
    }
    const double t1[2] = {S[3] / (double)a.N, S[5] / (double)a.N}, t2[2] = {S[4] / (double)a.N, S[6] / (double)a.N};      // fp64, as above
    const double gr[2] = {(double)pr[2] * (double)a.st[2], (double)pr[3] * (double)a.st[3]};
    for (long pix = blockIdx.x * 256L + threadIdx.x; pix < a.N; pix += (long)gridDim.x * 256) {
        const float2 uu = *reinterpret_cast<const float2 *>(a.u + pix * 2), dz = *reinterpret_cast<const float2 *>(a.dz + pix * 2);
        const float xh0 = (uu.x - a.st[0]) * a.st[2], xh1 = (uu.y - a.st[1]) * a.st[3];
        *reinterpret_cast<float2 *>(a.du + pix * 2) =
            make_float2((float)(gr[0] * ((double)dz.x - t1[0] - (double)xh0 * t2[0])), (float)(gr[1] * ((double)dz.y - t1[1] - (double)xh1 * t2[1])));
    }
}

// dstats = the transposed depthwise stencil of du
__global__ __launch_bounds__(256) void dwc_bwd_data_kernel(DwcArgs a) {
    const int k = a.k, pad = k >> 1;
    for (long pix = blockIdx.x * 256L + threadIdx.x; pix < a.N; pix += (long)gridDim.x * 256) {
        const int wv = (int)(pix % a.W), hv = (int)((pix / a.W) % a.H);
        float a0 = 0.f, a1 = 0.f;
        for (int r = 0; r < k; ++r) {
            const int ho = hv - (r - pad);                            // u[ho, wo] read stats[ho + r - pad, wo + q - pad]
            if ((unsigned)ho >= (unsigned)a.H) continue;
            for (int q = 0; q < k; ++q) {
                const int wo = wv - (q - pad);
                if ((unsigned)wo >= (unsigned)a.W) continue;
                const float2 g = *reinterpret_cast<const float2 *>(a.du + (pix - (long)(r - pad) * a.W - (q - pad)) * 2);
                a0 += g.x * a.params[r * k + q];
                a1 += g.y * a.params[(k + r) * k + q];
            }
        }
        *reinterpret_cast<float2 *>(a.dstats + pix * 2) = make_float2(a0, a1);
    }
}

// grid (chunks, 2 k k + 2): workgroup (chunk, jw) sums one tap gradient (jw < 2 k k, nn.Conv2d's (2,1,k,k) order) or one bias gradient over a chunk
__global__ __launch_bounds__(256) void dwc_bwd_weight_kernel(DwcArgs a) {
    __shared__ double red[4];
    const int k = a.k, kk = k * k, pad = k >> 1, jw = blockIdx.y;
    const long p0 = (long)blockIdx.x * DWC_WCHUNK, p1 = min(p0 + (long)DWC_WCHUNK, a.N);
    double acc = 0.0;
    if (jw >= 2 * kk) {
        const int j = jw - 2 * kk;
        for (long pix = p0 + threadIdx.x; pix < p1; pix += 256) acc += (double)a.du[pix * 2 + j];
    } else {
        const int j = jw / kk, r = (jw % kk) / k, q = jw % k;
        for (long pix = p0 + threadIdx.x; pix < p1; pix += 256) {
            const int wv = (int)(pix % a.W), hv = (int)((pix / a.W) % a.H);
            const int hi = hv + r - pad, wi = wv + q - pad;
            if ((unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W)
                acc += (double)a.du[pix * 2 + j] * (double)a.stats[(pix + (long)(r - pad) * a.W + (q - pad)) * 2 + j];
        }
    }
    const double t = dwc_block_sum(acc, red);
    if (threadIdx.x == 0) a.part[(long)blockIdx.x * (2 * kk + 2) + jw] = t;
}
// one workgroup per gradient: the chunk partials lane-strided, then the fixed-order workgroup sum
__global__ __launch_bounds__(256) void dwc_bwd_weight_final(DwcArgs a) {
    __shared__ double red[4];
    const int ncol = 2 * a.k * a.k + 2, jw = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < a.nprev; i += 256) s += a.prev[(long)i * ncol + jw];
    const double t = dwc_block_sum(s, red);
    if (threadIdx.x == 0) a.dparams[jw] += (float)t;               // taps, then depth_conv.bias: the first 2 k k + 2 entries of the layout
}

static int dwc_args_ok(const char *who, int B, int H, int W, int k) {
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 30), SOMI_EINVAL, "%s: bad sizes (fewer than 2^30 pixels)", who);
    SOMI_REQUIRE(k == 3 || k == 7, SOMI_EINVAL, "%s: kernel_size %d is not built, only 3 and 7", who, k);
    return 0;
}
// workspace layout in doubles: [bn1 | point | bn] partial rows of DWC_MAX_WG workgroups, the weight partial rows; then floats: dz, du
static size_t dwc_ws_doubles(long N, int k) { return (size_t)DWC_MAX_WG * (4 + 2 + 7) + (size_t)dwc_wchunks(N) * (2 * k * k + 2); }

}  // namespace somi

extern "C" size_t somi_dwc_gate_workspace_floats(int B, int H, int W, int k) {
    if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W >= (1L << 30) || (k != 3 && k != 7)) return 0;
    const long N = (long)B * H * W;
    return 2 * dwc_ws_doubles(N, k) + 4 * (size_t)N + 4;
}

extern "C" int somi_dwc_gate_trips(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W >= (1L << 30)) return 0;
    const long N = (long)B * H * W;
    return (int)((N + dwc_blocks(N) * 256L - 1) / (dwc_blocks(N) * 256L));
}

extern "C" int somi_dwc_gate_eval_f32(const float *stats, const float *params, const float *run, float *sa, int B, int H, int W, int k, float eps,
                                      somi_stream_t stream) {
    const char *who = "dwc gate eval";
    if (int rc = dwc_args_ok(who, B, H, W, k)) return rc;
    SOMI_REQUIRE(stats && params && run && sa && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0, SOMI_EINVAL,
                 "%s: stats (8-byte aligned), params, run and sa are required", who);
    DwcArgs a = {};
    a.stats = stats; a.params = params; a.run = const_cast<float *>(run); a.sa = sa; a.B = B; a.H = H; a.W = W; a.k = k; a.N = (long)B * H * W; a.eps = eps;
    hipLaunchKernelGGL(dwc_eval_kernel, dim3(dwc_blocks(a.N)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_dwc_gate_eval_f32");
}

extern "C" int somi_dwc_gate_train_f32(const float *stats, const float *params, float *u, float *p, float *st, float *run, float momentum, float eps,
                                       float *sa, float *workspace, size_t workspace_floats, int B, int H, int W, int k, somi_stream_t stream) {
    const char *who = "dwc gate train";
    if (int rc = dwc_args_ok(who, B, H, W, k)) return rc;
    SOMI_REQUIRE((long)B * H * W > 1, SOMI_EINVAL, "%s: batch statistics need more than one value per channel", who);
    SOMI_REQUIRE(stats && params && u && p && st && sa && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0 && (reinterpret_cast<uintptr_t>(u) & 7u) == 0,
                 SOMI_EINVAL, "%s: stats and u (8-byte aligned), params, p, st and sa are required", who);
    SOMI_REQUIRE(workspace && aligned16(workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
    SOMI_REQUIRE(workspace_floats >= somi_dwc_gate_workspace_floats(B, H, W, k), SOMI_EWORKSPACE, "%s: workspace too small", who);
    hipStream_t s = (hipStream_t)stream;
    DwcArgs a = {};
    a.stats = stats; a.params = params; a.u = u; a.p = p; a.st = st; a.run = run; a.sa = sa; a.B = B; a.H = H; a.W = W; a.k = k;
    a.N = (long)B * H * W; a.eps = eps; a.momentum = momentum;
    const int nb = dwc_blocks(a.N);
    double *pa = reinterpret_cast<double *>(workspace), *pb = pa + (size_t)DWC_MAX_WG * 4;
    a.part = pa;
    hipLaunchKernelGGL(dwc_fwd_conv_kernel, dim3(nb), dim3(256), 0, s, a);
    a.prev = pa; a.nprev = nb; a.part = pb;
    hipLaunchKernelGGL(dwc_fwd_point_kernel, dim3(nb), dim3(256), 0, s, a);
    a.prev = pb; a.part = nullptr;
    hipLaunchKernelGGL(dwc_fwd_gate_kernel, dim3(nb), dim3(256), 0, s, a);
    return launch_status("somi_dwc_gate_train_f32");
}

extern "C" int somi_dwc_gate_bwd_f32(const float *dsa, const float *stats, const float *u, const float *p, const float *st, const float *params,
                                     float *dstats, float *dparams_accumulate, float *workspace, size_t workspace_floats, int B, int H, int W, int k,
                                     somi_stream_t stream) {
    const char *who = "dwc gate bwd";
    if (int rc = dwc_args_ok(who, B, H, W, k)) return rc;
    SOMI_REQUIRE((long)B * H * W > 1, SOMI_EINVAL, "%s: batch statistics need more than one value per channel", who);
    SOMI_REQUIRE(dsa && stats && u && p && st && params && dstats && dparams_accumulate && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0 &&
                     (reinterpret_cast<uintptr_t>(u) & 7u) == 0 && (reinterpret_cast<uintptr_t>(dstats) & 7u) == 0, SOMI_EINVAL,
                 "%s: dsa, stats / u / dstats (8-byte aligned), p, st, params and dparams are required", who);
    SOMI_REQUIRE(workspace && aligned16(workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
    SOMI_REQUIRE(workspace_floats >= somi_dwc_gate_workspace_floats(B, H, W, k), SOMI_EWORKSPACE, "%s: workspace too small", who);
    hipStream_t s = (hipStream_t)stream;
    DwcArgs a = {};
    a.dsa = dsa; a.stats = stats; a.u = const_cast<float *>(u); a.p = const_cast<float *>(p); a.st = const_cast<float *>(st); a.params = params;
    a.dstats = dstats; a.dparams = dparams_accumulate; a.B = B; a.H = H; a.W = W; a.k = k; a.N = (long)B * H * W;
    const int nb = dwc_blocks(a.N), nch = dwc_wchunks(a.N), ncol = 2 * k * k + 2;
    double *p1 = reinterpret_cast<double *>(workspace), *p2 = p1 + (size_t)DWC_MAX_WG * 4, *p3 = p2 + (size_t)DWC_MAX_WG * 2;
    double *pw = p1 + (size_t)DWC_MAX_WG * 13;
    a.dz = reinterpret_cast<float *>(p1 + dwc_ws_doubles(a.N, k));
    a.du = a.dz + 2 * a.N;
    a.part = p2;
    hipLaunchKernelGGL(dwc_bwd_bn1_kernel, dim3(nb), dim3(256), 0, s, a);
    a.prev = p2; a.nprev = nb; a.part = p3;
    hipLaunchKernelGGL(dwc_bwd_point_kernel, dim3(nb), dim3(256), 0, s, a);
    a.prev = p3; a.part = nullptr;
    hipLaunchKernelGGL(dwc_bwd_bn_kernel, dim3(nb), dim3(256), 0, s, a);
    hipLaunchKernelGGL(dwc_bwd_data_kernel, dim3(nb), dim3(256), 0, s, a);
    a.part = pw;
    hipLaunchKernelGGL(dwc_bwd_weight_kernel, dim3(nch, ncol), dim3(256), 0, s, a);
    a.prev = pw; a.nprev = nch;
    hipLaunchKernelGGL(dwc_bwd_weight_final, dim3(ncol), dim3(256), 0, s, a);
    return launch_status("somi_dwc_gate_bwd_f32");
}
