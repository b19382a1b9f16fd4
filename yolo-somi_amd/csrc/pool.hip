// Max-pooling outside SPPF's chained 5x5 (layers.hip / train_blocks.hip): the strided 2x2 pool of nn.MaxPool2d(2, s, 0) with an optional ZERO pad folded
// into the read (yolov3-tiny: nn.ZeroPad2d([0, 1, 0, 1]) + nn.MaxPool2d(2, 1, 0)), ASFF's F.max_pool2d(x, 3, 2, 1) with its -inf pad, and the PARALLEL stride-1 windows of SPP(k) for any ascending set of
// odd k in 3..13 (yolov3-spp, yolov5-p6 (3, 5, 7), yolov5-p7 (3, 5)).  NHWC fp32, channel slices (cs, coff), a lane owns one channel quad of one pixel:
// 16-byte loads and stores, contiguous across the wave.  No LDS: every tap of a window is another lane's own pixel one row or column over, so the
// re-reads hit L1 / L2, and the kernels move one read of x and one write per output slice through HBM.
//
// Routing rule (both forms): a pooled value's gradient goes to the FIRST maximum of its full window in row-major order - what torch's max_pool2d
// autograd does on the CPU.  The forward walks the window row-major and replaces the running maximum only on a strict `>`, and leaves the winner's
// position r * k + q as one byte per pooled element; the backward is owner-computes (each dx element gathers, in a fixed order, the gradients of the
// outputs whose byte points at it): no search, no float atomics, run-to-run bit-identical.
#include "common.h"

namespace somi {

static inline int pool_grid(long items) {
    long g = (items + 255) / 256;
    const long cap = 256L * 8;   // 8 workgroups per CU, grid-stride beyond that
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// the item index is split into (image, row, column, channel quad) by divisions with run-time divisors: 32-bit ones when the item count allows (every
// shape of a 640 px batch does), 64-bit otherwise; addresses are 64-bit either way
static inline bool small_index(long items) { return items + 256L * 8 * 256 < (1L << 32); }

__device__ __forceinline__ uint32_t pack_codes(const int (&mi)[4]) {
    return (uint32_t)mi[0] | ((uint32_t)mi[1] << 8) | ((uint32_t)mi[2] << 16) | ((uint32_t)mi[3] << 24);
}

// ------------------------------------------------------------------------------------------------ 2x2, stride 1 or 2, zero pad (left, top) folded in
// y[b, ho, wo] = max over (r, q) in 2x2 of xp[b, ho*s + r, wo*s + q], xp = x zero-padded by (pl, pr, pt, pb).  A padded position is a real 0 that
// can win the max (after SiLU an activation may be negative); its code then points outside x and no dx element ever gathers it: the gradient is dropped,
// exactly as F.pad + max_pool2d does.
template <typename IDX>
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, uint8_t *__restrict__ codes, int B, int H,
                                                           int W, int Ho, int Wo, int C, int x_cs, int x_coff, int y_cs, int y_coff, int s, int pl,
                                                           int pt) {
    const int C4 = C >> 2;
    const IDX items = (IDX)B * Ho * Wo * C4;
    for (IDX it = (IDX)blockIdx.x * 256 + threadIdx.x; it < items; it += (IDX)gridDim.x * 256) {
        const int c = (int)(it % (IDX)C4) * 4;
        const IDX pixi = it / (IDX)C4, rowi = pixi / (IDX)Wo;
        const int wo = (int)(pixi - rowi * Wo), ho = (int)(rowi % (IDX)Ho);
        const long pix = (long)pixi, b = (long)(rowi / (IDX)Ho);
        f32x4 m = {0.f, 0.f, 0.f, 0.f};
        int mi[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int hi = ho * s - pt + r;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int wi = wo * s - pl + q;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if ((unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W)
                    v = *reinterpret_cast<const f32x4 *>(x + ((b * H + hi) * W + wi) * x_cs + x_coff + c);
                if (r == 0 && q == 0) { m = v; continue; }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v[e] > m[e]) { m[e] = v[e]; mi[e] = r * 2 + q; }
            }
        }
        *reinterpret_cast<f32x4 *>(y + pix * y_cs + y_coff + c) = m;
        if (codes) *reinterpret_cast<uint32_t *>(codes + pix * C + c) = pack_codes(mi);
    }
}

// dx[b, h, w] = sum over the outputs (ho, wo) whose window holds (h, w) at tap (r, q) and whose code is r * 2 + q, taps in row-major order.  At stride 2
// the windows do not overlap: at most one output per element, a pure scatter written from the owner's side.  Elements no window covers get 0.
template <typename IDX>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float *__restrict__ dy, const uint8_t *__restrict__ codes, float *__restrict__ dx, int B,
                                                           int H, int W, int Ho, int Wo, int C, int dy_cs, int dy_coff, int dx_cs, int dx_coff, int s,
                                                           int pl, int pt) {
    const int C4 = C >> 2;
    const IDX items = (IDX)B * H * W * C4;
    for (IDX it = (IDX)blockIdx.x * 256 + threadIdx.x; it < items; it += (IDX)gridDim.x * 256) {
        const int c = (int)(it % (IDX)C4) * 4;
        const IDX pixi = it / (IDX)C4, rowi = pixi / (IDX)W;
        const int wv = (int)(pixi - rowi * W), hv = (int)(rowi % (IDX)H);
        const long pix = (long)pixi, b = (long)(rowi / (IDX)H);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int th = hv + pt - r;
            if (th < 0 || th % s) continue;
            const int ho = th / s;
            if (ho >= Ho) continue;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int tw = wv + pl - q;
                if (tw < 0 || tw % s) continue;
                const int wo = tw / s;
                if (wo >= Wo) continue;
                const long o = (b * Ho + ho) * Wo + wo;
                const uint32_t code = *reinterpret_cast<const uint32_t *>(codes + o * C + c);
                const f32x4 d = *reinterpret_cast<const f32x4 *>(dy + o * dy_cs + dy_coff + c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (((code >> (8 * e)) & 0xFFu) == (uint32_t)(r * 2 + q)) acc[e] += d[e];
            }
        }
        *reinterpret_cast<f32x4 *>(dx + pix * dx_cs + dx_coff + c) = acc;
    }
}

// ------------------------------------------------------------------------------------------------ 3x3, stride 2, implicit -inf pad of 1
// F.max_pool2d(x, 3, stride=2, padding=1) (ASFF level 0, models/common.py:5536): y[b, ho, wo] = max over (r, q) in 3x3 of x[b, 2 ho - 1 + r, 2 wo - 1 + q],
// positions outside x never win (the pad is -inf, unlike maxpool2's zero border).  The centre tap (1, 1) is always inside x.
template <typename IDX>
__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, uint8_t *__restrict__ codes, int B, int H,
                                                             int W, int Ho, int Wo, int C, int x_cs, int x_coff, int y_cs, int y_coff) {
    const int C4 = C >> 2;
    const IDX items = (IDX)B * Ho * Wo * C4;
    for (IDX it = (IDX)blockIdx.x * 256 + threadIdx.x; it < items; it += (IDX)gridDim.x * 256) {
        const int c = (int)(it % (IDX)C4) * 4;
        const IDX pixi = it / (IDX)C4, rowi = pixi / (IDX)Wo;
        const int wo = (int)(pixi - rowi * Wo), ho = (int)(rowi % (IDX)Ho);
        const long pix = (long)pixi, b = (long)(rowi / (IDX)Ho);
        const float ninf = -__builtin_huge_valf();
        f32x4 m = {ninf, ninf, ninf, ninf};
        int mi[4] = {4, 4, 4, 4};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int hi = ho * 2 - 1 + r;
            if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int wi = wo * 2 - 1 + q;
                if ((unsigned)wi >= (unsigned)W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4 *>(x + ((b * H + hi) * W + wi) * x_cs + x_coff + c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v[e] > m[e]) { m[e] = v[e]; mi[e] = r * 3 + q; }
            }
        }
        *reinterpret_cast<f32x4 *>(y + pix * y_cs + y_coff + c) = m;
        if (codes) *reinterpret_cast<uint32_t *>(codes + pix * C + c) = pack_codes(mi);
    }
}

// dx[b, h, w] = sum over the up to four windows (ho, wo) that hold (h, w) at tap (r, q) and whose code is r * 3 + q, the WINDOWS in row-major order (taps
// descending) - the order in which torch's CPU backward adds them, so the sums agree bit for bit.  Written by the element's owner only.
template <typename IDX>
__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const float *__restrict__ dy, const uint8_t *__restrict__ codes, float *__restrict__ dx, int B,
                                                             int H, int W, int Ho, int Wo, int C, int dy_cs, int dy_coff, int dx_cs, int dx_coff) {
    const int C4 = C >> 2;
    const IDX items = (IDX)B * H * W * C4;
    for (IDX it = (IDX)blockIdx.x * 256 + threadIdx.x; it < items; it += (IDX)gridDim.x * 256) {
        const int c = (int)(it % (IDX)C4) * 4;
        const IDX pixi = it / (IDX)C4, rowi = pixi / (IDX)W;
        const int wv = (int)(pixi - rowi * W), hv = (int)(rowi % (IDX)H);
        const long pix = (long)pixi, b = (long)(rowi / (IDX)H);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 2; r >= 0; --r) {
            const int th = hv + 1 - r;
            if (th < 0 || (th & 1)) continue;
            const int ho = th >> 1;
            if (ho >= Ho) continue;
#pragma unroll
            for (int q = 2; q >= 0; --q) {
                const int tw = wv + 1 - q;
                if (tw < 0 || (tw & 1)) continue;
                const int wo = tw >> 1;
                if (wo >= Wo) continue;
                const long o = (b * Ho + ho) * Wo + wo;
                const uint32_t code = *reinterpret_cast<const uint32_t *>(codes + o * C + c);
                const f32x4 d = *reinterpret_cast<const f32x4 *>(dy + o * dy_cs + dy_coff + c);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (((code >> (8 * e)) & 0xFFu) == (uint32_t)(r * 3 + q)) acc[e] += d[e];
            }
        }
        *reinterpret_cast<f32x4 *>(dx + pix * dx_cs + dx_coff + c) = acc;
    }
}

// ------------------------------------------------------------------------------------------------ SPP: NK parallel stride-1 windows, -inf pad of k / 2
struct SppK { int k[3]; };

// One row-major walk over the LARGEST window serves every window of the set (a smaller window is the centre part of it, walked in the same order), so
// x is read once per tap of the largest window, not once per tap of each.  Slice i + 1 of the concat buffer = pool_k[i](slice 0); slice 0 is only read
// and slices 1.. only written, so the buffer is updated in place.
template <int NK, typename IDX>
__global__ __launch_bounds__(256) void spp_pool_fwd_kernel(float *buf, uint8_t *__restrict__ codes, int B, int H, int W, int C, int cs, int x_coff,
                                                           SppK kk) {
    const int C4 = C >> 2;
    const IDX items = (IDX)B * H * W * C4;
    const long plane = (long)B * H * W;
    const int P = kk.k[NK - 1] >> 1;
    for (IDX it = (IDX)blockIdx.x * 256 + threadIdx.x; it < items; it += (IDX)gridDim.x * 256) {
        const int c = (int)(it % (IDX)C4) * 4;
        const IDX pixi = it / (IDX)C4, rowi = pixi / (IDX)W;
        const int wv = (int)(pixi - rowi * W), hv = (int)(rowi % (IDX)H);
        const long pix = (long)pixi, b = (long)(rowi / (IDX)H);
        const float ninf = -__builtin_huge_valf();
        f32x4 m[NK];
        int mi[NK][4];
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int ctr = (kk.k[i] >> 1) * (kk.k[i] + 1);             // the centre; every window contains it
            m[i] = f32x4{ninf, ninf, ninf, ninf};
            mi[i][0] = mi[i][1] = mi[i][2] = mi[i][3] = ctr;
        }
        for (int dr = -P; dr <= P; ++dr) {
            const int hi = hv + dr;
            if ((unsigned)hi >= (unsigned)H) continue;
            const int adr = dr < 0 ? -dr : dr;
            for (int dq = -P; dq <= P; ++dq) {
                const int wi = wv + dq;
                if ((unsigned)wi >= (unsigned)W) continue;
                const int adq = dq < 0 ? -dq : dq;
                const f32x4 v = *reinterpret_cast<const f32x4 *>(buf + ((b * H + hi) * W + wi) * cs + x_coff + c);
#pragma unroll
                for (int i = 0; i < NK; ++i) {
                    const int p = kk.k[i] >> 1;
                    if (adr > p || adq > p) continue;                   // wave-uniform: this tap lies outside window i
                    const int code = (dr + p) * kk.k[i] + dq + p;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (v[e] > m[i][e]) { m[i][e] = v[e]; mi[i][e] = code; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            *reinterpret_cast<f32x4 *>(buf + pix * cs + x_coff + (i + 1) * C + c) = m[i];
            if (codes) *reinterpret_cast<uint32_t *>(codes + ((long)i * plane + pix) * C + c) = pack_codes(mi[i]);
        }
    }
}

// slice 0 of dbuf += the gradients of slices 1..NK routed by the codes: element p gathers from output o = p + (dh, dw) of window i when that output's
// code is (k/2 - dh) * k + (k/2 - dw), offsets row-major and windows ascending inside each offset.  Slice 0 is read and written by its owner only.
template <int NK, typename IDX>
__global__ __launch_bounds__(256) void spp_pool_bwd_kernel(const uint8_t *__restrict__ codes, float *dbuf, int B, int H, int W, int C, int cs,
                                                           int x_coff, SppK kk) {
    const int C4 = C >> 2;
    const IDX items = (IDX)B * H * W * C4;
    const long plane = (long)B * H * W;
    const int P = kk.k[NK - 1] >> 1;
    for (IDX it = (IDX)blockIdx.x * 256 + threadIdx.x; it < items; it += (IDX)gridDim.x * 256) {
        const int c = (int)(it % (IDX)C4) * 4;
        const IDX pixi = it / (IDX)C4, rowi = pixi / (IDX)W;
        const int wv = (int)(pixi - rowi * W), hv = (int)(rowi % (IDX)H);
        const long pix = (long)pixi, b = (long)(rowi / (IDX)H);
        float *mine = dbuf + pix * cs + x_coff + c;
        f32x4 acc = *reinterpret_cast<const f32x4 *>(mine);
        for (int dh = -P; dh <= P; ++dh) {
            const int ho = hv + dh;
            if ((unsigned)ho >= (unsigned)H) continue;
            const int adh = dh < 0 ? -dh : dh;
            for (int dw = -P; dw <= P; ++dw) {
                const int wo = wv + dw;
                if ((unsigned)wo >= (unsigned)W) continue;
                const int adw = dw < 0 ? -dw : dw;
                const long o = (b * H + ho) * W + wo;
#pragma unroll
                for (int i = 0; i < NK; ++i) {
                    const int p = kk.k[i] >> 1;
                    if (adh > p || adw > p) continue;
                    const uint32_t want = (uint32_t)((p - dh) * kk.k[i] + (p - dw));
                    const uint32_t x = *reinterpret_cast<const uint32_t *>(codes + ((long)i * plane + o) * C + c) ^ (want * 0x01010101u);
                    if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) continue;     // no zero byte: none of the four channels points here
                    const f32x4 d = *reinterpret_cast<const f32x4 *>(dbuf + o * cs + x_coff + (i + 1) * C + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (((x >> (8 * e)) & 0xFFu) == 0) acc[e] += d[e];
                }
            }
        }
        *reinterpret_cast<f32x4 *>(mine) = acc;
    }
}

static bool spp_windows_ok(int nk, int k0, int k1, int k2, SppK &kk) {
    const int k[3] = {k0, k1, k2};
    if (nk < 1 || nk > 3) return false;
    for (int i = 0; i < 3; ++i) kk.k[i] = i < nk ? k[i] : k[nk - 1];
    for (int i = 0; i < nk; ++i)
        if (k[i] < 3 || k[i] > 13 || !(k[i] & 1) || (i && k[i] <= k[i - 1])) return false;
    return true;
}

}  // namespace somi

using namespace somi;

static bool pool2_shape(int H, int W, int stride, int pl, int pr, int pt, int pb, int &Ho, int &Wo) {
    if (stride != 1 && stride != 2) return false;
    if (pl < 0 || pr < 0 || pt < 0 || pb < 0 || pl > 1 || pr > 1 || pt > 1 || pb > 1) return false;   // a pad wider than k - 1 would give all-pad windows
    if (H + pt + pb < 2 || W + pl + pr < 2) return false;
    Ho = (H + pt + pb - 2) / stride + 1;
    Wo = (W + pl + pr - 2) / stride + 1;
    return true;
}

extern "C" int somi_maxpool2_nhwc_f32(const float *x, float *y, void *codes, int B, int H, int W, int C, int x_cs, int x_coff, int y_cs, int y_coff,
                                      int stride, int pad_l, int pad_r, int pad_t, int pad_b, somi_stream_t stream) {
    int Ho = 0, Wo = 0;
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && C % 4 == 0 && (!codes || aligned16(codes)), SOMI_EINVAL,
                 "maxpool2: bad sizes (C a multiple of 4), or codes not 16-byte aligned");
    SOMI_REQUIRE(pool2_shape(H, W, stride, pad_l, pad_r, pad_t, pad_b, Ho, Wo), SOMI_EINVAL,
                 "maxpool2: kernel 2 with stride 1 or 2 and a zero pad of 0 or 1 per side only, and the padded map must hold one window");
    SOMI_REQUIRE_SLICES("maxpool2", {"x", x, x_cs, x_coff, C}, {"y", y, y_cs, y_coff, C});
    const long items = (long)B * Ho * Wo * (C / 4);
    if (small_index(items))
        hipLaunchKernelGGL(maxpool2_fwd_kernel<uint32_t>, dim3(pool_grid(items)), dim3(256), 0, (hipStream_t)stream, x, y, (uint8_t *)codes, B, H, W, Ho,
                           Wo, C, x_cs, x_coff, y_cs, y_coff, stride, pad_l, pad_t);
    else
        hipLaunchKernelGGL(maxpool2_fwd_kernel<uint64_t>, dim3(pool_grid(items)), dim3(256), 0, (hipStream_t)stream, x, y, (uint8_t *)codes, B, H, W, Ho,
                           Wo, C, x_cs, x_coff, y_cs, y_coff, stride, pad_l, pad_t);
    return launch_status("somi_maxpool2_nhwc_f32");
}

extern "C" int somi_maxpool2_bwd_nhwc_f32(const float *dy, const void *codes, float *dx, int B, int H, int W, int C, int dy_cs, int dy_coff, int dx_cs,
                                          int dx_coff, int stride, int pad_l, int pad_r, int pad_t, int pad_b, somi_stream_t stream) {
    int Ho = 0, Wo = 0;
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && C % 4 == 0 && codes && aligned16(codes), SOMI_EINVAL,
                 "maxpool2 bwd: bad sizes (C a multiple of 4), or no 16-byte aligned codes");
    SOMI_REQUIRE(pool2_shape(H, W, stride, pad_l, pad_r, pad_t, pad_b, Ho, Wo), SOMI_EINVAL,
                 "maxpool2 bwd: kernel 2 with stride 1 or 2 and a zero pad of 0 or 1 per side only, and the padded map must hold one window");
    SOMI_REQUIRE_SLICES("maxpool2 bwd", {"dy", dy, dy_cs, dy_coff, C}, {"dx", dx, dx_cs, dx_coff, C});
    const long items = (long)B * H * W * (C / 4);
    if (small_index(items))
        hipLaunchKernelGGL(maxpool2_bwd_kernel<uint32_t>, dim3(pool_grid(items)), dim3(256), 0, (hipStream_t)stream, dy, (const uint8_t *)codes, dx, B, H,
                           W, Ho, Wo, C, dy_cs, dy_coff, dx_cs, dx_coff, stride, pad_l, pad_t);
    else
        hipLaunchKernelGGL(maxpool2_bwd_kernel<uint64_t>, dim3(pool_grid(items)), dim3(256), 0, (hipStream_t)stream, dy, (const uint8_t *)codes, dx, B, H,
                           W, Ho, Wo, C, dy_cs, dy_coff, dx_cs, dx_coff, stride, pad_l, pad_t);
    return launch_status("somi_maxpool2_bwd_nhwc_f32");
}

extern "C" int somi_maxpool3s2_nhwc_f32(const somi_slice *x, const somi_slice *y, void *codes, int B, int H, int W, int C, somi_stream_t stream) {
    SOMI_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (!codes || aligned16(codes)), SOMI_EINVAL,
                 "maxpool3s2: bad sizes (C a multiple of 4), or codes not 16-byte aligned");
    SOMI_REQUIRE_SLICES("maxpool3s2", {"x", x->p, x->cs, x->coff, C}, {"y", y->p, y->cs, y->coff, C});
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long items = (long)B * Ho * Wo * (C / 4);
    if (small_index(items))
        hipLaunchKernelGGL(maxpool3s2_fwd_kernel<uint32_t>, dim3(pool_grid(items)), dim3(256), 0, (hipStream_t)stream, (const float *)x->p, y->p,
                           (uint8_t *)codes, B, H, W, Ho, Wo, C, x->cs, x->coff, y->cs, y->coff);
    else
        hipLaunchKernelGGL(maxpool3s2_fwd_kernel<uint64_t>, dim3(pool_grid(items)), dim3(256), 0, (hipStream_t)stream, (const float *)x->p, y->p,
                           (uint8_t *)codes, B, H, W, Ho, Wo, C, x->cs, x->coff, y->cs, y->coff);
    return launch_status("somi_maxpool3s2_nhwc_f32");
}

extern "C" int somi_maxpool3s2_bwd_nhwc_f32(const somi_slice *dy, const void *codes, const somi_slice *dx, int B, int H, int W, int C,
                                            somi_stream_t stream) {
    SOMI_REQUIRE(dy && dx && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && codes && aligned16(codes), SOMI_EINVAL,
                 "maxpool3s2 bwd: bad sizes (C a multiple of 4), or no 16-byte aligned codes");
    SOMI_REQUIRE_SLICES("maxpool3s2 bwd", {"dy", dy->p, dy->cs, dy->coff, C}, {"dx", dx->p, dx->cs, dx->coff, C});
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long items = (long)B * H * W * (C / 4);
    if (small_index(items))
        hipLaunchKernelGGL(maxpool3s2_bwd_kernel<uint32_t>, dim3(pool_grid(items)), dim3(256), 0, (hipStream_t)stream, (const float *)dy->p,
                           (const uint8_t *)codes, dx->p, B, H, W, Ho, Wo, C, dy->cs, dy->coff, dx->cs, dx->coff);
    else
        hipLaunchKernelGGL(maxpool3s2_bwd_kernel<uint64_t>, dim3(pool_grid(items)), dim3(256), 0, (hipStream_t)stream, (const float *)dy->p,
                           (const uint8_t *)codes, dx->p, B, H, W, Ho, Wo, C, dy->cs, dy->coff, dx->cs, dx->coff);
    return launch_status("somi_maxpool3s2_bwd_nhwc_f32");
}

extern "C" int somi_spp_pool_nhwc_f32(float *buf, void *codes, int B, int H, int W, int C, int cs, int x_coff, int nk, int k0, int k1, int k2,
                                      somi_stream_t stream) {
    SppK kk;
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (!codes || aligned16(codes)), SOMI_EINVAL,
                 "spp pool: bad sizes (C a multiple of 4), or codes not 16-byte aligned");
    SOMI_REQUIRE(spp_windows_ok(nk, k0, k1, k2, kk), SOMI_EINVAL, "spp pool: 1 to 3 ascending odd window sizes, each 3 <= k <= 13");
    SOMI_REQUIRE_SLICES("spp pool", {"buf", buf, cs, x_coff, (nk + 1) * C});
    const dim3 grid(pool_grid((long)B * H * W * (C / 4)));
    hipStream_t s = (hipStream_t)stream;
#define SOMI_SPP_FWD(NK, IDX) hipLaunchKernelGGL((spp_pool_fwd_kernel<NK, IDX>), grid, dim3(256), 0, s, buf, (uint8_t *)codes, B, H, W, C, cs, x_coff, kk)
    if (small_index((long)B * H * W * (C / 4))) {
        if (nk == 1) SOMI_SPP_FWD(1, uint32_t); else if (nk == 2) SOMI_SPP_FWD(2, uint32_t); else SOMI_SPP_FWD(3, uint32_t);
    } else {
        if (nk == 1) SOMI_SPP_FWD(1, uint64_t); else if (nk == 2) SOMI_SPP_FWD(2, uint64_t); else SOMI_SPP_FWD(3, uint64_t);
    }
#undef SOMI_SPP_FWD
    return launch_status("somi_spp_pool_nhwc_f32");
}

extern "C" int somi_spp_pool_bwd_nhwc_f32(const void *codes, float *dbuf, int B, int H, int W, int C, int cs, int x_coff, int nk, int k0, int k1, int k2,
                                          somi_stream_t stream) {
    SppK kk;
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && codes && aligned16(codes), SOMI_EINVAL,
                 "spp pool bwd: bad sizes (C a multiple of 4), or no 16-byte aligned codes");
    SOMI_REQUIRE(spp_windows_ok(nk, k0, k1, k2, kk), SOMI_EINVAL, "spp pool bwd: 1 to 3 ascending odd window sizes, each 3 <= k <= 13");
    SOMI_REQUIRE_SLICES("spp pool bwd", {"dbuf", dbuf, cs, x_coff, (nk + 1) * C});
    const dim3 grid(pool_grid((long)B * H * W * (C / 4)));
    hipStream_t s = (hipStream_t)stream;
#define SOMI_SPP_BWD(NK, IDX) hipLaunchKernelGGL((spp_pool_bwd_kernel<NK, IDX>), grid, dim3(256), 0, s, (const uint8_t *)codes, dbuf, B, H, W, C, cs, x_coff, kk)
    if (small_index((long)B * H * W * (C / 4))) {
        if (nk == 1) SOMI_SPP_BWD(1, uint32_t); else if (nk == 2) SOMI_SPP_BWD(2, uint32_t); else SOMI_SPP_BWD(3, uint32_t);
    } else {
        if (nk == 1) SOMI_SPP_BWD(1, uint64_t); else if (nk == 2) SOMI_SPP_BWD(2, uint64_t); else SOMI_SPP_BWD(3, uint64_t);
    }
#undef SOMI_SPP_BWD
    return launch_status("somi_spp_pool_bwd_nhwc_f32");
}
