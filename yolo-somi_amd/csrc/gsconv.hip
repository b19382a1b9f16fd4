// Slim-neck GSConv, NHWC fp32 (models/common.py:9586-9610): x1 = cv1(x), x_2 = cv2_2(cv2_1(x1)) - two stacked depthwise 3x3 Conv blocks - and
// the module's closing channel shuffle of s = cat(x1, x_2), out[o] = s[2 o] for o < Ch, s[2 (o - Ch) + 1] otherwise (Ch = c2 / 2).
//
// Every kernel here walks SOURCE quads: quad J of s (J < Ch / 2; J < Ch / 4 is x1's quad J, the rest x_2's) is one float4 in a lane's registers
// and leaves as two float2 - its even channels at out[2 J, 2 J + 2), its odd ones at out[Ch + 2 J, Ch + 2 J + 2).  Ch % 4 == 0 keeps both 8-byte
// aligned, adjacent lanes own adjacent quads, so a wave's stores are contiguous runs, and the group of eight source channels that straddles
// x1 | x_2 when Ch % 8 == 4 is no special case: the two halves of such an output quad come from two lanes.
//
// The tail (inference) keeps x1 with a 2-pixel halo and t = act(dw1(x1) + b1) with a 1-pixel halo in LDS: 16 x 16 pixels x 4 quads is
// (20 * 20 + 18 * 18) * 64 B = 46,336 B, 8 x 16 pixels x 8 quads (12 * 20 + 10 * 18) * 128 B = 53,760 B - two or three workgroups per CU of
// 160 KiB; x1 is read from memory once per tile (halo pixels once more by the neighbouring tile, from L2), and nothing between x1 and out is
// written.  The two streaming kernels (training) are one read and one write per element; like gconv.hip's, a workgroup is nq quads wide and
// 256 / nq pixels tall and walks `iters` such tiles.  No reductions, no atomics: every launch is bit-identical.
#include "common.h"

namespace somi {
namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_MAXQ = 64;                                       // source quads per channel chunk of the streaming kernels
constexpr int GS_BLOCKS = 2048;                                   // about this many workgroups per streaming launch
// the tail's workgroup: 16 x 16 pixels x 4 quads, or - from 8 quads (32 channels a half) up - 8 x 16 pixels x 8 quads, which reads and
// writes twice as long a run of every pixel's channel row
constexpr int GS_TILE = 16, GS_TAILQ = 4, GS_WIDEQ = 8, GS_WIDE_TH = 8;

struct GsPlan {
    int nq, pp, iters, nblk, nchunk;
};

static GsPlan gs_plan(long npix, int Ch) {
    GsPlan p;
    const int sq = Ch / 2;                                        // source quads of cat(x1, x_2)
    p.nchunk = cdiv(sq, GS_MAXQ);
    p.nq = 1;
    while (p.nq < (sq < GS_MAXQ ? sq : GS_MAXQ)) p.nq <<= 1;
    p.pp = GS_THREADS / p.nq;
    const long passes = (npix + p.pp - 1) / p.pp;
    const long it = passes * p.nchunk / GS_BLOCKS;
    p.iters = (int)(it < 1 ? 1 : (it > 64 ? 64 : it));
    p.nblk = (int)((passes + p.iters - 1) / p.iters);
    return p;
}

__device__ __forceinline__ f32x4 act4(f32x4 v, int act) {
    if (act == SOMI_ACT_SILU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * __builtin_amdgcn_rcpf(1.0f + __expf(-v[e]));     // v_rcp_f32: 1 ulp, no division sequence
    } else if (act != SOMI_ACT_NONE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = apply_act_rt(v[e], act);
    }
    return v;
}

// source quad J of one pixel -> its two places in the output row `o` (already at the pixel and the slice's offset), + the residual's
__device__ __forceinline__ void store_shuffled(float *o, const float *r, int Ch, int J, f32x4 v) {
    f32x2 ev = {v[0], v[2]}, od = {v[1], v[3]};
    if (r) {
        ev += *reinterpret_cast<const f32x2 *>(r + 2 * J);
        od += *reinterpret_cast<const f32x2 *>(r + Ch + 2 * J);
    }
    *reinterpret_cast<f32x2 *>(o + 2 * J) = ev;
    *reinterpret_cast<f32x2 *>(o + Ch + 2 * J) = od;
}

struct StreamArgs {
    somi_slice a, b, out, res;                                    // shuffle: z1, y2 -> out (+ res); unshuffle: out = dout (read) -> a = d1, b = d2
    const float *scale, *shift;
    long npix;
    int Ch, act;
    GsPlan p;
};

template <bool INVERSE>
__global__ __launch_bounds__(GS_THREADS) void gs_stream_kernel(StreamArgs a) {
    const int ql = threadIdx.x % a.p.nq, psub = threadIdx.x / a.p.nq;
    const int J = blockIdx.y * GS_MAXQ + ql, cq = a.Ch / 4;
    if (J >= 2 * cq) return;
    const bool first = J < cq;
    const int c0 = (first ? J : J - cq) * 4;                      // the quad's first channel inside x1 / x_2
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    const bool affine = !INVERSE && !first && a.scale;
    if (affine) {
        sc = ld4(a.scale + c0);
        sh = ld4(a.shift + c0);
    }
    const somi_slice half = first ? a.a : a.b;
    for (int it = 0; it < a.p.iters; ++it) {
        const long pix = ((long)blockIdx.x * a.p.iters + it) * a.p.pp + psub;
        if (pix >= a.npix) break;
        float *hp = half.p + (size_t)pix * half.cs + half.coff + c0;
        float *o = a.out.p + (size_t)pix * a.out.cs + a.out.coff;
        if constexpr (INVERSE) {
            const f32x2 ev = *reinterpret_cast<const f32x2 *>(o + 2 * J), od = *reinterpret_cast<const f32x2 *>(o + a.Ch + 2 * J);
            st4(hp, f32x4{ev[0], od[0], ev[1], od[1]});
        } else {
            f32x4 v = ld4(hp);
            if (!first) {
                if (affine) v = v * sc + sh;
                v = act4(v, a.act);
            }
            store_shuffled(o, a.res.p ? a.res.p + (size_t)pix * a.res.cs + a.res.coff : nullptr, a.Ch, J, v);
        }
    }
}

struct TailArgs {
    somi_slice x1, out, res;
    const float *w1, *b1, *w2, *b2;
    int w_cs, act, B, H, W, Ch, ntx, nty, nchunk;
};

// QP quads x TH x TW pixels per workgroup.  Consecutive workgroups are the quad chunks of ONE pixel tile, so the pieces of a pixel's channel
// row that different chunks read and write are in flight together: at 128 images of 80x80 this order alone took the launch from 468 to 355 us.
template <int QP, int TH, int TW>
__global__ __launch_bounds__(GS_THREADS) void gs_tail_kernel(TailArgs a) {
    constexpr int XH = TH + 4, XW = TW + 4, UH = TH + 2, UW = TW + 2, NP = GS_THREADS / QP;
    __shared__ f32x4 sx[XH * XW * QP];                            // x1, zero outside the image (dw1's padding)
    __shared__ f32x4 st[UH * UW * QP];                            // t, zero outside the image (dw2's padding)
    const int ql = threadIdx.x % QP, lp = threadIdx.x / QP;
    const int cq = a.Ch / 4, q = (blockIdx.x % a.nchunk) * QP + ql;
    const bool active = q < cq;
    const int tile = blockIdx.x / a.nchunk;
    const int w0 = (tile % a.ntx) * TW, h0 = (tile / a.ntx % a.nty) * TH, b = tile / (a.ntx * a.nty);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const size_t img = (size_t)b * a.H * a.W;

    for (int p = lp; p < XH * XW; p += NP) {
        const int h = h0 - 2 + p / XW, w = w0 - 2 + p % XW;
        f32x4 v = zero;
        if (active && h >= 0 && h < a.H && w >= 0 && w < a.W)
            v = ld4(a.x1.p + (img + (size_t)h * a.W + w) * a.x1.cs + a.x1.coff + q * 4);
        sx[p * QP + ql] = v;
    }
    __syncthreads();

    f32x4 wr[9], bias = zero;
#pragma unroll
    for (int t = 0; t < 9; ++t) wr[t] = active ? ld4(a.w1 + (size_t)t * a.w_cs + q * 4) : zero;
    if (active) bias = ld4(a.b1 + q * 4);
    for (int p = lp; p < UH * UW; p += NP) {
        const int r = p / UW, c = p % UW, h = h0 - 1 + r, w = w0 - 1 + c;
        f32x4 v = zero;
        if (active && h >= 0 && h < a.H && w >= 0 && w < a.W) {
            v = bias;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) v += wr[i * 3 + j] * sx[((r + i) * XW + c + j) * QP + ql];
            v = act4(v, a.act);
        }
        st[p * QP + ql] = v;
    }
    __syncthreads();

#pragma unroll
    for (int t = 0; t < 9; ++t) wr[t] = active ? ld4(a.w2 + (size_t)t * a.w_cs + q * 4) : zero;
    if (active) bias = ld4(a.b2 + q * 4);
    for (int p = lp; p < TH * TW; p += NP) {
        const int r = p / TW, c = p % TW, h = h0 + r, w = w0 + c;
        if (!active || h >= a.H || w >= a.W) continue;
        f32x4 v = bias;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) v += wr[i * 3 + j] * st[((r + i) * UW + c + j) * QP + ql];
        v = act4(v, a.act);
        const size_t pix = img + (size_t)h * a.W + w;
        float *o = a.out.p + pix * a.out.cs + a.out.coff;
        const float *res = a.res.p ? a.res.p + pix * a.res.cs + a.res.coff : nullptr;
        store_shuffled(o, res, a.Ch, q, sx[((r + 2) * XW + c + 2) * QP + ql]);
        store_shuffled(o, res, a.Ch, cq + q, v);
    }
}

template <int QP, int TH, int TW>
static void launch_tail(TailArgs a, hipStream_t s) {
    a.ntx = cdiv(a.W, TW); a.nty = cdiv(a.H, TH); a.nchunk = cdiv(a.Ch / 4, QP);
    hipLaunchKernelGGL((gs_tail_kernel<QP, TH, TW>), dim3((unsigned)((long)a.B * a.ntx * a.nty * a.nchunk)), dim3(GS_THREADS), 0, s, a);
}

static int check_width(const char *who, int Ch) {
    SOMI_REQUIRE(Ch > 0 && Ch % 4 == 0, SOMI_EINVAL, "%s: half width %d (a positive multiple of 4: the shuffle moves float2 pairs of channel quads)", who, Ch);
    return 0;
}

}  // namespace
}  // namespace somi

using namespace somi;

extern "C" int somi_gs_tiles_per_workgroup(long npix, int Ch) {
    if (npix <= 0 || Ch <= 0 || Ch % 4) return 0;
    return gs_plan(npix, Ch).iters;
}

extern "C" int somi_gs_tail_nhwc_f32(somi_slice x1, const float *w1, const float *b1, const float *w2, const float *b2, int w_cs, int act,
                                     somi_slice out, somi_slice residual, int B, int H, int W, int Ch, somi_stream_t stream) {
    if (int rc = check_width("gs tail", Ch)) return rc;
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0, SOMI_EINVAL, "gs tail: bad sizes (%d, %d, %d)", B, H, W);
    SOMI_REQUIRE(act >= 0 && act <= 6, SOMI_EINVAL, "gs tail: bad activation %d", act);
    SOMI_REQUIRE(w1 && w2 && b1 && b2 && aligned16(w1) && aligned16(w2) && aligned16(b1) && aligned16(b2), SOMI_EINVAL,
                 "gs tail: w1, b1, w2, b2 must be given and 16-byte aligned");
    SOMI_REQUIRE(w_cs % 4 == 0 && w_cs >= Ch, SOMI_EINVAL, "gs tail: the weights' row stride w_cs (%d) must be a multiple of 4 >= Ch (%d)", w_cs, Ch);
    SOMI_REQUIRE_SLICES("gs tail", {"x1", x1.p, x1.cs, x1.coff, Ch}, {"out", out.p, out.cs, out.coff, 2 * Ch},
                        {"residual", residual.p, residual.cs, residual.coff, 2 * Ch, kOptional});
    TailArgs a;
    a.x1 = x1; a.out = out; a.res = residual; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
    a.w_cs = w_cs; a.act = act; a.B = B; a.H = H; a.W = W; a.Ch = Ch;
    const int cq = Ch / 4;
    // the smallest tile and chunk of the three forms bound the grid of all of them
    SOMI_REQUIRE((long)B * cdiv(H, GS_WIDE_TH) * cdiv(W, GS_TILE) * cdiv(cq, GS_TAILQ) <= 0x7fffffffL, SOMI_EINVAL, "gs tail: too many tiles for one launch");
    hipStream_t s = (hipStream_t)stream;
    if (cq == 1) launch_tail<1, GS_TILE, GS_TILE>(a, s);
    else if (cq == 2) launch_tail<2, GS_TILE, GS_TILE>(a, s);
    else if (cq < GS_WIDEQ) launch_tail<GS_TAILQ, GS_TILE, GS_TILE>(a, s);
    else launch_tail<GS_WIDEQ, GS_WIDE_TH, GS_TILE>(a, s);
    return launch_status("somi_gs_tail_nhwc_f32");
}

extern "C" int somi_gs_shuffle_affine_act_nhwc_f32(somi_slice z1, somi_slice y2, const float *scale, const float *shift, int act, somi_slice out,
                                                   somi_slice residual, long npix, int Ch, somi_stream_t stream) {
    if (int rc = check_width("gs shuffle", Ch)) return rc;
    SOMI_REQUIRE(npix > 0, SOMI_EINVAL, "gs shuffle: %ld pixels", npix);
    SOMI_REQUIRE(act >= 0 && act <= 6, SOMI_EINVAL, "gs shuffle: bad activation %d", act);
    SOMI_REQUIRE(!scale == !shift && (!scale || (aligned16(scale) && aligned16(shift))), SOMI_EINVAL,
                 "gs shuffle: scale and shift come together, 16-byte aligned");
    SOMI_REQUIRE_SLICES("gs shuffle", {"z1", z1.p, z1.cs, z1.coff, Ch}, {"y2", y2.p, y2.cs, y2.coff, Ch}, {"out", out.p, out.cs, out.coff, 2 * Ch},
                        {"residual", residual.p, residual.cs, residual.coff, 2 * Ch, kOptional});
    StreamArgs a;
    a.a = z1; a.b = y2; a.out = out; a.res = residual; a.scale = scale; a.shift = shift; a.npix = npix; a.Ch = Ch; a.act = act;
    a.p = gs_plan(npix, Ch);
    hipLaunchKernelGGL((gs_stream_kernel<false>), dim3(a.p.nblk, a.p.nchunk), dim3(GS_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("somi_gs_shuffle_affine_act_nhwc_f32");
}

extern "C" int somi_gs_unshuffle_nhwc_f32(somi_slice dout, somi_slice d1, somi_slice d2, long npix, int Ch, somi_stream_t stream) {
    if (int rc = check_width("gs unshuffle", Ch)) return rc;
    SOMI_REQUIRE(npix > 0, SOMI_EINVAL, "gs unshuffle: %ld pixels", npix);
    SOMI_REQUIRE_SLICES("gs unshuffle", {"dout", dout.p, dout.cs, dout.coff, 2 * Ch}, {"d1", d1.p, d1.cs, d1.coff, Ch}, {"d2", d2.p, d2.cs, d2.coff, Ch});
    StreamArgs a;
    a.a = d1; a.b = d2; a.out = dout; a.res = somi_slice{nullptr, 0, 0}; a.scale = a.shift = nullptr; a.npix = npix; a.Ch = Ch; a.act = 0;
    a.p = gs_plan(npix, Ch);
    hipLaunchKernelGGL((gs_stream_kernel<true>), dim3(a.p.nblk, a.p.nchunk), dim3(GS_THREADS), 0, (hipStream_t)stream, a);
    return launch_status("somi_gs_unshuffle_nhwc_f32");
}
