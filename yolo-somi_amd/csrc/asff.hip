// Adaptive spatial feature fusion (ASFF, models/common.py:5551-5560): per output pixel a 3-way softmax over the logits of a 48 -> 3 1x1 conv of three
// 16-channel maps weighs three C-channel sources, fused = sum_i p_i * r_i.  The data-dependent cousin of the BiFPN fusion (layers.hip): every
// source and every weight map is read at (h >> up, w >> up) with its own up in {0, 1, 2}, so neither an upsampled map, nor the 48-channel concat,
// nor the logits, nor a per-source product reaches memory.  Training keeps p (3 floats per pixel), the only extra tensor backward needs.
//
// Both kernels give a workgroup a tile of 64 output pixels made of whole U x U blocks, U = 1 << (largest up of the six inputs): every child of a
// low-resolution pixel lies in its block, so the sums over the 4 or 16 children (dr_i of an upsampled source, dv_i of an upsampled weight map) are
// formed by the one lane that owns the low-resolution element, children in row-major order.  dW / db: one partial per workgroup (its pixels in
// order), then one fixed-order reduce.  No float atomics; two launches are bit-identical.
//
// fp32 NHWC channel slices, a lane owns one channel quad of one pixel in every sweep: 16-byte loads and stores, contiguous across the wave.
#include "common.h"

namespace somi {

constexpr int ASFF_TP = 64;       // output pixels per workgroup
constexpr int ASFF_VC = 16;       // channels of a weight map
constexpr int ASFF_NW = 3 * 3 * ASFF_VC + 3;      // dW (3 x 48) and db (3) of one workgroup
constexpr int ASFF_WS = 148;      // ... its row in the workspace

struct AsffArgs {
    const float *r[3], *v[3];
    int r_cs[3], r_coff[3], v_cs[3], v_coff[3], r_up[3], v_up[3];
    const float *w, *bias;
    float *out;                   // forward: fused; backward: dfused (read)
    int o_cs, o_coff;
    float *p;
    float *dr[3], *dv[3];
    int dr_cs[3], dr_coff[3], dv_cs[3], dv_coff[3], dr_acc[3];
    float *ws;
    int B, H, W, C, U;            // U: log2 of the block edge
};

// local pixel lp of workgroup wg -> its block and position; -> the output pixel index, or -1 past the end
__device__ __forceinline__ long asff_pixel(const AsffArgs &a, int wg, int lp, int &b, int &h, int &w) {
    const int U = a.U, bw = a.W >> U, bh = a.H >> U;
    const long blk = (long)wg * (ASFF_TP >> (2 * U)) + (lp >> (2 * U));
    if (blk >= (long)a.B * bh * bw) return -1;
    const int child = lp & ((1 << (2 * U)) - 1);
    const long row = blk / bw;
    w = ((int)(blk - row * bw) << U) + (child & ((1 << U) - 1));
    h = ((int)(row % bh) << U) + (child >> U);
    b = (int)(row / bh);
    return ((long)b * a.H + h) * a.W + w;
}

__device__ __forceinline__ long asff_src_pixel(const AsffArgs &a, int b, int h, int w, int up) {
    return ((long)b * (a.H >> up) + (h >> up)) * (a.W >> up) + (w >> up);
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void asff_fuse_fwd_kernel(AsffArgs a) {
    __shared__ float sp[ASFF_TP][3];
    __shared__ long spix[ASFF_TP][4];          // the three sources' pixels and the output pixel (-1: past the end)
    const int t = threadIdx.x;
    {   // four lanes per pixel: lane j < 3 takes weight map j's 16 channels, lane 0 then owns the softmax
        const int lp = t >> 2, j = t & 3;
        int b = 0, h = 0, w = 0;
        const long pix = asff_pixel(a, blockIdx.x, lp, b, h, w);
        float l0 = 0.f, l1 = 0.f, l2 = 0.f;
        if (pix >= 0 && j < 3) {
            spix[lp][j] = asff_src_pixel(a, b, h, w, a.r_up[j]);
            const float *vp = a.v[j] + asff_src_pixel(a, b, h, w, a.v_up[j]) * a.v_cs[j] + a.v_coff[j];
#pragma unroll
            for (int q = 0; q < ASFF_VC / 4; ++q) {
                const f32x4 x = ld4(vp + 4 * q);
                const f32x4 w0 = ld4(a.w + 0 * 48 + j * ASFF_VC + 4 * q);
                const f32x4 w1 = ld4(a.w + 1 * 48 + j * ASFF_VC + 4 * q);
                const f32x4 w2 = ld4(a.w + 2 * 48 + j * ASFF_VC + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) { l0 += w0[e] * x[e]; l1 += w1[e] * x[e]; l2 += w2[e] * x[e]; }
            }
        }
        // lane 0 of the four: (own + lane 1) + lane 2, a fixed order
        l0 = (l0 + __shfl_down(l0, 1)) + __shfl_down(l0, 2);
        l1 = (l1 + __shfl_down(l1, 1)) + __shfl_down(l1, 2);
        l2 = (l2 + __shfl_down(l2, 1)) + __shfl_down(l2, 2);
        if (j == 0) {
            spix[lp][3] = pix;
            if (pix >= 0) {
                l0 += a.bias[0]; l1 += a.bias[1]; l2 += a.bias[2];
                const float m = fmaxf(l0, fmaxf(l1, l2));
                const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m);
                const float inv = 1.f / ((e0 + e1) + e2);
                sp[lp][0] = e0 * inv; sp[lp][1] = e1 * inv; sp[lp][2] = e2 * inv;
                if (a.p) { a.p[pix * 3 + 0] = e0 * inv; a.p[pix * 3 + 1] = e1 * inv; a.p[pix * 3 + 2] = e2 * inv; }
            }
        }
    }
    __syncthreads();
    const int C4 = a.C >> 2, items = ASFF_TP * C4;
#pragma unroll 2
    for (int it = t; it < items; it += 256) {
        const int lp = it / C4, c = (it - lp * C4) * 4;
        const long pix = spix[lp][3];
        if (pix < 0) continue;
        const f32x4 x0 = ld4(a.r[0] + spix[lp][0] * a.r_cs[0] + a.r_coff[0] + c);
        const f32x4 x1 = ld4(a.r[1] + spix[lp][1] * a.r_cs[1] + a.r_coff[1] + c);
        const f32x4 x2 = ld4(a.r[2] + spix[lp][2] * a.r_cs[2] + a.r_coff[2] + c);
        const float p0 = sp[lp][0], p1 = sp[lp][1], p2 = sp[lp][2];
        const f32x4 o = x0 * p0 + x1 * p1 + x2 * p2;
        st4(a.out + pix * a.o_cs + a.o_coff + c, o);
    }
}

// ------------------------------------------------------------------------------------------------ backward
// local index of child (cy, cx) of the level-u pixel j of this workgroup (U >= u): blocks of (1 << U)^2 pixels hold (1 << (U - u))^2 such pixels
__device__ __forceinline__ int asff_child(int j, int u, int U, int cy, int cx) {
    const int per = 2 * (U - u), blk = j >> per, sub = j & ((1 << per) - 1);
    const int sy = sub >> (U - u), sx = sub & ((1 << (U - u)) - 1);
    return (blk << (2 * U)) + ((((sy << u) + cy)) << U) + (sx << u) + cx;
}

__global__ __launch_bounds__(256) void asff_fuse_bwd_kernel(AsffArgs a) {
    __shared__ float sp[ASFF_TP][3], sdl[ASFF_TP][3], sdot[ASFF_TP][3];
    __shared__ long spix[ASFF_TP][4];          // the three sources' pixels and the output pixel (-1: past the end)
    __shared__ long svpix[ASFF_TP][3];         // the three weight maps' pixels
    __shared__ float scat[ASFF_TP][3 * ASFF_VC + 1];
    const int t = threadIdx.x, U = a.U, C4 = a.C >> 2;
    if (t < ASFF_TP) {
        int b = 0, h = 0, w = 0;
        const long pix = asff_pixel(a, blockIdx.x, t, b, h, w);
        spix[t][3] = pix;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            spix[t][i] = pix < 0 ? 0 : asff_src_pixel(a, b, h, w, a.r_up[i]);
            svpix[t][i] = pix < 0 ? 0 : asff_src_pixel(a, b, h, w, a.v_up[i]);
            sp[t][i] = pix < 0 ? 0.f : a.p[pix * 3 + i];
        }
    }
    __syncthreads();
    // the weight maps' 48 values per pixel (for dW), and <dfused, r_i>: 16 lanes per pixel, 16 pixels per round, the lanes' partial dots
    // folded by xor shuffles (a fixed tree)
    for (int it = t; it < ASFF_TP * 3 * (ASFF_VC / 4); it += 256) {
        const int lp = it / 12, q = it - lp * 12, i = q >> 2, c = (q & 3) * 4;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (spix[lp][3] >= 0) x = ld4(a.v[i] + svpix[lp][i] * a.v_cs[i] + a.v_coff[i] + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) scat[lp][i * ASFF_VC + c + e] = x[e];
    }
    for (int round = 0; round < ASFF_TP / 16; ++round) {
        const int lp = round * 16 + (t >> 4), sub = t & 15;
        const long pix = spix[lp][3];
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (pix >= 0) {
            const float *dp = a.out + pix * a.o_cs + a.o_coff;
            const float *r0 = a.r[0] + spix[lp][0] * a.r_cs[0] + a.r_coff[0];
            const float *r1 = a.r[1] + spix[lp][1] * a.r_cs[1] + a.r_coff[1];
            const float *r2 = a.r[2] + spix[lp][2] * a.r_cs[2] + a.r_coff[2];
            for (int q = sub; q < C4; q += 16) {
                const f32x4 d = ld4(dp + 4 * q);
                const f32x4 x0 = ld4(r0 + 4 * q);
                const f32x4 x1 = ld4(r1 + 4 * q);
                const f32x4 x2 = ld4(r2 + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) { d0 += d[e] * x0[e]; d1 += d[e] * x1[e]; d2 += d[e] * x2[e]; }
            }
        }
#pragma unroll
        for (int s = 8; s > 0; s >>= 1) { d0 += __shfl_xor(d0, s); d1 += __shfl_xor(d1, s); d2 += __shfl_xor(d2, s); }
        if (sub == 0) { sdot[lp][0] = d0; sdot[lp][1] = d1; sdot[lp][2] = d2; }
    }
    __syncthreads();
    if (t < ASFF_TP) {                          // dL_i = p_i (D_i - sum_j p_j D_j); 0 past the end (p is 0 there)
        const float s = (sp[t][0] * sdot[t][0] + sp[t][1] * sdot[t][1]) + sp[t][2] * sdot[t][2];
#pragma unroll
        for (int i = 0; i < 3; ++i) sdl[t][i] = sp[t][i] * (sdot[t][i] - s);
    }
    __syncthreads();
    // dr_i = p_i dfused, written (or added to what dr_i holds) by the lane that owns the element; an upsampled source sums its children row-major
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (!a.dr[i]) continue;
        const int u = a.r_up[i], n = ASFF_TP >> (2 * u), side = 1 << u;
        for (int it = t; it < n * C4; it += 256) {
            const int j = it / C4, c = (it - j * C4) * 4;
            const int first = asff_child(j, u, U, 0, 0);
            if (spix[first][3] < 0) continue;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int cy = 0; cy < side; ++cy)
                for (int cx = 0; cx < side; ++cx) {
                    const int lp = asff_child(j, u, U, cy, cx);
                    acc += ld4(a.out + spix[lp][3] * a.o_cs + a.o_coff + c) * sp[lp][i];
                }
            float *dst = a.dr[i] + spix[first][i] * a.dr_cs[i] + a.dr_coff[i] + c;
            if (a.dr_acc[i]) acc += ld4(dst);
            st4(dst, acc);
        }
    }
    // dv_i = W^T (sum over the children of dL), 16 channels per weight-map pixel
    for (int i = 0; i < 3; ++i) {
        const int u = a.v_up[i], n = ASFF_TP >> (2 * u), side = 1 << u;
        for (int it = t; it < n * (ASFF_VC / 4); it += 256) {
            const int j = it >> 2, c = (it & 3) * 4;
            const int first = asff_child(j, u, U, 0, 0);
            if (spix[first][3] < 0) continue;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            for (int cy = 0; cy < side; ++cy)
                for (int cx = 0; cx < side; ++cx) {
                    const int lp = asff_child(j, u, U, cy, cx);
                    g0 += sdl[lp][0]; g1 += sdl[lp][1]; g2 += sdl[lp][2];
                }
            const f32x4 w0 = ld4(a.w + 0 * 48 + i * ASFF_VC + c);
            const f32x4 w1 = ld4(a.w + 1 * 48 + i * ASFF_VC + c);
            const f32x4 w2 = ld4(a.w + 2 * 48 + i * ASFF_VC + c);
            const f32x4 dvi = w0 * g0 + w1 * g1 + w2 * g2;
            st4(a.dv[i] + svpix[first][i] * a.dv_cs[i] + a.dv_coff[i] + c, dvi);
        }
    }
    // this workgroup's dW[k][m] = sum_pixels dL_k * cat(v)[m] and db[k] = sum_pixels dL_k, pixels in order
    if (t < ASFF_NW) {
        const int k = t < 144 ? t / 48 : t - 144, m = t < 144 ? t % 48 : 0;
        float acc = 0.f;
        for (int lp = 0; lp < ASFF_TP; ++lp) acc += sdl[lp][k] * (t < 144 ? scat[lp][m] : 1.f);
        a.ws[(long)blockIdx.x * ASFF_WS + t] = acc;
    }
}

// dW / db += the workgroups' partials: one wave per value, every lane a strided part in order, then a fixed shuffle tree
__global__ __launch_bounds__(64) void asff_wgrad_reduce_kernel(const float *__restrict__ ws, int nwg, float *dw, float *db) {
    const int o = blockIdx.x, lane = threadIdx.x;
    float acc = 0.f;
    for (int g = lane; g < nwg; g += 64) acc += ws[(long)g * ASFF_WS + o];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
    if (lane == 0) {
        float *dst = o < 144 ? dw + o : db + (o - 144);
        *dst += acc;
    }
}

static int asff_unpack(const somi_asff_desc *d, bool bwd, AsffArgs &a, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C % 4 == 0 && (long)d->B * d->H * d->W < (1L << 31) - ASFF_TP, SOMI_EINVAL,
                 "%s: bad sizes (C a multiple of 4, fewer than 2^31 pixels)", who);
    SOMI_REQUIRE(d->w && d->bias && aligned16(d->w), SOMI_EINVAL, "%s: the 3x48 weight (16-byte aligned) and the 3 biases are required", who);
    int U = 0;
    for (int i = 0; i < 3; ++i) {
        SOMI_REQUIRE(d->r_up[i] >= 0 && d->r_up[i] <= 2 && d->v_up[i] >= 0 && d->v_up[i] <= 2, SOMI_EINVAL, "%s: up must be 0, 1 or 2", who);
        U = d->r_up[i] > U ? d->r_up[i] : U;
        U = d->v_up[i] > U ? d->v_up[i] : U;
    }
    SOMI_REQUIRE(d->H % (1 << U) == 0 && d->W % (1 << U) == 0, SOMI_EINVAL, "%s: H and W must be multiples of %d, the largest upsampling factor", who,
                 1 << U);
    SOMI_REQUIRE_SLICES(who, {"r0", d->r[0].p, d->r[0].cs, d->r[0].coff, d->C}, {"r1", d->r[1].p, d->r[1].cs, d->r[1].coff, d->C},
                        {"r2", d->r[2].p, d->r[2].cs, d->r[2].coff, d->C}, {"v0", d->v[0].p, d->v[0].cs, d->v[0].coff, ASFF_VC},
                        {"v1", d->v[1].p, d->v[1].cs, d->v[1].coff, ASFF_VC}, {"v2", d->v[2].p, d->v[2].cs, d->v[2].coff, ASFF_VC},
                        {bwd ? "dfused" : "fused", d->out.p, d->out.cs, d->out.coff, d->C});
    if (bwd) {
        SOMI_REQUIRE(d->p && d->dw && d->db && d->workspace && aligned16(d->workspace), SOMI_EINVAL,
                     "%s: p, dw, db and a 16-byte aligned workspace are required", who);
        SOMI_REQUIRE(d->workspace_floats >= somi_asff_fuse_bwd_workspace_floats(d->B, d->H, d->W), SOMI_EWORKSPACE, "%s: workspace too small", who);
        SOMI_REQUIRE_SLICES(who, {"dr0", d->dr[0].p, d->dr[0].cs, d->dr[0].coff, d->C, kOptional},
                            {"dr1", d->dr[1].p, d->dr[1].cs, d->dr[1].coff, d->C, kOptional},
                            {"dr2", d->dr[2].p, d->dr[2].cs, d->dr[2].coff, d->C, kOptional},
                            {"dv0", d->dv[0].p, d->dv[0].cs, d->dv[0].coff, ASFF_VC}, {"dv1", d->dv[1].p, d->dv[1].cs, d->dv[1].coff, ASFF_VC},
                            {"dv2", d->dv[2].p, d->dv[2].cs, d->dv[2].coff, ASFF_VC});
    }
    for (int i = 0; i < 3; ++i) {
        a.r[i] = d->r[i].p; a.r_cs[i] = d->r[i].cs; a.r_coff[i] = d->r[i].coff; a.r_up[i] = d->r_up[i];
        a.v[i] = d->v[i].p; a.v_cs[i] = d->v[i].cs; a.v_coff[i] = d->v[i].coff; a.v_up[i] = d->v_up[i];
        a.dr[i] = bwd ? d->dr[i].p : nullptr; a.dr_cs[i] = d->dr[i].cs; a.dr_coff[i] = d->dr[i].coff; a.dr_acc[i] = d->dr_accumulate[i];
        a.dv[i] = bwd ? d->dv[i].p : nullptr; a.dv_cs[i] = d->dv[i].cs; a.dv_coff[i] = d->dv[i].coff;
    }
    a.w = d->w; a.bias = d->bias; a.out = d->out.p; a.o_cs = d->out.cs; a.o_coff = d->out.coff; a.p = d->p; a.ws = d->workspace;
    a.B = d->B; a.H = d->H; a.W = d->W; a.C = d->C; a.U = U;
    return 0;
}

}  // namespace somi

using namespace somi;

extern "C" size_t somi_asff_desc_bytes(void) { return sizeof(somi_asff_desc); }

extern "C" size_t somi_asff_fuse_bwd_workspace_floats(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)cdiv((long)B * H * W, ASFF_TP) * ASFF_WS;
}

extern "C" int somi_asff_fuse_nhwc_f32(const somi_asff_desc *d, somi_stream_t stream) {
    AsffArgs a;
    if (int rc = asff_unpack(d, false, a, "asff fuse")) return rc;
    hipLaunchKernelGGL(asff_fuse_fwd_kernel, dim3(cdiv((long)a.B * a.H * a.W, ASFF_TP)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_asff_fuse_nhwc_f32");
}

extern "C" int somi_asff_fuse_bwd_nhwc_f32(const somi_asff_desc *d, somi_stream_t stream) {
    AsffArgs a;
    if (int rc = asff_unpack(d, true, a, "asff fuse bwd")) return rc;
    const int nwg = cdiv((long)a.B * a.H * a.W, ASFF_TP);
    hipLaunchKernelGGL(asff_fuse_bwd_kernel, dim3(nwg), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(asff_wgrad_reduce_kernel, dim3(ASFF_NW), dim3(64), 0, (hipStream_t)stream, (const float *)a.ws, nwg, d->dw, d->db);
    return launch_status("somi_asff_fuse_bwd_nhwc_f32");
}
