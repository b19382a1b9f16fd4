// Coordinate attention (CoorAttention / CABottleneck, models/common.py:1399-1450, 4884-4922): the four passes over the (B,H,W,C) map.
//   means     pool[b, h, c]     = mean_w x[b,h,w,c],   pool[b, H + w, c] = mean_h x[b,h,w,c]          (the reference's cat([x_h, x_w.permute], dim=2))
//   apply     out = [res +] x * a_h[b,h,c] * a_w[b,w,c]                                                 (no expanded gate, no x * a_w product in memory)
//   gates bwd da_h[b,h,c] = sum_w dout x a_w,   da_w[b,w,c] = sum_h dout x a_h                          (dout and x read once for both)
//   input bwd dx = dout a_h a_w + gh[b,h,c] / W + gw[b,w,c] / H                                         (gh, gw: the gradients of the two means)
// The small tensors between them (conv1, bn1, h-swish, conv_h / conv_w, sigmoid on B * (H + W) rows) run on the conv and BatchNorm kernels.
//
// One geometry for all four: a workgroup takes RH rows x NL columns of one image, lane (l, q) of its 256 = NL x QW owns column w0 + l and channel
// quad q and walks the rows, four at a time with the loads issued together; a row step of the workgroup is one contiguous run of NL * QW * 16 bytes.
// What depends on (b, w, c) only - a_w, gw / H, the column sum - stays in registers over the walk.  RH shrinks from 32 until about a thousand
// workgroups exist (small maps), see ca_plan.
//
// The two reductions: the column sum of the workgroup's rows is formed in the lane's register, rows in order; the row sum over its NL columns goes
// through LDS, columns in order.  Both land as partials in the caller's workspace - row partials [B][H][nWc][C], column partials [B][nHc][W][C] -
// and a second launch adds each output's partials in order.  No float atomics: two launches are bit-identical.
#include "common.h"

namespace somi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CA_RU = 4;          // rows in flight per lane

struct CaPlan {
    int QW, NL;                   // quads and columns of a workgroup: QW * NL <= 256
    int nQc, nWc, nHc, RH;        // quad chunks (C / 4 > 256 only), column chunks, row chunks, rows per chunk
};

static CaPlan ca_plan(int B, int H, int W, int C) {
    CaPlan p;
    const int C4 = C / 4;
    p.QW = C4 < 256 ? C4 : 256;
    p.NL = 256 / p.QW;
    p.nQc = cdiv(C4, 256);
    p.nWc = cdiv(W, p.NL);
    p.RH = 32;
    while (p.RH > CA_RU && (long)B * p.nQc * p.nWc * cdiv(H, p.RH) < 1024) p.RH /= 2;
    p.nHc = cdiv(H, p.RH);
    return p;
}

struct CaRows { float *p; int cs, coff, rows; };       // a (B, rows, cs) tensor read or written at [b][r][coff + c], r < H or r < W

struct CaArgs {
    const float *x; int x_cs, x_coff;
    const float *y; int y_cs, y_coff;                  // dout of the two backward passes
    const float *res; int res_cs, res_coff;
    float *out; int o_cs, o_coff;                      // apply: out;  input bwd: dx
    CaRows ah, aw, rh, rw;                             // the gates;  rh / rw: gh / gw of the input backward
    float *rowpart, *colpart;
    int accumulate;
    int H, W, C4, QW, NL, nQc, nWc, nHc, RH;
};

struct CaLane { int b, q, w, h0, h1; bool on; };

__device__ __forceinline__ CaLane ca_lane(const CaArgs &a) {
    CaLane l;
    const int t = threadIdx.x, lane = t / a.QW;
    l.b = blockIdx.z / a.nQc;
    l.q = (blockIdx.z - l.b * a.nQc) * 256 + (t - lane * a.QW);
    l.w = blockIdx.x * a.NL + lane;
    l.h0 = blockIdx.y * a.RH;
    l.h1 = min(a.H, l.h0 + a.RH);
    l.on = lane < a.NL && l.q < a.C4 && l.w < a.W;
    return l;
}

__device__ __forceinline__ f32x4 ca_row(const CaRows &r, int b, int i, int q) {
    return *reinterpret_cast<const f32x4 *>(r.p + ((long)b * r.rows + i) * r.cs + r.coff + 4 * q);
}

// ------------------------------------------------------------------------------------------------ the two reductions, stage 1
// BWD = false: row and column sums of x.  BWD = true: of dout * x * a_w (rows) and dout * x * a_h (columns).
template <bool BWD>
__global__ __launch_bounds__(256) void ca_reduce_kernel(CaArgs a) {
    __shared__ f32x4 srow[CA_RU][256];
    const int t = threadIdx.x;
    const CaLane l = ca_lane(a);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 col = zero, aw = zero;
    if (BWD && l.on) aw = ca_row(a.aw, l.b, l.w, l.q);
    for (int g = l.h0; g < l.h1; g += CA_RU) {
        f32x4 v[CA_RU], d[CA_RU], ah[CA_RU];
#pragma unroll
        for (int r = 0; r < CA_RU; ++r) {
            v[r] = d[r] = ah[r] = zero;
            if (l.on && g + r < l.h1) {
                const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
                v[r] = *reinterpret_cast<const f32x4 *>(a.x + pix * a.x_cs + a.x_coff + 4 * l.q);
                if (BWD) {
                    d[r] = *reinterpret_cast<const f32x4 *>(a.y + pix * a.y_cs + a.y_coff + 4 * l.q);
                    ah[r] = ca_row(a.ah, l.b, g + r, l.q);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < CA_RU; ++r) {
            if (BWD) {
                const f32x4 dv = d[r] * v[r];
                col += dv * ah[r];
                srow[r][t] = dv * aw;
            } else {
                col += v[r];
                srow[r][t] = v[r];
            }
        }
        __syncthreads();
        // the row sums over this workgroup's columns, columns in order: one lane per (row, quad)
        for (int it = t; it < CA_RU * a.QW; it += 256) {
            const int r = it / a.QW, qq = it - r * a.QW;
            const int q = (blockIdx.z % a.nQc) * 256 + qq;
            if (g + r < l.h1 && q < a.C4) {
                f32x4 s = srow[r][qq];
                for (int k = 1; k < a.NL; ++k) s += srow[r][k * a.QW + qq];
                *reinterpret_cast<f32x4 *>(a.rowpart + (((long)l.b * a.H + g + r) * a.nWc + blockIdx.x) * (4 * a.C4) + 4 * q) = s;
            }
        }
        __syncthreads();
    }
    if (l.on) *reinterpret_cast<f32x4 *>(a.colpart + (((long)l.b * a.nHc + blockIdx.y) * a.W + l.w) * (4 * a.C4) + 4 * l.q) = col;
}

// stage 2: one lane per (image, row of the (H + W)-row layout, quad) adds its partials in order;  MEAN divides by the number of elements
template <bool MEAN>
__global__ __launch_bounds__(256) void ca_reduce_finish_kernel(CaArgs a, int B) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * (a.H + a.W) * a.C4) return;
    const int q = (int)(i % a.C4);
    const long br = i / a.C4;
    const int r = (int)(br % (a.H + a.W)), b = (int)(br / (a.H + a.W));
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (r < a.H) {
        const float *p = a.rowpart + ((long)b * a.H + r) * a.nWc * (4 * a.C4) + 4 * q;
        for (int k = 0; k < a.nWc; ++k) s += *reinterpret_cast<const f32x4 *>(p + (long)k * (4 * a.C4));
        if (MEAN) s = s / (float)a.W;
        *reinterpret_cast<f32x4 *>(a.rh.p + ((long)b * a.rh.rows + r) * a.rh.cs + a.rh.coff + 4 * q) = s;
    } else {
        const int w = r - a.H;
        const float *p = a.colpart + ((long)b * a.nHc * a.W + w) * (4 * a.C4) + 4 * q;
        for (int k = 0; k < a.nHc; ++k) s += *reinterpret_cast<const f32x4 *>(p + (long)k * a.W * (4 * a.C4));
        if (MEAN) s = s / (float)a.H;
        *reinterpret_cast<f32x4 *>(a.rw.p + ((long)b * a.rw.rows + w) * a.rw.cs + a.rw.coff + 4 * q) = s;
    }
}

// ------------------------------------------------------------------------------------------------ the two element-wise passes
// BWD = false: out = [res +] x * a_h * a_w.  BWD = true: dx = [dx +] dout * a_h * a_w + gh / W + gw / H   (x is not read).
template <bool BWD>
__global__ __launch_bounds__(256) void ca_apply_kernel(CaArgs a) {
    const CaLane l = ca_lane(a);
    if (!l.on) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 aw = ca_row(a.aw, l.b, l.w, l.q);
    f32x4 gw = zero;
    if (BWD) gw = ca_row(a.rw, l.b, l.w, l.q) / (float)a.H;
    const float *src = BWD ? a.y : a.x;
    const int s_cs = BWD ? a.y_cs : a.x_cs, s_coff = BWD ? a.y_coff : a.x_coff;
    const bool add = BWD ? a.accumulate != 0 : a.res != nullptr;
    for (int g = l.h0; g < l.h1; g += CA_RU) {
        f32x4 v[CA_RU], ah[CA_RU], e[CA_RU], gh[CA_RU];
#pragma unroll
        for (int r = 0; r < CA_RU; ++r) {
            if (g + r >= l.h1) continue;
            const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
            v[r] = *reinterpret_cast<const f32x4 *>(src + pix * s_cs + s_coff + 4 * l.q);
            ah[r] = ca_row(a.ah, l.b, g + r, l.q);
            e[r] = zero;
            if (add) e[r] = BWD ? *reinterpret_cast<const f32x4 *>(a.out + pix * a.o_cs + a.o_coff + 4 * l.q)
                                : *reinterpret_cast<const f32x4 *>(a.res + pix * a.res_cs + a.res_coff + 4 * l.q);
            if (BWD) gh[r] = ca_row(a.rh, l.b, g + r, l.q);
        }
#pragma unroll
        for (int r = 0; r < CA_RU; ++r) {
            if (g + r >= l.h1) continue;
            const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
            f32x4 o = v[r] * aw * ah[r];
            if (BWD) o += gh[r] / (float)a.W + gw;
            if (add) o += e[r];
            *reinterpret_cast<f32x4 *>(a.out + pix * a.o_cs + a.o_coff + 4 * l.q) = o;
        }
    }
}

enum CaOp { CA_MEANS, CA_APPLY, CA_GATES_BWD, CA_INPUT_BWD };

static CaRows ca_rows(const somi_slice &s, int rows) { return CaRows{s.p, s.cs, s.coff, rows}; }

// checks the descriptor for `op` and fills the kernel arguments; nothing is launched on an error
static int ca_unpack(const somi_coordatt_desc *d, CaOp op, CaArgs &a, CaPlan &p, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C % 4 == 0 && (long)d->B * d->H * d->W < (1L << 31) &&
                 (long)d->B * (d->H + d->W) * (d->C / 4) < (1L << 31) && (long)d->B * cdiv(d->C / 4, 256) <= 65535 && d->H <= CA_RU * 65535,
                 SOMI_EINVAL, "%s: bad sizes (C a multiple of 4, fewer than 2^31 pixels)", who);
    const int C = d->C;
    if (op == CA_MEANS) {
        SOMI_REQUIRE_SLICES(who, {"x", d->x.p, d->x.cs, d->x.coff, C}, {"pool", d->pool.p, d->pool.cs, d->pool.coff, C});
    } else {
        SOMI_REQUIRE(d->a_h_rows >= d->H && d->a_w_rows >= d->W, SOMI_EINVAL, "%s: a_h needs at least H rows per image and a_w at least W", who);
        SOMI_REQUIRE_SLICES(who, {"a_h", d->a_h.p, d->a_h.cs, d->a_h.coff, C}, {"a_w", d->a_w.p, d->a_w.cs, d->a_w.coff, C});
    }
    if (op == CA_APPLY)
        SOMI_REQUIRE_SLICES(who, {"x", d->x.p, d->x.cs, d->x.coff, C}, {"out", d->y.p, d->y.cs, d->y.coff, C},
                            {"res", d->res.p, d->res.cs, d->res.coff, C, kOptional});
    if (op == CA_GATES_BWD)
        SOMI_REQUIRE_SLICES(who, {"x", d->x.p, d->x.cs, d->x.coff, C}, {"dout", d->y.p, d->y.cs, d->y.coff, C},
                            {"da_h", d->r_h.p, d->r_h.cs, d->r_h.coff, C}, {"da_w", d->r_w.p, d->r_w.cs, d->r_w.coff, C});
    if (op == CA_INPUT_BWD)
        SOMI_REQUIRE_SLICES(who, {"dout", d->y.p, d->y.cs, d->y.coff, C}, {"gh", d->r_h.p, d->r_h.cs, d->r_h.coff, C},
                            {"gw", d->r_w.p, d->r_w.cs, d->r_w.coff, C}, {"dx", d->dx.p, d->dx.cs, d->dx.coff, C});
    if (op == CA_GATES_BWD || op == CA_INPUT_BWD)
        SOMI_REQUIRE(d->r_h_rows >= d->H && d->r_w_rows >= d->W, SOMI_EINVAL, "%s: %s needs at least H rows per image and %s at least W", who,
                     op == CA_GATES_BWD ? "da_h" : "gh", op == CA_GATES_BWD ? "da_w" : "gw");
    if (op == CA_MEANS || op == CA_GATES_BWD) {
        SOMI_REQUIRE(d->workspace && aligned16(d->workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
        SOMI_REQUIRE(d->workspace_floats >= somi_coordatt_workspace_floats(d->B, d->H, d->W, C), SOMI_EWORKSPACE, "%s: workspace too small", who);
    }
    p = ca_plan(d->B, d->H, d->W, C);
    a = CaArgs{};
    a.x = d->x.p; a.x_cs = d->x.cs; a.x_coff = d->x.coff;
    a.y = d->y.p; a.y_cs = d->y.cs; a.y_coff = d->y.coff;
    a.res = d->res.p; a.res_cs = d->res.cs; a.res_coff = d->res.coff;
    a.ah = ca_rows(d->a_h, d->a_h_rows); a.aw = ca_rows(d->a_w, d->a_w_rows);
    a.rh = ca_rows(d->r_h, d->r_h_rows); a.rw = ca_rows(d->r_w, d->r_w_rows);
    if (op == CA_MEANS) {                            // the two halves of pool (B, H + W, .)
        a.rh = CaRows{d->pool.p, d->pool.cs, d->pool.coff, d->H + d->W};
        a.rw = CaRows{d->pool.p + (long)d->H * d->pool.cs, d->pool.cs, d->pool.coff, d->H + d->W};
    }
    if (op == CA_APPLY) { a.out = d->y.p; a.o_cs = d->y.cs; a.o_coff = d->y.coff; }
    if (op == CA_INPUT_BWD) { a.out = d->dx.p; a.o_cs = d->dx.cs; a.o_coff = d->dx.coff; }
    a.accumulate = d->accumulate;
    a.rowpart = d->workspace;
    a.colpart = d->workspace ? d->workspace + (size_t)d->B * d->H * p.nWc * C : nullptr;
    a.H = d->H; a.W = d->W; a.C4 = C / 4;
    a.QW = p.QW; a.NL = p.NL; a.nQc = p.nQc; a.nWc = p.nWc; a.nHc = p.nHc; a.RH = p.RH;
    return 0;
}

static dim3 ca_grid(const somi_coordatt_desc *d, const CaPlan &p) { return dim3(p.nWc, p.nHc, d->B * p.nQc); }

}  // namespace somi

using namespace somi;

extern "C" size_t somi_coordatt_desc_bytes(void) { return sizeof(somi_coordatt_desc); }

extern "C" size_t somi_coordatt_workspace_floats(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return 0;
    const CaPlan p = ca_plan(B, H, W, C);
    return ((size_t)B * H * p.nWc + (size_t)B * p.nHc * W) * C;
}

extern "C" int somi_coordatt_means_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream) {
    CaArgs a;
    CaPlan p;
    if (int rc = ca_unpack(d, CA_MEANS, a, p, "coordatt means")) return rc;
    hipLaunchKernelGGL(ca_reduce_kernel<false>, ca_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(ca_reduce_finish_kernel<true>, dim3(cdiv((long)d->B * (d->H + d->W) * a.C4, 256)), dim3(256), 0, (hipStream_t)stream, a, d->B);
    return launch_status("somi_coordatt_means_nhwc_f32");
}

extern "C" int somi_coordatt_apply_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream) {
    CaArgs a;
    CaPlan p;
    if (int rc = ca_unpack(d, CA_APPLY, a, p, "coordatt apply")) return rc;
    hipLaunchKernelGGL(ca_apply_kernel<false>, ca_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_coordatt_apply_nhwc_f32");
}

extern "C" int somi_coordatt_bwd_gates_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream) {
    CaArgs a;
    CaPlan p;
    if (int rc = ca_unpack(d, CA_GATES_BWD, a, p, "coordatt bwd gates")) return rc;
    hipLaunchKernelGGL(ca_reduce_kernel<true>, ca_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(ca_reduce_finish_kernel<false>, dim3(cdiv((long)d->B * (d->H + d->W) * a.C4, 256)), dim3(256), 0, (hipStream_t)stream, a, d->B);
    return launch_status("somi_coordatt_bwd_gates_nhwc_f32");
}

extern "C" int somi_coordatt_bwd_input_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream) {
    CaArgs a;
    CaPlan p;
    if (int rc = ca_unpack(d, CA_INPUT_BWD, a, p, "coordatt bwd input")) return rc;
    hipLaunchKernelGGL(ca_apply_kernel<true>, ca_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_coordatt_bwd_input_nhwc_f32");
}
