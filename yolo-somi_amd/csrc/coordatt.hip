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
// workgroups exist (small maps): map_plan and map_lane of common.h.
//
// The two reductions: the column sum of the workgroup's rows is formed in the lane's register, rows in order; the row sum over its NL columns goes
// through LDS, columns in order.  Both land as partials in the caller's workspace - row partials [B][H][nWc][C], column partials [B][nHc][W][C] -
// and a second launch adds each output's partials in order.  No float atomics: two launches are bit-identical.
#include "common.h"

namespace somi {

constexpr int CA_RU = 4;          // rows in flight per lane

struct CaRows { float *p; int cs, coff, rows; };       // a (B, rows, cs) tensor read or written at [b][r][coff + c], r < H or r < W

struct CaArgs {
    somi_slice x;
    somi_slice y;                                      // dout of the two backward passes
    somi_slice res;
    somi_slice out;                                    // apply: out;  input bwd: dx
    CaRows ah, aw, rh, rw;                             // the gates;  rh / rw: gh / gw of the input backward
    float *rowpart, *colpart;
    int accumulate;
    int H, W, C4, QW, NL, nQc, nWc, nHc, RH;
};

__device__ __forceinline__ f32x4 ca_row(const CaRows &r, int b, int i, int q) {
    return ld4(r.p + ((long)b * r.rows + i) * r.cs + r.coff + 4 * q);
}

// ------------------------------------------------------------------------------------------------ the two reductions, stage 1
// BWD = false: row and column sums of x.  BWD = true: of dout * x * a_w (rows) and dout * x * a_h (columns).
template <bool BWD>
__global__ __launch_bounds__(256) void ca_reduce_kernel(CaArgs a) {
    __shared__ f32x4 srow[CA_RU][256];
    const int t = threadIdx.x;
    const MapLane l = map_lane(a);
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
                v[r] = ld4(at(a.x, pix, l.q));
                if (BWD) {
                    d[r] = ld4(at(a.y, pix, l.q));
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
                st4(a.rowpart + (((long)l.b * a.H + g + r) * a.nWc + blockIdx.x) * (4 * a.C4) + 4 * q, s);
            }
        }
        __syncthreads();
    }
    if (l.on) st4(a.colpart + (((long)l.b * a.nHc + blockIdx.y) * a.W + l.w) * (4 * a.C4) + 4 * l.q, col);
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
        for (int k = 0; k < a.nWc; ++k) s += ld4(p + (long)k * (4 * a.C4));
        if (MEAN) s = s / (float)a.W;
        st4(a.rh.p + ((long)b * a.rh.rows + r) * a.rh.cs + a.rh.coff + 4 * q, s);
    } else {
        const int w = r - a.H;
        const float *p = a.colpart + ((long)b * a.nHc * a.W + w) * (4 * a.C4) + 4 * q;
        for (int k = 0; k < a.nHc; ++k) s += ld4(p + (long)k * a.W * (4 * a.C4));
        if (MEAN) s = s / (float)a.H;
        st4(a.rw.p + ((long)b * a.rw.rows + w) * a.rw.cs + a.rw.coff + 4 * q, s);
    }
}

// ------------------------------------------------------------------------------------------------ the two element-wise passes
// BWD = false: out = [res +] x * a_h * a_w.  BWD = true: dx = [dx +] dout * a_h * a_w + gh / W + gw / H   (x is not read).
template <bool BWD>
__global__ __launch_bounds__(256) void ca_apply_kernel(CaArgs a) {
    const MapLane l = map_lane(a);
    if (!l.on) return;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 aw = ca_row(a.aw, l.b, l.w, l.q);
    f32x4 gw = zero;
    if (BWD) gw = ca_row(a.rw, l.b, l.w, l.q) / (float)a.H;
    const somi_slice src = BWD ? a.y : a.x;
    const bool add = BWD ? a.accumulate != 0 : a.res.p != nullptr;
    for (int g = l.h0; g < l.h1; g += CA_RU) {
        f32x4 v[CA_RU], ah[CA_RU], e[CA_RU], gh[CA_RU];
#pragma unroll
        for (int r = 0; r < CA_RU; ++r) {
            if (g + r >= l.h1) continue;
            const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
            v[r] = ld4(at(src, pix, l.q));
            ah[r] = ca_row(a.ah, l.b, g + r, l.q);
            e[r] = zero;
            // spelled out: the helpers schedule this one select differently
            if (add) e[r] = BWD ? *reinterpret_cast<const f32x4 *>(a.out.p + pix * a.out.cs + a.out.coff + 4 * l.q)
                                : *reinterpret_cast<const f32x4 *>(a.res.p + pix * a.res.cs + a.res.coff + 4 * l.q);
            if (BWD) gh[r] = ca_row(a.rh, l.b, g + r, l.q);
        }
#pragma unroll
        for (int r = 0; r < CA_RU; ++r) {
            if (g + r >= l.h1) continue;
            const long pix = ((long)l.b * a.H + g + r) * a.W + l.w;
            f32x4 o = v[r] * aw * ah[r];
            if (BWD) o += gh[r] / (float)a.W + gw;
            if (add) o += e[r];
            st4(at_w(a.out, pix, l.q), o);
        }
    }
}

enum CaOp { CA_MEANS, CA_APPLY, CA_GATES_BWD, CA_INPUT_BWD };

static CaRows ca_rows(const somi_slice &s, int rows) { return CaRows{s.p, s.cs, s.coff, rows}; }

// checks the descriptor for `op` and fills the kernel arguments; nothing is launched on an error
static int ca_unpack(const somi_coordatt_desc *d, CaOp op, CaArgs &a, MapPlan &p, const char *who) {
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
    p = map_plan(d->B, d->H, d->W, C, CA_RU);
    a = CaArgs{};
    a.x = d->x; a.y = d->y; a.res = d->res;
    a.ah = ca_rows(d->a_h, d->a_h_rows); a.aw = ca_rows(d->a_w, d->a_w_rows);
    a.rh = ca_rows(d->r_h, d->r_h_rows); a.rw = ca_rows(d->r_w, d->r_w_rows);
    if (op == CA_MEANS) {                            // the two halves of pool (B, H + W, .)
        a.rh = CaRows{d->pool.p, d->pool.cs, d->pool.coff, d->H + d->W};
        a.rw = CaRows{d->pool.p + (long)d->H * d->pool.cs, d->pool.cs, d->pool.coff, d->H + d->W};
    }
    if (op == CA_APPLY) a.out = d->y;
    if (op == CA_INPUT_BWD) a.out = d->dx;
    a.accumulate = d->accumulate;
    a.rowpart = d->workspace;
    a.colpart = d->workspace ? d->workspace + (size_t)d->B * d->H * p.nWc * C : nullptr;
    a.H = d->H; a.W = d->W; a.C4 = C / 4;
    a.QW = p.QW; a.NL = p.NL; a.nQc = p.nQc; a.nWc = p.nWc; a.nHc = p.nHc; a.RH = p.RH;
    return 0;
}

static dim3 ca_grid(const somi_coordatt_desc *d, const MapPlan &p) { return dim3(p.nWc, p.nHc, d->B * p.nQc); }

}  // namespace somi

using namespace somi;

extern "C" size_t somi_coordatt_desc_bytes(void) { return sizeof(somi_coordatt_desc); }

extern "C" size_t somi_coordatt_workspace_floats(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return 0;
    const MapPlan p = map_plan(B, H, W, C, CA_RU);
    return ((size_t)B * H * p.nWc + (size_t)B * p.nHc * W) * C;
}

extern "C" int somi_coordatt_means_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream) {
    CaArgs a;
    MapPlan p;
    if (int rc = ca_unpack(d, CA_MEANS, a, p, "coordatt means")) return rc;
    hipLaunchKernelGGL(ca_reduce_kernel<false>, ca_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(ca_reduce_finish_kernel<true>, dim3(cdiv((long)d->B * (d->H + d->W) * a.C4, 256)), dim3(256), 0, (hipStream_t)stream, a, d->B);
    return launch_status("somi_coordatt_means_nhwc_f32");
}

extern "C" int somi_coordatt_apply_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream) {
    CaArgs a;
    MapPlan p;
    if (int rc = ca_unpack(d, CA_APPLY, a, p, "coordatt apply")) return rc;
    hipLaunchKernelGGL(ca_apply_kernel<false>, ca_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_coordatt_apply_nhwc_f32");
}

extern "C" int somi_coordatt_bwd_gates_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream) {
    CaArgs a;
    MapPlan p;
    if (int rc = ca_unpack(d, CA_GATES_BWD, a, p, "coordatt bwd gates")) return rc;
    hipLaunchKernelGGL(ca_reduce_kernel<true>, ca_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(ca_reduce_finish_kernel<false>, dim3(cdiv((long)d->B * (d->H + d->W) * a.C4, 256)), dim3(256), 0, (hipStream_t)stream, a, d->B);
    return launch_status("somi_coordatt_bwd_gates_nhwc_f32");
}

extern "C" int somi_coordatt_bwd_input_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream) {
    CaArgs a;
    MapPlan p;
    if (int rc = ca_unpack(d, CA_INPUT_BWD, a, p, "coordatt bwd input")) return rc;
    hipLaunchKernelGGL(ca_apply_kernel<true>, ca_grid(d, p), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_coordatt_bwd_input_nhwc_f32");
}
