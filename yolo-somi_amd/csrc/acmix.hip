// ACmix (models/common.py:7281-7365): a 7x7 sliding-window multi-head attention with reflection padding and a linear position term, mixed with
// a grouped 3x3 conv over the same q / k / v.  With C = out_planes, 4 heads, D = C / 4, channel (h, d) = h * D + d, s = D ** -0.5, taps j over the
// 7x7 window, r(.) the reflected index (-i below 0, 2 (n - 1) - i above n - 1), lx(x) = -1 + 2 x / (W - 1), ly likewise:
//   score_j = s * (q_p . k_r(p+j) + qwx_p * (lx(p) - lx(r(p+j))) + qwy_p * (ly(p) - ly(r(p+j)))),  qwx_p = q_p . Wp[:, 0], qwy_p = q_p . Wp[:, 1]
//   a = softmax_j(score), att_p = sum_j a_j v_r(p+j);  out = rate1 * att + rate2 * mix
//   mix[., 4 d + o] = bias[4 d + o] + sum_(t, tap) Weff[t][tap][d][o] * src_t[p + tap][d],  the 12 sources t = 4 * (q, k, v) + head
// conv_p's bias and the position map itself never appear: only differences of pe enter.
//
// Attention kernels: a workgroup of 256 lanes owns an 8 x 8 tile of pixels of one image, lane = (head, pixel).  The tile and its 3-pixel halo of
// the windowed operand sit in LDS as [head][quad of d][halo pixel], 16 values of d per head at a time (AC_DC): neighbouring lanes read neighbouring
// float4s.  Staging goes through the reflected indices (k, v) or zero-fills outside the map (bwd kv, whose window is over the queries), so the
// 49-tap loops carry no border branch.  The scores live in registers (49 per lane) and accumulate over the chunks of d.
//   forward  scores over the chunks of k, softmax (maximum subtracted), output per chunk of v with the mix in the epilogue; training: lse
//   bwd q    probabilities from q, k and lse; e_j = dout_p . v_j over the chunks of v; dS; dq over the chunks of k; per (pixel, head) into aux:
//            delta, qwx, qwy, gx = sum_j dS_j dx_j, gy, the factor that puts sum_j a_j back to 1; the workgroup's sums of dout . att and
//            dout . mix in a fixed order
//   bwd kv   the owner pixel p' gathers: every query p of the clipped 7x7 window around p' reaches p' through m = my * mx taps (1 + one per
//            border whose reflection maps a tap of p onto p'), all with the same score, so dv_p' = sum_p m a_pp' rate1 dout_p and
//            dk_p' = s sum_p m dS_pp' q_p with q and dout staged as the windowed operands.  Reads aux: bwd q runs first.
// No value is added to memory by more than one lane: the reductions (drate1, drate2, dWp, dWeff, the bias gradient) go through per-workgroup
// partials folded in a fixed order.
#include "common.h"

namespace somi {

constexpr int AC_T = 8;                      // tile edge
constexpr int AC_HALO = AC_T + 6;            // 14
constexpr int AC_HP = AC_HALO * AC_HALO;     // 196 halo pixels
constexpr int AC_DC4 = 4;                    // quads of d per head and chunk (16 values)
constexpr int AC_AUX = 24;                   // delta, qwx, qwy, gx, gy, 1 / sum_j exp(score_j - lse) per head
constexpr int AC_WG_ROWS = 12 * 9 * 4;       // Weff values per d
constexpr size_t AC_WGRAD_CAP = 4u << 20;    // floats of weight-gradient partials at most

struct AcArgs {
    somi_slice q, k, v, mix, out, lse, aux, dq, dk, dv;
    const float *wp, *rate1, *rate2, *weff, *bias;
    float *dwp, *drates, *dweff, *dbias, *part;
    int accumulate;
    int B, H, W, C, D, nty, ntx, nP, rows_per;
    float scale;
};

__device__ __forceinline__ int ac_refl(int i, int n) { return i < 0 ? -i : (i > n - 1 ? 2 * (n - 1) - i : i); }

// the tile's halo of `src`, channels h * D + d0 + [0, 4 n4) of every head -> sm[(h * AC_DC4 + i4) * AC_HP + halo pixel]
template <bool REFLECT>
__device__ __forceinline__ void ac_stage(const AcArgs &a, const somi_slice &src, f32x4 *sm, int b, int y0, int x0, int d0, int n4) {
    const int per = 4 * n4, total = AC_HP * per;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int hp = i / per, c = i - hp * per, h = c / n4, i4 = c - h * n4;
        const int hy = hp / AC_HALO, hx = hp - hy * AC_HALO;
        int gy = y0 - 3 + hy, gx = x0 - 3 + hx;
        f32x4 val = {0.f, 0.f, 0.f, 0.f};
        bool in;
        if (REFLECT) {
            in = gy <= a.H + 2 && gx <= a.W + 2;                  // beyond the pad of a ragged tile: never read by an active lane
            gy = ac_refl(gy, a.H);
            gx = ac_refl(gx, a.W);
        } else {
            in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        }
        if (in) val = ld4(at_ch(src, ((long)b * a.H + gy) * a.W + gx, h * a.D + d0 + 4 * i4));
        sm[(h * AC_DC4 + i4) * AC_HP + hp] = val;
    }
}

struct AcLane { int b, h, ty, tx, y, x, y0, x0; bool on; long pix; };

__device__ __forceinline__ AcLane ac_lane(const AcArgs &a) {
    AcLane l;
    const int t = threadIdx.x, pl = t & 63;
    l.h = t >> 6;
    l.ty = pl >> 3;
    l.tx = pl & 7;
    l.b = blockIdx.z;
    l.y0 = blockIdx.y * AC_T;
    l.x0 = blockIdx.x * AC_T;
    l.y = l.y0 + l.ty;
    l.x = l.x0 + l.tx;
    l.on = l.y < a.H && l.x < a.W;
    l.pix = ((long)l.b * a.H + (l.on ? l.y : 0)) * a.W + (l.on ? l.x : 0);
    return l;
}

// sc[j] += q_p . w_j over the staged chunk (w = the windowed operand), own = this lane's chunk of the centred operand
__device__ __forceinline__ void ac_dots(const f32x4 *sm, const AcLane &l, const f32x4 (&own)[AC_DC4], int n4, float (&sc)[49]) {
#pragma unroll
    for (int i4 = 0; i4 < AC_DC4; ++i4) {
        if (i4 >= n4) break;
        const f32x4 *row = sm + (l.h * AC_DC4 + i4) * AC_HP + l.ty * AC_HALO + l.tx;
#pragma unroll
        for (int jy = 0; jy < 7; ++jy)
#pragma unroll
            for (int jx = 0; jx < 7; ++jx) sc[jy * 7 + jx] += dot4(own[i4], row[jy * AC_HALO + jx]);
    }
}

// acc[i4] += sum_j w[j] * staged_j
__device__ __forceinline__ void ac_gather(const f32x4 *sm, const AcLane &l, const float (&w)[49], int n4, f32x4 (&acc)[AC_DC4]) {
#pragma unroll
    for (int i4 = 0; i4 < AC_DC4; ++i4) {
        if (i4 >= n4) break;
        const f32x4 *row = sm + (l.h * AC_DC4 + i4) * AC_HP + l.ty * AC_HALO + l.tx;
#pragma unroll
        for (int jy = 0; jy < 7; ++jy)
#pragma unroll
            for (int jx = 0; jx < 7; ++jx) acc[i4] += w[jy * 7 + jx] * row[jy * AC_HALO + jx];
    }
}

__device__ __forceinline__ void ac_own(const somi_slice &s, const AcLane &l, int D, int d0, int n4, f32x4 (&o)[AC_DC4]) {
#pragma unroll
    for (int i4 = 0; i4 < AC_DC4; ++i4) o[i4] = (l.on && i4 < n4) ? ld4(at_ch(s, l.pix, l.h * D + d0 + 4 * i4)) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// scores of the query at this lane over its reflected window: sc = s * (q . k_j + qwx * dx_j + qwy * dy_j); qwx / qwy returned
__device__ __forceinline__ void ac_query_scores(const AcArgs &a, const AcLane &l, f32x4 *sm, float (&sc)[49], float (&dxs)[7], float (&dys)[7],
                                                float &qwx, float &qwy) {
#pragma unroll
    for (int j = 0; j < 49; ++j) sc[j] = 0.f;
    qwx = qwy = 0.f;
    for (int d0 = 0; d0 < a.D; d0 += 4 * AC_DC4) {
        const int n4 = min(AC_DC4, (a.D - d0) / 4);
        ac_stage<true>(a, a.k, sm, l.b, l.y0, l.x0, d0, n4);
        f32x4 qv[AC_DC4];
        ac_own(a.q, l, a.D, d0, n4, qv);
#pragma unroll
        for (int i4 = 0; i4 < AC_DC4; ++i4) {
            if (i4 >= n4) break;
            const float *w = a.wp + 2 * (d0 + 4 * i4);
            qwx += qv[i4].x * w[0] + qv[i4].y * w[2] + qv[i4].z * w[4] + qv[i4].w * w[6];
            qwy += qv[i4].x * w[1] + qv[i4].y * w[3] + qv[i4].z * w[5] + qv[i4].w * w[7];
        }
        __syncthreads();
        if (l.on) ac_dots(sm, l, qv, n4, sc);
        __syncthreads();
    }
    const float ix = 2.0f / (float)(a.W - 1), iy = 2.0f / (float)(a.H - 1);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        dxs[j] = (float)(l.x - ac_refl(l.x + j - 3, a.W)) * ix;
        dys[j] = (float)(l.y - ac_refl(l.y + j - 3, a.H)) * iy;
    }
#pragma unroll
    for (int jy = 0; jy < 7; ++jy)
#pragma unroll
        for (int jx = 0; jx < 7; ++jx) sc[jy * 7 + jx] = a.scale * (sc[jy * 7 + jx] + qwx * dxs[jx] + qwy * dys[jy]);
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void ac_attn_kernel(AcArgs a) {
    __shared__ f32x4 sm[4 * AC_DC4 * AC_HP];
    const AcLane l = ac_lane(a);
    float sc[49], dxs[7], dys[7], qwx, qwy;
    ac_query_scores(a, l, sm, sc, dxs, dys, qwx, qwy);
    float mx = sc[0];
#pragma unroll
    for (int j = 1; j < 49; ++j) mx = fmaxf(mx, sc[j]);
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < 49; ++j) { sc[j] = expf(sc[j] - mx); den += sc[j]; }
    const float inv = 1.0f / den;
#pragma unroll
    for (int j = 0; j < 49; ++j) sc[j] *= inv;
    if (a.lse.p && l.on) a.lse.p[l.pix * a.lse.cs + a.lse.coff + l.h] = mx + logf(den);
    const float r1 = a.rate1[0], r2 = a.rate2[0];
    for (int d0 = 0; d0 < a.D; d0 += 4 * AC_DC4) {
        const int n4 = min(AC_DC4, (a.D - d0) / 4);
        ac_stage<true>(a, a.v, sm, l.b, l.y0, l.x0, d0, n4);
        __syncthreads();
        if (l.on) {
            f32x4 acc[AC_DC4] = {};
            ac_gather(sm, l, sc, n4, acc);
#pragma unroll
            for (int i4 = 0; i4 < AC_DC4; ++i4) {
                if (i4 >= n4) break;
                const int c = l.h * a.D + d0 + 4 * i4;
                f32x4 o = r1 * acc[i4];
                if (a.mix.p) o += r2 * ld4(at_ch(a.mix, l.pix, c));
                st4(at_ch_w(a.out, l.pix, c), o);
            }
        }
        __syncthreads();
    }
}

// the workgroup's lanes added in lane order -> part[wg * K + k]
template <int K>
__device__ __forceinline__ void ac_fold_wg(float *red, const float (&v)[K], float *part) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * 256 + t] = v[k];
    __syncthreads();
    if (t < K) {
        float s = 0.f;
        for (int i = 0; i < 256; ++i) s += red[t * 256 + i];
        const long wg = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[wg * K + t] = s;
    }
}

// ------------------------------------------------------------------------------------------------ query-centred backward
__global__ __launch_bounds__(256) void ac_bwd_q_kernel(AcArgs a) {
    __shared__ f32x4 sm[4 * AC_DC4 * AC_HP];
    const AcLane l = ac_lane(a);
    float sc[49], e[49], dxs[7], dys[7], qwx, qwy;
    ac_query_scores(a, l, sm, sc, dxs, dys, qwx, qwy);
    const float lse = l.on ? a.lse.p[l.pix * a.lse.cs + a.lse.coff + l.h] : 0.f;
#pragma unroll
    for (int j = 0; j < 49; ++j) { sc[j] = expf(sc[j] - lse); e[j] = 0.f; }
    // lse is an fp32 number of the scores' size: at scores near 100 it leaves sum_j a_j off 1 by 1e-5, which dS_j = a_j (r1 e_j - sum a r1 e)
    // does not forgive where one a_j is nearly 1.  The saved value spares the pass for the maximum; the 49 values are put back to sum 1.
    float asum = 0.f;
#pragma unroll
    for (int j = 0; j < 49; ++j) asum += sc[j];
    const float ainv = 1.0f / asum;
#pragma unroll
    for (int j = 0; j < 49; ++j) sc[j] *= ainv;
    float sums[2] = {0.f, 0.f};                                   // dout . att, dout . mix
    for (int d0 = 0; d0 < a.D; d0 += 4 * AC_DC4) {
        const int n4 = min(AC_DC4, (a.D - d0) / 4);
        ac_stage<true>(a, a.v, sm, l.b, l.y0, l.x0, d0, n4);
        f32x4 g[AC_DC4];
        ac_own(a.out, l, a.D, d0, n4, g);
        if (a.mix.p && l.on)
#pragma unroll
            for (int i4 = 0; i4 < AC_DC4; ++i4)
                if (i4 < n4) sums[1] += dot4(g[i4], ld4(at_ch(a.mix, l.pix, l.h * a.D + d0 + 4 * i4)));
        __syncthreads();
        if (l.on) ac_dots(sm, l, g, n4, e);
        __syncthreads();
    }
    const float r1 = a.rate1[0];
    float pe = 0.f;
#pragma unroll
    for (int j = 0; j < 49; ++j) pe += sc[j] * e[j];
    sums[0] = l.on ? pe : 0.f;
    const float delta = r1 * pe;
    float gx = 0.f, gy = 0.f;
#pragma unroll
    for (int jy = 0; jy < 7; ++jy)
#pragma unroll
        for (int jx = 0; jx < 7; ++jx) {
            const int j = jy * 7 + jx;
            e[j] = sc[j] * (r1 * e[j] - delta);                   // dS_j
            gx += e[j] * dxs[jx];
            gy += e[j] * dys[jy];
        }
    if (l.on) {
        float *ax = a.aux.p + l.pix * a.aux.cs + a.aux.coff;
        ax[l.h] = delta; ax[4 + l.h] = qwx; ax[8 + l.h] = qwy; ax[12 + l.h] = gx; ax[16 + l.h] = gy; ax[20 + l.h] = ainv;
    }
    for (int d0 = 0; d0 < a.D; d0 += 4 * AC_DC4) {
        const int n4 = min(AC_DC4, (a.D - d0) / 4);
        ac_stage<true>(a, a.k, sm, l.b, l.y0, l.x0, d0, n4);
        __syncthreads();
        if (l.on) {
            f32x4 acc[AC_DC4] = {};
            ac_gather(sm, l, e, n4, acc);
#pragma unroll
            for (int i4 = 0; i4 < AC_DC4; ++i4) {
                if (i4 >= n4) break;
                const int c = l.h * a.D + d0 + 4 * i4;
                const float *w = a.wp + 2 * (d0 + 4 * i4);
                const f32x4 wx = {w[0], w[2], w[4], w[6]}, wy = {w[1], w[3], w[5], w[7]};
                f32x4 o = a.scale * (acc[i4] + gx * wx + gy * wy);
                if (a.accumulate) o += ld4(at_ch(a.dq, l.pix, c));
                st4(at_ch_w(a.dq, l.pix, c), o);
            }
        }
        __syncthreads();
    }
    ac_fold_wg<2>(reinterpret_cast<float *>(sm), sums, a.part);
}

// one workgroup: the nP partial pairs in order -> drates[0..1]
__global__ __launch_bounds__(256) void ac_rates_finish_kernel(AcArgs a) {
    __shared__ float red[2][256];
    const int t = threadIdx.x;
    float s0 = 0.f, s1 = 0.f;
    for (int i = t; i < a.nP; i += 256) { s0 += a.part[2 * i]; s1 += a.part[2 * i + 1]; }
    red[0][t] = s0; red[1][t] = s1;
    __syncthreads();
    if (t < 2) {
        float s = 0.f;
        for (int i = 0; i < 256; ++i) s += red[t][i];
        a.drates[t] = s;
    }
}

// dWp[d][xy] = s * sum_(pixel, h) q[pixel][h D + d] * g_xy[pixel][h]: block i takes the pixels i, i + nB, ... and one lane per channel
__global__ __launch_bounds__(256) void ac_dwp_partial_kernel(AcArgs a, float *part, int nB) {
    const long npix = (long)a.B * a.H * a.W;
    for (int c = threadIdx.x; c < a.C; c += 256) {
        const int h = c / a.D;
        float sx = 0.f, sy = 0.f;
        for (long p = blockIdx.x; p < npix; p += nB) {
            const float qv = a.q.p[p * a.q.cs + a.q.coff + c];
            const float *ax = a.aux.p + p * a.aux.cs + a.aux.coff;
            sx += qv * ax[12 + h];
            sy += qv * ax[16 + h];
        }
        part[((long)blockIdx.x * a.C + c) * 2] = sx;
        part[((long)blockIdx.x * a.C + c) * 2 + 1] = sy;
    }
}

__global__ __launch_bounds__(256) void ac_dwp_finish_kernel(AcArgs a, const float *part, int nB) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * a.D) return;
    const int d = i >> 1, xy = i & 1;
    float s = 0.f;
    for (int b = 0; b < nB; ++b)
        for (int h = 0; h < 4; ++h) s += part[((long)b * a.C + h * a.D + d) * 2 + xy];
    a.dwp[i] = a.scale * s;
}

// ------------------------------------------------------------------------------------------------ key-centred backward
__device__ __forceinline__ int ac_mult(int p, int o, int n) {     // taps of the query at p that reach the owner at o along one axis (|o - p| <= 3)
    return 1 + (o > 0 && o + p <= 3 ? 1 : 0) + (o < n - 1 && 2 * (n - 1) - o - p <= 3 ? 1 : 0);
}

__global__ __launch_bounds__(256) void ac_bwd_kv_kernel(AcArgs a) {
    __shared__ f32x4 sm[4 * AC_DC4 * AC_HP];
    const AcLane l = ac_lane(a);
    float sc[49], e[49];
#pragma unroll
    for (int j = 0; j < 49; ++j) sc[j] = e[j] = 0.f;
    for (int d0 = 0; d0 < a.D; d0 += 4 * AC_DC4) {
        const int n4 = min(AC_DC4, (a.D - d0) / 4);
        f32x4 own[AC_DC4];
        ac_stage<false>(a, a.q, sm, l.b, l.y0, l.x0, d0, n4);
        ac_own(a.k, l, a.D, d0, n4, own);
        __syncthreads();
        if (l.on) ac_dots(sm, l, own, n4, sc);
        __syncthreads();
        ac_stage<false>(a, a.out, sm, l.b, l.y0, l.x0, d0, n4);
        ac_own(a.v, l, a.D, d0, n4, own);
        __syncthreads();
        if (l.on) ac_dots(sm, l, own, n4, e);
        __syncthreads();
    }
    const float r1 = a.rate1[0];
    const float ix = 2.0f / (float)(a.W - 1), iy = 2.0f / (float)(a.H - 1);
    if (l.on) {
#pragma unroll
        for (int jy = 0; jy < 7; ++jy)
#pragma unroll
            for (int jx = 0; jx < 7; ++jx) {
                const int j = jy * 7 + jx, py = l.y + jy - 3, px = l.x + jx - 3;
                float cv = 0.f, ck = 0.f;
                if (py >= 0 && py < a.H && px >= 0 && px < a.W) {
                    const long qp = ((long)l.b * a.H + py) * a.W + px;
                    const float *ax = a.aux.p + qp * a.aux.cs + a.aux.coff;
                    const float lse = a.lse.p[qp * a.lse.cs + a.lse.coff + l.h];
                    const float s = a.scale * (sc[j] + ax[4 + l.h] * ((float)(px - l.x) * ix) + ax[8 + l.h] * ((float)(py - l.y) * iy));
                    const float pm = (float)(ac_mult(py, l.y, a.H) * ac_mult(px, l.x, a.W)) * expf(s - lse) * ax[20 + l.h];
                    cv = pm * r1;
                    ck = pm * (r1 * e[j] - ax[l.h]) * a.scale;
                }
                sc[j] = cv;
                e[j] = ck;
            }
    }
    for (int d0 = 0; d0 < a.D; d0 += 4 * AC_DC4) {
        const int n4 = min(AC_DC4, (a.D - d0) / 4);
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            ac_stage<false>(a, pass ? a.q : a.out, sm, l.b, l.y0, l.x0, d0, n4);
            __syncthreads();
            if (l.on) {
                f32x4 acc[AC_DC4] = {};
                if (pass) ac_gather(sm, l, e, n4, acc); else ac_gather(sm, l, sc, n4, acc);
                const somi_slice &dst = pass ? a.dk : a.dv;
#pragma unroll
                for (int i4 = 0; i4 < AC_DC4; ++i4) {
                    if (i4 >= n4) break;
                    const int c = l.h * a.D + d0 + 4 * i4;
                    f32x4 o = acc[i4];
                    if (a.accumulate) o += ld4(at_ch(dst, l.pix, c));
                    st4(at_ch_w(dst, l.pix, c), o);
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------ the conv half
// weff[((t * 9 + tap) * D + d) * 4 + o].  One lane per (image row, group of 4 columns, d), d fastest.
__device__ __forceinline__ const somi_slice &ac_src(const AcArgs &a, int t) { return t < 4 ? a.q : (t < 8 ? a.k : a.v); }

__global__ __launch_bounds__(256) void ac_conv_kernel(AcArgs a) {
    const int nxg = (a.W + 3) / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.B * a.H * nxg * a.D) return;
    const int d = (int)(i % a.D);
    const long r = i / a.D;
    const int xg = (int)(r % nxg), y = (int)((r / nxg) % a.H), b = (int)(r / nxg / a.H), x0 = xg * 4;
    const f32x4 bias = ld4(a.bias + 4 * d);
    f32x4 acc[4] = {bias, bias, bias, bias};
    for (int t = 0; t < 12; ++t) {
        const somi_slice &s = ac_src(a, t);
        const int c = (t & 3) * a.D + d;
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + ky - 1;
            if (yy < 0 || yy >= a.H) continue;
            float in[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int xx = x0 - 1 + k;
                in[k] = (xx >= 0 && xx < a.W) ? s.p[(((long)b * a.H + yy) * a.W + xx) * s.cs + s.coff + c] : 0.f;
            }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x4 w = ld4(a.weff + (((long)t * 9 + ky * 3 + kx) * a.D + d) * 4);
#pragma unroll
                for (int px = 0; px < 4; ++px) acc[px] += w * in[px + kx];
            }
        }
    }
#pragma unroll
    for (int px = 0; px < 4; ++px)
        if (x0 + px < a.W) st4(at_ch_w(a.mix, ((long)b * a.H + y) * a.W + x0 + px, 4 * d), acc[px]);
}

// dsrc_t[p][d] (+)= rate2 * sum_(tap, o) weff[t][tap][d][o] * dout[p - tap][4 d + o]
__global__ __launch_bounds__(256) void ac_conv_bwd_data_kernel(AcArgs a) {
    const int nxg = (a.W + 3) / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.B * a.H * nxg * a.D) return;
    const int d = (int)(i % a.D);
    const long r = i / a.D;
    const int xg = (int)(r % nxg), y = (int)((r / nxg) % a.H), b = (int)(r / nxg / a.H), x0 = xg * 4;
    float acc[12][4];
#pragma unroll
    for (int t = 0; t < 12; ++t)
#pragma unroll
        for (int px = 0; px < 4; ++px) acc[t][px] = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = y - (ky - 1);
        if (yy < 0 || yy >= a.H) continue;
        f32x4 g[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int xx = x0 - 1 + k;
            g[k] = (xx >= 0 && xx < a.W) ? ld4(at_ch(a.out, ((long)b * a.H + yy) * a.W + xx, 4 * d)) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int t = 0; t < 12; ++t) {
                const f32x4 w = ld4(a.weff + (((long)t * 9 + ky * 3 + kx) * a.D + d) * 4);
#pragma unroll
                for (int px = 0; px < 4; ++px) acc[t][px] += dot4(w, g[px - kx + 2]);
            }
    }
    const float r2 = a.rate2[0];
#pragma unroll
    for (int t = 0; t < 12; ++t) {
        const somi_slice &s = t < 4 ? a.dq : (t < 8 ? a.dk : a.dv);
        const int c = (t & 3) * a.D + d;
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            if (x0 + px >= a.W) continue;
            float *o = s.p + (((long)b * a.H + y) * a.W + x0 + px) * s.cs + s.coff + c;
            *o = a.accumulate ? *o + r2 * acc[t][px] : r2 * acc[t][px];
        }
    }
}

// weight-gradient partials: workgroup (chunk of 16 d, chunk of image rows), lane (t, d); part[chunk][(t * 9 + tap) * D + d][o], then C bias sums
__global__ __launch_bounds__(192) void ac_conv_bwd_weight_kernel(AcArgs a) {
    const int t = threadIdx.x >> 4, d = blockIdx.x * 16 + (threadIdx.x & 15);
    if (d >= a.D) return;
    const somi_slice &s = ac_src(a, t);
    const int c = (t & 3) * a.D + d;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[9], bs = zero;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = zero;
    const int rows = a.B * a.H, r0 = blockIdx.y * a.rows_per, r1 = min(rows, r0 + a.rows_per);
    for (int r = r0; r < r1; ++r) {
        const int b = r / a.H, y = r - b * a.H;
        for (int x = 0; x < a.W; ++x) {
            const f32x4 g = ld4(at_ch(a.out, (long)r * a.W + x, 4 * d));
            bs += g;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = y + ky - 1;
                if (yy < 0 || yy >= a.H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = x + kx - 1;
                    if (xx < 0 || xx >= a.W) continue;
                    acc[ky * 3 + kx] += g * s.p[(((long)b * a.H + yy) * a.W + xx) * s.cs + s.coff + c];
                }
            }
        }
    }
    float *part = a.part + (long)blockIdx.y * (AC_WG_ROWS + 4) * a.D;
#pragma unroll
    for (int k = 0; k < 9; ++k) st4(part + (((long)t * 9 + k) * a.D + d) * 4, acc[k]);
    if (t == 0) st4(part + (long)AC_WG_ROWS * a.D + 4 * d, bs);
}

// the partials in order, times rate2 -> dweff (108 C values) and dbias (C values)
__global__ __launch_bounds__(256) void ac_conv_bwd_weight_finish_kernel(AcArgs a) {
    const long n = (long)(AC_WG_ROWS + 4) * a.D, i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int p = 0; p < a.nP; ++p) s += a.part[p * n + i];
    s *= a.rate2[0];
    if (i < (long)AC_WG_ROWS * a.D) a.dweff[i] = s; else a.dbias[i - (long)AC_WG_ROWS * a.D] = s;
}

// weff[t][tap][d][o] = sum_j dep[4 d + o][j][tap] * fc[j][t]   (dep: (C, 9, 3, 3), fc: (9, 12))
__global__ __launch_bounds__(256) void ac_fold_weff_kernel(const float *fc, const float *dep, float *weff, int D) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)AC_WG_ROWS * D) return;
    const int o = (int)(i & 3), d = (int)((i >> 2) % D), tt = (int)((i >> 2) / D), tap = tt % 9, t = tt / 9;
    float s = 0.f;
    for (int j = 0; j < 9; ++j) s += dep[((long)(4 * d + o) * 9 + j) * 9 + tap] * fc[j * 12 + t];
    weff[i] = s;
}

// ddep[4 d + o][j][tap] = sum_t dweff[t][tap][d][o] * fc[j][t]
__global__ __launch_bounds__(256) void ac_split_dep_kernel(const float *dweff, const float *fc, float *ddep, int D) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)4 * D * 81) return;
    const int tap = (int)(i % 9), j = (int)((i / 9) % 9), ch = (int)(i / 81), d = ch >> 2, o = ch & 3;
    float s = 0.f;
    for (int t = 0; t < 12; ++t) s += dweff[(((long)t * 9 + tap) * D + d) * 4 + o] * fc[j * 12 + t];
    ddep[i] = s;
}

// dfc[j][t] = sum_(ch, tap) dep[ch][j][tap] * dweff[t][tap][ch]: one workgroup per (j, t), lanes stride the 9 * 4 D terms, then lane order
__global__ __launch_bounds__(256) void ac_split_fc_kernel(const float *dweff, const float *dep, float *dfc, int D) {
    __shared__ float red[256];
    const int j = blockIdx.x / 12, t = blockIdx.x % 12, n = 4 * D * 9;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int tap = i % 9, ch = i / 9;
        s += dep[((long)ch * 9 + j) * 9 + tap] * dweff[(((long)t * 9 + tap) * D + (ch >> 2)) * 4 + (ch & 3)];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = 0.f;
        for (int i = 0; i < 256; ++i) r += red[i];
        dfc[blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------------------------------------ host side
enum AcOp { AC_ATTN, AC_BWD_Q, AC_BWD_KV, AC_CONV, AC_CONV_BWD_DATA, AC_CONV_BWD_WEIGHT };

static bool ac_sizes_ok(int B, int H, int W, int C) {
    return B > 0 && H >= 4 && W >= 4 && C >= 16 && C % 16 == 0 && C <= 1024 && B <= 65535 && cdiv(H, AC_T) <= 65535 &&
           (long)B * H * W * 24 < (1L << 31);
}

static int ac_wgrad_chunks(int B, int H, int C) {
    const long rows = (long)B * H, cap = (long)(AC_WGRAD_CAP / ((size_t)(AC_WG_ROWS + 4) * (C / 4)));
    long n = rows < 256 ? rows : 256;
    if (n > cap) n = cap;
    return (int)(n < 1 ? 1 : n);
}

static int ac_dwp_blocks(int B, int H, int W) {
    const long npix = (long)B * H * W;
    return (int)(npix < 256 ? npix : 256);
}

static size_t ac_workspace_floats(int B, int H, int W, int C) {
    const size_t wg = (size_t)B * cdiv(H, AC_T) * cdiv(W, AC_T);
    const size_t bq = align_up(2 * wg, 4) + (size_t)ac_dwp_blocks(B, H, W) * C * 2;
    const size_t wgrad = (size_t)ac_wgrad_chunks(B, H, C) * (AC_WG_ROWS + 4) * (C / 4);
    return bq > wgrad ? bq : wgrad;
}

// checks the descriptor for `op` and fills the kernel arguments; nothing is launched on an error
static int ac_unpack(const somi_acmix_desc *d, AcOp op, AcArgs &a, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->B <= 65535 && cdiv(d->H, AC_T) <= 65535 &&
                 (long)d->B * d->H * d->W < (1L << 31), SOMI_EINVAL, "%s: bad sizes", who);
    const int C = d->C;
    SOMI_REQUIRE(C % 16 == 0, SOMI_ENOTIMPL, "%s: %d channels: 4 heads of a multiple of 4 channels are needed (C %% 16 == 0)", who, C);
    SOMI_REQUIRE(C <= 1024, SOMI_ENOTIMPL, "%s: %d channels: at most 1024", who, C);
    SOMI_REQUIRE(d->H >= 4 && d->W >= 4, SOMI_EINVAL, "%s: a %d x %d map: the reflection pad of 3 needs at least 4 x 4", who, d->H, d->W);
    const somi_slice *maps[] = {&d->q, &d->k, &d->v, &d->mix, &d->out, &d->dq, &d->dk, &d->dv};
    for (const somi_slice *m : maps)
        SOMI_REQUIRE(!m->p || (long)d->B * d->H * d->W * (m->cs > 0 ? m->cs : 1) <= (1L << 30), SOMI_ENOTIMPL,
                     "%s: a tensor of more than 2^30 floats", who);
    const bool attn = op == AC_ATTN || op == AC_BWD_Q || op == AC_BWD_KV;
    if (op != AC_CONV_BWD_DATA)
        SOMI_REQUIRE_SLICES(who, {"q", d->q.p, d->q.cs, d->q.coff, C}, {"k", d->k.p, d->k.cs, d->k.coff, C}, {"v", d->v.p, d->v.cs, d->v.coff, C});
    if (attn) SOMI_REQUIRE(d->wp && d->rate1 && d->rate2, SOMI_EINVAL, "%s: wp, rate1 and rate2 are required", who);
    if (op == AC_ATTN)
        SOMI_REQUIRE_SLICES(who, {"out", d->out.p, d->out.cs, d->out.coff, C}, {"mix", d->mix.p, d->mix.cs, d->mix.coff, C, kOptional},
                            {"lse", d->lse.p, d->lse.cs, d->lse.coff, 4, kOptional});
    if (op == AC_BWD_Q) {
        SOMI_REQUIRE_SLICES(who, {"dout", d->out.p, d->out.cs, d->out.coff, C}, {"mix", d->mix.p, d->mix.cs, d->mix.coff, C, kOptional},
                            {"lse", d->lse.p, d->lse.cs, d->lse.coff, 4}, {"aux", d->aux.p, d->aux.cs, d->aux.coff, AC_AUX},
                            {"dq", d->dq.p, d->dq.cs, d->dq.coff, C});
        SOMI_REQUIRE(d->dwp && d->drates, SOMI_EINVAL, "%s: dwp and drates are required", who);
    }
    if (op == AC_BWD_KV)
        SOMI_REQUIRE_SLICES(who, {"dout", d->out.p, d->out.cs, d->out.coff, C}, {"lse", d->lse.p, d->lse.cs, d->lse.coff, 4},
                            {"aux", d->aux.p, d->aux.cs, d->aux.coff, AC_AUX}, {"dk", d->dk.p, d->dk.cs, d->dk.coff, C},
                            {"dv", d->dv.p, d->dv.cs, d->dv.coff, C});
    if (op == AC_CONV) {
        SOMI_REQUIRE_SLICES(who, {"mix", d->mix.p, d->mix.cs, d->mix.coff, C});
        SOMI_REQUIRE(d->weff && d->bias, SOMI_EINVAL, "%s: weff and bias are required", who);
    }
    if (op == AC_CONV_BWD_DATA) {
        SOMI_REQUIRE_SLICES(who, {"dout", d->out.p, d->out.cs, d->out.coff, C}, {"dq", d->dq.p, d->dq.cs, d->dq.coff, C},
                            {"dk", d->dk.p, d->dk.cs, d->dk.coff, C}, {"dv", d->dv.p, d->dv.cs, d->dv.coff, C});
        SOMI_REQUIRE(d->weff && d->rate2, SOMI_EINVAL, "%s: weff and rate2 are required", who);
    }
    if (op == AC_CONV_BWD_WEIGHT) {
        SOMI_REQUIRE_SLICES(who, {"dout", d->out.p, d->out.cs, d->out.coff, C});
        SOMI_REQUIRE(d->dweff && d->dbias && d->rate2, SOMI_EINVAL, "%s: dweff, dbias and rate2 are required", who);
    }
    if (op == AC_BWD_Q || op == AC_CONV_BWD_WEIGHT) {
        SOMI_REQUIRE(d->workspace && aligned16(d->workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
        SOMI_REQUIRE(d->workspace_floats >= ac_workspace_floats(d->B, d->H, d->W, C), SOMI_EWORKSPACE, "%s: workspace too small", who);
    }
    a = AcArgs{};
    a.q = d->q; a.k = d->k; a.v = d->v; a.mix = d->mix; a.out = d->out; a.lse = d->lse;
    a.aux = d->aux; a.dq = d->dq; a.dk = d->dk; a.dv = d->dv;
    a.wp = d->wp; a.rate1 = d->rate1; a.rate2 = d->rate2; a.weff = d->weff; a.bias = d->bias;
    a.dwp = d->dwp; a.drates = d->drates; a.dweff = d->dweff; a.dbias = d->dbias; a.part = d->workspace;
    a.accumulate = d->accumulate;
    a.B = d->B; a.H = d->H; a.W = d->W; a.C = C; a.D = C / 4;
    a.nty = cdiv(d->H, AC_T); a.ntx = cdiv(d->W, AC_T);
    a.scale = 1.0f / sqrtf((float)a.D);
    return 0;
}

static dim3 ac_grid(const AcArgs &a) { return dim3(a.ntx, a.nty, a.B); }

}  // namespace somi

using namespace somi;

extern "C" size_t somi_acmix_desc_bytes(void) { return sizeof(somi_acmix_desc); }

extern "C" size_t somi_acmix_workspace_floats(int B, int H, int W, int C) { return ac_sizes_ok(B, H, W, C) ? ac_workspace_floats(B, H, W, C) : 0; }

extern "C" int somi_acmix_plan(int H, int W, int *tile, int *tiles_y, int *tiles_x) {
    if (H < 4 || W < 4 || !tile || !tiles_y || !tiles_x) return SOMI_EINVAL;
    *tile = AC_T;
    *tiles_y = cdiv(H, AC_T);
    *tiles_x = cdiv(W, AC_T);
    return 0;
}

extern "C" int somi_acmix_attn_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream) {
    AcArgs a;
    if (int rc = ac_unpack(d, AC_ATTN, a, "acmix attn")) return rc;
    hipLaunchKernelGGL(ac_attn_kernel, ac_grid(a), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_acmix_attn_nhwc_f32");
}

extern "C" int somi_acmix_attn_bwd_q_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream) {
    AcArgs a;
    if (int rc = ac_unpack(d, AC_BWD_Q, a, "acmix attn bwd q")) return rc;
    hipStream_t s = (hipStream_t)stream;
    a.nP = a.B * a.nty * a.ntx;
    const int nB = ac_dwp_blocks(a.B, a.H, a.W);
    float *wpart = d->workspace + align_up(2 * (size_t)a.nP, 4);
    hipLaunchKernelGGL(ac_bwd_q_kernel, ac_grid(a), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ac_rates_finish_kernel, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ac_dwp_partial_kernel, dim3(nB), dim3(256), 0, s, a, wpart, nB);
    hipLaunchKernelGGL(ac_dwp_finish_kernel, dim3(cdiv(2 * a.D, 256)), dim3(256), 0, s, a, (const float *)wpart, nB);
    return launch_status("somi_acmix_attn_bwd_q_nhwc_f32");
}

extern "C" int somi_acmix_attn_bwd_kv_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream) {
    AcArgs a;
    if (int rc = ac_unpack(d, AC_BWD_KV, a, "acmix attn bwd kv")) return rc;
    hipLaunchKernelGGL(ac_bwd_kv_kernel, ac_grid(a), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_acmix_attn_bwd_kv_nhwc_f32");
}

static int ac_lanes_grid(const AcArgs &a) { return cdiv((long)a.B * a.H * ((a.W + 3) / 4) * a.D, 256); }

extern "C" int somi_acmix_conv_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream) {
    AcArgs a;
    if (int rc = ac_unpack(d, AC_CONV, a, "acmix conv")) return rc;
    hipLaunchKernelGGL(ac_conv_kernel, dim3(ac_lanes_grid(a)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_acmix_conv_nhwc_f32");
}

extern "C" int somi_acmix_conv_bwd_data_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream) {
    AcArgs a;
    if (int rc = ac_unpack(d, AC_CONV_BWD_DATA, a, "acmix conv bwd data")) return rc;
    hipLaunchKernelGGL(ac_conv_bwd_data_kernel, dim3(ac_lanes_grid(a)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("somi_acmix_conv_bwd_data_nhwc_f32");
}

extern "C" int somi_acmix_conv_bwd_weight_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream) {
    AcArgs a;
    if (int rc = ac_unpack(d, AC_CONV_BWD_WEIGHT, a, "acmix conv bwd weight")) return rc;
    hipStream_t s = (hipStream_t)stream;
    a.nP = ac_wgrad_chunks(a.B, a.H, a.C);
    a.rows_per = cdiv((long)a.B * a.H, a.nP);
    hipLaunchKernelGGL(ac_conv_bwd_weight_kernel, dim3(cdiv(a.D, 16), a.nP), dim3(192), 0, s, a);
    hipLaunchKernelGGL(ac_conv_bwd_weight_finish_kernel, dim3(cdiv((long)(AC_WG_ROWS + 4) * a.D, 256)), dim3(256), 0, s, a);
    return launch_status("somi_acmix_conv_bwd_weight_nhwc_f32");
}

static int ac_param_check(const void *a, const void *b, const void *c, const void *e, int C, const char *who) {
    SOMI_REQUIRE(a && b && c && e, SOMI_EINVAL, "%s: every pointer is required", who);
    SOMI_REQUIRE(aligned16(a) && aligned16(b) && aligned16(c) && aligned16(e), SOMI_EINVAL, "%s: pointers must be 16-byte aligned", who);
    SOMI_REQUIRE(C > 0, SOMI_EINVAL, "%s: bad sizes", who);
    SOMI_REQUIRE(C % 16 == 0 && C <= 1024, SOMI_ENOTIMPL, "%s: %d channels: a multiple of 16, at most 1024", who, C);
    return 0;
}

extern "C" int somi_acmix_fold_weff_f32(const float *fc, const float *dep, float *weff, int C, somi_stream_t stream) {
    if (int rc = ac_param_check(fc, dep, weff, weff, C, "acmix fold weff")) return rc;
    hipLaunchKernelGGL(ac_fold_weff_kernel, dim3(cdiv((long)AC_WG_ROWS * (C / 4), 256)), dim3(256), 0, (hipStream_t)stream, fc, dep, weff, C / 4);
    return launch_status("somi_acmix_fold_weff_f32");
}

extern "C" int somi_acmix_split_dweff_f32(const float *dweff, const float *fc, const float *dep, float *dfc, float *ddep, int C,
                                          somi_stream_t stream) {
    if (int rc = ac_param_check(dweff, fc, dep, dfc, C, "acmix split dweff")) return rc;
    SOMI_REQUIRE(ddep && aligned16(ddep), SOMI_EINVAL, "acmix split dweff: ddep is required, 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ac_split_dep_kernel, dim3(cdiv((long)C * 81, 256)), dim3(256), 0, s, dweff, fc, ddep, C / 4);
    hipLaunchKernelGGL(ac_split_fc_kernel, dim3(108), dim3(256), 0, s, dweff, dep, dfc, C / 4);
    return launch_status("somi_acmix_split_dweff_f32");
}
