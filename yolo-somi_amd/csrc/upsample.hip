// The two learned 2x upsamplers of the neck: CARAFE (models/common.py:4450-4490) and DySample with style 'lp' (models/common.py:4246-4309).  NHWC fp32,
// channel slices (cs, coff) in and out, a lane owns one channel quad: 16-byte loads and stores, 16 lanes = 64 contiguous channels of one pixel.
//
// CARAFE   out[c, 2h+dy, 2w+dx] = sum_{a,b} softmax_t(logits[t*4 + dy*2 + dx, h, w])[a*k+b] * X[c, h+a-r, w+b-r], X zero outside the map.  The reference
//          unfolds the upsampled map into (B, C, k*k, 2H, 2W) and runs an einsum over it; here a workgroup takes an 8x8 tile of SOURCE pixels, turns their
//          4*k*k logits into the four softmaxes once (LDS), stages the (8+2r)^2 window of X per 64-channel chunk in LDS and writes the four output pixels
//          of every source pixel.  Nothing of size C*k*k per pixel exists.  Training keeps the softmax weights (B, 2H, 2W, k*k) - all backward needs.
//          Backward, two kernels: dlogits = p * (dp - sum p*dp) with dp[a*k+b] = sum_c dOut * X (the channel sum is a 16-lane butterfly per chunk, chunks
//          added in order by one owner lane), and dX owner-computes: every source pixel gathers the k*k source pixels around it x 4 sub-pixels in a fixed
//          order.  No float atomics.
// DySample sx = w + 0.25*o[j] + init_pos[j], sy = h + 0.25*o[4G+j] + init_pos[4G+j] with j = g*4 + dy*2 + dx, clamped to the map, bilinear sample of the
//          group's channels there (grid_sample, align_corners=False, padding_mode='border' after the reference's normalisation).  The 0.25, init_pos, the
//          clamp and the pixel-shuffle indexing happen here: no relayout pass.  Backward: dx owner-computes over the output pixels whose source pixel lies
//          within 2 pixels; a tap farther than that from its source pixel is added with an fp32 atomic and counted (0 <=> bit-reproducible), the policy of
//          the windowed DCNv3 backward.  doffset is a serial, fixed-order sum over the group's channels, 0 where the coordinate was clamped.
#include "common.h"

namespace somi {

constexpr int kUpTile = 8;      // source pixels per tile side
constexpr int kUpChunk = 64;    // channels per LDS chunk: 16 quads


// stages channels [c0, c0 + 64) of the (8+2R)^2 window around the tile into LDS as [wy][wx][64]; zero outside the map and beyond C
template <int R>
__device__ __forceinline__ void stage_window(float *s_win, const float *__restrict__ x, long b, int H, int W, int C, int x_cs, int x_coff, int h0, int w0,
                                             int c0) {
    constexpr int WW = kUpTile + 2 * R;
    const int nq = (C - c0 < kUpChunk ? C - c0 : kUpChunk) >> 2;
    for (int i = threadIdx.x; i < WW * WW * 16; i += 256) {
        const int q = i & 15, wp = i >> 4;
        const int hy = h0 - R + wp / WW, wx = w0 - R + wp % WW;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < nq && (unsigned)hy < (unsigned)H && (unsigned)wx < (unsigned)W)
            v = *reinterpret_cast<const f32x4 *>(x + ((b * H + hy) * W + wx) * x_cs + x_coff + c0 + q * 4);
        *reinterpret_cast<f32x4 *>(s_win + wp * kUpChunk + q * 4) = v;
    }
}

// ------------------------------------------------------------------------------------------------ CARAFE forward
template <int K>
__global__ __launch_bounds__(256) void carafe_fwd_kernel(const float *__restrict__ x, const float *__restrict__ logits, float *__restrict__ out,
                                                         float *__restrict__ wts, int H, int W, int C, int x_cs, int x_coff, int l_cs, int l_coff,
                                                         int o_cs, int o_coff, int tilesH, int tilesW) {
    constexpr int R = K / 2, KK = K * K, WW = kUpTile + 2 * R;
    __shared__ __attribute__((aligned(16))) float s_win[WW * WW * kUpChunk];
    __shared__ __attribute__((aligned(16))) float s_p[64 * KK * 4];          // [pixel][tap][sub-pixel]: the logits' own channel order
    const int tid = threadIdx.x;
    const int tw = blockIdx.x % tilesW, th = (blockIdx.x / tilesW) % tilesH;
    const long b = blockIdx.x / (tilesW * tilesH);
    const int h0 = th * kUpTile, w0 = tw * kUpTile;
    {   // one (source pixel, sub-pixel) softmax per thread, the maximum subtracted
        const int pix = tid >> 2, sub = tid & 3;
        const int h = h0 + (pix >> 3), w = w0 + (pix & 7);
        float v[KK];
        if (h < H && w < W) {
            const float *l = logits + ((b * H + h) * W + w) * l_cs + l_coff + sub;
            float m = -__builtin_huge_valf(), s = 0.f;
#pragma unroll
            for (int t = 0; t < KK; ++t) { v[t] = l[t * 4]; m = fmaxf(m, v[t]); }
#pragma unroll
            for (int t = 0; t < KK; ++t) { v[t] = expf(v[t] - m); s += v[t]; }
            const float inv = 1.0f / s;
#pragma unroll
            for (int t = 0; t < KK; ++t) v[t] *= inv;
            if (wts) {
                float *wp = wts + ((b * 2 * H + 2 * h + (sub >> 1)) * 2 * W + 2 * w + (sub & 1)) * KK;
#pragma unroll
                for (int t = 0; t < KK; ++t) wp[t] = v[t];
            }
        } else {
#pragma unroll
            for (int t = 0; t < KK; ++t) v[t] = 0.f;
        }
#pragma unroll
        for (int t = 0; t < KK; ++t) s_p[(pix * KK + t) * 4 + sub] = v[t];
    }
    const int q = tid & 15, slot = tid >> 4;
    for (int c0 = 0; c0 < C; c0 += kUpChunk) {
        __syncthreads();                                          // s_p is complete / the previous chunk's window is no longer read
        stage_window<R>(s_win, x, b, H, W, C, x_cs, x_coff, h0, w0, c0);
        __syncthreads();
        if (c0 + q * 4 >= C) continue;
        f32x4 acc[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[j][s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int a = 0; a < K; ++a)
            for (int bb = 0; bb < K; ++bb) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int pix = slot + 16 * j, py = pix >> 3, px = pix & 7;
                    const f32x4 xv = *reinterpret_cast<const f32x4 *>(s_win + ((py + a) * WW + px + bb) * kUpChunk + q * 4);
                    const f32x4 pv = *reinterpret_cast<const f32x4 *>(s_p + (pix * KK + a * K + bb) * 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[j][s] += pv[s] * xv;
                }
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pix = slot + 16 * j, h = h0 + (pix >> 3), w = w0 + (pix & 7);
            if (h >= H || w >= W) continue;
#pragma unroll
            for (int s = 0; s < 4; ++s)
                *reinterpret_cast<f32x4 *>(out + ((b * 2 * H + 2 * h + (s >> 1)) * 2 * W + 2 * w + (s & 1)) * o_cs + o_coff + c0 + q * 4) = acc[j][s];
        }
    }
}

// ------------------------------------------------------------------------------------------------ CARAFE backward: dlogits
template <int K>
__global__ __launch_bounds__(256) void carafe_bwd_logits_kernel(const float *__restrict__ dout, const float *__restrict__ x, const float *__restrict__ wts,
                                                                float *__restrict__ dlogits, int H, int W, int C, int d_cs, int d_coff, int x_cs,
                                                                int x_coff, int dl_cs, int dl_coff, int tilesH, int tilesW) {
    constexpr int R = K / 2, KK = K * K, WW = kUpTile + 2 * R;
    __shared__ __attribute__((aligned(16))) float s_win[WW * WW * kUpChunk];
    __shared__ __attribute__((aligned(16))) float s_dp[64 * KK * 4];         // [pixel][tap][sub-pixel]
    const int tid = threadIdx.x;
    const int tw = blockIdx.x % tilesW, th = (blockIdx.x / tilesW) % tilesH;
    const long b = blockIdx.x / (tilesW * tilesH);
    const int h0 = th * kUpTile, w0 = tw * kUpTile;
    for (int i = tid; i < 64 * KK * 4; i += 256) s_dp[i] = 0.f;
    const int q = tid & 15, slot = tid >> 4;
    for (int c0 = 0; c0 < C; c0 += kUpChunk) {
        __syncthreads();
        stage_window<R>(s_win, x, b, H, W, C, x_cs, x_coff, h0, w0, c0);   // quads beyond C are staged as zeros: every lane takes part in the butterfly
        __syncthreads();
        const bool live = c0 + q * 4 < C;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int pix = slot + 16 * j, py = pix >> 3, px = pix & 7;
            const int h = h0 + py, w = w0 + px;
            f32x4 d[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                d[s] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (live && h < H && w < W)
                    d[s] = *reinterpret_cast<const f32x4 *>(dout + ((b * 2 * H + 2 * h + (s >> 1)) * 2 * W + 2 * w + (s & 1)) * d_cs + d_coff + c0 + q * 4);
            }
            for (int a = 0; a < K; ++a)
                for (int bb = 0; bb < K; ++bb) {
                    const f32x4 xv = *reinterpret_cast<const f32x4 *>(s_win + ((py + a) * WW + px + bb) * kUpChunk + q * 4);
                    const int tap = a * K + bb;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float v = dot4(d[s], xv);
                        v += __shfl_xor(v, 1, 16);                // the 16 quads of the chunk: every lane ends with the same sum, in one order
                        v += __shfl_xor(v, 2, 16);
                        v += __shfl_xor(v, 4, 16);
                        v += __shfl_xor(v, 8, 16);
                        if (q == ((tap & 3) * 4 + s)) s_dp[(pix * KK + tap) * 4 + s] += v;     // one owner lane per entry, chunks in order
                    }
                }
        }
    }
    __syncthreads();
    const int pix = tid >> 2, sub = tid & 3;
    const int h = h0 + (pix >> 3), w = w0 + (pix & 7);
    if (h < H && w < W) {
        const float *wp = wts + ((b * 2 * H + 2 * h + (sub >> 1)) * 2 * W + 2 * w + (sub & 1)) * KK;
        float p[KK], s = 0.f;
#pragma unroll
        for (int t = 0; t < KK; ++t) { p[t] = wp[t]; s += p[t] * s_dp[(pix * KK + t) * 4 + sub]; }
        float *dl = dlogits + ((b * H + h) * W + w) * dl_cs + dl_coff + sub;
#pragma unroll
        for (int t = 0; t < KK; ++t) dl[t * 4] = p[t] * (s_dp[(pix * KK + t) * 4 + sub] - s);
    }
}

// ------------------------------------------------------------------------------------------------ CARAFE backward: dX, owner-computes
// dX[c, y, x] = sum_{a,b} sum_{sub} p[(y-a+r, x-b+r), sub][a*k+b] * dOut[c, 2(y-a+r)+dy, 2(x-b+r)+dx], taps row-major, sub-pixels inside a tap
template <int K>
__global__ __launch_bounds__(256) void carafe_bwd_dx_kernel(const float *__restrict__ dout, const float *__restrict__ wts, float *__restrict__ dx, int H,
                                                            int W, int C, int d_cs, int d_coff, int dx_cs, int dx_coff, int tilesH, int tilesW) {
    constexpr int R = K / 2, KK = K * K, WW = kUpTile + 2 * R;
    __shared__ __attribute__((aligned(16))) float s_p[WW * WW * KK * 4];     // [window pixel][tap][sub-pixel], 0 outside the map
    const int tid = threadIdx.x;
    const int tw = blockIdx.x % tilesW, th = (blockIdx.x / tilesW) % tilesH;
    const long b = blockIdx.x / (tilesW * tilesH);
    const int h0 = th * kUpTile, w0 = tw * kUpTile;
    for (int i = tid; i < WW * WW * 4 * KK; i += 256) {
        const int t = i % KK, rest = i / KK, sub = rest & 3, wp = rest >> 2;
        const int hy = h0 - R + wp / WW, wx = w0 - R + wp % WW;
        float v = 0.f;
        if ((unsigned)hy < (unsigned)H && (unsigned)wx < (unsigned)W)
            v = wts[((b * 2 * H + 2 * hy + (sub >> 1)) * 2 * W + 2 * wx + (sub & 1)) * KK + t];
        s_p[(wp * KK + t) * 4 + sub] = v;
    }
    __syncthreads();
    const int q = tid & 15, slot = tid >> 4;
    for (int c = q * 4; c < C; c += kUpChunk) {
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int pix = slot + 16 * j, py = pix >> 3, px = pix & 7;
            const int y = h0 + py, xx = w0 + px;
            if (y >= H || xx >= W) continue;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int a = 0; a < K; ++a) {
                const int h = y - a + R;
                if ((unsigned)h >= (unsigned)H) continue;
                for (int bb = 0; bb < K; ++bb) {
                    const int w = xx - bb + R;
                    if ((unsigned)w >= (unsigned)W) continue;
                    const f32x4 pv = *reinterpret_cast<const f32x4 *>(s_p + (((py - a + 2 * R) * WW + px - bb + 2 * R) * KK + a * K + bb) * 4);
                    const float *dp = dout + ((b * 2 * H + 2 * h) * 2 * W + 2 * w) * d_cs + d_coff + c;
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc += pv[s] * *reinterpret_cast<const f32x4 *>(dp + ((long)(s >> 1) * 2 * W + (s & 1)) * d_cs);
                }
            }
            *reinterpret_cast<f32x4 *>(dx + ((b * H + y) * W + xx) * dx_cs + dx_coff + c) = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ DySample
struct DyPos {
    int x0, x1, y0, y1;
    float fx, fy;
    bool ux, uy;          // the coordinate was not clamped: its gradient flows
};

// The same expression in the forward and both backward kernels (explicit fma, so no call site contracts it differently).  NaN clamps to 0.
__device__ __forceinline__ DyPos dy_position(float ox, float oy, float ipx, float ipy, int h, int w, int H, int W) {
    DyPos p;
    float sx = __fmaf_rn(0.25f, ox, ipx) + (float)w, sy = __fmaf_rn(0.25f, oy, ipy) + (float)h;
    p.ux = sx > 0.f && sx < (float)(W - 1);
    p.uy = sy > 0.f && sy < (float)(H - 1);
    sx = fminf(fmaxf(sx, 0.f), (float)(W - 1));
    sy = fminf(fmaxf(sy, 0.f), (float)(H - 1));
    const float flx = floorf(sx), fly = floorf(sy);
    p.x0 = (int)flx, p.y0 = (int)fly;
    p.fx = sx - flx, p.fy = sy - fly;
    p.x1 = p.x0 + 1 < W ? p.x0 + 1 : W - 1;
    p.y1 = p.y0 + 1 < H ? p.y0 + 1 : H - 1;
    return p;
}

static inline int up_grid(long items) {
    long g = (items + 255) / 256;
    const long cap = 256L * 8;   // 8 workgroups per CU, grid-stride beyond that
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// item = (image, source row, source column, channel quad): four output pixels of one quad
__global__ __launch_bounds__(256) void dysample_fwd_kernel(const float *__restrict__ x, const float *__restrict__ off, const float *__restrict__ init_pos,
                                                           float *__restrict__ out, int B, int H, int W, int C, int G, int x_cs, int x_coff, int f_cs,
                                                           int f_coff, int o_cs, int o_coff) {
    const int C4 = C >> 2, Cg = C / G;
    const unsigned items = (unsigned)B * H * W * C4;
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int c = (int)(it % (unsigned)C4) * 4;
        const unsigned pixi = it / (unsigned)C4, rowi = pixi / (unsigned)W;
        const int w = (int)(pixi - rowi * W), h = (int)(rowi % (unsigned)H);
        const long b = rowi / (unsigned)H;
        const int g = c / Cg;
        const float *o = off + (long)pixi * f_cs + f_coff;
        const float *xb = x + b * H * W * x_cs + x_coff + c;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = g * 4 + s;
            const DyPos p = dy_position(o[j], o[4 * G + j], init_pos[j], init_pos[4 * G + j], h, w, H, W);
            const f32x4 v00 = *reinterpret_cast<const f32x4 *>(xb + ((long)p.y0 * W + p.x0) * x_cs);
            const f32x4 v01 = *reinterpret_cast<const f32x4 *>(xb + ((long)p.y0 * W + p.x1) * x_cs);
            const f32x4 v10 = *reinterpret_cast<const f32x4 *>(xb + ((long)p.y1 * W + p.x0) * x_cs);
            const f32x4 v11 = *reinterpret_cast<const f32x4 *>(xb + ((long)p.y1 * W + p.x1) * x_cs);
            const f32x4 v = (v00 * (1.f - p.fx) + v01 * p.fx) * (1.f - p.fy) + (v10 * (1.f - p.fx) + v11 * p.fx) * p.fy;
            *reinterpret_cast<f32x4 *>(out + ((b * 2 * H + 2 * h + (s >> 1)) * 2 * W + 2 * w + (s & 1)) * o_cs + o_coff + c) = v;
        }
    }
}

// dx, owner-computes: item = (image, row, column, channel quad) of x; it walks the 5x5 source pixels around it x 4 sub-pixels row-major and adds the
// taps that land on it (a tap = one corner of a bilinear sample, corners in the order 00, 01, 10, 11).  Every element is written.
__global__ __launch_bounds__(256) void dysample_bwd_dx_kernel(const float *__restrict__ dout, const float *__restrict__ off,
                                                              const float *__restrict__ init_pos, float *__restrict__ dx, int B, int H, int W, int C, int G,
                                                              int d_cs, int d_coff, int f_cs, int f_coff, int dx_cs, int dx_coff) {
    const int C4 = C >> 2, Cg = C / G;
    const unsigned items = (unsigned)B * H * W * C4;
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int c = (int)(it % (unsigned)C4) * 4;
        const unsigned pixi = it / (unsigned)C4, rowi = pixi / (unsigned)W;
        const int xx = (int)(pixi - rowi * W), y = (int)(rowi % (unsigned)H);
        const long b = rowi / (unsigned)H;
        const int g = c / Cg;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int dh = -2; dh <= 2; ++dh) {
            const int h = y + dh;
            if ((unsigned)h >= (unsigned)H) continue;
            for (int dw = -2; dw <= 2; ++dw) {
                const int w = xx + dw;
                if ((unsigned)w >= (unsigned)W) continue;
                const float *o = off + ((b * H + h) * W + w) * f_cs + f_coff;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int j = g * 4 + s;
                    const DyPos p = dy_position(o[j], o[4 * G + j], init_pos[j], init_pos[4 * G + j], h, w, H, W);
                    const bool r0 = p.y0 == y, r1 = p.y1 == y, q0 = p.x0 == xx, q1 = p.x1 == xx;
                    if (!((r0 || r1) && (q0 || q1))) continue;
                    const f32x4 d = *reinterpret_cast<const f32x4 *>(dout + ((b * 2 * H + 2 * h + (s >> 1)) * 2 * W + 2 * w + (s & 1)) * d_cs + d_coff + c);
                    if (r0 && q0) acc += ((1.f - p.fy) * (1.f - p.fx)) * d;
                    if (r0 && q1) acc += ((1.f - p.fy) * p.fx) * d;
                    if (r1 && q0) acc += (p.fy * (1.f - p.fx)) * d;
                    if (r1 && q1) acc += (p.fy * p.fx) * d;
                }
            }
        }
        *reinterpret_cast<f32x4 *>(dx + (long)pixi * dx_cs + dx_coff + c) = acc;
    }
}

// doffset: item = (image, source row, source column, group, sub-pixel); a serial sum over the group's channels.  A corner farther than 2 pixels from
// the source pixel is outside every owner's walk above: it is added here with fp32 atomics (after the dx kernel, same stream) and counted.
__global__ __launch_bounds__(256) void dysample_bwd_off_kernel(const float *__restrict__ dout, const float *__restrict__ x, const float *__restrict__ off,
                                                               const float *__restrict__ init_pos, float *dx, float *__restrict__ doff,
                                                               unsigned *far_count, int B, int H, int W, int C, int G, int d_cs, int d_coff, int x_cs,
                                                               int x_coff, int f_cs, int f_coff, int dx_cs, int dx_coff, int df_cs, int df_coff) {
    const int Cg = C / G, G4 = G * 4;
    const unsigned items = (unsigned)B * H * W * G4;
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int j = (int)(it % (unsigned)G4), g = j >> 2, s = j & 3;
        const unsigned pixi = it / (unsigned)G4, rowi = pixi / (unsigned)W;
        const int w = (int)(pixi - rowi * W), h = (int)(rowi % (unsigned)H);
        const long b = rowi / (unsigned)H;
        const float *o = off + (long)pixi * f_cs + f_coff;
        const DyPos p = dy_position(o[j], o[G4 + j], init_pos[j], init_pos[G4 + j], h, w, H, W);
        const long img = b * H * W;
        const long t00 = img + (long)p.y0 * W + p.x0, t01 = img + (long)p.y0 * W + p.x1, t10 = img + (long)p.y1 * W + p.x0, t11 = img + (long)p.y1 * W + p.x1;
        const float *dp = dout + ((b * 2 * H + 2 * h + (s >> 1)) * 2 * W + 2 * w + (s & 1)) * d_cs + d_coff + g * Cg;
        const float *xg = x + x_coff + g * Cg;
        const bool fy0 = p.y0 - h > 2 || h - p.y0 > 2, fy1 = p.y1 - h > 2 || h - p.y1 > 2;
        const bool fx0 = p.x0 - w > 2 || w - p.x0 > 2, fx1 = p.x1 - w > 2 || w - p.x1 > 2;
        const bool isfar[4] = {fy0 || fx0, fy0 || fx1, fy1 || fx0, fy1 || fx1};
        const long tp[4] = {t00, t01, t10, t11};
        const float wt[4] = {(1.f - p.fy) * (1.f - p.fx), (1.f - p.fy) * p.fx, p.fy * (1.f - p.fx), p.fy * p.fx};
        const bool any_far = isfar[0] || isfar[1] || isfar[2] || isfar[3];
        float gx = 0.f, gy = 0.f;
        for (int c = 0; c < Cg; c += 4) {
            const f32x4 d = *reinterpret_cast<const f32x4 *>(dp + c);
            const f32x4 v00 = *reinterpret_cast<const f32x4 *>(xg + t00 * x_cs + c), v01 = *reinterpret_cast<const f32x4 *>(xg + t01 * x_cs + c);
            const f32x4 v10 = *reinterpret_cast<const f32x4 *>(xg + t10 * x_cs + c), v11 = *reinterpret_cast<const f32x4 *>(xg + t11 * x_cs + c);
            gx += dot4(d, (v01 - v00) * (1.f - p.fy) + (v11 - v10) * p.fy);
            gy += dot4(d, (v10 - v00) * (1.f - p.fx) + (v11 - v01) * p.fx);
            if (any_far) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (isfar[k]) {
                        float *t = dx + tp[k] * dx_cs + dx_coff + g * Cg + c;
#pragma unroll
                        for (int e = 0; e < 4; ++e) atomicAdd(t + e, wt[k] * d[e]);
                    }
            }
        }
        float *df = doff + (long)pixi * df_cs + df_coff;
        df[j] = p.ux ? 0.25f * gx : 0.f;
        df[G4 + j] = p.uy ? 0.25f * gy : 0.f;
        if (any_far) atomicAdd(far_count, (unsigned)isfar[0] + (unsigned)isfar[1] + (unsigned)isfar[2] + (unsigned)isfar[3]);
    }
}

}  // namespace somi

using namespace somi;

extern "C" int somi_carafe_nhwc_f32(const float *x, const float *logits, float *out, float *weights, int B, int H, int W, int C, int k_up, int x_cs,
                                    int x_coff, int l_cs, int l_coff, int o_cs, int o_coff, somi_stream_t stream) {
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && C % 4 == 0 && (k_up == 3 || k_up == 5) && (!weights || aligned16(weights)), SOMI_EINVAL,
                 "carafe: bad shape, C not a multiple of 4, k_up not 3 or 5, or weights not 16-byte aligned");
    SOMI_REQUIRE_SLICES("carafe", {"x", x, x_cs, x_coff, C}, {"logits", logits, l_cs, l_coff, 4 * k_up * k_up}, {"out", out, o_cs, o_coff, C});
    const int tH = cdiv(H, kUpTile), tW = cdiv(W, kUpTile);
    SOMI_REQUIRE((long)B * tH * tW < (1L << 31), SOMI_EINVAL, "carafe: too many tiles for one launch");
    const dim3 grid((unsigned)((long)B * tH * tW));
    if (k_up == 5)
        hipLaunchKernelGGL(carafe_fwd_kernel<5>, grid, dim3(256), 0, (hipStream_t)stream, x, logits, out, weights, H, W, C, x_cs, x_coff, l_cs, l_coff, o_cs,
                           o_coff, tH, tW);
    else
        hipLaunchKernelGGL(carafe_fwd_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, x, logits, out, weights, H, W, C, x_cs, x_coff, l_cs, l_coff, o_cs,
                           o_coff, tH, tW);
    return launch_status("somi_carafe_nhwc_f32");
}

extern "C" int somi_carafe_bwd_nhwc_f32(const float *dout, const float *x, const float *weights, float *dx, float *dlogits, int B, int H, int W, int C,
                                        int k_up, int d_cs, int d_coff, int x_cs, int x_coff, int dx_cs, int dx_coff, int dl_cs, int dl_coff,
                                        somi_stream_t stream) {
    SOMI_REQUIRE(B > 0 && H > 0 && W > 0 && C % 4 == 0 && (k_up == 3 || k_up == 5) && weights && aligned16(weights), SOMI_EINVAL,
                 "carafe bwd: bad shape, C not a multiple of 4, k_up not 3 or 5, or no 16-byte aligned weights");
    SOMI_REQUIRE_SLICES("carafe bwd", {"dout", dout, d_cs, d_coff, C}, {"x", x, x_cs, x_coff, C}, {"dx", dx, dx_cs, dx_coff, C},
                        {"dlogits", dlogits, dl_cs, dl_coff, 4 * k_up * k_up});
    const int tH = cdiv(H, kUpTile), tW = cdiv(W, kUpTile);
    SOMI_REQUIRE((long)B * tH * tW < (1L << 31), SOMI_EINVAL, "carafe bwd: too many tiles for one launch");
    const dim3 grid((unsigned)((long)B * tH * tW));
    hipStream_t s = (hipStream_t)stream;
    if (k_up == 5) {
        hipLaunchKernelGGL(carafe_bwd_dx_kernel<5>, grid, dim3(256), 0, s, dout, weights, dx, H, W, C, d_cs, d_coff, dx_cs, dx_coff, tH, tW);
        hipLaunchKernelGGL(carafe_bwd_logits_kernel<5>, grid, dim3(256), 0, s, dout, x, weights, dlogits, H, W, C, d_cs, d_coff, x_cs, x_coff, dl_cs, dl_coff,
                           tH, tW);
    } else {
        hipLaunchKernelGGL(carafe_bwd_dx_kernel<3>, grid, dim3(256), 0, s, dout, weights, dx, H, W, C, d_cs, d_coff, dx_cs, dx_coff, tH, tW);
        hipLaunchKernelGGL(carafe_bwd_logits_kernel<3>, grid, dim3(256), 0, s, dout, x, weights, dlogits, H, W, C, d_cs, d_coff, x_cs, x_coff, dl_cs, dl_coff,
                           tH, tW);
    }
    return launch_status("somi_carafe_bwd_nhwc_f32");
}

static bool dysample_shape_ok(int B, int H, int W, int C, int G) {
    return B > 0 && H > 0 && W > 0 && G > 0 && C > 0 && C % G == 0 && (C / G) % 4 == 0 && (long)B * H * W * (C / 4 > 4 * G ? C / 4 : 4 * G) + 256L * 8 * 256 < (1L << 32);
}

extern "C" int somi_dysample_nhwc_f32(const float *x, const float *offset, const float *init_pos, float *out, int B, int H, int W, int C, int groups,
                                      int x_cs, int x_coff, int f_cs, int f_coff, int o_cs, int o_coff, somi_stream_t stream) {
    SOMI_REQUIRE(dysample_shape_ok(B, H, W, C, groups), SOMI_EINVAL,
                 "dysample: needs C %% groups == 0, (C / groups) %% 4 == 0 and fewer than 2^32 (pixel, channel quad) items");
    SOMI_REQUIRE_SLICES("dysample", {"x", x, x_cs, x_coff, C}, {"offset", offset, f_cs, f_coff, 8 * groups}, {"out", out, o_cs, o_coff, C});
    SOMI_REQUIRE(init_pos, SOMI_EINVAL, "dysample: init_pos is NULL");
    hipLaunchKernelGGL(dysample_fwd_kernel, dim3(up_grid((long)B * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, offset, init_pos, out, B, H, W, C,
                       groups, x_cs, x_coff, f_cs, f_coff, o_cs, o_coff);
    return launch_status("somi_dysample_nhwc_f32");
}

extern "C" int somi_dysample_bwd_nhwc_f32(const float *dout, const float *x, const float *offset, const float *init_pos, float *dx, float *doffset,
                                          void *far_count, int B, int H, int W, int C, int groups, int d_cs, int d_coff, int x_cs, int x_coff, int f_cs,
                                          int f_coff, int dx_cs, int dx_coff, int df_cs, int df_coff, somi_stream_t stream) {
    SOMI_REQUIRE(dysample_shape_ok(B, H, W, C, groups), SOMI_EINVAL,
                 "dysample bwd: needs C %% groups == 0, (C / groups) %% 4 == 0 and fewer than 2^32 (pixel, channel quad) items");
    SOMI_REQUIRE_SLICES("dysample bwd", {"dout", dout, d_cs, d_coff, C}, {"x", x, x_cs, x_coff, C}, {"offset", offset, f_cs, f_coff, 8 * groups},
                        {"dx", dx, dx_cs, dx_coff, C}, {"doffset", doffset, df_cs, df_coff, 8 * groups});
    SOMI_REQUIRE(init_pos && far_count, SOMI_EINVAL, "dysample bwd: init_pos or far_count is NULL");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dysample_bwd_dx_kernel, dim3(up_grid((long)B * H * W * (C / 4))), dim3(256), 0, s, dout, offset, init_pos, dx, B, H, W, C, groups, d_cs,
                       d_coff, f_cs, f_coff, dx_cs, dx_coff);
    hipLaunchKernelGGL(dysample_bwd_off_kernel, dim3(up_grid((long)B * H * W * 4 * groups)), dim3(256), 0, s, dout, x, offset, init_pos, dx, doffset,
                       (unsigned *)far_count, B, H, W, C, groups, d_cs, d_coff, x_cs, x_coff, f_cs, f_coff, dx_cs, dx_coff, df_cs, df_coff);
    return launch_status("somi_dysample_bwd_nhwc_f32");
}
