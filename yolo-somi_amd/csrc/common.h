// Shared helpers for the libsomi_hip.so kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>
#include "../../include/somi_hip.h"

namespace somi {

void set_error(const char *fmt, ...);

#define SOMI_REQUIRE(cond, code, ...)            \
    do {                                         \
        if (!(cond)) {                           \
            ::somi::set_error(__VA_ARGS__);      \
            return (code);                       \
        }                                        \
    } while (0)

static inline int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline int r4(int c) { return (c + 3) / 4 * 4; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// THE channel-slice rule (include/somi_hip.h, Conventions): nullptr if the channels [coff, coff + width) of a cs-channel NHWC tensor at p can be
// walked by the float4 paths (p + pix * cs + coff), else why not.  width = what the entry point's kernels really touch.
static inline const char *slice_fault(const void *p, int cs, int coff, int width) {
    if (!p) return "null pointer";
    if (!aligned16(p)) return "base not 16-byte aligned";
    if (cs <= 0 || cs % 4) return "channel stride not a positive multiple of 4";
    if (coff < 0 || coff % 4) return "channel offset not a non-negative multiple of 4";
    if (width <= 0) return "no channels";
    if ((long)coff + width > cs) return "runs past the channel stride";
    return nullptr;
}

// One slice argument of an entry point; name = its pointer parameter as the header spells it.  An optional slice is checked when its pointer is given.
struct Slice { const char *name; const void *p; int cs, coff, width; bool optional; };
constexpr bool kOptional = true;
static inline int slices_status(const char *who, std::initializer_list<Slice> slices) {
    for (const Slice &s : slices)
        if (const char *why = s.optional && !s.p ? nullptr : slice_fault(s.p, s.cs, s.coff, s.width)) {
            set_error("%s: %s = [%d, %ld) of %d channels: %s", who, s.name, s.coff, (long)s.coff + s.width, s.cs, why);
            return SOMI_EINVAL;
        }
    return 0;
}
// SOMI_REQUIRE_SLICES("add", {"a", a, a_cs, a_coff, C}, {"out", out, o_cs, o_coff, C}, {"residual", res, res_cs, res_coff, C, kOptional});
#define SOMI_REQUIRE_SLICES(who, ...)                                          \
    do {                                                                       \
        if (::somi::slices_status(who, {__VA_ARGS__})) return SOMI_EINVAL;     \
    } while (0)

constexpr int kNumXCD = 8;

// depthwise 3x3 stencil (layers.hip); flip = taps walked backwards (the data gradient)
void launch_dwconv3x3(bool flip, const float *x, const float *w, const float *bias, const float *ps, const float *pt, const float *res,
                      float *y, int B, int H, int W, int C, int act, hipStream_t s);

// Bijective XCD-aware remap of a 1-D block id: blocks with equal (id % 8) share an XCD (observed round-robin
// dispatch), so give each XCD one contiguous chunk of logical tile ids.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk / kNumXCD, r = nblk % kNumXCD;
    const int xcd = bid % kNumXCD, idx = bid / kNumXCD;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + idx;
}

// ------------------------------------------------------------------------------------------------ vector types and the float4 vocabulary
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// 16-byte load / store at a 16-byte aligned float address
__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }
__device__ __forceinline__ f32x4 splat4(float v) { return f32x4{v, v, v, v}; }
// channel quad q of pixel pix of a slice (the slice rule above), to read and to write
__device__ __forceinline__ const float *at(const somi_slice &s, long pix, int q) { return s.p + pix * s.cs + s.coff + 4 * q; }
__device__ __forceinline__ float *at_w(const somi_slice &s, long pix, int q) { return s.p + pix * s.cs + s.coff + 4 * q; }
// the same by channel c (a multiple of 4), for the kernels that count channels, not quads
__device__ __forceinline__ const float *at_ch(const somi_slice &s, long pix, int c) { return s.p + pix * s.cs + s.coff + c; }
__device__ __forceinline__ float *at_ch_w(const somi_slice &s, long pix, int c) { return s.p + pix * s.cs + s.coff + c; }
// four-lane dot product, added left to right
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// the xor butterfly over the 64 lanes of a wave: every lane ends with the sum
__device__ __forceinline__ float wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// sum of a float4 over the lanes of a THREADS-wide workgroup that share a quad: lanes (wave, ql + j * nq) -> lanes ql < nq of thread 0's wave
// `red` holds THREADS / 64 waves x 64 float4; returns the total in threads t < nq (others: garbage)
template <int THREADS>
__device__ __forceinline__ f32x4 block_quad_sum(f32x4 v, int nq, f32x4 *red) {
    for (int off = nq; off < 64; off <<= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < nq) red[wave * 64 + lane] = v;
    __syncthreads();
    f32x4 s = v;
    if (threadIdx.x < nq) {
        s = red[threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < THREADS / 64; ++wv) s += red[wv * 64 + threadIdx.x];
    }
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------------------------------------ the map-pass geometry
// A workgroup of 256 lanes = NL columns x QW channel quads takes RH rows x NL columns of one image; lane (l, q) owns column w0 + l and channel
// quad q and walks the rows ru at a time.  Grid: (nWc, nHc, B * nQc).  RH shrinks from 32 until about a thousand workgroups exist (small maps).
struct MapShape {
    int QW, NL;                   // quads and columns of a workgroup: QW * NL <= 256
    int nQc;                      // quad chunks (C / 4 > 256 only)
};
static inline MapShape map_shape(int C) {
    MapShape s;
    const int C4 = C / 4;
    s.QW = C4 < 256 ? C4 : 256;
    s.NL = 256 / s.QW;
    s.nQc = cdiv(C4, 256);
    return s;
}

struct MapPlan {
    int QW, NL, nQc;              // map_shape(C)
    int nWc, nHc, RH;             // column chunks, row chunks, rows per chunk
};
static inline MapPlan map_plan(int B, int H, int W, int C, int ru) {
    const MapShape s = map_shape(C);
    MapPlan p;
    p.QW = s.QW; p.NL = s.NL; p.nQc = s.nQc;
    p.nWc = cdiv(W, p.NL);
    p.RH = 32;
    while (p.RH > ru && (long)B * p.nQc * p.nWc * cdiv(H, p.RH) < 1024) p.RH /= 2;
    p.nHc = cdiv(H, p.RH);
    return p;
}

struct MapLane { int b, q, w, h0, h1, lane; bool on; };

// Args: any kernel argument struct with the plan's QW, NL, nQc, RH and the map's H, W, C4
template <class Args>
__device__ __forceinline__ MapLane map_lane(const Args &a) {
    MapLane l;
    const int t = threadIdx.x;
    l.lane = t / a.QW;
    l.b = blockIdx.z / a.nQc;
    l.q = (blockIdx.z - l.b * a.nQc) * 256 + (t - l.lane * a.QW);
    l.w = blockIdx.x * a.NL + l.lane;
    l.h0 = blockIdx.y * a.RH;
    l.h1 = min(a.H, l.h0 + a.RH);
    l.on = l.lane < a.NL && l.q < a.C4 && l.w < a.W;
    return l;
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// BiFPN fusion weights w_i / (sum_j swish(w_j) + eps) (models/common.py:3696, Swish :8210) from the raw parameter on the device
__device__ __forceinline__ void bifpn_norm(const float *__restrict__ w, int n_in, float eps, float (&wn)[3]) {
    float s = 0.f;
    for (int i = 0; i < n_in; ++i) s += w[i] * (1.0f / (1.0f + expf(-w[i])));
    for (int i = 0; i < 3; ++i) wn[i] = i < n_in ? w[i] / (s + eps) : 0.f;
}

template <int ACT>
__device__ __forceinline__ float apply_act(float v) {
    if constexpr (ACT == SOMI_ACT_SILU) return v / (1.0f + expf(-v));
    else if constexpr (ACT == SOMI_ACT_GELU) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    else if constexpr (ACT == SOMI_ACT_RELU) return fmaxf(v, 0.0f);
    else if constexpr (ACT == SOMI_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    else if constexpr (ACT == SOMI_ACT_LEAKY) return v > 0.0f ? v : 0.1f * v;
    else if constexpr (ACT == SOMI_ACT_HSWISH) return v * fminf(fmaxf(v + 3.0f, 0.0f), 6.0f) * (1.0f / 6.0f);
    else return v;
}

__device__ __forceinline__ float gelu_grad(float v) {               // d/dv [0.5 v (1 + erf(v/sqrt2))]
    return 0.5f * (1.f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

__device__ __forceinline__ float apply_act_rt(float v, int act) {
    switch (act) {
        case SOMI_ACT_SILU: return apply_act<SOMI_ACT_SILU>(v);
        case SOMI_ACT_GELU: return apply_act<SOMI_ACT_GELU>(v);
        case SOMI_ACT_RELU: return apply_act<SOMI_ACT_RELU>(v);
        case SOMI_ACT_SIGMOID: return apply_act<SOMI_ACT_SIGMOID>(v);
        case SOMI_ACT_LEAKY: return apply_act<SOMI_ACT_LEAKY>(v);
        case SOMI_ACT_HSWISH: return apply_act<SOMI_ACT_HSWISH>(v);
        default: return v;
    }
}

}  // namespace somi
