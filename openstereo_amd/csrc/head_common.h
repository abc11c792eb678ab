// What the fused upsample + soft-argmin heads (softargmin.hip) and their backward kernels (backward.hip) share, each defined once: the
// source-index rule of the linear interpolation, the interpolation arguments and their host-side fill, the choice of the x4 streaming
// kernel, and the device steps every one-thread-per-pixel kernel opens with -- the pixel, its bilinear footprint in the low-res plane, the
// [Dl][NT] LDS column of its samples and one trilinear sample out of that column.
// The library is built with -ffp-contract=off: forward and backward kernels get bit-identical samples because they run these expressions.
#pragma once
#include "osa_common.h"

namespace osa {

// PyTorch's area_pixel_compute_source_index (linear modes)
__device__ __forceinline__ void src_index(int dst, float scale, int align, int in_size, int& i0, int& i1, float& l1) {
    float s;
    if (align) s = scale * (float)dst;
    else { s = scale * ((float)dst + 0.5f) - 0.5f; s = s < 0.f ? 0.f : s; }
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
    l1 = s - (float)i0;
}

static inline float lin_scale(int in, int out, int align) {
    // at::native::area_pixel_compute_scale
    if (align) return (out > 1) ? (float)(in - 1) / (float)(out - 1) : 0.f;
    return (float)in / (float)out;
}

// the interpolation part of the kernel arguments, forward and backward
struct UpDims {
    int B, Dl, Hl, Wl, D, H, W;
    int align;
    float sd, sh, sw;    // input/output scale per dim
};

static inline UpDims up_dims(int B, int Dl, int Hl, int Wl, int D, int H, int W, int align_corners) {
    UpDims g;
    g.B = B; g.Dl = Dl; g.Hl = Hl; g.Wl = Wl; g.D = D; g.H = H; g.W = W;
    g.align = align_corners ? 1 : 0;
    g.sd = lin_scale(Dl, D, g.align); g.sh = lin_scale(Hl, H, g.align); g.sw = lin_scale(Wl, W, g.align);
    return g;
}

// exact x4 in all three dimensions, align_corners = False, and a low-res plane whose offsets fit an int: the streaming kernel's case
static inline bool up_is_x4(const UpDims& g) {
    return !g.align && g.D == 4 * g.Dl && g.H == 4 * g.Hl && g.W == 4 * g.Wl && (long long)g.Hl * g.Wl < (1ll << 30);
}

// The output pixel of a thread where one thread owns one pixel and a workgroup NT consecutive ones.  Threads past the end stay for the
// kernel's LDS traffic on pixel 0 and store nothing (`live`).
struct UpPixel {
    long long i;
    bool live;
    int b, hw, y, x;
};
template <int NT>
__device__ __forceinline__ UpPixel up_pixel(const UpDims& g) {
    UpPixel q;
    const long long HW = (long long)g.H * g.W;
    q.i = (long long)blockIdx.x * NT + threadIdx.x;
    q.live = q.i < (long long)g.B * HW;
    const long long ii = q.live ? q.i : 0;
    q.b = (int)(ii / HW);
    q.hw = (int)(ii - (long long)q.b * HW);
    q.y = q.hw / g.W; q.x = q.hw - q.y * g.W;
    return q;
}

// The bilinear footprint of output pixel (y, x) in a low-res plane: four corner offsets (Off = int where the plane is known to fit) and
// their weights; f(cp) is the pixel's interpolated value of the plane at cp.
template <class Off>
struct Bilinear {
    Off o00, o01, o10, o11;
    float w00, w01, w10, w11;
    __device__ __forceinline__ Bilinear(int y, int x, float sh, float sw, int align, int Hl, int Wl) {
        int y0, y1, x0, x1; float ly, lx;
        src_index(y, sh, align, Hl, y0, y1, ly);
        src_index(x, sw, align, Wl, x0, x1, lx);
        w00 = (1.f - ly) * (1.f - lx); w01 = (1.f - ly) * lx; w10 = ly * (1.f - lx); w11 = ly * lx;
        o00 = (Off)y0 * Wl + x0; o01 = (Off)y0 * Wl + x1; o10 = (Off)y1 * Wl + x0; o11 = (Off)y1 * Wl + x1;
    }
    __device__ __forceinline__ float operator()(const float* cp) const {
        return w00 * cp[o00] + w01 * cp[o01] + w10 * cp[o10] + w11 * cp[o11];
    }
};

// The thread's Dl interpolated low-res costs into its column of cl[Dl][NT] in LDS (layout [dl][thread]: conflict free).  c: the batch
// item's low-res cost.
template <int NT>
__device__ __forceinline__ void stage_column(const Bilinear<size_t>& f, const float* c, size_t plane, int Dl, float* cl) {
    const int tid = threadIdx.x;
#pragma unroll 4
    for (int dl = 0; dl < Dl; ++dl) cl[dl * NT + tid] = f(c + (size_t)dl * plane);
}

// upsampled sample d of the thread's column: the linear interpolation of two of its entries
template <int NT>
__device__ __forceinline__ float up_sample(const float* cl, int d, const UpDims& g) {
    const int tid = threadIdx.x;
    int d0, d1; float ld;
    src_index(d, g.sd, g.align, g.Dl, d0, d1, ld);
    return (1.f - ld) * cl[d0 * NT + tid] + ld * cl[d1 * NT + tid];
}

}  // namespace osa
