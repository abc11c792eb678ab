// Backward kernels of the memory-bound hot-path ops, reference NCDHW layouts.
// The reference gets these from autograd through its slice-assignment loops; here they are explicit:
//
//  volume (gwc part)   dL[b,c,h,w]  = (1/K) sum_{d<=min(w,D-1)} dV[b,g,d,h,w]   * R[b,c,h,w-d]
//                      dR[b,c,h,w'] = (1/K) sum_{d<D, w'+d<W}   dV[b,g,d,h,w'+d] * L[b,c,h,w'+d]
//  volume (concat)     dL[b,c,h,w]  = sum_{d<=w (all d if left unmasked)} dV[b,c,d,h,w]
//                      dR[b,c,h,w'] = sum_{d, w'+d<W} dV[b,C+c,d,h,w'+d]
//  soft-argmin         dprob[b,d,h,w] = d * dout[b,h,w]
//  softmax+soft-argmin dcost[b,d,h,w] = p_d * (d - disp) * dout          (p = softmax(cost))
//  upsample+softmax+soft-argmin: the same g_d at full resolution, pushed back through the transposed
//                      trilinear interpolation (8 corner weights) with float atomics into the low-res cost.
// All are streaming kernels with lanes along w.
//
// The heads that also return the per-pixel variance (softargmin.hip) have two incoming gradients per pixel.  The logits form and the fold
// pass of the fused form are ONE body each, `template <bool VAR>`, with the variance's share inside `if constexpr (VAR)`; the `__global__`
// kernels are the named wrappers of the two instantiations.  The fused kernels open with the steps of head_common.h, which the forward
// kernels run too: the recomputed samples are the forward's bit for bit.
#include "head_common.h"

namespace osa {

struct VolBwdArgs {
    const float* dV; const float* L; const float* R; float* dL; float* dR;
    int B, C, H, W, D, G, K, VC, coff;   // gwc: channels [coff, coff+G) of dV
    int concat, mask_left;               // concat: C = per-side channels, left at coff, right at coff+C
};

__global__ __launch_bounds__(256) void volume_bwd_kernel(const VolBwdArgs p) {
    const size_t plane = (size_t)p.H * p.W;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over B*C*H*W
    if (i >= (size_t)p.B * p.C * plane) return;
    const int w = i % p.W; size_t r = i / p.W;
    const int h = r % p.H; r /= p.H;
    const int c = r % p.C; const int b = r / p.C;
    const size_t hw = (size_t)h * p.W + w;
    const size_t dstride = plane;                                     // dV stride along d
    float gl = 0.f, gr = 0.f;
    if (!p.concat) {
        const int g = c / p.K;
        const float* dv = p.dV + (((size_t)b * p.VC + p.coff + g) * p.D) * plane + hw;
        const float* Lr = p.L + ((size_t)b * p.C + c) * plane + (size_t)h * p.W;
        const float* Rr = p.R + ((size_t)b * p.C + c) * plane + (size_t)h * p.W;
        for (int d = 0; d < p.D; ++d) {
            if (d <= w) gl = fmaf(dv[(size_t)d * dstride], Rr[w - d], gl);
            if (w + d < p.W) gr = fmaf(dv[(size_t)d * dstride + d], Lr[w + d], gr);
        }
        const float invK = 1.0f / (float)p.K;
        gl *= invK; gr *= invK;
    } else {
        const float* dvl = p.dV + (((size_t)b * p.VC + p.coff + c) * p.D) * plane + hw;
        const float* dvr = p.dV + (((size_t)b * p.VC + p.coff + p.C + c) * p.D) * plane + hw;
        for (int d = 0; d < p.D; ++d) {
            if (d <= w || !p.mask_left) gl += dvl[(size_t)d * dstride];
            if (w + d < p.W) gr += dvr[(size_t)d * dstride + d];
        }
    }
    p.dL[i] = gl;
    p.dR[i] = gr;
}

__global__ __launch_bounds__(256) void softargmin_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dprob,
                                                             int D, long long HW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;    // over B*D*H*W
    if (i >= total) return;
    const long long hw = i % HW; const long long bd = i / HW;
    const int d = (int)(bd % D); const long long b = bd / D;
    dprob[i] = (float)d * dout[b * HW + hw];
}

// logits (p = softmax, mu = sum p d, var = sum p (d - mu)^2), g / gv the gradients of the disparity / the variance:
//     dcost[k] = p_k (k - mu) g                                 and with VAR   dcost[k] = p_k [ (k - mu) g + ((k - mu)^2 - var) gv ]
// (the variance's dependence on its own mean drops out: sum_d p_d (d - mu) = 0).  One thread per pixel, serial over d: fixed order.
template <bool VAR>
__device__ __forceinline__ void softmax_softargmin_bwd_body(const float* __restrict__ cost, const float* __restrict__ dout,
                                                            const float* __restrict__ dvar, float* __restrict__ dcost,
                                                            int D, long long HW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;    // over B*H*W
    if (i >= total) return;
    const long long b = i / HW, hw = i - b * HW;
    const float* c = cost + (size_t)b * D * HW + hw;
    float m = -INFINITY;
    for (int d = 0; d < D; ++d) m = fmaxf(m, c[(size_t)d * HW]);
    float se = 0.f, sd = 0.f;
    for (int d = 0; d < D; ++d) { const float e = expf(c[(size_t)d * HW] - m); se += e; sd = fmaf(e, (float)d, sd); }
    const float inv = 1.f / se, disp = sd * inv, g = dout[i];
    float gv = 0.f, var = 0.f;
    if constexpr (VAR) {
        gv = dvar[i];
        float sv = 0.f;
        for (int d = 0; d < D; ++d) { const float t = (float)d - disp; sv = fmaf(expf(c[(size_t)d * HW] - m), t * t, sv); }
        var = sv * inv;
    }
    float* dc = dcost + (size_t)b * D * HW + hw;
    for (int d = 0; d < D; ++d) {
        const float t = (float)d - disp, pd = expf(c[(size_t)d * HW] - m) * inv;
        dc[(size_t)d * HW] = VAR ? pd * fmaf(t * t - var, gv, t * g) : pd * t * g;
    }
}

__global__ __launch_bounds__(256) void softmax_softargmin_bwd_kernel(const float* __restrict__ cost, const float* __restrict__ dout,
                                                                     float* __restrict__ dcost, int D, long long HW, long long total) {
    softmax_softargmin_bwd_body<false>(cost, dout, nullptr, dcost, D, HW, total);
}
__global__ __launch_bounds__(256) void softmax_softargmin_var_bwd_kernel(const float* __restrict__ cost, const float* __restrict__ dout,
                                                                         const float* __restrict__ dvar, float* __restrict__ dcost,
                                                                         int D, long long HW, long long total) {
    softmax_softargmin_bwd_body<true>(cost, dout, dvar, dcost, D, HW, total);
}

struct UpBwdArgs {
    const float* cost; const float* dout; float* dcost;   // dcost must be zero-initialised (one-kernel form only)
    UpDims g;
};
struct UpVarBwdArgs {
    UpBwdArgs a;
    const float* dvar;
};

// The backward's staging: the thread's Dl interpolated low-res costs into its column of cl[Dl][NT], as the forward's stage_column, with a zeroed
// gradient column in gl[Dl][NT] beside it.  Returns the column's maximum (no sample exceeds it: the softmax's shift).
template <int NT>
__device__ __forceinline__ float stage_columns_bwd(const Bilinear<size_t>& f, const float* c, size_t plane, int Dl, float* cl, float* gl) {
    const int tid = threadIdx.x;
    float m = -INFINITY;
    for (int dl = 0; dl < Dl; ++dl) {
        const float v = f(c + (size_t)dl * plane);
        cl[dl * NT + tid] = v; gl[dl * NT + tid] = 0.f;
        m = fmaxf(m, v);
    }
    return m;
}

// one thread per output pixel: recompute its D up-sampled costs, softmax and disparity, fold
// g_d = p_d (d - disp) dout along d into the Dl low-res planes (LDS, [dl][thread]), then add the 4
// (y,x) corner contributions with float atomics.
__global__ __launch_bounds__(256) void upsample_softargmin_bwd_kernel(const UpBwdArgs p) {
    extern __shared__ float sh[];            // cl[Dl][256] then gl[Dl][256]
    const UpDims& q = p.g;
    float* cl = sh; float* gl = sh + (size_t)q.Dl * 256;
    const int tid = threadIdx.x;
    const UpPixel px = up_pixel<256>(q);
    const Bilinear<size_t> f(px.y, px.x, q.sh, q.sw, q.align, q.Hl, q.Wl);
    const size_t plane = (size_t)q.Hl * q.Wl;
    const float m = stage_columns_bwd<256>(f, p.cost + (size_t)px.b * q.Dl * plane, plane, q.Dl, cl, gl);
    float se = 0.f, sdisp = 0.f;
    for (int d = 0; d < q.D; ++d) {
        const float e = expf(up_sample<256>(cl, d, q) - m);
        se += e; sdisp = fmaf(e, (float)d, sdisp);
    }
    const float inv = 1.f / se, disp = sdisp * inv;
    const float g = px.live ? p.dout[px.i] : 0.f;
    for (int d = 0; d < q.D; ++d) {
        int d0, d1; float ld;
        src_index(d, q.sd, q.align, q.Dl, d0, d1, ld);
        const float e = expf((1.f - ld) * cl[d0 * 256 + tid] + ld * cl[d1 * 256 + tid] - m);    // up_sample(d), and where it came from
        const float gd = e * inv * ((float)d - disp) * g;
        gl[d0 * 256 + tid] += (1.f - ld) * gd;
        gl[d1 * 256 + tid] += ld * gd;
    }
    if (!px.live) return;
    float* dc = p.dcost + (size_t)px.b * q.Dl * plane;
    for (int dl = 0; dl < q.Dl; ++dl) {
        const float gv = gl[dl * 256 + tid];
        float* dp = dc + (size_t)dl * plane;
        atomicAdd(dp + f.o00, f.w00 * gv); atomicAdd(dp + f.o01, f.w01 * gv);
        atomicAdd(dp + f.o10, f.w10 * gv); atomicAdd(dp + f.o11, f.w11 * gv);
    }
}


// ---- two-pass, atomic-free form (osa_upsample_softargmin_bwd_ws_f32) ---------------------------------------------------------------
// The one-kernel form above scatters 4 * Dl float atomics per output pixel (25 M of them for one 256x512 pair, ~25 pixels contending for
// every low-res cell): 0.75 ms per head, 6.7 % of a GwcNet training step, and a run-dependent summation order.
// pass 1 (fold): one thread per output pixel, as above, but the Dl folded gradients go to a scratch tensor G[b][dl][y][x] (coalesced).
// pass 2 (gather): one thread per low-res cell sums w_y * w_x * G over the output pixels whose bilinear footprint contains the cell, in
// a fixed order -- deterministic, no zero-fill, no atomics.
// VAR: the per-sample coefficient of the logits form above, with one more pass over the LDS-resident samples for the variance.
template <int NT, bool VAR>
__device__ __forceinline__ void upsample_softargmin_bwd_fold_body(const UpBwdArgs& p, const float* dvar, float* __restrict__ G) {
    extern __shared__ float sh[];            // cl[Dl][NT] then gl[Dl][NT]
    const UpDims& q = p.g;
    float* cl = sh; float* gl = sh + (size_t)q.Dl * NT;
    const int tid = threadIdx.x;
    const UpPixel px = up_pixel<NT>(q);
    const Bilinear<size_t> f(px.y, px.x, q.sh, q.sw, q.align, q.Hl, q.Wl);
    const size_t plane = (size_t)q.Hl * q.Wl;
    const float m = stage_columns_bwd<NT>(f, p.cost + (size_t)px.b * q.Dl * plane, plane, q.Dl, cl, gl);
    float se = 0.f, sdisp = 0.f;
    for (int d = 0; d < q.D; ++d) {
        const float e = expf(up_sample<NT>(cl, d, q) - m);
        se += e; sdisp = fmaf(e, (float)d, sdisp);
    }
    const float inv = 1.f / se, disp = sdisp * inv;
    float var = 0.f;
    if constexpr (VAR) {
        float sv = 0.f;
        for (int d = 0; d < q.D; ++d) {
            const float t = (float)d - disp;
            sv = fmaf(expf(up_sample<NT>(cl, d, q) - m), t * t, sv);
        }
        var = sv * inv;
    }
    const float g = px.live ? p.dout[px.i] : 0.f, gv = (VAR && px.live) ? dvar[px.i] : 0.f;
    for (int d = 0; d < q.D; ++d) {
        int d0, d1; float ld;
        src_index(d, q.sd, q.align, q.Dl, d0, d1, ld);
        const float e = expf((1.f - ld) * cl[d0 * NT + tid] + ld * cl[d1 * NT + tid] - m);    // up_sample(d), and where it came from
        const float pd = e * inv, t = (float)d - disp;
        const float gd = VAR ? pd * fmaf(t * t - var, gv, t * g) : pd * t * g;
        gl[d0 * NT + tid] += (1.f - ld) * gd;
        gl[d1 * NT + tid] += ld * gd;
    }
    if (!px.live) return;
    const long long HW = (long long)q.H * q.W;
    float* gp = G + (size_t)px.b * q.Dl * HW + px.hw;
    for (int dl = 0; dl < q.Dl; ++dl) gp[(size_t)dl * HW] = gl[dl * NT + tid];
}

template <int NT>
__global__ __launch_bounds__(NT) void upsample_softargmin_bwd_fold_kernel(const UpBwdArgs p, float* __restrict__ G) {
    upsample_softargmin_bwd_fold_body<NT, false>(p, nullptr, G);
}
template <int NT>
__global__ __launch_bounds__(NT) void upsample_softargmin_var_bwd_fold_kernel(const UpVarBwdArgs q, float* __restrict__ G) {
    upsample_softargmin_bwd_fold_body<NT, true>(q.a, q.dvar, G);
}

// output positions whose source interval can contain low-res index `il` (a conservative range; the exact test is src_index)
__device__ __forceinline__ void footprint(int il, float scale, int align, int out_size, int& lo, int& hi) {
    if (scale <= 0.f) { lo = 0; hi = out_size - 1; return; }
    const float off = align ? 0.f : 0.5f;
    const float a = ((float)il - 1.f + off) / scale - off, b = ((float)il + 1.f + off) / scale - off;
    lo = (int)floorf(a) - 1; hi = (int)ceilf(b) + 1;
    if (lo < 0) lo = 0;
    if (hi > out_size - 1) hi = out_size - 1;
}

__global__ __launch_bounds__(256) void upsample_softargmin_bwd_gather_kernel(const UpBwdArgs p, const float* __restrict__ G) {
    const long long total = (long long)p.g.B * p.g.Dl * p.g.Hl * p.g.Wl;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int xl = (int)(i % p.g.Wl); long long r = i / p.g.Wl;
    const int yl = (int)(r % p.g.Hl); r /= p.g.Hl;               // r = b * Dl + dl
    int ylo, yhi, xlo, xhi;
    footprint(yl, p.g.sh, p.g.align, p.g.H, ylo, yhi);
    footprint(xl, p.g.sw, p.g.align, p.g.W, xlo, xhi);
    const float* g = G + (size_t)r * p.g.H * p.g.W;
    float acc = 0.f;
    for (int y = ylo; y <= yhi; ++y) {
        int y0, y1; float ly;
        src_index(y, p.g.sh, p.g.align, p.g.Hl, y0, y1, ly);
        const float wy = ((y0 == yl) ? (1.f - ly) : 0.f) + ((y1 == yl) ? ly : 0.f);
        if (wy == 0.f) continue;
        const float* gr = g + (size_t)y * p.g.W;
        float row = 0.f;
        for (int x = xlo; x <= xhi; ++x) {
            int x0, x1; float lx;
            src_index(x, p.g.sw, p.g.align, p.g.Wl, x0, x1, lx);
            const float wx = ((x0 == xl) ? (1.f - lx) : 0.f) + ((x1 == xl) ? lx : 0.f);
            row = fmaf(wx, gr[x], row);
        }
        acc = fmaf(wy, row, acc);
    }
    p.dcost[i] = acc;
}

// ---- backward of the probabilities-form disparity + variance head (softargmin.hip) ------------------------------------------------------
// Two incoming gradients per pixel: g of the disparity, gv of the variance.  One thread per pixel, serial over d: no atomics, fixed order.
//  probabilities + given disparity `delta`:  dprob[d] = d g + (d - delta)^2 gv;   ddelta = -2 gv sum_d prob[d] (d - delta)
__global__ __launch_bounds__(256) void softargmin_var_bwd_kernel(const float* __restrict__ prob, const float* __restrict__ disparity,
                                                                 const float* __restrict__ dout, const float* __restrict__ dvar,
                                                                 float* __restrict__ dprob, float* __restrict__ ddisp,
                                                                 int D, long long HW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;    // over B*H*W
    if (i >= total) return;
    const long long b = i / HW, hw = i - b * HW;
    const float* p = prob + (size_t)b * D * HW + hw;
    float* dp = dprob + (size_t)b * D * HW + hw;
    // fp64 arithmetic, one rounding per result: the kernel is bound by its two D-plane streams, and d - delta, its square and the sum each
    // cost an fp32 rounding that the reference's own fp32 autograd (the test's yardstick, ~1 ulp) leaves no room for
    const double mu = disparity[i], g = dout ? dout[i] : 0.f, gv = dvar[i];
    double s = 0.0;
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
        const double t = (double)d - mu;
        s = fma((double)p[(size_t)d * HW], t, s);
        dp[(size_t)d * HW] = (float)fma((double)d, g, t * t * gv);
    }
    ddisp[i] = (float)(-2.0 * gv * s);
}

}  // namespace osa

using namespace osa;

extern "C" int osa_build_volume_bwd_f32(const float* dvol, const float* left, const float* right,
                                        float* dleft, float* dright,
                                        int B, int C, int H, int W, int maxdisp, int num_groups,
                                        int concat, int mask_left_concat, int vol_channels, int c_off,
                                        void* stream) {
    OSA_REQUIRE(dvol && dleft && dright, "build_volume_bwd: NULL pointer");
    OSA_REQUIRE(concat || (left && right), "build_volume_bwd: the gwc part needs the forward features");
    OSA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && maxdisp > 0, "build_volume_bwd: bad dims");
    VolBwdArgs a;
    a.dV = dvol; a.L = left; a.R = right; a.dL = dleft; a.dR = dright;
    a.B = B; a.C = C; a.H = H; a.W = W; a.D = maxdisp; a.VC = vol_channels; a.coff = c_off;
    a.concat = concat ? 1 : 0; a.mask_left = mask_left_concat ? 1 : 0;
    a.G = num_groups; a.K = 1;
    if (!concat) {
        OSA_REQUIRE(num_groups > 0 && C % num_groups == 0, "build_volume_bwd: C=%d not divisible by groups=%d", C, num_groups);
        a.K = C / num_groups;
        OSA_REQUIRE(c_off + num_groups <= vol_channels, "build_volume_bwd: channel range exceeds vol_channels");
    } else {
        OSA_REQUIRE(c_off + 2 * C <= vol_channels, "build_volume_bwd: channel range exceeds vol_channels");
    }
    const long long total = (long long)B * C * H * W;
    hipLaunchKernelGGL(volume_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, a);
    OSA_LAUNCH_CHECK("build_volume_bwd");
    return 0;
}

extern "C" int osa_softargmin_bwd_f32(const float* dout, float* dprob, int B, int D, int H, int W, void* stream) {
    OSA_REQUIRE(dout && dprob, "softargmin_bwd: NULL pointer");
    const long long HW = (long long)H * W, total = HW * B * D;
    hipLaunchKernelGGL(softargmin_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, dout, dprob, D, HW, total);
    OSA_LAUNCH_CHECK("softargmin_bwd");
    return 0;
}

extern "C" int osa_softmax_softargmin_bwd_f32(const float* cost, const float* dout, float* dcost,
                                              int B, int D, int H, int W, void* stream) {
    OSA_REQUIRE(cost && dout && dcost, "softmax_softargmin_bwd: NULL pointer");
    const long long HW = (long long)H * W, total = HW * B;
    hipLaunchKernelGGL(softmax_softargmin_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       cost, dout, dcost, D, HW, total);
    OSA_LAUNCH_CHECK("softmax_softargmin_bwd");
    return 0;
}

extern "C" int osa_upsample_softargmin_bwd_f32(const float* cost_lowres, const float* dout, float* dcost_lowres,
                                               int B, int Dl, int Hl, int Wl, int D, int H, int W,
                                               int align_corners, void* stream) {
    OSA_REQUIRE(cost_lowres && dout && dcost_lowres, "upsample_softargmin_bwd: NULL pointer");
    const size_t lds = (size_t)Dl * 256 * sizeof(float) * 2;
    OSA_REQUIRE(lds <= 160 * 1024, "upsample_softargmin_bwd: Dl=%d too large for LDS", Dl);
    UpBwdArgs a;
    a.cost = cost_lowres; a.dout = dout; a.dcost = dcost_lowres;
    a.g = up_dims(B, Dl, Hl, Wl, D, H, W, align_corners);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(dcost_lowres, 0, (size_t)B * Dl * Hl * Wl * sizeof(float), st);
    OSA_REQUIRE(e == hipSuccess, "upsample_softargmin_bwd: memset failed: %s", hipGetErrorString(e));
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)upsample_softargmin_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const long long total = (long long)B * H * W;
    hipLaunchKernelGGL(upsample_softargmin_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), lds, st, a);
    OSA_LAUNCH_CHECK("upsample_softargmin_bwd");
    return 0;
}

extern "C" size_t osa_upsample_softargmin_bwd_workspace_bytes(int B, int Dl, int H, int W) {
    if (B <= 0 || Dl <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * Dl * H * W * sizeof(float);
}

// the two-pass form with (dvar != NULL) or without the variance's gradient: its fold pass, then the gather pass both share
static int launch_upsample_softargmin_bwd_ws(const float* cost_lowres, const float* dout, const float* dvar, float* dcost_lowres,
                                             int B, int Dl, int Hl, int Wl, int D, int H, int W,
                                             int align_corners, void* workspace, size_t workspace_bytes, hipStream_t st) {
    const char* name = dvar ? "upsample_softargmin_var_bwd_ws" : "upsample_softargmin_bwd_ws";
    OSA_REQUIRE(workspace_bytes >= osa_upsample_softargmin_bwd_workspace_bytes(B, Dl, H, W) && ((size_t)workspace & 15) == 0,
                "%s: workspace too small or misaligned (osa_upsample_softargmin_bwd_workspace_bytes)", name);
    constexpr int NT = 128;
    const size_t lds = (size_t)Dl * NT * sizeof(float) * 2;
    OSA_REQUIRE(lds <= 160 * 1024, "%s: Dl=%d too large for LDS", name, Dl);
    UpVarBwdArgs q;
    UpBwdArgs& a = q.a;
    a.cost = cost_lowres; a.dout = dout; a.dcost = dcost_lowres; q.dvar = dvar;
    a.g = up_dims(B, Dl, Hl, Wl, D, H, W, align_corners);
    const void* fold = dvar ? (const void*)upsample_softargmin_var_bwd_fold_kernel<NT> : (const void*)upsample_softargmin_bwd_fold_kernel<NT>;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(fold, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    float* G = static_cast<float*>(workspace);
    const dim3 grid(cdiv((long long)B * H * W, NT));
    if (dvar) hipLaunchKernelGGL(upsample_softargmin_var_bwd_fold_kernel<NT>, grid, dim3(NT), lds, st, q, G);
    else hipLaunchKernelGGL(upsample_softargmin_bwd_fold_kernel<NT>, grid, dim3(NT), lds, st, a, G);
    OSA_LAUNCH_CHECK(dvar ? "upsample_softargmin_var_bwd_ws (fold)" : "upsample_softargmin_bwd_ws (fold)");
    hipLaunchKernelGGL(upsample_softargmin_bwd_gather_kernel, dim3(cdiv((long long)B * Dl * Hl * Wl, 256)), dim3(256), 0, st, a, (const float*)G);
    OSA_LAUNCH_CHECK(dvar ? "upsample_softargmin_var_bwd_ws (gather)" : "upsample_softargmin_bwd_ws (gather)");
    return 0;
}

extern "C" int osa_upsample_softargmin_bwd_ws_f32(const float* cost_lowres, const float* dout, float* dcost_lowres,
                                                  int B, int Dl, int Hl, int Wl, int D, int H, int W,
                                                  int align_corners, void* workspace, size_t workspace_bytes, void* stream) {
    OSA_REQUIRE(cost_lowres && dout && dcost_lowres && workspace, "upsample_softargmin_bwd_ws: NULL pointer");
    return launch_upsample_softargmin_bwd_ws(cost_lowres, dout, nullptr, dcost_lowres, B, Dl, Hl, Wl, D, H, W, align_corners,
                                             workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- disparity + variance heads ---------------------------------------------------------------------------------------------------
extern "C" int osa_softargmin_var_bwd_f32(const float* prob, const float* disparity, const float* dout, const float* dvar,
                                          float* dprob, float* ddisparity, int B, int D, int H, int W, void* stream) {
    OSA_REQUIRE(prob && disparity && dvar && dprob && ddisparity, "softargmin_var_bwd: NULL pointer");     // dout may be NULL: no disparity gradient
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "softargmin_var_bwd: bad dims");
    const long long HW = (long long)H * W, total = HW * B;
    hipLaunchKernelGGL(softargmin_var_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       prob, disparity, dout, dvar, dprob, ddisparity, D, HW, total);
    OSA_LAUNCH_CHECK("softargmin_var_bwd");
    return 0;
}

extern "C" int osa_softmax_softargmin_var_bwd_f32(const float* cost, const float* dout, const float* dvar, float* dcost,
                                                  int B, int D, int H, int W, void* stream) {
    OSA_REQUIRE(cost && dout && dvar && dcost, "softmax_softargmin_var_bwd: NULL pointer");
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "softmax_softargmin_var_bwd: bad dims");
    const long long HW = (long long)H * W, total = HW * B;
    hipLaunchKernelGGL(softmax_softargmin_var_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       cost, dout, dvar, dcost, D, HW, total);
    OSA_LAUNCH_CHECK("softmax_softargmin_var_bwd");
    return 0;
}

extern "C" int osa_upsample_softargmin_var_bwd_ws_f32(const float* cost_lowres, const float* dout, const float* dvar, float* dcost_lowres,
                                                      int B, int Dl, int Hl, int Wl, int D, int H, int W,
                                                      int align_corners, void* workspace, size_t workspace_bytes, void* stream) {
    OSA_REQUIRE(cost_lowres && dout && dvar && dcost_lowres && workspace, "upsample_softargmin_var_bwd_ws: NULL pointer");
    OSA_REQUIRE(B > 0 && Dl > 0 && Hl > 0 && Wl > 0 && D > 0 && H > 0 && W > 0, "upsample_softargmin_var_bwd_ws: bad dims");
    return launch_upsample_softargmin_bwd_ws(cost_lowres, dout, dvar, dcost_lowres, B, Dl, Hl, Wl, D, H, W, align_corners,
                                             workspace, workspace_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------ IGEV++ multi-range volumes (mr_volume.h) ----
// dgwc[g,d] = [d<S] dV0[g,d] + [d<M] sum_o P0[o,g,d%k0] dV1[o,d/k0] + sum_o P1[o,g,d%k1] dV2[o,d/k1] is recomputed wherever it is needed.
#include "mr_volume.h"
namespace osa {

// Data gradients, no atomics: a lane owns one pixel of ONE image and CPB channels of one group (blockIdx.y), and walks d.
// RIGHT = false: dL[c,w] = (1/K) sum_{d<=w} dgwc[g,d,w] R[c,w-d];  RIGHT = true: dR[c,x] = (1/K) sum_{x+d<W} dgwc[g,d,x+d] L[c,x+d].
template <int CPB, int K0, int K1, bool CL, bool RIGHT>
__global__ __launch_bounds__(64) void mr_volume_bwd_data_kernel(const MrArgs p) {
    unsigned bid = blockIdx.x;
    const int wt = bid % p.nWt; bid /= p.nWt;
    const int h = bid % p.H, b = bid / p.H;
    const int px = wt * MR_WT + (int)threadIdx.x;
    if (px >= p.W) return;
    const int c0 = blockIdx.y * CPB, g = c0 / p.K;
    const size_t plane = (size_t)p.H * p.W;
    const float* F = (RIGHT ? p.L : p.R) + ((size_t)b * p.C + c0) * plane + (size_t)h * p.W;     // the other image's features
    const int D1 = p.M / K0, D2 = p.D / K1;
    float w0r[K0][MR_G], w1r[K1][MR_G];                     // this group's patch weights (uniform)
#pragma unroll
    for (int o = 0; o < MR_G; ++o) {
#pragma unroll
        for (int j = 0; j < K0; ++j) w0r[j][o] = p.P0[(o * MR_G + g) * K0 + j];
#pragma unroll
        for (int j = 0; j < K1; ++j) w1r[j][o] = p.P1[(o * MR_G + g) * K1 + j];
    }
    float acc[CPB];
#pragma unroll
    for (int k = 0; k < CPB; ++k) acc[k] = 0.f;
    const int dend = RIGHT ? min(p.D, p.W - px) : min(p.D, px + 1);       // the planes at which this pixel is paired
    for (int d4 = 0; d4 < dend; d4 += 4) {
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {                    // d % 4 == j4: the patch taps are compile-time
            const int d = d4 + j4;
            if (d < dend) {
                const int wq = RIGHT ? px + d : px, xo = RIGHT ? px + d : px - d;
                float dg = 0.f, v[MR_G];
                if (p.V0 && d < p.S) dg = p.V0[mr_vox<CL>(b, g, d, p.S, h, p.H, wq, p.W)];
                if (p.V1 && d < p.M) {
                    mr_load8<CL>(v, p.V1, b, d / K0, D1, h, p.H, wq, p.W);
#pragma unroll
                    for (int o = 0; o < MR_G; ++o) dg = fmaf(w0r[j4 % K0][o], v[o], dg);
                }
                if (p.V2) {
                    mr_load8<CL>(v, p.V2, b, d / K1, D2, h, p.H, wq, p.W);
#pragma unroll
                    for (int o = 0; o < MR_G; ++o) dg = fmaf(w1r[j4 % K1][o], v[o], dg);
                }
#pragma unroll
                for (int k = 0; k < CPB; ++k) acc[k] = fmaf(dg, F[(size_t)k * plane + xo], acc[k]);
            }
        }
    }
    float* out = (RIGHT ? p.dR : p.dL) + ((size_t)b * p.C + c0) * plane + (size_t)h * p.W + px;
    const float Kf = (float)p.K;
#pragma unroll
    for (int k = 0; k < CPB; ++k) out[(size_t)k * plane] = acc[k] / Kf;
}

// Weight gradients, stage 1: dP[o,g,j] = sum dV[o,d',w] gwc[g,k d'+j,w] with gwc recomputed as in the forward.  Four waves share a pixel
// tile and its ring; wave r walks the planes d = r (mod 4), for which both taps j0 = r % k0 and j1 = r % k1 are fixed, so a lane keeps
// 64 + 64 partial sums.  They are reduced over the wave in a fixed order and written to ws[chunk][block][r][128]: no atomics.
template <int KT, int K0, int K1, bool CL>
__global__ __launch_bounds__(256) void mr_volume_bwd_w_kernel(const MrArgs p) {
    constexpr int CT = MR_G * KT;
    __shared__ float ring[KT ? CT * MR_RING : 1];
    unsigned bid = blockIdx.x;
    const int wt = bid % p.nWt; bid /= p.nWt;
    const int h = bid % p.H, b = bid / p.H;
    const int tid = threadIdx.x, lane = tid & 63, r = tid >> 6, w0 = wt * MR_WT, w = w0 + lane;
    const bool live = w < p.W;
    const size_t plane = (size_t)p.H * p.W;
    const float* Lrow = p.L + (size_t)b * p.C * plane + (size_t)h * p.W;
    const float* Rrow = p.R + (size_t)b * p.C * plane + (size_t)h * p.W;
    const float Kf = (float)p.K;
    const int D1 = p.M / K0, D2 = p.D / K1;
    const int d0 = blockIdx.y * p.DCH, dend = min(p.D, d0 + p.DCH);
    float a1[64], a2[64];                                   // [o][g]
#pragma unroll
    for (int i = 0; i < 64; ++i) a1[i] = a2[i] = 0.f;
    if (d0 <= w0 + MR_WT - 1) {                             // (else no pixel of the tile reaches this chunk: its partial sums are zero)
        float Lr[KT ? CT : 1];
        if constexpr (KT > 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) Lr[c] = live ? Lrow[(size_t)c * plane + w] : 0.f;
            mr_stage<CT, 256>(ring, Rrow, plane, p.W, w0 - d0 - MR_DS + 1, MR_WT + MR_DS - 1, tid);
        }
        __syncthreads();
        for (int ds = d0; ds < dend; ds += MR_DS) {
            [[maybe_unused]] float nb[KT ? CT * MR_DS / 256 : 1];
            const int xn = w0 + 1 - ds - 2 * MR_DS;
            const bool more = ds + MR_DS < dend;
            if constexpr (KT > 0) if (more) mr_fetch<CT, 256>(nb, Rrow, plane, p.W, xn, tid);
#pragma unroll 1
            for (int d = ds + r; d < min(ds + MR_DS, dend); d += 4) {
                if (live && w >= d) {                       // (elsewhere gwc is zero)
                    float c[MR_G], v[MR_G];
                    mr_gwc<KT>(c, Lr, ring, Lrow, Rrow, plane, p.K, Kf, w, d, live);
                    if (p.V1 && d < p.M) {
                        mr_load8<CL>(v, p.V1, b, d / K0, D1, h, p.H, w, p.W);
#pragma unroll
                        for (int o = 0; o < MR_G; ++o)
#pragma unroll
                            for (int g = 0; g < MR_G; ++g) a1[o * MR_G + g] = fmaf(v[o], c[g], a1[o * MR_G + g]);
                    }
                    if (p.V2) {
                        mr_load8<CL>(v, p.V2, b, d / K1, D2, h, p.H, w, p.W);
#pragma unroll
                        for (int o = 0; o < MR_G; ++o)
#pragma unroll
                            for (int g = 0; g < MR_G; ++g) a2[o * MR_G + g] = fmaf(v[o], c[g], a2[o * MR_G + g]);
                    }
                }
            }
            if constexpr (KT > 0) {
                if (more) mr_commit<CT, 256>(ring, nb, xn, tid);
                __syncthreads();
            }
        }
    }
    float* out = p.ws + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + r) * 128;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        float x = a1[i], y = a2[i];
#pragma unroll
        for (int off = 32; off; off >>= 1) { x += __shfl_xor(x, off); y += __shfl_xor(y, off); }
        if (lane == 0) { out[i] = x; out[64 + i] = y; }
    }
}

// stage 2: block i < 128 (patch i / 64, (o, g) = i % 64) sums the partials of every stage-1 block in a fixed order
__global__ __launch_bounds__(64) void mr_volume_bwd_w_reduce_kernel(const float* __restrict__ ws, int nblk, float* __restrict__ dP0, float* __restrict__ dP1, int k0, int k1) {
    const int i = blockIdx.x, lane = threadIdx.x;
    float part[4];
    for (int r = 0; r < 4; ++r) {
        float s = 0.f;
        for (int blk = lane; blk < nblk; blk += 64) s += ws[((size_t)blk * 4 + r) * 128 + i];
#pragma unroll
        for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
        part[r] = s;
    }
    if (lane == 0) {
        const int k = (i < 64) ? k0 : k1;
        float* dP = (i < 64) ? dP0 : dP1;
        for (int j = 0; j < k; ++j) {
            float s = 0.f;
            for (int r = j; r < 4; r += k) s += part[r];
            dP[(i & 63) * k + j] = s;
        }
    }
}

}  // namespace osa

extern "C" size_t osa_mr_volume_bwd_workspace_bytes(int B, int H, int W, int maxdisp) {
    if (B <= 0 || H <= 0 || W <= 0 || maxdisp <= 0) return 0;
    const long long nblk = (long long)B * H * cdiv(W, MR_WT);
    if (nblk > 0x7fffffffLL) return 0;
    return (size_t)nblk * cdiv(maxdisp, mr_chunk((int)nblk, maxdisp)) * 4 * 128 * sizeof(float);
}

extern "C" int osa_mr_volume_bwd_ws_f32(const float* dv0, const float* dv1, const float* dv2, int layout,
                                        const float* left, const float* right, const float* patch0, const float* patch1,
                                        float* dleft, float* dright, float* dpatch0, float* dpatch1,
                                        int B, int C, int H, int W, int num_groups, int out_channels, int maxdisp, int s_range, int m_range, int k0, int k1,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = mr_check("mr_volume_bwd_ws", left && right && patch0 && patch1 && dleft && dright && dpatch0 && dpatch1 && workspace,
                          B, C, H, W, num_groups, out_channels, maxdisp, s_range, m_range, k0, k1, layout)) return rc;
    const size_t need = osa_mr_volume_bwd_workspace_bytes(B, H, W, maxdisp);
    OSA_REQUIRE(workspace_bytes >= need, "mr_volume_bwd_ws: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    MrArgs a{left, right, patch0, patch1, const_cast<float*>(dv0), const_cast<float*>(dv1), const_cast<float*>(dv2), dleft, dright, (float*)workspace,
             B, C, H, W, maxdisp, s_range, m_range, C / num_groups, cdiv(W, MR_WT), 0};
    const int nblk = B * H * a.nWt;
    a.DCH = mr_chunk(nblk, maxdisp);
    const int nch = cdiv(maxdisp, a.DCH);
    hipStream_t st = (hipStream_t)stream;
    mr_dispatch(a.K, k0, k1, layout, [&](auto kt, auto c0, auto c1, auto cl) {
        constexpr int KT = decltype(kt)::value, A = decltype(c0)::value, E = decltype(c1)::value;
        constexpr bool CL = decltype(cl)::value;
        constexpr int CPB = KT ? KT : 1;                    // channels per lane of the data passes (any K: one)
        hipLaunchKernelGGL((mr_volume_bwd_data_kernel<CPB, A, E, CL, false>), dim3(nblk, C / CPB), dim3(64), 0, st, a);
        hipLaunchKernelGGL((mr_volume_bwd_data_kernel<CPB, A, E, CL, true>), dim3(nblk, C / CPB), dim3(64), 0, st, a);
        hipLaunchKernelGGL((mr_volume_bwd_w_kernel<KT, A, E, CL>), dim3(nblk, nch), dim3(256), 0, st, a);
    });
    hipLaunchKernelGGL(mr_volume_bwd_w_reduce_kernel, dim3(128), dim3(64), 0, st, (const float*)workspace, nblk * nch, dpatch0, dpatch1, k0, k1);
    OSA_LAUNCH_CHECK("mr_volume_bwd_ws");
    return 0;
}
