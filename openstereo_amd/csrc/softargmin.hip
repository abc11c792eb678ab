// Disparity regression kernels for gfx950.
//
//  * softargmin          : out = sum_d d * prob[d]                      (disp_regression.py:8-12)
//  * softmax_softargmin  : softmax over D fused with the expectation    (stereobase_gru.py:163-164)
//  * upsample_softargmin : trilinear x(D/Dl, H/Hl, W/Wl) upsample of the low-res cost, softmax over
//                          D and expectation in ONE pass: the [B,D,H,W] upsampled cost, its softmax
//                          and the p*d product (3 x 401 MB in the reference,
//                          gwcnet_disp_processor.py:128-133) never exist.  6.3 MB in, 2.1 MB out.
// All are HBM/L2-bound streaming kernels: lanes run along w (coalesced), D is a serial loop.
//
// Every head also exists with the per-pixel variance of the distribution beside the disparity (`*_var_kernel`):
// var = sum_d p_d (d - disp)^2, the reference's disparity_variance (models/cfnet/submodule.py:128-134, models/igevpp/submodule.py:153-159).
// A head is ONE body, `template <bool VAR>`, and the variance is the lines inside its `if constexpr (VAR)`: the disparity of a `_var`
// kernel is its twin's because it is the same source, operation for operation (same samples, same products, same accumulation order) --
// bit-identical, and nothing of the variance feeds it.  The `__global__` kernels are named wrappers of the two instantiations (profilers and
// tools know the heads by these names).  The variance is NEVER formed as E[d^2] - E[d]^2: for a sharp distribution near the top of the
// range that difference cancels 5 of fp32's 7 digits.  The bodies that can revisit their samples centre a further pass on
// the mean; the streaming body carries a centred second moment.
#include "head_common.h"

namespace osa {

// prob need not be normalised and, with VAR, `disparity` (the centre of the variance) need not be its mean: the reference takes both as given
template <bool VAR>
__device__ __forceinline__ void softargmin_body(const float* __restrict__ prob, const float* __restrict__ disparity,
                                                float* __restrict__ out, float* __restrict__ var, int D, long long HW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // over B*H*W
    if (i >= total) return;
    const long long b = i / HW, hw = i - b * HW;
    const float* p = prob + (size_t)b * D * HW + hw;
    float mu = 0.f;
    if constexpr (VAR) mu = disparity[i];
    float s = 0.f, sv = 0.f;
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
        const float pd = p[(size_t)d * HW];
        s = fmaf(pd, (float)d, s);
        if constexpr (VAR) { const float t = (float)d - mu; sv = fmaf(pd, t * t, sv); }
    }
    if (!VAR || out) out[i] = s;
    if constexpr (VAR) var[i] = sv;
}

__global__ __launch_bounds__(256) void softargmin_kernel(const float* __restrict__ prob, float* __restrict__ out,
                                                         int D, long long HW, long long total) {
    softargmin_body<false>(prob, nullptr, out, nullptr, D, HW, total);
}
__global__ __launch_bounds__(256) void softargmin_var_kernel(const float* __restrict__ prob, const float* __restrict__ disparity,
                                                             float* __restrict__ out, float* __restrict__ var,
                                                             int D, long long HW, long long total) {
    softargmin_body<true>(prob, disparity, out, var, D, HW, total);
}

// without VAR either of prob / out may be NULL; with VAR there is no prob and out is written
template <bool VAR>
__device__ __forceinline__ void softmax_softargmin_body(const float* __restrict__ cost, float* __restrict__ prob, float* __restrict__ out,
                                                        float* __restrict__ var, int D, long long HW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long b = i / HW, hw = i - b * HW;
    const float* c = cost + (size_t)b * D * HW + hw;
    float m = -INFINITY;
#pragma unroll 8
    for (int d = 0; d < D; ++d) m = fmaxf(m, c[(size_t)d * HW]);
    float se = 0.f, sd = 0.f;
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
        const float e = expf(c[(size_t)d * HW] - m);
        se += e;
        sd = fmaf(e, (float)d, sd);
    }
    const float inv = 1.0f / se, disp = sd * inv;
    if constexpr (VAR) {
        float sv = 0.f;
#pragma unroll 8
        for (int d = 0; d < D; ++d) {                                // third pass, about the mean (the column is in L2 by now)
            const float t = (float)d - disp;
            sv = fmaf(expf(c[(size_t)d * HW] - m), t * t, sv);
        }
        out[i] = disp;
        var[i] = sv * inv;
    } else {
        if (out) out[i] = disp;
        if (prob) {
            float* pp = prob + (size_t)b * D * HW + hw;
#pragma unroll 8
            for (int d = 0; d < D; ++d) pp[(size_t)d * HW] = expf(c[(size_t)d * HW] - m) * inv;
        }
    }
}

__global__ __launch_bounds__(256) void softmax_softargmin_kernel(const float* __restrict__ cost, float* __restrict__ prob,
                                                                 float* __restrict__ out, int D, long long HW, long long total) {
    softmax_softargmin_body<false>(cost, prob, out, nullptr, D, HW, total);
}
__global__ __launch_bounds__(256) void softmax_softargmin_var_kernel(const float* __restrict__ cost, float* __restrict__ out,
                                                                     float* __restrict__ var, int D, long long HW, long long total) {
    softmax_softargmin_body<true>(cost, nullptr, out, var, D, HW, total);
}

struct UpArgs {
    const float* cost; float* out;
    UpDims g;
};
struct UpVarArgs {
    UpArgs a;
    float* var;
};

// exp(x) for x <= 0 on the transcendental unit with a compensated argument: t = x * log2(e) is formed as
// hi + lo (lo = the rounding error of the product plus the low bits of the constant), exp2(hi) comes from
// v_exp_f32 and the lo part is applied to first order.  ~1.5 ulp, 6 VALU operations (expf: ~20).
__device__ __forceinline__ float exp_neg(float x) {
    const float L2E = 1.44269502162933349609375f, L2E_LO = 1.92596299112661746e-8f;
    const float t = x * L2E;
    const float lo = fmaf(x, L2E, -t) + x * L2E_LO;
    const float e = __builtin_amdgcn_exp2f(t);
    return (t < -126.f) ? e : fmaf(e, lo * 0.693147182464599609375f, e);     // x = -inf: e = 0 (lo would be NaN)
}

// Generic path (any output size, align_corners either way): one thread per output pixel; its Dl bilinearly
// interpolated low-res costs live in LDS (layout [dl][thread] -> conflict free), then two serial passes over the
// D upsampled samples: their maximum (the softmax is normalised by the maximum of the SAMPLES, as the reference's
// F.softmax does -- the plane maximum can lie far above every sample when costs are large, and exp() of all of
// them would underflow), then the exponentials.  VAR: a third pass over the LDS-resident samples, centred on the disparity.
template <bool VAR>
__device__ __forceinline__ void upsample_softargmin_body(const UpArgs& p, float* var) {
    extern __shared__ float cl[];   // [Dl][256]
    const UpDims& g = p.g;
    const UpPixel px = up_pixel<256>(g);
    const Bilinear<size_t> f(px.y, px.x, g.sh, g.sw, g.align, g.Hl, g.Wl);
    const size_t plane = (size_t)g.Hl * g.Wl;
    stage_column<256>(f, p.cost + (size_t)px.b * g.Dl * plane, plane, g.Dl, cl);
    float m = -INFINITY;
#pragma unroll 4
    for (int d = 0; d < g.D; ++d) m = fmaxf(m, up_sample<256>(cl, d, g));
    float se = 0.f, sdisp = 0.f;
#pragma unroll 4
    for (int d = 0; d < g.D; ++d) {
        const float e = expf(up_sample<256>(cl, d, g) - m);
        se += e;
        sdisp = fmaf(e, (float)d, sdisp);
    }
    const float disp = sdisp / se;
    float sv = 0.f;
    if constexpr (VAR) {
#pragma unroll 4
        for (int d = 0; d < g.D; ++d) {
            const float t = (float)d - disp;
            sv = fmaf(expf(up_sample<256>(cl, d, g) - m), t * t, sv);
        }
    }
    if (px.live) {
        p.out[px.i] = disp;
        if constexpr (VAR) var[px.i] = sv / se;
    }
}

__global__ __launch_bounds__(256) void upsample_softargmin_kernel(const UpArgs p) { upsample_softargmin_body<false>(p, nullptr); }
__global__ __launch_bounds__(256) void upsample_softargmin_var_kernel(const UpVarArgs q) { upsample_softargmin_body<true>(q.a, q.var); }

// Fast path: exact x4 in all three dimensions, align_corners = False (GwcNet: [48,136,240] -> [192,544,960],
// gwcnet_disp_processor.py:99-133).  The four output disparities 4k .. 4k+3 depend on planes k-1, k, k+1 only, with
// the constant weights (.375,.625) (.125,.875) (.875,.125) (.625,.375), so a thread streams over the low-res planes
// with a 3-value window of bilinear samples and an ONLINE softmax (running maximum of the samples seen so far;
// one rescale + four exponentials per plane) -- no LDS, ~40 registers, 8 waves per SIMD to hide the L1/L2 latency
// of the 4 taps per plane.  Sample values are bit-identical to the generic path (same products, same order).
// r4: a workgroup is a 64 x 4 pixel tile (its four waves sample the same two or three low-res rows: L1 hits instead of four trips to L2) and
// the tiles are numbered through xcd_remap, so that every XCD walks a contiguous band of the image: with the plain linear numbering the
// four output rows that share a low-res row sat in workgroups 3.75 ids apart, i.e. on different XCDs, and every private L2 fetched the same
// cost rows again (PMC r3: 337 MB per launch for 66.9 MB of input, 5.0x).  Same samples, same order: bit-identical.
//
// VAR: a weighted mean and a centred second moment M2 of the samples seen so far beside (m, se, sd), which are untouched -- they alone
// produce the disparity.  Per low-res plane the four samples 4k .. 4k+3 form a group:
// weight wg (the very sum `se` takes in), mean offset og in [0, 3] and centred moment m2g, all sums of non-negative terms over the small
// offsets 0 .. 3; the group joins the running state by the pairwise update of Chan, Golub & LeVeque (1979), with the online softmax's
// rescale r applied to M2 as to se:
//     M2' = r M2 + m2g + delta^2 (r se) wg / se',     mean' = (r se mean + wg mean_g) / se',     delta = mean_g - mean
// The running mean is kept as nu = mean - 4k, RELATIVE to the current plane, and updated as the weighted average above rather than as
// mean + delta wg / se': a mean of ~180 carries an absolute rounding error of 1e-5 in fp32, which the next plane's delta (~4) would turn
// into a 5e-6 relative error of its cross term; nu is of the order of the offsets wherever its weight counts.
// One reciprocal per plane (of se' * wg, from which 1 / wg and 1 / se' follow; se' >= 1 once a plane is in, wg <= 4) beside the five
// exponentials.  A group whose weight underflowed contributes nothing.
template <bool VAR>
__device__ __forceinline__ void upsample4_softargmin_body(const UpArgs& p, float* var) {
    const UpDims& g = p.g;
    const long long HW = (long long)g.H * g.W;
    const int tilesX = (g.W + 63) >> 6, tilesY = (g.H + 3) >> 2;
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = bid % tilesX; bid /= tilesX;
    const int ty = bid % tilesY;
    const int b = bid / tilesY;
    const int x = tx * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
    if (x >= g.W || y >= g.H) return;
    const long long i = (long long)b * HW + (long long)y * g.W + x;
    const Bilinear<int> f(y, x, 0.25f, 0.25f, 0, g.Hl, g.Wl);
    const int plane = g.Hl * g.Wl;
    const float* c = p.cost + (size_t)b * g.Dl * plane;
    auto bil = [&](int k) { return f(c + (size_t)k * plane); };
    float vm = 0.f, vc = bil(0), vn = (g.Dl > 1) ? bil(1) : vc;
    float m = -INFINITY, se = 0.f, sd = 0.f;
    float nu = 0.f, M2 = 0.f;
    for (int k = 0; k < g.Dl; ++k) {
        const float vnn = (k + 2 < g.Dl) ? bil(k + 2) : 0.f;          // requested one plane ahead of its use
        // samples 4k .. 4k+3 (src = k - .375, k - .125, k + .125, k + .375; clamped to 0 below plane 0, i1 = i0 above the last)
        const float s0 = (k == 0) ? 1.f * vc + 0.f * vn : 0.375f * vm + 0.625f * vc;
        const float s1 = (k == 0) ? 1.f * vc + 0.f * vn : 0.125f * vm + 0.875f * vc;
        const float up = (k + 1 < g.Dl) ? vn : vc;
        const float s2 = 0.875f * vc + 0.125f * up;
        const float s3 = 0.625f * vc + 0.375f * up;
        const float mn = fmaxf(fmaxf(m, fmaxf(s0, s1)), fmaxf(s2, s3));
        const float r = exp_neg(m - mn);                               // m = -inf at k = 0: r = 0
        const float e0 = exp_neg(s0 - mn), e1 = exp_neg(s1 - mn), e2 = exp_neg(s2 - mn), e3 = exp_neg(s3 - mn);
        const float d0 = (float)(4 * k);
        const float wg = (e0 + e1) + (e2 + e3);
        const float wr = se * r;                                       // the running weight on the new scale (VAR)
        se = fmaf(se, r, wg);
        sd = fmaf(sd, r, fmaf(e0, d0, fmaf(e1, d0 + 1.f, fmaf(e2, d0 + 2.f, e3 * (d0 + 3.f)))));
        if constexpr (VAR) {                                           // the variance's own state: nothing here feeds m, se or sd
            const float rc = (wg > 1e-30f) ? __builtin_amdgcn_rcpf(se * wg) : 0.f;
            const float iwg = se * rc, ise = wg * rc;                  // 1 / wg, 1 / se'
            const float fg = wg * ise, fr = wr * ise;                  // the two weights' shares of se'
            const float og = fmaf(e3, 3.f, fmaf(e2, 2.f, e1)) * iwg;
            const float t1 = 1.f - og, t2 = 2.f - og, t3 = 3.f - og;
            const float m2g = fmaf(e0, og * og, fmaf(e1, t1 * t1, fmaf(e2, t2 * t2, e3 * (t3 * t3))));
            const float nk = nu - 4.f;                                 // the running mean seen from this plane (weight 0 at k = 0)
            const float delta = og - nk;
            M2 = fmaf(M2, r, fmaf(delta * delta, wr * fg, m2g));
            nu = (rc != 0.f) ? fmaf(nk, fr, og * fg) : nk;
        }
        m = mn;
        vm = vc; vc = vn; vn = vnn;
    }
    p.out[i] = sd / se;
    if constexpr (VAR) var[i] = M2 / se;
}

__global__ __launch_bounds__(256) void upsample4_softargmin_kernel(const UpArgs p) { upsample4_softargmin_body<false>(p, nullptr); }
__global__ __launch_bounds__(256) void upsample4_softargmin_var_kernel(const UpVarArgs q) { upsample4_softargmin_body<true>(q.a, q.var); }

}  // namespace osa

using namespace osa;

extern "C" int osa_softargmin_f32(const float* prob, float* out, int B, int D, int H, int W, void* stream) {
    OSA_REQUIRE(prob && out, "softargmin: NULL pointer");
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "softargmin: bad dims");
    const long long HW = (long long)H * W, total = HW * B;
    hipLaunchKernelGGL(softargmin_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, prob, out, D, HW, total);
    OSA_LAUNCH_CHECK("softargmin");
    return 0;
}

extern "C" int osa_softmax_softargmin_f32(const float* cost, float* prob, float* out,
                                          int B, int D, int H, int W, void* stream) {
    OSA_REQUIRE(cost && (out || prob), "softmax_softargmin: NULL pointer");
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "softmax_softargmin: bad dims");
    const long long HW = (long long)H * W, total = HW * B;
    hipLaunchKernelGGL(softmax_softargmin_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       cost, prob, out, D, HW, total);
    OSA_LAUNCH_CHECK("softmax_softargmin");
    return 0;
}

// the fused head with (var != NULL) or without the variance: the x4 streaming kernel where it applies, else the generic one
static int launch_upsample_softargmin(const char* name, const float* cost_lowres, float* out, float* var,
                                      int B, int Dl, int Hl, int Wl, int D, int H, int W, int align_corners, hipStream_t st) {
    OSA_REQUIRE(B > 0 && Dl > 0 && Hl > 0 && Wl > 0 && D > 0 && H > 0 && W > 0, "%s: bad dims", name);
    const size_t lds = (size_t)Dl * 256 * sizeof(float);
    OSA_REQUIRE(lds <= 160 * 1024, "%s: Dl=%d too large for LDS", name, Dl);
    UpVarArgs q;
    q.a.cost = cost_lowres; q.a.out = out; q.var = var;
    q.a.g = up_dims(B, Dl, Hl, Wl, D, H, W, align_corners);
    if (up_is_x4(q.a.g)) {
        const long long tiles = (long long)B * ((H + 3) / 4) * ((W + 63) / 64);
        OSA_REQUIRE(tiles < (1ll << 31), "%s: grid too large", name);
        if (var) hipLaunchKernelGGL(upsample4_softargmin_var_kernel, dim3((unsigned)tiles), dim3(256), 0, st, q);
        else hipLaunchKernelGGL(upsample4_softargmin_kernel, dim3((unsigned)tiles), dim3(256), 0, st, q.a);
        OSA_LAUNCH_CHECK(var ? "upsample4_softargmin_var" : "upsample4_softargmin");
        return 0;
    }
    const void* kernel = var ? (const void*)upsample_softargmin_var_kernel : (const void*)upsample_softargmin_kernel;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid(cdiv((long long)B * H * W, 256));
    if (var) hipLaunchKernelGGL(upsample_softargmin_var_kernel, grid, dim3(256), lds, st, q);
    else hipLaunchKernelGGL(upsample_softargmin_kernel, grid, dim3(256), lds, st, q.a);
    OSA_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int osa_upsample_softargmin_f32(const float* cost_lowres, float* out,
                                           int B, int Dl, int Hl, int Wl, int D, int H, int W,
                                           int align_corners, void* stream) {
    OSA_REQUIRE(cost_lowres && out, "upsample_softargmin: NULL pointer");
    return launch_upsample_softargmin("upsample_softargmin", cost_lowres, out, nullptr, B, Dl, Hl, Wl, D, H, W, align_corners, (hipStream_t)stream);
}

// ---- disparity + variance ---------------------------------------------------------------------------------------------------------
extern "C" int osa_softargmin_var_f32(const float* prob, const float* disparity, float* out, float* var,
                                      int B, int D, int H, int W, void* stream) {
    OSA_REQUIRE(prob && disparity && var, "softargmin_var: NULL pointer");
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "softargmin_var: bad dims");
    const long long HW = (long long)H * W, total = HW * B;
    hipLaunchKernelGGL(softargmin_var_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, prob, disparity, out, var, D, HW, total);
    OSA_LAUNCH_CHECK("softargmin_var");
    return 0;
}

extern "C" int osa_softmax_softargmin_var_f32(const float* cost, float* out, float* var,
                                              int B, int D, int H, int W, void* stream) {
    OSA_REQUIRE(cost && out && var, "softmax_softargmin_var: NULL pointer");
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "softmax_softargmin_var: bad dims");
    const long long HW = (long long)H * W, total = HW * B;
    hipLaunchKernelGGL(softmax_softargmin_var_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       cost, out, var, D, HW, total);
    OSA_LAUNCH_CHECK("softmax_softargmin_var");
    return 0;
}

extern "C" int osa_upsample_softargmin_var_f32(const float* cost_lowres, float* out, float* var,
                                               int B, int Dl, int Hl, int Wl, int D, int H, int W,
                                               int align_corners, void* stream) {
    OSA_REQUIRE(cost_lowres && out && var, "upsample_softargmin_var: NULL pointer");
    return launch_upsample_softargmin("upsample_softargmin_var", cost_lowres, out, var, B, Dl, Hl, Wl, D, H, W, align_corners, (hipStream_t)stream);
}
