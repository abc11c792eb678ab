// What MobileStereoNet's two fused inverted-residual blocks (mv2_block3d.hip, mv2_block2d.hip) share: the packed parameter block and its
// one small pack launch, the folded-BatchNorm epilogues, the launchers' checks and their request for dynamic LDS.  The carving of the
// block into nine pointers and the depthwise row walk stay written out in each kernel: as shared functions they changed the instruction
// streams of the kernels (profiles/mv2_block2d/README.md).
//
// Packed parameters for a depthwise kernel of T taps (27 in 3-D, 9 in 2-D), Ch (Ci + Co + T + 4) + 2 Co floats:
//   W1 [Ch][Ci] | s1 [Ch] | b1 [Ch] | DW [T][Ch] | s2 [Ch] | b2 [Ch] | W3 [Co][Ch] | s3 [Co] | b3 [Co]
#pragma once
#include "osa_common.h"

namespace osa {

__device__ __forceinline__ float relu6f(float v) { return fminf(fmaxf(v, 0.f), 6.f); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// folded BatchNorm of four channels, plain and followed by ReLU6; a: float4, or an MFMA accumulator as it is
template <class V>
__device__ __forceinline__ float4 mv2_bn(const V& a, const float4& sc, const float4& sh) {
    return make_float4(fmaf(a[0], sc.x, sh.x), fmaf(a[1], sc.y, sh.y), fmaf(a[2], sc.z, sh.z), fmaf(a[3], sc.w, sh.w));
}
template <class V>
__device__ __forceinline__ float4 mv2_bn_relu6(const V& a, const float4& sc, const float4& sh) {
    return make_float4(relu6f(fmaf(a[0], sc.x, sh.x)), relu6f(fmaf(a[1], sc.y, sh.y)), relu6f(fmaf(a[2], sc.z, sh.z)), relu6f(fmaf(a[3], sc.w, sh.w)));
}

static inline size_t mv2_packed_floats(int taps, int Ci, int Ch, int Co) { return (size_t)Ch * (Ci + Co + taps + 4) + 2 * (size_t)Co; }

// the weights in the reference's layouts: w1 [Ch,Ci,1..], wd [Ch,1,taps] (-> [taps][Ch]), w3 [Co,Ch,1..]
template <int TAPS>
__global__ __launch_bounds__(256) void mv2_pack_kernel(const float* __restrict__ w1, const float* __restrict__ wd, const float* __restrict__ w3,
                                                        const float* __restrict__ s1, const float* __restrict__ b1, const float* __restrict__ s2,
                                                        const float* __restrict__ b2, const float* __restrict__ s3, const float* __restrict__ b3,
                                                        float* __restrict__ pk, int Ci, int Ch, int Co) {
    const int n1 = Ch * Ci, n3 = Co * Ch, total = n1 + (TAPS + 4) * Ch + n3 + 2 * Co;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v;
    if (i < n1) v = w1[i];
    else if ((i -= n1) < Ch) v = s1[i];
    else if ((i -= Ch) < Ch) v = b1[i];
    else if ((i -= Ch) < TAPS * Ch) v = wd[(i % Ch) * TAPS + i / Ch];
    else if ((i -= TAPS * Ch) < Ch) v = s2[i];
    else if ((i -= Ch) < Ch) v = b2[i];
    else if ((i -= Ch) < n3) v = w3[i];
    else if ((i -= n3) < Co) v = s3[i];
    else v = b3[i - Co];
    pk[blockIdx.x * 256 + threadIdx.x] = v;
}

static inline int mv2_check_channels(const char* who, int Ci, int Ch, int Co, int max_cio, int max_ch) {
    OSA_REQUIRE(Ci > 0 && Ch > 0 && Co > 0, "%s: bad dims", who);
    OSA_REQUIRE(Ci % 8 == 0 && Ch % 8 == 0 && Co % 8 == 0, "%s: channels %d -> %d -> %d (supported: multiples of 8)", who, Ci, Ch, Co);
    OSA_REQUIRE(Ci <= max_cio && Co <= max_cio && Ch <= max_ch, "%s: channels %d -> %d -> %d (supported: input and output <= %d, hidden <= %d)",
                who, Ci, Ch, Co, max_cio, max_ch);
    return 0;
}

// the checks of a block launch that depend on neither rank nor tile, in the order the callers report them
static inline int mv2_check_block(const char* who, int stride, int Ci, int Ch, int Co, int residual, int max_cio, int max_ch) {
    OSA_REQUIRE(stride == 1 || stride == 2, "%s: stride %d (supported: 1 and 2)", who, stride);
    if (int rc = mv2_check_channels(who, Ci, Ch, Co, max_cio, max_ch)) return rc;
    OSA_REQUIRE(!residual || (stride == 1 && Ci == Co), "%s: residual needs stride 1 and equal channels, got stride %d and %d -> %d", who, stride, Ci, Co);
    return 0;
}

// allow `bytes` of dynamic LDS per workgroup for KERNEL, once per process
template <auto KERNEL>
static int mv2_allow_lds(const char* who, int bytes) {
    static bool done = false;
    if (!done) {
        OSA_REQUIRE(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess,
                    "%s: %d KiB of LDS per workgroup refused", who, bytes / 1024);
        done = true;
    }
    return 0;
}

template <int TAPS>
static inline int mv2_pack(const char* who, const float* w_expand, const float* w_dw, const float* w_project, const float* scale1, const float* shift1,
                           const float* scale2, const float* shift2, const float* scale3, const float* shift3, float* packed, int Ci, int Ch, int Co,
                           int max_cio, int max_ch, hipStream_t st) {
    OSA_REQUIRE(w_expand && w_dw && w_project && scale1 && shift1 && scale2 && shift2 && scale3 && shift3 && packed, "%s: NULL pointer", who);
    if (int rc = mv2_check_channels(who, Ci, Ch, Co, max_cio, max_ch)) return rc;
    const int total = (int)mv2_packed_floats(TAPS, Ci, Ch, Co);
    hipLaunchKernelGGL(mv2_pack_kernel<TAPS>, dim3(cdiv(total, 256)), dim3(256), 0, st, w_expand, w_dw, w_project, scale1, shift1, scale2, shift2, scale3,
                       shift3, packed, Ci, Ch, Co);
    OSA_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace osa
