// The interlaced cost volume of MobileStereoNet's MSNet2D (models/msnet/MSNet2D.py:143-162) and of StereoBase's InterlacedVolume
// (stereo/modeling/cost_volume/cost_volume.py:120-169) in eval mode as ONE launch.  Per disparity plane i the reference crops the left
// features to x >= i and the right ones to x < W - i, interweaves their channels (left at even, right at odd positions: X has 2C channels),
// views X as a one-channel volume and runs three Conv3d + BN + ReLU whose depth stride equals their depth kernel (k1, k2, k3 with
// k1 k2 k3 = 2C, widths 16, 32, 16), then a 1x1 Conv2d + BN + ReLU to F features.  Because stride == kernel along depth, every layer is
// a 2-D 3x3 convolution over (kd x Cin) channels applied to independent depth groups with shared weights:
//
//   A1[g] = relu(bn1(conv3x3(X[8g .. 8g+7])))                      g < k2 k3     8 -> 16
//   A2[g] = relu(bn2(conv3x3(A1[k2 g .. k2 g + k2 - 1])))          g < k3    16 k2 -> 32
//   A3    = relu(bn3(conv3x3(A2[0 .. k3 - 1])))                              32 k3 -> 16
//   V[:, :, i, :, i:] = relu(bn4(W4 A3))                                        16 -> F
//
// Each layer pads ITS OWN input with zeros outside the crop [0,H) x [0,W-i): X, A1 and A2 are true zeros there (not relu(shift)).
//
// A workgroup of 8 waves owns an 8 x 16 tile of output pixels of one (b, i) and streams along depth, outermost to innermost:
//   for g3 < k3:  for g2 < k2:  load the 8 interwoven channels of A1 group g3 k2 + g2 on tile + 3 halo into LDS (interweave and crop are
//                               address arithmetic), compute the group's A1 on tile + 2 halo into LDS, accumulate its contribution
//                               into the A2 accumulators (tile + 1 halo, 32 channels, registers)
//                 finish A2 (affine, ReLU, zero outside the crop) into LDS, accumulate its contribution into the A3 accumulators
//   finish A3 into LDS, 1x1 head, store.
// Only one A1 group and one A2 group are ever resident (49 KB of LDS: three workgroups per CU); nothing but V reaches memory.
//
// All three convolutions run on v_mfma_f32_16x16x4_f32 with rows = 16 output channels (A operand: packed weights, from global memory
// through L1/L2), columns = 16 pixels of the layer's region in row-major order (B operand: the LDS image [pixel][channel] at the tap's
// offset).  Lane quarter q (lane >> 4) supplies channels 4q + j of a 16-channel K step as one 16-byte read (2q + j of the 8 channels of
// layer 1), issued as 4 (2) MFMAs; a lane ends with 4 consecutive output channels of one pixel, which it writes as one 16-byte LDS store.
// The MFMA is an fmaf chain in a fixed order and every output voxel is computed by one workgroup: exact fp32, no atomics, no scratch,
// the bits depend neither on the batch size nor on the run.  Columns x < i of plane i and whole planes i >= W are written as zeros by
// the workgroups of the same grid (every element of V is stored exactly once).
//
// Packed parameters (osa_interlaced_volume_pack_f32), 1280 + 4608 (k2 + k3) + 18 F floats:
//   W1 [9 taps][16][8] | W2 [k2][9][32][16] | W3 [k3][9][16][32] | W4 [F][16] | s1 t1 [16] | s2 t2 [32] | s3 t3 [16] | s4 t4 [F]
#include "osa_common.h"

namespace osa {

constexpr int ILV_NT = 512, ILV_NW = ILV_NT / 64, ILV_TH = 8, ILV_TW = 16, ILV_K1 = 8, ILV_MAXF = 16;
typedef osa_f32x4_t ilv_f32x4;

struct IlvArgs {
    const float* fl; const float* fr; const float* pk; float* out;
    int B, C, H, W, D, F, nTx, nTy;
};

static inline size_t ilv_packed_floats(int k2, int k3, int F) { return 1280 + 4608 * (size_t)(k2 + k3) + 18 * (size_t)F; }
static inline bool ilv_supported(int C, int k2, int k3) { return (C == 32 && k2 == 4 && k3 == 2) || (C == 96 && k2 == 8 && k3 == 3); }

__device__ __forceinline__ float4 ilv_affine_relu(const ilv_f32x4 a, const float* s, const float* t, bool inside) {
    if (!inside) return make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(fmaxf(fmaf(a[0], s[0], t[0]), 0.f), fmaxf(fmaf(a[1], s[1], t[1]), 0.f), fmaxf(fmaf(a[2], s[2], t[2]), 0.f), fmaxf(fmaf(a[3], s[3], t[3]), 0.f));
}

template <int K2, int K3>
__global__ __launch_bounds__(ILV_NT) void interlaced_volume_kernel(const IlvArgs p) {
    constexpr int TH = ILV_TH, TW = ILV_TW;
    constexpr int XW = TW + 6, PX = (TH + 6) * XW;          // X  on tile + 3
    constexpr int R1W = TW + 4, P1 = (TH + 4) * R1W;        // A1 on tile + 2
    constexpr int R2W = TW + 2, P2 = (TH + 2) * R2W;        // A2 on tile + 1
    constexpr int P3 = TH * TW;
    constexpr int NB1 = (P1 + 15) / 16, NB2 = (P2 + 15) / 16, NB3 = P3 / 16;
    constexpr int NT2 = (2 * NB2 + ILV_NW - 1) / ILV_NW;     // A2 tiles (16 pixels x 16 of the 32 channels) per wave
    static_assert(NB3 == ILV_NW && P3 * 16 <= P1 * 16, "one A3 tile per wave; the A3 stage reuses the A1 image");
    __shared__ __attribute__((aligned(16))) float Xs[PX * 8];
    __shared__ __attribute__((aligned(16))) float A1s[P1 * 16];
    __shared__ __attribute__((aligned(16))) float A2s[P2 * 32];

    const float* const W1 = p.pk;
    const float* const W2 = W1 + 1152;
    const float* const W3 = W2 + 4608 * K2;
    const float* const W4 = W3 + 4608 * K3;
    const float* const s1 = W4 + 16 * p.F; const float* const t1 = s1 + 16;
    const float* const s2 = t1 + 16;       const float* const t2 = s2 + 32;
    const float* const s3 = t2 + 32;       const float* const t3 = s3 + 16;
    const float* const s4 = t3 + 16;       const float* const t4 = s4 + p.F;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
    const int H = p.H, W = p.W;
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = bid % p.nTx; bid /= p.nTx;
    const int ty = bid % p.nTy; bid /= p.nTy;
    const int i = bid % p.D, b = bid / p.D;
    const int Wc = W - i, y0 = ty * TH, x0 = tx * TW;
    float* const oplane = p.out + ((size_t)b * p.F * p.D + i) * H * W;      // + f * D * H * W
    const size_t ofs = (size_t)p.D * H * W;

    // ---- zeros: image columns [x0, x0 + TW) below i (all of them when i >= W)
    {
        const int zc = min(min(x0 + TW, i), W) - x0;
        if (zc > 0)
            for (int e = tid; e < p.F * TH * zc; e += ILV_NT) {
                const int x = e % zc, r = e / zc % TH, f = e / (zc * TH);
                if (y0 + r < H) oplane[f * ofs + (size_t)(y0 + r) * W + x0 + x] = 0.f;
            }
    }
    if (x0 >= Wc) return;                                     // nothing of the crop in this tile (uniform: before any barrier)

    const float* const flb = p.fl + (size_t)b * p.C * H * W;
    const float* const frb = p.fr + (size_t)b * p.C * H * W;

    // pixel of this lane in each layer's tiles (clamped: rows past the region compute a copy that is not stored)
    int xo1[2], p1[2];                                       // layer 1: at most 2 tiles of 16 A1 pixels per wave
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        p1[j] = (wave + ILV_NW * j) * 16 + l16;
        const int pc = min(p1[j], P1 - 1);
        xo1[j] = (pc / R1W * XW + pc % R1W) * 8 + 2 * q;
    }
    static_assert(NB1 <= 2 * ILV_NW, "layer 1: two tiles per wave");
    const int cb = wave & 1;                                 // layer 2: this wave's half of the 32 channels
    int ao2[NT2], p2[NT2];
#pragma unroll
    for (int j = 0; j < NT2; ++j) {
        p2[j] = ((wave + ILV_NW * j) >> 1) * 16 + l16;
        const int pc = min(p2[j], P2 - 1);
        ao2[j] = (pc / R2W * R1W + pc % R2W) * 16 + 4 * q;
    }
    const int p3 = wave * 16 + l16;
    const int ao3 = (p3 / TW * R2W + p3 % TW) * 32 + 4 * q;

    ilv_f32x4 acc3 = {};
    for (int g3 = 0; g3 < K3; ++g3) {
        ilv_f32x4 acc2[NT2];
#pragma unroll
        for (int j = 0; j < NT2; ++j) acc2[j] = ilv_f32x4{};
        for (int g2 = 0; g2 < K2; ++g2) {
            const int g = g3 * K2 + g2;
            __syncthreads();                                 // the previous group's readers of Xs and A1s are done
            // ---- X: channels 8g .. 8g+7 = left / right channels 4g .. 4g+3 interwoven, zero outside the crop
            for (int e = tid; e < PX * 8; e += ILV_NT) {
                const int ch = e & 7, pix = e >> 3, y = y0 - 3 + pix / XW, x = x0 - 3 + pix % XW;
                float v = 0.f;
                if (y >= 0 && y < H && x >= 0 && x < Wc) {
                    const size_t o = ((size_t)(4 * g + (ch >> 1)) * H + y) * W + x;
                    v = (ch & 1) ? frb[o] : flb[o + i];
                }
                Xs[e] = v;
            }
            __syncthreads();
            // ---- A1 of this group on tile + 2: K = 9 taps x 8 channels
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (wave + ILV_NW * j >= NB1) break;
                ilv_f32x4 acc = {};
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const float2 a = *reinterpret_cast<const float2*>(W1 + (tap * 16 + l16) * 8 + 2 * q);
                    const float2 v = *reinterpret_cast<const float2*>(Xs + xo1[j] + ((tap / 3) * XW + tap % 3) * 8);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, v.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, v.y, acc, 0, 0, 0);
                }
                if (p1[j] < P1) {
                    const int y = y0 - 2 + p1[j] / R1W, x = x0 - 2 + p1[j] % R1W;
                    *reinterpret_cast<float4*>(A1s + p1[j] * 16 + 4 * q) = ilv_affine_relu(acc, s1 + 4 * q, t1 + 4 * q, y >= 0 && y < H && x >= 0 && x < Wc);
                }
            }
            __syncthreads();
            // ---- its contribution to A2 on tile + 1: K = 9 taps x 16 channels
            const float* const w2 = W2 + (size_t)g2 * 4608 + (cb * 16 + l16) * 16 + 4 * q;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float4 a = *reinterpret_cast<const float4*>(w2 + tap * 512);
#pragma unroll
                for (int j = 0; j < NT2; ++j) {
                    if (wave + ILV_NW * j >= 2 * NB2) break;
                    acc2[j] = mfma_k16(a, *reinterpret_cast<const float4*>(A1s + ao2[j] + ((tap / 3) * R1W + tap % 3) * 16), acc2[j]);
                }
            }
        }
        // ---- finish A2 group g3 (the previous group's readers of A2s passed two barriers since)
#pragma unroll
        for (int j = 0; j < NT2; ++j) {
            if (wave + ILV_NW * j >= 2 * NB2 || p2[j] >= P2) continue;
            const int y = y0 - 1 + p2[j] / R2W, x = x0 - 1 + p2[j] % R2W, c0 = cb * 16 + 4 * q;
            *reinterpret_cast<float4*>(A2s + p2[j] * 32 + c0) = ilv_affine_relu(acc2[j], s2 + c0, t2 + c0, y >= 0 && y < H && x >= 0 && x < Wc);
        }
        __syncthreads();
        // ---- its contribution to A3 on the tile: K = 9 taps x 32 channels
        const float* const w3 = W3 + (size_t)g3 * 4608 + l16 * 32 + 4 * q;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                acc3 = mfma_k16(*reinterpret_cast<const float4*>(w3 + tap * 512 + 16 * h),
                                 *reinterpret_cast<const float4*>(A2s + ao3 + ((tap / 3) * R2W + tap % 3) * 32 + 16 * h), acc3);
        }
    }
    // ---- A3 -> LDS (over the A1 image: its last readers passed the barrier after the last A2 finish), 1x1 head, store
    float* const A3s = A1s;
    *reinterpret_cast<float4*>(A3s + p3 * 16 + 4 * q) = ilv_affine_relu(acc3, s3 + 4 * q, t3 + 4 * q, true);
    __syncthreads();
    for (int e = tid; e < p.F * P3; e += ILV_NT) {
        const int f = e / P3, px = e % P3, y = y0 + px / TW, x = x0 + px % TW;
        if (y >= H || x >= Wc) continue;
        const float* const a = A3s + px * 16;
        const float* const w = W4 + f * 16;
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) sum = fmaf(w[c], a[c], sum);
        oplane[f * ofs + (size_t)y * W + x + i] = fmaxf(fmaf(sum, s4[f], t4[f]), 0.f);
    }
}

// the reference's layouts -> the packed block (see the head of this file)
__global__ __launch_bounds__(256) void interlaced_volume_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ w3,
                                                                      const float* __restrict__ w4, const float* __restrict__ s1, const float* __restrict__ t1,
                                                                      const float* __restrict__ s2, const float* __restrict__ t2, const float* __restrict__ s3,
                                                                      const float* __restrict__ t3, const float* __restrict__ s4, const float* __restrict__ t4,
                                                                      float* __restrict__ pk, int k2, int k3, int F, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int i = idx;
    float v;
    if (i < 1152) { const int t = i & 7, o = i >> 3 & 15, tap = i >> 7; v = w1[(o * 8 + t) * 9 + tap]; }                                   // [16,1,8,3,3]
    else if ((i -= 1152) < 4608 * k2) { const int c = i & 15, o = i >> 4 & 31, tap = i / 512 % 9, t = i / 4608; v = w2[((o * 16 + c) * k2 + t) * 9 + tap]; }   // [32,16,k2,3,3]
    else if ((i -= 4608 * k2) < 4608 * k3) { const int c = i & 31, o = i >> 5 & 15, tap = i / 512 % 9, t = i / 4608; v = w3[((o * 32 + c) * k3 + t) * 9 + tap]; }   // [16,32,k3,3,3]
    else if ((i -= 4608 * k3) < 16 * F) v = w4[i];                                                                                           // [F,16,1,1]
    else if ((i -= 16 * F) < 16) v = s1[i];
    else if ((i -= 16) < 16) v = t1[i];
    else if ((i -= 16) < 32) v = s2[i];
    else if ((i -= 32) < 32) v = t2[i];
    else if ((i -= 32) < 16) v = s3[i];
    else if ((i -= 16) < 16) v = t3[i];
    else if ((i -= 16) < F) v = s4[i];
    else v = t4[i - F];
    pk[idx] = v;
}

static int ilv_check_config(const char* who, int C, int k2, int k3, int F) {
    OSA_REQUIRE(ilv_supported(C, k2, k3), "%s: C = %d with depth kernels (%d, %d, %d) (supported: C = 32 with (8, 4, 2) and C = 96 with (8, 8, 3))", who, C, ILV_K1, k2, k3);
    OSA_REQUIRE(F >= 1 && F <= ILV_MAXF, "%s: %d output features (supported: 1 .. %d)", who, F, ILV_MAXF);
    return 0;
}

}  // namespace osa

using namespace osa;

extern "C" size_t osa_interlaced_volume_packed_floats(int C, int k2, int k3, int F) {
    return (ilv_supported(C, k2, k3) && F >= 1 && F <= ILV_MAXF) ? ilv_packed_floats(k2, k3, F) : 0;
}

extern "C" int osa_interlaced_volume_pack_f32(const float* w1, const float* w2, const float* w3, const float* w4, const float* scale1, const float* shift1,
                                              const float* scale2, const float* shift2, const float* scale3, const float* shift3, const float* scale4,
                                              const float* shift4, float* packed, int C, int k2, int k3, int F, void* stream) {
    OSA_REQUIRE(w1 && w2 && w3 && w4 && scale1 && shift1 && scale2 && shift2 && scale3 && shift3 && scale4 && shift4 && packed, "interlaced_volume_pack: NULL pointer");
    if (int rc = ilv_check_config("interlaced_volume_pack", C, k2, k3, F)) return rc;
    const int total = (int)ilv_packed_floats(k2, k3, F);
    hipLaunchKernelGGL(interlaced_volume_pack_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w1, w2, w3, w4, scale1, shift1, scale2, shift2,
                       scale3, shift3, scale4, shift4, packed, k2, k3, F, total);
    OSA_LAUNCH_CHECK("interlaced_volume_pack");
    return 0;
}

extern "C" int osa_interlaced_volume_f32(const float* featL, const float* featR, const float* packed, float* out, int B, int C, int H, int W, int D, int k2, int k3,
                                         int F, void* stream) {
    OSA_REQUIRE(featL && featR && packed && out, "interlaced_volume: NULL pointer");
    OSA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && D > 0, "interlaced_volume: bad dims");
    if (int rc = ilv_check_config("interlaced_volume", C, k2, k3, F)) return rc;
    OSA_REQUIRE((long long)B * C * H * W < (1ll << 31) && (long long)B * F * D * H * W < (1ll << 31), "interlaced_volume: a feature map or the volume has 2^31 elements or more");
    IlvArgs a{featL, featR, packed, out, B, C, H, W, D, F, cdiv(W, ILV_TW), cdiv(H, ILV_TH)};
    const long long blocks = (long long)B * D * a.nTx * a.nTy;
    OSA_REQUIRE(blocks <= 0x7fffffffLL, "interlaced_volume: grid too large");
    if (k3 == 2) hipLaunchKernelGGL((interlaced_volume_kernel<4, 2>), dim3((unsigned)blocks), dim3(ILV_NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((interlaced_volume_kernel<8, 3>), dim3((unsigned)blocks), dim3(ILV_NT), 0, (hipStream_t)stream, a);
    OSA_LAUNCH_CHECK("interlaced_volume");
    return 0;
}
