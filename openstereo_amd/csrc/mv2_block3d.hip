// MobileStereoNet's 3-D inverted-residual block (models/msnet/submodule.py:136-173, MobileV2_Residual_3D) in eval mode as ONE launch:
//
//   h1 = relu6(bn1(W1 x))              1x1x1 expansion   Ci -> Ch
//   h2 = relu6(bn2(dw3x3x3(h1)))       depthwise, stride 1 or 2, padding 1 (zeros around h1, NOT around x: relu6(shift1) != 0)
//   y  = bn3(W3 h2) (+ x)              1x1x1 projection  Ch -> Co
//
// x and y are fp32 NDHWC; h1 and h2 (expanse_ratio x the channels of x) never reach memory.  A workgroup of 8 waves owns a TH x TW tile
// of output pixels and walks along d.  Per INPUT plane it expands the tile's footprint ((TH-1) S + 3) x ((TW-1) S + 3) once, on
// v_mfma_f32_32x32x2_f32 (rows = footprint pixels, columns = hidden channels, K = Ci), into slot (plane mod 3) of an LDS ring; entries
// outside the volume are written as zeros, planes outside it are skipped by the taps.  Per OUTPUT plane the 27 taps run on the VALU: a
// work item is (4 hidden channels, WS = 4 or 2 neighbouring outputs of one output row); it reads each of its 9 ring row segments ONCE and
// keeps the WS partial sums in registers.  The result goes to an LDS stage [pixel][Ch] that the projection reads as the B operand of
// v_mfma_f32_16x16x4_f32 (rows = output channels, columns = pixels, K = Ch; 16 x 16 tiles so that 32 output channels of 64 pixels occupy
// all 8 waves), so a lane ends with 4 consecutive channels of a pixel: folded BN3, the residual and a 16-byte store.
// Exact fp32 everywhere (the MFMA is an fmaf chain), no atomics, every output voxel is computed by one lane in a fixed order: the bits do
// not depend on the batch size, on the chunking of d or on the run.
//
// K order of the expansion: a step of 8 channels is 4 MFMAs, lane half h (lane >> 5) supplies channels 8c + 4h + j (one float4 per
// operand); of the projection: 16 channels are 4 MFMAs, lane quarter q supplies 16c + 4q + j.
// LDS rows are Ch + 4 floats apart: 16-byte aligned, and neighbouring rows of an operand read start four banks apart.
//
// Tile per (Ch, S), ring + stage (+ the footprint's offset table) within 160 KiB:
//   S = 1: Ch <= 96: 8 x 8 (146 KB at 96)   Ch <= 128: 6 x 8 (152 KB)   Ch <= 256: 4 x 4 (129 KB)
//   S = 2: Ch <= 64: 4 x 8 (134 KB)         Ch <= 128: 4 x 4 (137 KB)   Ch <= 256: 2 x 4 (149 KB)
//
// Packed parameters (osa_mv2_block3d_pack_f32): the layout of mv2_common.h with T = 27; the folded-BN epilogues and the launcher's checks
// shared with the 2-D block are there too.
#include "mv2_common.h"
#include <algorithm>

namespace osa {

constexpr int MV2_NT = 512, MV2_MAX_CIO = 128, MV2_MAX_CH = 256;
typedef float mv2_f32x16 __attribute__((ext_vector_type(16)));

struct Mv2Args {
    const float* x; const float* pk; float* y;
    int B, D, H, W, Ci, Ch, Co, Do, Ho, Wo, res;
    int nTx, nTy, DCH, nCh;                  // tiles along w / h, output planes per workgroup, chunks of planes
};

__device__ __forceinline__ mv2_f32x16 mfma8(const float4 a, const float4 b, mv2_f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
}

template <int S, int TH, int TW>
struct Mv2Geo {
    static constexpr int FH = (TH - 1) * S + 3, FW = (TW - 1) * S + 3, FP = FH * FW, NPIX = TH * TW;
    static constexpr int WS = S == 2 ? 2 : (TW >= 8 ? 4 : TW);     // outputs per depthwise work item: enough items for 8 waves
    static constexpr int ITEMS_PER_QUAD = TH * (TW / WS);         // depthwise work items per quad of hidden channels
    static size_t lds_bytes(int Ch) { return ((size_t)(3 * FP + NPIX) * (Ch + 4) + FP) * sizeof(float); }
};

template <int S, int TH, int TW>
__global__ __launch_bounds__(MV2_NT) void mv2_block3d_kernel(const Mv2Args p) {
    using G = Mv2Geo<S, TH, TW>;
    constexpr int FW = G::FW, FP = G::FP, NPIX = G::NPIX, NWV = MV2_NT / 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Ci = p.Ci, Ch = p.Ch, Co = p.Co, CHP = Ch + 4;
    float* const ring = smem;                              // [3][FP][CHP]
    float* const stage = smem + 3 * FP * CHP;              // [NPIX][CHP]
    int* const inb = reinterpret_cast<int*>(stage + NPIX * CHP);   // [FP]: pixel offset inside an input plane, -1 outside the volume

    const float* const W1 = p.pk;
    const float* const s1 = W1 + (size_t)Ch * Ci; const float* const b1 = s1 + Ch;
    const float* const DW = b1 + Ch;
    const float* const s2 = DW + 27 * Ch; const float* const b2 = s2 + Ch;
    const float* const W3 = b2 + Ch;
    const float* const s3 = W3 + (size_t)Co * Ch; const float* const b3 = s3 + Co;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, half = lane >> 5;
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = bid % p.nTx; bid /= p.nTx;
    const int ty = bid % p.nTy; bid /= p.nTy;
    const int chunk = bid % p.nCh, b = bid / p.nCh;
    const int oy0 = ty * TH, ox0 = tx * TW, iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
    const int od0 = chunk * p.DCH, od1 = min(p.Do, od0 + p.DCH);

    for (int q = tid; q < FP; q += MV2_NT) {
        const int gy = iy0 + q / FW, gx = ix0 + q % FW;
        inb[q] = (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) ? gy * p.W + gx : -1;
    }
    __syncthreads();

    // ---- expansion of input plane pz into its ring slot: (32 footprint pixels) x (32 hidden channels) per MFMA tile
    auto expand = [&](int pz) {
        const float* const xpl = p.x + ((size_t)b * p.D + pz) * p.H * p.W * Ci;
        float* const slot = ring + (pz % 3) * FP * CHP;
        const int MT = (FP + 31) / 32, NTL = (Ch + 31) / 32;
        for (int t = wave; t < MT * NTL; t += NWV) {
            const int mt = t / NTL, nt = t - mt * NTL;
            const int q = mt * 32 + l32, off = q < FP ? inb[q] : -1;
            const int n = nt * 32 + l32, nc = min(n, Ch - 1);
            const float* ap = xpl + (size_t)max(off, 0) * Ci + 4 * half;
            const float* bp = W1 + (size_t)nc * Ci + 4 * half;
            mv2_f32x16 acc = {};
#pragma unroll 4
            for (int c = 0; c < Ci; c += 8) {
                const float4 a = off >= 0 ? ld4(ap + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                acc = mfma8(a, ld4(bp + c), acc);
            }
            const float sc = s1[nc], sh = b1[nc];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (qr < FP && n < Ch) slot[qr * CHP + n] = inb[qr] >= 0 ? relu6f(fmaf(acc[r], sc, sh)) : 0.f;
            }
        }
    };

    // ---- depthwise 3x3x3 of output plane od, ring -> stage: item = (4 hidden channels, WS outputs of one output row).  There are at
    // most MV2_NT items (the launcher checks), so a thread keeps ONE item for the whole walk and its 27 tap weights, scale and shift in registers.
    constexpr int WS = G::WS, FWS = (WS - 1) * S + 3;
    const int NQ = Ch >> 2, rs = tid / NQ, c4 = (tid - rs * NQ) * 4, r = rs % TH, ow0 = rs / TH * WS;
    const bool has_item = tid < NQ * G::ITEMS_PER_QUAD;
    float4 wt[27], sc2 = make_float4(0.f, 0.f, 0.f, 0.f), sh2 = sc2;
#pragma unroll
    for (int i = 0; i < 27; ++i) wt[i] = has_item ? ld4(DW + i * Ch + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_item) { sc2 = ld4(s2 + c4); sh2 = ld4(b2 + c4); }
    auto depthwise = [&](int od) {
        if (has_item) {
            float4 acc[WS];
#pragma unroll
            for (int i = 0; i < WS; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int kd = 0; kd < 3; ++kd) {
                const int pz = od * S + kd - 1;
                if (pz < 0 || pz >= p.D) continue;
                const float* const slot = ring + (pz % 3) * FP * CHP + c4;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const float4* const w = wt + (kd * 3 + kh) * 3;
                    const float* const row = slot + ((r * S + kh) * FW + ow0 * S) * CHP;
#pragma unroll
                    for (int fx = 0; fx < FWS; ++fx) {
                        const float4 v = ld4(row + fx * CHP);
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            if (fx - kw >= 0 && (fx - kw) % S == 0 && (fx - kw) / S < WS) {
                                float4& a = acc[(fx - kw) / S];
                                a.x = fmaf(v.x, w[kw].x, a.x); a.y = fmaf(v.y, w[kw].y, a.y);
                                a.z = fmaf(v.z, w[kw].z, a.z); a.w = fmaf(v.w, w[kw].w, a.w);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < WS; ++i) *reinterpret_cast<float4*>(stage + (r * TW + ow0 + i) * CHP + c4) = mv2_bn_relu6(acc[i], sc2, sh2);
        }
    };

    // ---- projection of output plane od, stage -> y: (16 output channels) x (16 pixels) per tile of v_mfma_f32_16x16x4_f32, so that 32
    // output channels of an 8 x 8 tile give every wave a tile; 16 channels of K are 4 MFMAs, lane quarter q supplies channels 16c + 4q + j
    auto project = [&](int od) {
        const int l16 = lane & 15, q4 = (lane >> 4) * 4;
        const int MT = (Co + 15) / 16, NTL = (NPIX + 15) / 16;
        for (int t = wave; t < MT * NTL; t += NWV) {
            const int mt = t / NTL, nt = t - mt * NTL;
            const int co = min(mt * 16 + l16, Co - 1), px = nt * 16 + l16;
            const float* ap = W3 + (size_t)co * Ch + q4;
            const float* bp = stage + min(px, NPIX - 1) * CHP + q4;
            osa_f32x4_t acc = {};
#pragma unroll 4
            for (int c = 0; c < Ch; c += 16) {
                const bool live = c + q4 < Ch;                 // Ch % 16 == 8: the last step has two quarters only
                acc = mfma_k16(live ? ld4(ap + c) : make_float4(0.f, 0.f, 0.f, 0.f), live ? ld4(bp + c) : make_float4(0.f, 0.f, 0.f, 0.f), acc);
            }
            const int oy = oy0 + px / TW, ox = ox0 + px % TW, c0 = mt * 16 + q4;
            if (px >= NPIX || oy >= p.Ho || ox >= p.Wo || c0 >= Co) continue;
            const float4 sc = ld4(s3 + c0), sh = ld4(b3 + c0);
            float4 v = mv2_bn(acc, sc, sh);
            if (p.res) {                                       // S == 1, Ci == Co
                const float4 xr = ld4(p.x + ((((size_t)b * p.D + od) * p.H + oy) * p.W + ox) * Ci + c0);
                v.x += xr.x; v.y += xr.y; v.z += xr.z; v.w += xr.w;
            }
            store16(p.y + ((((size_t)b * p.Do + od) * p.Ho + oy) * p.Wo + ox) * Co + c0, v);
        }
    };

    int next = max(od0 * S - 1, 0);                        // every input plane is expanded once, in ascending order
    for (int od = od0; od < od1; ++od) {
        for (const int hi = min(od * S + 1, p.D - 1); next <= hi; ++next) expand(next);
        __syncthreads();                                   // ring complete; the previous plane's projection has left the stage
        depthwise(od);
        __syncthreads();                                   // stage complete; the ring slots the next expansion overwrites are free
        project(od);
    }
}

template <int S, int TH, int TW>
static int mv2_launch(Mv2Args a, hipStream_t st) {
    using G = Mv2Geo<S, TH, TW>;
    const size_t lds = G::lds_bytes(a.Ch);
    OSA_REQUIRE(lds <= 160 * 1024, "mv2_block3d: %zu bytes of LDS for %d hidden channels", lds, a.Ch);
    OSA_REQUIRE(a.Ch / 4 * G::ITEMS_PER_QUAD <= MV2_NT, "mv2_block3d: %d depthwise work items for %d threads", a.Ch / 4 * G::ITEMS_PER_QUAD, MV2_NT);
    a.nTx = cdiv(a.Wo, TW); a.nTy = cdiv(a.Ho, TH);
    // a walk of all planes by few workgroups leaves CUs idle: cut d into chunks for about 1024 workgroups, at least 8 planes each
    // (a chunk re-expands the one or two input planes below its first output plane)
    const long long tiles = (long long)a.B * a.nTx * a.nTy;
    const int nch = (int)std::max<long long>(1, std::min<long long>(1024 / tiles, a.Do / 8));
    a.DCH = cdiv(a.Do, nch); a.nCh = cdiv(a.Do, a.DCH);
    OSA_REQUIRE(tiles * a.nCh <= 0x7fffffffLL, "mv2_block3d: grid too large");
    if (int rc = mv2_allow_lds<mv2_block3d_kernel<S, TH, TW>>("mv2_block3d", 160 * 1024)) return rc;
    hipLaunchKernelGGL((mv2_block3d_kernel<S, TH, TW>), dim3((unsigned)(tiles * a.nCh)), dim3(MV2_NT), lds, st, a);
    OSA_LAUNCH_CHECK("mv2_block3d");
    return 0;
}

}  // namespace osa

using namespace osa;

extern "C" size_t osa_mv2_block3d_packed_floats(int Ci, int Ch, int Co) {
    return (Ci > 0 && Ch > 0 && Co > 0) ? mv2_packed_floats(27, Ci, Ch, Co) : 0;
}

extern "C" int osa_mv2_block3d_pack_f32(const float* w_expand, const float* w_dw, const float* w_project, const float* scale1, const float* shift1,
                                        const float* scale2, const float* shift2, const float* scale3, const float* shift3, float* packed,
                                        int Ci, int Ch, int Co, void* stream) {
    return mv2_pack<27>("mv2_block3d_pack", w_expand, w_dw, w_project, scale1, shift1, scale2, shift2, scale3, shift3, packed, Ci, Ch, Co, MV2_MAX_CIO, MV2_MAX_CH,
                        (hipStream_t)stream);
}

extern "C" int osa_mv2_block3d_f32(const float* x, const float* packed, float* y, int B, int D, int H, int W, int Ci, int Ch, int Co, int stride, int residual,
                                   void* stream) {
    OSA_REQUIRE(x && packed && y, "mv2_block3d: NULL pointer");
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "mv2_block3d: bad dims");
    if (int rc = mv2_check_block("mv2_block3d", stride, Ci, Ch, Co, residual, MV2_MAX_CIO, MV2_MAX_CH)) return rc;
    Mv2Args a{x, packed, y, B, D, H, W, Ci, Ch, Co, (D - 1) / stride + 1, (H - 1) / stride + 1, (W - 1) / stride + 1, residual ? 1 : 0, 0, 0, 0, 0};
    OSA_REQUIRE((long long)B * D * H * W * Ci < (1ll << 31) && (long long)B * a.Do * a.Ho * a.Wo * Co < (1ll << 31),
                "mv2_block3d: x or y has 2^31 elements or more");
    const hipStream_t st = (hipStream_t)stream;
    if (stride == 1) return Ch <= 96 ? mv2_launch<1, 8, 8>(a, st) : Ch <= 128 ? mv2_launch<1, 6, 8>(a, st) : mv2_launch<1, 4, 4>(a, st);
    return Ch <= 64 ? mv2_launch<2, 4, 8>(a, st) : Ch <= 128 ? mv2_launch<2, 4, 4>(a, st) : mv2_launch<2, 2, 4>(a, st);
}
