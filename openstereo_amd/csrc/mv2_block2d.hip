// MobileStereoNet's 2-D inverted-residual block (models/msnet/submodule.py:94-133, MobileV2_Residual) in eval mode as ONE launch:
//
//   h1 = relu6(bn1(W1 x))              1x1 expansion   Ci -> Ch
//   h2 = relu6(bn2(dw3x3(h1)))         depthwise, stride 1 or 2, padding 1 (zeros around h1, NOT around x: relu6(shift1) != 0)
//   y  = bn3(W3 h2) (+ x) (+ addend)   1x1 projection  Ch -> Co, then the optional ReLU of the caller
//
// x, y and addend are fp32 NHWC; h1 and h2 never reach memory.  A workgroup of 8 waves owns a TH x TW tile of output pixels.  It copies
// the tile's footprint ((TH-1) S + 3) x ((TW-1) S + 3) of x into LDS ONCE (zeros outside the map) and then loops over chunks of
// MV2D_CK = 48 hidden channels, so LDS does not grow with Ch:
//   a. the chunk's rows of W1 go to LDS;
//   b. expansion on v_mfma_f32_16x16x4_f32: rows = hidden channels of the chunk, columns = footprint pixels, K = Ci; a lane ends with 4
//      consecutive channels of a pixel: folded BN1, ReLU6 (or zero outside the map) and one 16-byte LDS store into h1 [pixel][chunk];
//   c. the chunk's columns of W3 go to LDS, and the 9 taps run on the VALU: a work item is (4 hidden channels, WS = 4 or 2 neighbouring
//      outputs of one row), reads each of its 3 h1 row segments once and writes relu6(bn2(.)) into the stage [output pixel][chunk];
//   d. projection on v_mfma_f32_16x16x4_f32: rows = output channels, columns = output pixels, K = the chunk.  The accumulators of a
//      wave's tiles live in registers ACROSS the chunks, so K = Ch is summed chunk by chunk in a fixed order.
// Three barriers per chunk (after a, b and c): W1 is restaged while slower waves still project, W3 and the stage only after every wave
// has left the projection (it passed the barrier after b).  After the last chunk a lane holds 4 consecutive output channels of a pixel:
// folded BN3, the residual (from the LDS copy of x), the addend, the ReLU and a 16-byte store.
// Exact fp32 everywhere (the MFMA is an fmaf chain), no atomics, every output element is computed by one lane in a fixed order: the bits
// do not depend on the batch size or on the run.
//
// K order of both products: 16 channels are 4 MFMAs, lane quarter q (lane >> 4) supplies channels 16c + 4q + j (one float4 per operand);
// a K that is 8 modulo 16 ends with two live quarters.  LDS rows are K + 4 floats apart: 16-byte aligned, and the 16 rows an operand
// read touches start on 16 different multiples of four banks.
//
// Tiles (the launcher takes the first whose LDS fits 160 KiB and that gives at least 128 workgroups, else the last):
//   S = 1: 8 x 16, 4 x 8, 4 x 4        S = 2: 4 x 8, 4 x 4          x is read footprint / tile times: 1.41, 1.88, 2.25 | 1.20, 1.27
// LDS floats: FP (Ci + 4) + FP 52 + TH TW 52 + 48 (Ci + 4) + Co 52 + FP   (FP = footprint pixels); DESIGN.md 3.4e has the table.
//
// Packed parameters (osa_mv2_block2d_pack_f32): the layout of mv2_common.h with T = 9; the folded-BN epilogues and the launcher's checks
// shared with the 3-D block are there too.
#include "mv2_common.h"

namespace osa {

constexpr int MV2D_NT = 512, MV2D_NWV = MV2D_NT / 64, MV2D_MAX_CIO = 192, MV2D_MAX_CH = 384, MV2D_CK = 48, MV2D_CKP = MV2D_CK + 4;
constexpr size_t MV2D_MAX_LDS = 160 * 1024;
constexpr long long MV2D_MIN_WG = 128;                      // a tile that leaves fewer workgroups than this gives way to a smaller one

struct Mv2dArgs {
    const float* x; const float* pk; const float* add; float* y;
    int B, H, W, Ci, Ch, Co, Ho, Wo, res, relu;
    int nTx, nTy;                                           // tiles along w / h
};

template <int S, int TH, int TW>
struct Mv2dGeo {
    static constexpr int FH = (TH - 1) * S + 3, FW = (TW - 1) * S + 3, FP = FH * FW, NPIX = TH * TW;
    static constexpr int WS = S == 2 ? 2 : 4;                       // outputs per depthwise work item
    static constexpr int NTF = (FP + 15) / 16, NTP = (NPIX + 15) / 16;   // MFMA column tiles of the footprint / of the outputs
    static constexpr int PT = (MV2D_MAX_CIO / 16 * NTP + MV2D_NWV - 1) / MV2D_NWV;   // projection tiles a wave can own
    static size_t lds_bytes(int Ci, int Co) {
        return ((size_t)FP * (Ci + 4) + (size_t)(FP + NPIX) * MV2D_CKP + (size_t)MV2D_CK * (Ci + 4) + (size_t)Co * MV2D_CKP + FP) * sizeof(float);
    }
};

template <int S, int TH, int TW>
__global__ __launch_bounds__(MV2D_NT) void mv2_block2d_kernel(const Mv2dArgs p) {
    using G = Mv2dGeo<S, TH, TW>;
    constexpr int FW = G::FW, FP = G::FP, NPIX = G::NPIX, CK = MV2D_CK, CKP = MV2D_CKP, NT = MV2D_NT, NWV = MV2D_NWV;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Ci = p.Ci, Ch = p.Ch, Co = p.Co, CIP = Ci + 4, CI4 = Ci >> 2;
    float* const xs = smem;                                 // [FP][CIP]   the footprint of x, zeros outside the map
    float* const h1 = xs + FP * CIP;                        // [FP][CKP]   the chunk of the hidden tensor, zeros outside the map
    float* const stage = h1 + FP * CKP;                     // [NPIX][CKP] the chunk after the depthwise convolution
    float* const w1s = stage + NPIX * CKP;                  // [CK][CIP]   the chunk's rows of W1
    float* const w3s = w1s + CK * CIP;                      // [Co][CKP]   the chunk's columns of W3
    int* const inb = reinterpret_cast<int*>(w3s + Co * CKP);   // [FP]: 1 inside the map

    const float* const W1 = p.pk;
    const float* const s1 = W1 + (size_t)Ch * Ci; const float* const b1 = s1 + Ch;
    const float* const DW = b1 + Ch;
    const float* const s2 = DW + 9 * Ch; const float* const b2 = s2 + Ch;
    const float* const W3 = b2 + Ch;
    const float* const s3 = W3 + (size_t)Co * Ch; const float* const b3 = s3 + Co;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q4 = (lane >> 4) * 4;
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = bid % p.nTx; bid /= p.nTx;
    const int ty = bid % p.nTy, b = bid / p.nTy;
    const int oy0 = ty * TH, ox0 = tx * TW, iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int i = tid; i < FP * CI4; i += NT) {
        const int q = i / CI4, c = (i - q * CI4) * 4, gy = iy0 + q / FW, gx = ix0 + q % FW;
        const bool in = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        *reinterpret_cast<float4*>(xs + q * CIP + c) = in ? ld4(p.x + (((size_t)b * p.H + gy) * p.W + gx) * Ci + c) : zero4;
        if (c == 0) inb[q] = in ? 1 : 0;
    }

    // the projection tiles of this wave: tile t = wave + NWV i is (16 output channels mt) x (16 output pixels nt)
    const int ntiles = ((Co + 15) >> 4) * G::NTP;
    osa_f32x4_t acc[G::PT];
#pragma unroll
    for (int i = 0; i < G::PT; ++i) acc[i] = osa_f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int ch0 = 0; ch0 < Ch; ch0 += CK) {
        const int ckl = min(CK, Ch - ch0), NQ = ckl >> 2;

        // ---- a. W1 rows ch0 .. ch0 + ckl
        for (int i = tid; i < ckl * CI4; i += NT) {
            const int n = i / CI4, c = (i - n * CI4) * 4;
            *reinterpret_cast<float4*>(w1s + n * CIP + c) = ld4(W1 + (size_t)(ch0 + n) * Ci + c);
        }
        __syncthreads();

        // ---- b. expansion, xs x w1s -> h1
        for (int t = wave; t < ((ckl + 15) >> 4) * G::NTF; t += NWV) {
            const int mt = t / G::NTF, nt = t - mt * G::NTF;
            const float* const ap = w1s + min(mt * 16 + l16, ckl - 1) * CIP + q4;
            const float* const bp = xs + min(nt * 16 + l16, FP - 1) * CIP + q4;
            osa_f32x4_t e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
            for (int c = 0; c < Ci; c += 16) {
                const bool live = c + q4 < Ci;              // Ci % 16 == 8: the last step has two quarters only
                e = mfma_k16(live ? ld4(ap + c) : zero4, live ? ld4(bp + c) : zero4, e);
            }
            const int c0 = mt * 16 + q4, q = nt * 16 + l16;
            if (c0 < ckl && q < FP) {
                const float4 sc = ld4(s1 + ch0 + c0), sh = ld4(b1 + ch0 + c0);
                *reinterpret_cast<float4*>(h1 + q * CKP + c0) = inb[q] ? mv2_bn_relu6(e, sc, sh) : zero4;
            }
        }
        __syncthreads();

        // ---- c. W3 columns ch0 .. ch0 + ckl; depthwise 3x3, h1 -> stage: item = (4 hidden channels, WS outputs of one output row)
        for (int i = tid; i < Co * NQ; i += NT) {
            const int co = i / NQ, c = (i - co * NQ) * 4;
            *reinterpret_cast<float4*>(w3s + co * CKP + c) = ld4(W3 + (size_t)co * Ch + ch0 + c);
        }
        constexpr int WS = G::WS, FWS = (WS - 1) * S + 3;
        for (int it = tid; it < NQ * TH * (TW / WS); it += NT) {
            const int rs = it / NQ, c4 = (it - rs * NQ) * 4, r = rs % TH, ow0 = rs / TH * WS;
            const float* const dw = DW + ch0 + c4;
            float4 a[WS];
#pragma unroll
            for (int i = 0; i < WS; ++i) a[i] = zero4;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const float4 w[3] = {ld4(dw + (kh * 3) * Ch), ld4(dw + (kh * 3 + 1) * Ch), ld4(dw + (kh * 3 + 2) * Ch)};
                const float* const row = h1 + ((r * S + kh) * FW + ow0 * S) * CKP + c4;
#pragma unroll
                for (int fx = 0; fx < FWS; ++fx) {
                    const float4 v = ld4(row + fx * CKP);
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        if (fx - kw >= 0 && (fx - kw) % S == 0 && (fx - kw) / S < WS) {
                            float4& o = a[(fx - kw) / S];
                            o.x = fmaf(v.x, w[kw].x, o.x); o.y = fmaf(v.y, w[kw].y, o.y);
                            o.z = fmaf(v.z, w[kw].z, o.z); o.w = fmaf(v.w, w[kw].w, o.w);
                        }
                    }
                }
            }
            const float4 sc = ld4(s2 + ch0 + c4), sh = ld4(b2 + ch0 + c4);
#pragma unroll
            for (int i = 0; i < WS; ++i) *reinterpret_cast<float4*>(stage + (r * TW + ow0 + i) * CKP + c4) = mv2_bn_relu6(a[i], sc, sh);
        }
        __syncthreads();

        // ---- d. projection, stage x w3s, accumulated over the chunks
#pragma unroll
        for (int i = 0; i < G::PT; ++i) {
            const int t = wave + NWV * i;
            if (t < ntiles) {
                const int mt = t / G::NTP, nt = t - mt * G::NTP;
                const float* const ap = w3s + min(mt * 16 + l16, Co - 1) * CKP + q4;
                const float* const bp = stage + min(nt * 16 + l16, NPIX - 1) * CKP + q4;
#pragma unroll
                for (int c = 0; c < CK; c += 16) {
                    const bool live = c + q4 < ckl;         // the last chunk may be short, and 8 modulo 16
                    acc[i] = mfma_k16(live ? ld4(ap + c) : zero4, live ? ld4(bp + c) : zero4, acc[i]);
                }
            }
        }
    }

    // ---- folded BN3, residual, addend, ReLU: 4 consecutive output channels of one pixel per lane and tile
#pragma unroll
    for (int i = 0; i < G::PT; ++i) {
        const int t = wave + NWV * i;
        if (t >= ntiles) continue;
        const int mt = t / G::NTP, nt = t - mt * G::NTP, px = nt * 16 + l16, c0 = mt * 16 + q4;
        const int r = px / TW, cx = px - r * TW, oy = oy0 + r, ox = ox0 + cx;
        if (px >= NPIX || oy >= p.Ho || ox >= p.Wo || c0 >= Co) continue;
        const float4 sc = ld4(s3 + c0), sh = ld4(b3 + c0);
        float4 v = mv2_bn(acc[i], sc, sh);
        if (p.res) {                                        // S == 1, Ci == Co: x + y, from the LDS copy of x
            const float4 xr = ld4(xs + ((r + 1) * FW + cx + 1) * CIP + c0);
            v.x = xr.x + v.x; v.y = xr.y + v.y; v.z = xr.z + v.z; v.w = xr.w + v.w;
        }
        const size_t off = ((((size_t)b * p.Ho + oy) * p.Wo + ox) * Co) + c0;
        if (p.add) {
            const float4 ad = ld4(p.add + off);
            v.x += ad.x; v.y += ad.y; v.z += ad.z; v.w += ad.w;
        }
        if (p.relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
        store16(p.y + off, v);
    }
}

template <int S, int TH, int TW>
static bool mv2d_tile_fits(const Mv2dArgs& a, long long min_wg) {
    using G = Mv2dGeo<S, TH, TW>;
    return G::lds_bytes(a.Ci, a.Co) <= MV2D_MAX_LDS && (long long)a.B * cdiv(a.Wo, TW) * cdiv(a.Ho, TH) >= min_wg;
}

template <int S, int TH, int TW>
static int mv2d_launch(Mv2dArgs a, hipStream_t st) {
    using G = Mv2dGeo<S, TH, TW>;
    const size_t lds = G::lds_bytes(a.Ci, a.Co);
    OSA_REQUIRE(lds <= MV2D_MAX_LDS, "mv2_block2d: %zu bytes of LDS for channels %d -> %d -> %d", lds, a.Ci, a.Ch, a.Co);
    a.nTx = cdiv(a.Wo, TW); a.nTy = cdiv(a.Ho, TH);
    const long long wgs = (long long)a.B * a.nTx * a.nTy;
    OSA_REQUIRE(wgs <= 0x7fffffffLL, "mv2_block2d: grid too large");
    if (int rc = mv2_allow_lds<mv2_block2d_kernel<S, TH, TW>>("mv2_block2d", (int)MV2D_MAX_LDS)) return rc;
    hipLaunchKernelGGL((mv2_block2d_kernel<S, TH, TW>), dim3((unsigned)wgs), dim3(MV2D_NT), lds, st, a);
    OSA_LAUNCH_CHECK("mv2_block2d");
    return 0;
}

}  // namespace osa

using namespace osa;

extern "C" size_t osa_mv2_block2d_packed_floats(int Ci, int Ch, int Co) {
    return (Ci > 0 && Ch > 0 && Co > 0) ? mv2_packed_floats(9, Ci, Ch, Co) : 0;
}

extern "C" int osa_mv2_block2d_pack_f32(const float* w_expand, const float* w_dw, const float* w_project, const float* scale1, const float* shift1,
                                        const float* scale2, const float* shift2, const float* scale3, const float* shift3, float* packed,
                                        int Ci, int Ch, int Co, void* stream) {
    return mv2_pack<9>("mv2_block2d_pack", w_expand, w_dw, w_project, scale1, shift1, scale2, shift2, scale3, shift3, packed, Ci, Ch, Co, MV2D_MAX_CIO, MV2D_MAX_CH,
                       (hipStream_t)stream);
}

extern "C" int osa_mv2_block2d_f32(const float* x, const float* packed, const float* addend, float* y, int B, int H, int W, int Ci, int Ch, int Co, int stride,
                                   int residual, int relu, void* stream) {
    OSA_REQUIRE(x && packed && y, "mv2_block2d: NULL pointer");
    OSA_REQUIRE(B > 0 && H > 0 && W > 0, "mv2_block2d: bad dims");
    if (int rc = mv2_check_block("mv2_block2d", stride, Ci, Ch, Co, residual, MV2D_MAX_CIO, MV2D_MAX_CH)) return rc;
    Mv2dArgs a{x, packed, addend, y, B, H, W, Ci, Ch, Co, (H - 1) / stride + 1, (W - 1) / stride + 1, residual ? 1 : 0, relu ? 1 : 0, 0, 0};
    const long long nx = (long long)B * H * W * Ci, ny = (long long)B * a.Ho * a.Wo * Co;
    OSA_REQUIRE(nx < (1ll << 31) && ny < (1ll << 31), "mv2_block2d: x or y has 2^31 elements or more");
    const uintptr_t px = (uintptr_t)x, py = (uintptr_t)y, pa = (uintptr_t)addend, bx = (uintptr_t)nx * sizeof(float), by = (uintptr_t)ny * sizeof(float);
    OSA_REQUIRE((py + by <= px || px + bx <= py) && (!addend || py + by <= pa || pa + by <= py), "mv2_block2d: y overlaps x or addend");
    const hipStream_t st = (hipStream_t)stream;
    if (stride == 1) {
        if (mv2d_tile_fits<1, 8, 16>(a, MV2D_MIN_WG)) return mv2d_launch<1, 8, 16>(a, st);
        if (mv2d_tile_fits<1, 4, 8>(a, MV2D_MIN_WG)) return mv2d_launch<1, 4, 8>(a, st);
        return mv2d_launch<1, 4, 4>(a, st);
    }
    if (mv2d_tile_fits<2, 4, 8>(a, MV2D_MIN_WG)) return mv2d_launch<2, 4, 8>(a, st);
    return mv2d_launch<2, 4, 4>(a, st);
}
