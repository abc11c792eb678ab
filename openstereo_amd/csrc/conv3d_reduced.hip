// FoundationStereo's Conv3dNormActReduced (foundationstereo/core/submodule.py:87-112, fast_foundationstereo/core/submodule.py:90-115) in
// eval mode as ONE launch:
//
//   h = relu(s1 * conv_{1 x ks x ks}(x) + t1)          hidden, Ch channels, never in memory
//   y = relu(s2 * conv_{kd x 1 x 1}(h) + t2)           over the disparity axis; h is ZERO outside [0, D) (not relu(t1))
//
// with both BatchNorms (running statistics) and both convolution biases folded into s* / t* by the pack launch.
//
// A workgroup of 4 waves owns an 8 x 16 pixel tile (and one segment of D) and marches through the planes; a wave owns 2 x 16 pixels, the
// N of v_mfma_f32_32x32x2_f32, and the output channels are M.  Both weight sets stay in LDS, every tap a zero-padded 32 x 32 matrix packed
// [in / 4][out = 32][in % 4] as in disparity_attention.hip: float4 number 64 g + lane is a lane's A operand of K steps 4g .. 4g+3, which
// are the channels 8g + 4hh + j of lane half hh = lane >> 5.
//   conv1: the plane's 10 x 18 halo tile lies in LDS channels-last with a pixel stride of 36 floats (zero outside the map and on the pad
//          channels), double buffered: the next plane is loaded to registers before the products and stored behind them, ONE barrier per
//          plane.  The B operand of steps 4g .. 4g+3 is one float4 of the pixel at the tap's offset.
//   conv2: the hidden plane leaves conv1 in the accumulator layout -- the lane holds pixel (lane & 31), register r the channel
//          (r & 3) + 8 (r >> 2) + 4 hh -- which IS the B operand of the next product for weights packed as above, so the
//          window of the last 17 hidden planes is an array of 17 x 16 registers, indexed at compile time and shifted by register moves
//          once per plane.  Tap t of a kd-tap kernel reads window slot 17 - kd + t; taps whose plane lies outside [0, D) are skipped
//          (wave-uniform), which is what makes those planes zero.
// Output plane o is complete when hidden plane o + kd / 2 is in the window.  D may be cut into segments (the launcher does so when the
// pixel tiles alone leave most of the GPU idle); a segment recomputes the kd - 1 hidden planes around it and sums every output in the
// same order, so the bits do not depend on the cut.  Exact fp32 (the MFMA is an fmaf chain), no atomics, a fixed order: the bits do not
// depend on the batch size, the memory format or the run.
//
// Packed parameters (osa_conv3d_reduced_pack_f32), (ks * ks + kd) * 1024 + 128 floats:
//   W1 [ks * ks][8][32][4] | W2 [kd][8][32][4] | s1 [32] | t1 [32] | s2 [32] | t2 [32]
#include "mv2_common.h"

namespace osa {

typedef float cr_f32x16 __attribute__((ext_vector_type(16)));

constexpr int CR_NT = 256, CR_TH = 8, CR_TW = 16, CR_HW = CR_TW + 2, CR_PIX = (CR_TH + 2) * CR_HW, CR_PS = 36, CR_BUF = CR_PIX * CR_PS;
constexpr int CR_MAT = 1024, CR_VEC = 32, CR_WIN = 17, CR_ELEMS = CR_PIX * 8, CR_LD = (CR_ELEMS + CR_NT - 1) / CR_NT, CR_CUS = 256;
constexpr size_t CR_MAX_LDS = 160 * 1024;

static inline size_t cr_packed_floats(int ks, int kd) { return (size_t)(ks * ks + kd) * CR_MAT + 4 * CR_VEC; }

struct CrArgs {
    const float* x; const float* pk; float* y;
    int cl;                                                 // 1: [B,D,H,W,C], 0: [B,C,D,H,W]
    int Ci, Ch, Co, ks, kd, D, H, W, tiles_x, tiles_y, nseg, seg;   // seg: output planes per segment
};

// register r = vec[(r & 3) + 8 (r >> 2) + 4 hh]: a per-channel vector in the accumulator's form
__device__ __forceinline__ cr_f32x16 cr_rows(const float* vec, int hh) {
    cr_f32x16 o;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v = ld4(vec + 8 * g + 4 * hh);
        o[4 * g] = v.x; o[4 * g + 1] = v.y; o[4 * g + 2] = v.z; o[4 * g + 3] = v.w;
    }
    return o;
}

__device__ __forceinline__ cr_f32x16 cr_zero() {
    cr_f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    return o;
}

__global__ __launch_bounds__(CR_NT) void conv3d_reduced_kernel(const CrArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pix = lane & 31, hh = lane >> 5;
    const int ks = p.ks, kd = p.kd, D = p.D, H = p.H, W = p.W, Ci = p.Ci, Ch = p.Ch, Co = p.Co;
    const int nw = (ks * ks + kd) * CR_MAT + 4 * CR_VEC;
    const float* const w1 = smem;
    const float* const w2 = smem + ks * ks * CR_MAT;
    const float* const vec = w2 + kd * CR_MAT;
    float* const buf = smem + nw;
    for (int i = tid; i < nw / 4; i += CR_NT) reinterpret_cast<float4*>(smem)[i] = ld4(p.pk + (size_t)i * 4);

    int t = blockIdx.x;
    const int sg = t % p.nseg; t /= p.nseg;
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y, b = t / p.tiles_y;
    const int y0 = ty * CR_TH, x0 = tx * CR_TW, pad = kd / 2;
    const int o_lo = sg * p.seg, o_hi = min(D, o_lo + p.seg);          // this workgroup's output planes
    const int d_lo = max(0, o_lo - pad), d_hi = min(D, o_hi + pad);    // the hidden planes they read
    const long long HWl = (long long)H * W;
    const long long cs = p.cl ? 1 : (long long)D * HWl, ps = p.cl ? HWl * Ci : HWl;   // channel and plane strides of x

    // the halo tile as CR_ELEMS float4 (pixel, four channels); this thread's share: where it comes from (plane 0) and where it goes
    long long goff[CR_LD];
    int loff[CR_LD];
#pragma unroll
    for (int k = 0; k < CR_LD; ++k) {
        const int e = tid + k * CR_NT;
        const int hp = p.cl ? e >> 3 : e % CR_PIX, cg = p.cl ? e & 7 : e / CR_PIX;   // consecutive lanes: channels (NDHWC) or pixels (NCDHW)
        const int gy = y0 - 1 + hp / CR_HW, gx = x0 - 1 + hp % CR_HW;
        loff[k] = e < CR_ELEMS ? hp * CR_PS + 4 * cg : -1;
        goff[k] = -1;
        if (e < CR_ELEMS && gy >= 0 && gy < H && gx >= 0 && gx < W && 4 * cg < Ci)
            goff[k] = p.cl ? (((long long)b * D * H + gy) * W + gx) * Ci + 4 * cg : (((long long)b * Ci + 4 * cg) * D * H + gy) * W + gx;
    }
    auto load_plane = [&](int d, float4* v) {
#pragma unroll
        for (int k = 0; k < CR_LD; ++k) {
            v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (goff[k] >= 0) {
                const float* s = p.x + goff[k] + d * ps;
                v[k] = p.cl ? ld4(s) : make_float4(s[0], s[cs], s[2 * cs], s[3 * cs]);
            }
        }
    };
    auto store_plane = [&](float* dst, const float4* v) {
#pragma unroll
        for (int k = 0; k < CR_LD; ++k)
            if (loff[k] >= 0) *reinterpret_cast<float4*>(dst + loff[k]) = v[k];
    };
    {
        float4 v[CR_LD];
        load_plane(d_lo, v);
        store_plane(buf + (d_lo & 1) * CR_BUF, v);
    }
    __syncthreads();

    const int py = 2 * wave + (pix >> 4), px = pix & 15;                // this lane's pixel of the tile
    const bool live = y0 + py < H && x0 + px < W;
    const int xoff = ((py + (ks == 3 ? 0 : 1)) * CR_HW + px + (ks == 3 ? 0 : 1)) * CR_PS + 4 * hh;   // tap (0, 0) of this pixel in the halo tile
    const long long ybase = p.cl ? (((long long)b * D * H + y0 + py) * W + x0 + px) * Co : ((long long)b * Co * D * H + y0 + py) * W + x0 + px;
    const long long ycs = p.cl ? 1 : (long long)D * HWl, yps = p.cl ? HWl * Co : HWl;

    cr_f32x16 win[CR_WIN];
#pragma unroll
    for (int i = 0; i < CR_WIN; ++i) win[i] = cr_zero();

    for (int dd = d_lo; dd < o_hi + pad; ++dd) {                        // win[i] = hidden plane dd - 16 + i
        float4 v[CR_LD];
        const bool more = dd + 1 < d_hi;
        if (more) load_plane(dd + 1, v);
#pragma unroll
        for (int i = 0; i + 1 < CR_WIN; ++i) win[i] = win[i + 1];
        win[CR_WIN - 1] = cr_zero();
        if (dd < D) {
            cr_f32x16 acc = cr_zero();
            const float* const xb = buf + (dd & 1) * CR_BUF + xoff;
            for (int dy = 0; dy < ks; ++dy)
                for (int dx = 0; dx < ks; ++dx) {
                    const float* const wt = w1 + (dy * ks + dx) * CR_MAT + lane * 4;
                    const float* const xt = xb + (dy * CR_HW + dx) * CR_PS;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (8 * g < Ci) {
                            const float4 a = ld4(wt + 256 * g), x4 = ld4(xt + 8 * g);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, x4.x, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, x4.y, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, x4.z, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, x4.w, acc, 0, 0, 0);
                        }
                }
            const cr_f32x16 s1 = cr_rows(vec, hh), t1 = cr_rows(vec + CR_VEC, hh);   // zero on the pad channels
#pragma unroll
            for (int r = 0; r < 16; ++r) win[CR_WIN - 1][r] = fmaxf(fmaf(acc[r], s1[r], t1[r]), 0.f);
        }
        const int o = dd - pad;
        if (o >= o_lo) {
            cr_f32x16 acc = cr_zero();
#pragma unroll
            for (int j = 0; j < CR_WIN; ++j) {
                const int tap = j - (CR_WIN - kd), pl = dd - (CR_WIN - 1) + j;
                if (tap >= 0 && pl >= 0 && pl < D) {                    // wave-uniform
                    const float* const wt = w2 + tap * CR_MAT + lane * 4;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (8 * g < Ch) {
                            const float4 a = ld4(wt + 256 * g);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, win[j][4 * g], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, win[j][4 * g + 1], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, win[j][4 * g + 2], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, win[j][4 * g + 3], acc, 0, 0, 0);
                        }
                }
            }
            const cr_f32x16 s2 = cr_rows(vec + 2 * CR_VEC, hh), t2 = cr_rows(vec + 3 * CR_VEC, hh);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = fmaxf(fmaf(acc[r], s2[r], t2[r]), 0.f);
            float* const yo = p.y + ybase + o * yps;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = 8 * g + 4 * hh;
                if (live && c0 < Co) {                                  // Co is a multiple of 4
                    if (p.cl) store16(yo + c0, make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]));
                    else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) yo[(c0 + j) * ycs] = acc[4 * g + j];
                    }
                }
            }
        }
        if (more) store_plane(buf + ((dd + 1) & 1) * CR_BUF, v);
        __syncthreads();                                                // plane dd + 1 is in LDS; nobody reads plane dd any more
    }
}

// one thread per packed float.  The weights in the reference's layouts: w1 [Ch,Ci,1,ks,ks], w2 [Co,Ch,kd,1,1]; scale / shift are the
// eval-mode BatchNorm folds (y = x * scale + shift), b1 / b2 the convolutions' biases: t = shift + b * scale
__global__ __launch_bounds__(256) void conv3d_reduced_pack_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ scale1,
                                                                   const float* __restrict__ shift1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                                   const float* __restrict__ scale2, const float* __restrict__ shift2, float* __restrict__ pk, int Ci,
                                                                   int Ch, int Co, int ks2, int kd, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float v = 0.f;
    if (idx < (ks2 + kd) * CR_MAT) {
        const int m = idx / CR_MAT, e = idx - m * CR_MAT, in = (e >> 7) * 4 + (e & 3), out = (e >> 2) & 31;
        if (m < ks2) { if (out < Ch && in < Ci) v = w1[((size_t)out * Ci + in) * ks2 + m]; }
        else if (out < Co && in < Ch) v = w2[((size_t)out * Ch + in) * kd + (m - ks2)];
    } else {
        const int i = idx - (ks2 + kd) * CR_MAT, k = i / CR_VEC, c = i - k * CR_VEC;
        if (k == 0) { if (c < Ch) v = scale1[c]; }
        else if (k == 1) { if (c < Ch) v = fmaf(b1[c], scale1[c], shift1[c]); }
        else if (k == 2) { if (c < Co) v = scale2[c]; }
        else if (c < Co) v = fmaf(b2[c], scale2[c], shift2[c]);
    }
    pk[idx] = v;
}

static inline bool cr_supported(int Ci, int Ch, int Co, int ks, int kd) {
    const auto ch = [](int c) { return c > 0 && c <= 32 && c % 4 == 0; };
    return ch(Ci) && ch(Ch) && ch(Co) && (ks == 1 || ks == 3) && kd >= 1 && kd <= CR_WIN && kd % 2 == 1;
}
static inline int cr_check_config(const char* who, int Ci, int Ch, int Co, int ks, int kd) {
    OSA_REQUIRE(cr_supported(Ci, Ch, Co, ks, kd),
                "%s: channels %d -> %d -> %d, kernels (1,%d,%d) and (%d,1,1) (supported: channels multiples of 4 up to 32, ks 1 or 3, kd odd up to %d)", who, Ci, Ch,
                Co, ks, ks, kd, CR_WIN);
    return 0;
}

}  // namespace osa

using namespace osa;

extern "C" size_t osa_conv3d_reduced_packed_floats(int Ci, int Ch, int Co, int ks, int kd) {
    return cr_supported(Ci, Ch, Co, ks, kd) ? cr_packed_floats(ks, kd) : 0;
}

extern "C" int osa_conv3d_reduced_pack_f32(const float* w1, const float* b1, const float* scale1, const float* shift1, const float* w2, const float* b2,
                                           const float* scale2, const float* shift2, float* packed, int Ci, int Ch, int Co, int ks, int kd, void* stream) {
    OSA_REQUIRE(w1 && b1 && scale1 && shift1 && w2 && b2 && scale2 && shift2 && packed, "conv3d_reduced_pack: NULL pointer");
    if (int rc = cr_check_config("conv3d_reduced_pack", Ci, Ch, Co, ks, kd)) return rc;
    const int total = (int)cr_packed_floats(ks, kd);
    hipLaunchKernelGGL(conv3d_reduced_pack_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w1, b1, scale1, shift1, w2, b2, scale2, shift2, packed, Ci,
                       Ch, Co, ks * ks, kd, total);
    OSA_LAUNCH_CHECK("conv3d_reduced_pack");
    return 0;
}

extern "C" int osa_conv3d_reduced_f32(const float* x, const float* packed, float* y, int layout, int B, int D, int H, int W, int Ci, int Ch, int Co, int ks, int kd,
                                      void* stream) {
    OSA_REQUIRE(x && packed && y, "conv3d_reduced: NULL pointer");
    OSA_REQUIRE(layout == OSA_NCDHW || layout == OSA_NDHWC, "conv3d_reduced: layout %d", layout);
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "conv3d_reduced: bad dims");
    if (int rc = cr_check_config("conv3d_reduced", Ci, Ch, Co, ks, kd)) return rc;
    const long long vox = (long long)B * D * H * W, tiles_x = cdiv(W, CR_TW), tiles_y = cdiv(H, CR_TH), tiles = (long long)B * tiles_x * tiles_y;
    const uintptr_t px = (uintptr_t)x, py = (uintptr_t)y, bx = (uintptr_t)vox * Ci * sizeof(float), by = (uintptr_t)vox * Co * sizeof(float);
    OSA_REQUIRE(py + by <= px || px + bx <= py, "conv3d_reduced: y overlaps x");
    OSA_REQUIRE((((uintptr_t)packed | (layout == OSA_NDHWC ? px | py : 0)) & 15) == 0, "conv3d_reduced: packed and channels-last tensors must be 16-byte aligned");
    // D is cut only when the pixel tiles leave more than half of the GPU idle, into segments of at least 2 (kd - 1) output planes: a
    // segment recomputes kd - 1 hidden planes
    long long nseg = 1;
    if (2 * tiles <= CR_CUS) {
        const long long want = CR_CUS / tiles, most = D / (2 * (kd - 1) > 8 ? 2 * (kd - 1) : 8);
        nseg = want < most ? want : most;
        if (nseg < 1) nseg = 1;
    }
    const int seg = cdiv(D, nseg);
    nseg = cdiv(D, seg);
    OSA_REQUIRE(tiles * nseg <= 0x7fffffffLL, "conv3d_reduced: %lld workgroups", tiles * nseg);
    const size_t lds = (cr_packed_floats(ks, kd) + 2 * CR_BUF) * sizeof(float);
    if (int rc = mv2_allow_lds<conv3d_reduced_kernel>("conv3d_reduced", (int)CR_MAX_LDS)) return rc;
    const CrArgs a{x, packed, y, layout == OSA_NDHWC ? 1 : 0, Ci, Ch, Co, ks, kd, D, H, W, (int)tiles_x, (int)tiles_y, (int)nseg, seg};
    hipLaunchKernelGGL(conv3d_reduced_kernel, dim3((unsigned)(tiles * nseg)), dim3(CR_NT), lds, (hipStream_t)stream, a);
    OSA_LAUNCH_CHECK("conv3d_reduced");
    return 0;
}
