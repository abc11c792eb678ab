// FoundationStereo's disparity transformer (foundationstereo/core/submodule.py:540-562, CostVolumeDisparityAttention, with its layers at
// :195-291 and :506-536) in eval mode as ONE launch.  For every pixel of cv [B,C,L,H,W] the L disparity planes are a sequence t [L,C]:
//
//   t = t + pe[:L]                                            once
//   per layer:  q,k,v = t Wq^T + bq, t Wk^T + bk, t Wv^T + bv   nhead heads of dh = C / nhead channels
//               o     = concat_h softmax(q_h k_h^T / sqrt(dh)) v_h
//               t     = LayerNorm1(t + o Wo^T + bo)
//               t     = LayerNorm2(t + gelu(t W1^T + b1) W2^T + b2)      erf GELU, eps 1e-5
//
// A wave owns one sequence and keeps it TRANSPOSED as one zero-padded 32 x 32 tile in the 16 accumulator registers of
// v_mfma_f32_32x32x2_f32: the lane holds the token (lane & 31), register r of lane half hh = lane >> 5 holds channel
//   row(r, hh) = (r & 3) + 8 (r >> 2) + 4 hh                  (the C/D map of the instruction).
// In that form the tile IS the operand of the next product, with no LDS round trip and no lane movement: K step s of an MFMA takes
// register s, so lane half hh supplies channel row(s, hh), and the other operand has to supply the same channel.  For a weight that is
// W[out = lane & 31][row(s, hh)], and four steps 4g .. 4g+3 are the four consecutive floats W[out][8g + 4hh ..] -- the pack launch stores
// every matrix as [in / 4][out = 32][in % 4], zero padded to 32 x 32, so that float4 number 64 g + lane of a matrix is a lane's operand
// of steps 4g .. 4g+3.  K is summed in the order of the steps: channels 0,1,2,3,8,9,.. on one half, 4,5,6,7,12,.. on the other.
//   X^T = W t^T  : the weight is the A operand, the tile the B operand -> [out channel][token], the tile's own form (q, k, Wo, W1, W2)
//   X   = t W^T  : the operands swapped                               -> [token][out channel]                       (v)
//   s^T = k q^T  : k^T registers as A (zero outside the head's channels), q^T registers as B -> [key][query]
//   o^T = v^T p^T: v registers as A (zero on lanes outside the head's channels), p^T registers as B, summed over the heads
// The softmax over the keys and the LayerNorm sums over the channels are then sums over a lane's 16 registers and ONE exchange with the
// other lane half.  Keys >= L are masked before the maximum and get the probability 0; LayerNorm sums run over the C real channels and
// the pad channels stay zero (their weights, biases, gains and shifts are zero in the packed block).  K steps beyond C, ff, L or the
// head's channels are skipped (wave-uniform tests).
//
// A workgroup of 8 waves takes 8 consecutive sequences (pixels along w, so that NCDHW loads and stores meet in 32-byte runs) and loops
// over the groups of 8; all layers' parameters stay in LDS when they fit 160 KiB (up to 6 layers), else each layer is staged in turn.
// Exact fp32 (the MFMA is an fmaf chain; expf, erff and 1 / sqrtf are the library's), no atomics, one wave computes a sequence in a
// fixed order: the bits do not depend on the batch size, the memory format or the run.
//
// Packed parameters (osa_disparity_attention_pack_f32), per layer DA_LAYER = 6 * 1024 + 10 * 32 floats:
//   Wq | Wk | Wv | Wo | W1 | W2  (each [8][32][4] as above)  | bq | bk | bv | bo | b1 | b2 | g1 | e1 | g2 | e2  (each [32])
#include "mv2_common.h"

namespace osa {

typedef float da_f32x16 __attribute__((ext_vector_type(16)));

constexpr int DA_NT = 512, DA_NWV = DA_NT / 64, DA_MAT = 1024, DA_VEC = 32, DA_LAYER = 6 * DA_MAT + 10 * DA_VEC;
constexpr int DA_MAX_LAYERS = 8, DA_MAX_GRID = 256;
constexpr size_t DA_MAX_LDS = 160 * 1024;
constexpr float DA_EPS = 1e-5f;

struct DaArgs {
    const float* x; const float* pe; const float* pk; float* y;
    int cl;                                                 // 1: [B,L,H,W,C], 0: [B,C,L,H,W]
    int C, L, nhead, ff, layers, resident;
    long long HW, nseq;
};

__device__ __forceinline__ int da_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// register r = vec[row(r, hh)]: a per-channel vector in the tile's form
__device__ __forceinline__ da_f32x16 da_rows(const float* vec, int hh) {
    da_f32x16 o;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v = ld4(vec + 8 * g + 4 * hh);
        o[4 * g] = v.x; o[4 * g + 1] = v.y; o[4 * g + 2] = v.z; o[4 * g + 3] = v.w;
    }
    return o;
}

// acc += W x (W_IS_A: [out][token]) or x W^T ([token][out]) over the first kdim channels of the tile x; kdim is a multiple of 4
template <bool W_IS_A>
__device__ __forceinline__ da_f32x16 da_linear(const float* wm, const da_f32x16& x, da_f32x16 acc, int lane, int kdim) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (8 * g < kdim) {
            const float4 w4 = ld4(wm + (64 * g + lane) * 4);
            const float w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc = W_IS_A ? __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], x[4 * g + j], acc, 0, 0, 0)
                             : __builtin_amdgcn_mfma_f32_32x32x2f32(x[4 * g + j], w[j], acc, 0, 0, 0);
        }
    }
    return acc;
}

// LayerNorm over the C real channels of every token of the tile; gain and shift are zero on the pad channels
__device__ __forceinline__ da_f32x16 da_layernorm(const da_f32x16& a, const float* gain, const float* shift, int hh, int C) {
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum += a[r];               // the pad channels are zero
    sum += __shfl_xor(sum, 32);
    const float mean = sum / (float)C;
    da_f32x16 d;
    float sq = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        d[r] = da_row(r, hh) < C ? a[r] - mean : 0.f;
        sq += d[r] * d[r];
    }
    sq += __shfl_xor(sq, 32);
    const float rstd = 1.f / sqrtf(sq / (float)C + DA_EPS);
    const da_f32x16 g = da_rows(gain, hh), e = da_rows(shift, hh);
#pragma unroll
    for (int r = 0; r < 16; ++r) d[r] = d[r] * rstd * g[r] + e[r];
    return d;
}

__global__ __launch_bounds__(DA_NT) void disparity_attention_kernel(const DaArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tok = lane & 31, hh = lane >> 5;
    const int C = p.C, L = p.L, dh = C / p.nhead;
    const float scale = 1.f / sqrtf((float)dh);
    const long long ngroups = (p.nseq + DA_NWV - 1) / DA_NWV;

    if (p.resident) {
        for (int i = tid; i < p.layers * (DA_LAYER / 4); i += DA_NT) reinterpret_cast<float4*>(smem)[i] = ld4(p.pk + (size_t)i * 4);
        __syncthreads();
    }

    for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long seq = grp * DA_NWV + wave;
        const bool live = seq < p.nseq && tok < L;          // this lane's token exists
        const long long b = seq / p.HW, pix = seq - b * p.HW;
        // element (token, channel c) of this wave's sequence: base + c * cstride
        const size_t base = p.cl ? (((size_t)b * L + tok) * p.HW + pix) * C : ((size_t)b * C * L + tok) * p.HW + pix;
        const size_t cstride = p.cl ? 1 : (size_t)L * p.HW;

        da_f32x16 t;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = 8 * g + 4 * hh;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && c0 < C) {                           // C is a multiple of 4
                const float4 e = ld4(p.pe + (size_t)tok * C + c0);
                if (p.cl) v = ld4(p.x + base + c0);
                else v = make_float4(p.x[base + c0 * cstride], p.x[base + (c0 + 1) * cstride], p.x[base + (c0 + 2) * cstride], p.x[base + (c0 + 3) * cstride]);
                v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
            }
            t[4 * g] = v.x; t[4 * g + 1] = v.y; t[4 * g + 2] = v.z; t[4 * g + 3] = v.w;
        }

        for (int layer = 0; layer < p.layers; ++layer) {
            const float* wl = smem + (p.resident ? layer * DA_LAYER : 0);
            if (!p.resident) {
                __syncthreads();                            // every wave has left the layer before
                for (int i = tid; i < DA_LAYER / 4; i += DA_NT) reinterpret_cast<float4*>(smem)[i] = ld4(p.pk + (size_t)layer * DA_LAYER + (size_t)i * 4);
                __syncthreads();
            }
            const float* const vec = wl + 6 * DA_MAT;

            const da_f32x16 qt = da_linear<true>(wl, t, da_rows(vec, hh), lane, C);
            const da_f32x16 kt = da_linear<true>(wl + DA_MAT, t, da_rows(vec + DA_VEC, hh), lane, C);
            da_f32x16 v;
            const float bv = vec[2 * DA_VEC + tok];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = bv;
            v = da_linear<false>(wl + 2 * DA_MAT, t, v, lane, C);      // [token][channel = lane & 31]

            da_f32x16 o;
#pragma unroll
            for (int r = 0; r < 16; ++r) o[r] = 0.f;
            for (int h = 0; h < p.nhead; ++h) {
                const int c0 = h * dh, c1 = c0 + dh;
                da_f32x16 s;
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {              // s^T [key][query] over the head's channels
                    const int ca = da_row(r, 0), cb = da_row(r, 1), c = da_row(r, hh);
                    if ((ca >= c0 && ca < c1) || (cb >= c0 && cb < c1))
                        s = __builtin_amdgcn_mfma_f32_32x32x2f32((c >= c0 && c < c1) ? kt[r] : 0.f, qt[r], s, 0, 0, 0);
                }
                float m = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = da_row(r, hh) < L ? s[r] * scale : -INFINITY;
                    m = fmaxf(m, s[r]);
                }
                m = fmaxf(m, __shfl_xor(m, 32));            // key 0 exists: m is finite
                float sum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = da_row(r, hh) < L ? expf(s[r] - m) : 0.f;
                    sum += s[r];
                }
                sum += __shfl_xor(sum, 32);
                const float inv = 1.f / sum;
                const bool mine = tok >= c0 && tok < c1;    // as an operand of o^T, this lane is channel `tok` of v
#pragma unroll
                for (int r = 0; r < 16; ++r)                // o^T [channel][query] += v^T p^T over the keys
                    if (da_row(r, 0) < L) o = __builtin_amdgcn_mfma_f32_32x32x2f32(mine ? v[r] : 0.f, s[r] * inv, o, 0, 0, 0);
            }

            da_f32x16 a = t + da_rows(vec + 3 * DA_VEC, hh);
            a = da_linear<true>(wl + 3 * DA_MAT, o, a, lane, C);
            t = da_layernorm(a, vec + 6 * DA_VEC, vec + 7 * DA_VEC, hh, C);

            da_f32x16 f = da_linear<true>(wl + 4 * DA_MAT, t, da_rows(vec + 4 * DA_VEC, hh), lane, C);
#pragma unroll
            for (int r = 0; r < 16; ++r) f[r] = 0.5f * f[r] * (1.f + erff(f[r] * 0.70710678118654752440f));
            a = t + da_rows(vec + 5 * DA_VEC, hh);
            a = da_linear<true>(wl + 5 * DA_MAT, f, a, lane, p.ff);
            t = da_layernorm(a, vec + 8 * DA_VEC, vec + 9 * DA_VEC, hh, C);
        }

#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = 8 * g + 4 * hh;
            if (live && c0 < C) {
                if (p.cl) store16(p.y + base + c0, make_float4(t[4 * g], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3]));
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) p.y[base + (c0 + j) * cstride] = t[4 * g + j];
                }
            }
        }
    }
}

// one thread per packed float; the sources are stacked over the layers: w_attn [N][4][C][C] (q, k, v, out), b_attn [N][4][C],
// w1 [N][ff][C], b1 [N][ff], w2 [N][C][ff], b2 [N][C], ln [N][4][C] (gain1, shift1, gain2, shift2)
__global__ __launch_bounds__(256) void disparity_attention_pack_kernel(const float* __restrict__ w_attn, const float* __restrict__ b_attn, const float* __restrict__ w1,
                                                                        const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                                        const float* __restrict__ ln, float* __restrict__ pk, int C, int ff, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int n = idx / DA_LAYER, i = idx - n * DA_LAYER;
    float v = 0.f;
    if (i < 6 * DA_MAT) {
        const int m = i / DA_MAT, e = i - m * DA_MAT, in = (e >> 7) * 4 + (e & 3), out = (e >> 2) & 31;
        const int nout = m == 4 ? ff : C, nin = m == 5 ? ff : C;
        if (out < nout && in < nin) {
            if (m < 4) v = w_attn[(((size_t)n * 4 + m) * C + out) * C + in];
            else if (m == 4) v = w1[((size_t)n * ff + out) * C + in];
            else v = w2[((size_t)n * C + out) * ff + in];
        }
    } else {
        const int k = (i - 6 * DA_MAT) / DA_VEC, c = (i - 6 * DA_MAT) - k * DA_VEC;
        if (k < 4) { if (c < C) v = b_attn[((size_t)n * 4 + k) * C + c]; }
        else if (k == 4) { if (c < ff) v = b1[(size_t)n * ff + c]; }
        else if (k == 5) { if (c < C) v = b2[(size_t)n * C + c]; }
        else if (c < C) v = ln[((size_t)n * 4 + (k - 6)) * C + c];
    }
    pk[idx] = v;
}

static inline bool da_supported(int C, int nhead, int ff, int layers) {
    return C > 0 && C <= 32 && C % 4 == 0 && nhead > 0 && C % nhead == 0 && ff > 0 && ff <= 32 && ff % 4 == 0 && layers >= 1 && layers <= DA_MAX_LAYERS;
}
static inline int da_check_config(const char* who, int C, int nhead, int ff, int layers) {
    OSA_REQUIRE(da_supported(C, nhead, ff, layers),
                "%s: C %d, nhead %d, ff %d, layers %d (supported: C and ff multiples of 4 up to 32, nhead a divisor of C, 1 .. %d layers)", who, C, nhead, ff, layers,
                DA_MAX_LAYERS);
    return 0;
}

}  // namespace osa

using namespace osa;

extern "C" size_t osa_disparity_attention_packed_floats(int C, int nhead, int ff, int layers) {
    return da_supported(C, nhead, ff, layers) ? (size_t)layers * DA_LAYER : 0;
}

extern "C" int osa_disparity_attention_pack_f32(const float* w_attn, const float* b_attn, const float* w1, const float* b1, const float* w2, const float* b2,
                                                const float* ln, float* packed, int C, int nhead, int ff, int layers, void* stream) {
    OSA_REQUIRE(w_attn && b_attn && w1 && b1 && w2 && b2 && ln && packed, "disparity_attention_pack: NULL pointer");
    if (int rc = da_check_config("disparity_attention_pack", C, nhead, ff, layers)) return rc;
    const int total = layers * DA_LAYER;
    hipLaunchKernelGGL(disparity_attention_pack_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w_attn, b_attn, w1, b1, w2, b2, ln, packed, C, ff, total);
    OSA_LAUNCH_CHECK("disparity_attention_pack");
    return 0;
}

extern "C" int osa_disparity_attention_f32(const float* cv, const float* pe, const float* packed, float* out, int layout, int B, int C, int L, int H, int W,
                                           int nhead, int ff, int layers, void* stream) {
    OSA_REQUIRE(cv && pe && packed && out, "disparity_attention: NULL pointer");
    OSA_REQUIRE(layout == OSA_NCDHW || layout == OSA_NDHWC, "disparity_attention: layout %d", layout);
    OSA_REQUIRE(B > 0 && H > 0 && W > 0, "disparity_attention: bad dims");
    if (int rc = da_check_config("disparity_attention", C, nhead, ff, layers)) return rc;
    OSA_REQUIRE(L >= 1 && L <= 32, "disparity_attention: %d disparity planes (supported: 1 .. 32)", L);
    const long long hw = (long long)H * W, nseq = (long long)B * hw;
    const uintptr_t px = (uintptr_t)cv, py = (uintptr_t)out, bytes = (uintptr_t)nseq * L * C * sizeof(float);
    OSA_REQUIRE(py + bytes <= px || px + bytes <= py, "disparity_attention: out overlaps cv");
    OSA_REQUIRE((((uintptr_t)pe | (uintptr_t)packed | (layout == OSA_NDHWC ? px | py : 0)) & 15) == 0,
                "disparity_attention: pe, packed and channels-last tensors must be 16-byte aligned");
    const int resident = (size_t)layers * DA_LAYER * sizeof(float) <= DA_MAX_LDS ? 1 : 0;
    const size_t lds = (size_t)(resident ? layers : 1) * DA_LAYER * sizeof(float);
    if (int rc = mv2_allow_lds<disparity_attention_kernel>("disparity_attention", (int)DA_MAX_LDS)) return rc;
    const long long ngroups = (nseq + DA_NWV - 1) / DA_NWV;
    const DaArgs a{cv, pe, packed, out, layout == OSA_NDHWC ? 1 : 0, C, L, nhead, ff, layers, resident, hw, nseq};
    hipLaunchKernelGGL(disparity_attention_kernel, dim3((unsigned)(ngroups < DA_MAX_GRID ? ngroups : DA_MAX_GRID)), dim3(DA_NT), lds, (hipStream_t)stream, a);
    OSA_LAUNCH_CHECK("disparity_attention");
    return 0;
}
